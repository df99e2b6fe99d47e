"""The threshold / class-scale sweep on the MI355X: xv2_calibrate_hist (csrc/calibrate.hip) and xv2_postprocess_ex
(csrc/postproc.hip) through ops and utils/calibrate.py, against the numpy restatement of tests/calibrate_ref.py.  Every value
is an integer, so every comparison is == / torch.equal.  Each direct call runs between canary stretches around its outputs,
and its inputs are compared with their copies afterwards."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import calibrate_ref as C
import postproc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64
FILL = 0x5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, fill=FILL):
    buf = torch.full((2 * CAN + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, what, fill=FILL):
    assert bool((buf[:CAN] == fill).all()) and bool((buf[-CAN:] == fill).all()), what + ": canary overwritten"


def _same(a, b):
    """bitwise equality (loc holds NaN, which torch.equal calls unequal to itself)"""
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _kind(dmg):
    return {4: 0, 5: 1}[dmg.shape[1]] if dmg.ndim == 4 else 2


def _grid(n):
    from xview2_amd.utils import calibrate
    return {1: np.array([0.3], dtype=np.float32), 2: np.array([0.1, 0.3], dtype=np.float32),
            100: calibrate.threshold_grid(0.01), 128: calibrate.threshold_grid(1 / 128.0)}[n]


def _hist_call(loc, dmg, lt, dt, T, scales=None, calls=1):
    """`calls` xv2_calibrate_hist on caller-owned buffers (numpy in, batched) -> numpy (hist [S, n+1, 4, 2, 5], bad)"""
    from xview2_amd import _capi
    ins = [_dev(loc.astype(np.float32)), _dev(dmg.astype(np.float32) if dmg.ndim == 4 else dmg.astype(np.int32)), _dev(lt),
           _dev(dt), _dev(np.asarray(T, dtype=np.float32))]
    if scales is not None:
        ins.append(_dev(np.asarray(scales, dtype=np.float32)))
    keep = [t.clone() for t in ins]
    B, H, W = loc.shape
    n, S = len(T), 1 if scales is None else len(scales)
    h_buf, h = _guarded(S * (n + 1) * 40, torch.int64)
    b_buf, bad = _guarded(1, torch.int64)
    h.zero_()
    bad.zero_()
    torch.cuda.synchronize()
    for _ in range(calls):
        _capi.call("xv2_calibrate_hist", ins[0], ins[1], _kind(dmg), ins[2], ins[3], B, H, W, ins[4], n,
                   ins[5] if scales is not None else None, S, h, bad)
    torch.cuda.synchronize()
    _intact(h_buf, "hist")
    _intact(b_buf, "bad")
    assert all(_same(a, b) for a, b in zip(ins, keep)), "an input was written"
    return h.cpu().numpy().reshape(S, n + 1, 4, 2, 5), int(bad.item())


def _ex_call(loc, dmg, a, b, scale=None, components=False, rate=0):
    """one xv2_postprocess_ex on caller-owned buffers (numpy in, batched) -> numpy uint8 (pre, post)"""
    from xview2_amd import _capi
    import ctypes
    ins = [_dev(loc.astype(np.float32)), _dev(dmg.astype(np.float32) if dmg.ndim == 4 else dmg.astype(np.int32))]
    keep = [t.clone() for t in ins]
    B, H, W = loc.shape
    need = int(_capi.query("xv2_postprocess_workspace", B, H, W, 1 if components else 0))
    ws_buf = torch.full((512 + need,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws_buf[256:256 + need]
    assert ws.data_ptr() % 256 == 0
    p_buf, pre = _guarded(B * H * W, torch.uint8)
    q_buf, post = _guarded(B * H * W, torch.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    cs = (ctypes.c_float * 4)(*scale) if scale is not None else None
    torch.cuda.synchronize()
    _capi.call("xv2_postprocess_ex", ins[0], ins[1], _kind(dmg), B, H, W, 1 if components else 0, rate,
               ws if (components or rate) else None, pre, post, status, float(np.float32(a)), float(np.float32(b)),
               ctypes.addressof(cs) if cs is not None else None)
    torch.cuda.synchronize()
    _intact(p_buf, "pre")
    _intact(q_buf, "post")
    assert bool((ws_buf[:256] == 0xA5).all()) and bool((ws_buf[256 + need:] == 0xA5).all()), "workspace: canary overwritten"
    assert all(_same(x, y) for x, y in zip(ins, keep)), "an input was written"
    return pre.cpu().numpy().reshape(B, H, W), post.cpu().numpy().reshape(B, H, W), int(status.item())


def _inputs(seed, B, H, W, T, kind):
    """(loc, dmg, lt, dt) batched: loc on every threshold, its neighbours, NaN, -1, 2; tied and flipping damage scores, or a
    label map over -1..5; targets with dt > 0 on lt = 0 and the values 5 and 255"""
    loc = np.stack([C.edge_loc(seed + b, (H, W), T) for b in range(B)])
    if kind == 2:
        dmg = np.stack([R.hash_int(seed + 50 + b, (H, W), 7) - 1 for b in range(B)])
    else:
        dmg = np.stack([C.tie_dmg(seed + 50 + b, (H, W), 4 + kind) for b in range(B)])
    tg = [C.targets(seed + 100 + 7 * b, (H, W)) for b in range(B)]
    return loc, dmg, np.stack([t[0] for t in tg]), np.stack([t[1] for t in tg])


# ---- the histogram ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (64, 64), (65, 67), (3, 1001)])
def test_hist_equals_the_restatement(H, W, B):
    for n in (1, 2, 100, 128):
        T = _grid(n)
        for kind in (0, 1, 2):
            loc, dmg, lt, dt = _inputs(1000 * n + 10 * kind + H, B, H, W, T, kind)
            for scales in ((None,) if kind == 2 else (None, C.SCALES)):
                got, bad = _hist_call(loc, dmg, lt, dt, T, scales)
                want, wbad = C.hist(list(loc), list(dmg), list(lt), list(dt), T, scales)
                assert np.array_equal(got, want), (n, kind, scales is not None, int(np.abs(got - want).sum()))
                assert bad == wbad
                assert got.sum() == (1 if scales is None else 3) * (B * H * W - wbad)


def test_wide_targets_leave_the_bins_alone():
    T = _grid(100)
    loc, dmg, lt, dt = _inputs(77, 2, 65, 67, T, 0)
    got, bad = _hist_call(loc, dmg, lt, dt, T, C.SCALES)
    wide = (lt > 4) | (dt > 4)
    assert bad == int(wide.sum()) > 0 and ((dt > 0) & (lt == 0)).any()
    # the same tiles with those pixels' targets made valid but their probabilities' bins removed by hand
    lt2, dt2 = np.where(wide, 0, lt).astype(np.uint8), np.where(wide, 0, dt).astype(np.uint8)
    full, bad2 = _hist_call(loc, dmg, lt2, dt2, T, C.SCALES)
    only, _ = C.hist([l[w][None] for l, w in zip(loc, wide)], [d[:, w][:, None] for d, w in zip(dmg, wide)],
                     [np.zeros((1, int(w.sum())), np.uint8) for w in wide], [np.zeros((1, int(w.sum())), np.uint8) for w in wide],
                     T, C.SCALES)
    assert bad2 == 0 and np.array_equal(full - only, got)


def test_a_second_call_doubles_every_bin():
    T = _grid(100)
    loc, dmg, lt, dt = _inputs(5, 3, 65, 67, T, 1)
    once, bad1 = _hist_call(loc, dmg, lt, dt, T, C.SCALES)
    twice, bad2 = _hist_call(loc, dmg, lt, dt, T, C.SCALES, calls=2)
    assert np.array_equal(twice, 2 * once) and bad2 == 2 * bad1 and bad1 > 0


def test_one_bin_holds_a_whole_tile():
    T = _grid(100)
    loc = np.full((1, 256, 256), 0.5, dtype=np.float32)
    dmg = np.zeros((1, 4, 256, 256), dtype=np.float32)
    dmg[:, 1] = 1
    lt = np.ones((1, 256, 256), dtype=np.uint8)
    dt = np.full((1, 256, 256), 2, dtype=np.uint8)
    got, bad = _hist_call(loc, dmg, lt, dt, T)
    want = np.zeros_like(got)
    want[0, 50, 1, 1, 2] = 65536          # T_50 = 0.5f is not below 0.5f: k = 50
    assert np.array_equal(got, want) and bad == 0


def _buildings_tile(H=256, W=256):
    cls = R.buildings(11)[:H, :W]
    dt = R.buildings(500)[:H, :W].astype(np.uint8)
    return (R.loc_from_mask(12, cls > 0)[None], R.probs_from_classes(13, cls, 4)[None], (dt > 0).astype(np.uint8)[None],
            dt[None])


def test_a_crop_of_the_buildings_tile():
    T = _grid(100)
    loc, dmg, lt, dt = _buildings_tile()
    got, bad = _hist_call(loc, dmg, lt, dt, T, C.SCALES)
    want, _ = C.hist(list(loc), list(dmg), list(lt), list(dt), T, C.SCALES)
    assert np.array_equal(got, want) and bad == 0
    # most pixels are background below 0.1: ten values of k times four of r, with t = d = 0
    assert got[0, :11, :, 0, 0].sum() > 0.5 * 256 * 256 and got[0, 0].sum() == 0


def test_ops_accumulates_and_checks():
    from xview2_amd import ops
    T = _grid(100)
    loc, dmg, lt, dt = _inputs(9, 2, 33, 40, T, 0)
    args = [_dev(x) for x in (loc, dmg, lt, dt)]
    h, bad = ops.calibrate_hist(*args, T, C.SCALES)
    assert h.shape == (3, 101, 4, 2, 5) and h.dtype == torch.int64
    h2, bad2 = ops.calibrate_hist(*args, T, C.SCALES, h.clone(), bad.clone())
    want, wbad = C.hist(list(loc), list(dmg), list(lt), list(dt), T, C.SCALES)
    assert np.array_equal(h.cpu().numpy(), want) and np.array_equal(h2.cpu().numpy(), 2 * want)
    assert int(bad) == wbad and int(bad2) == 2 * wbad
    plain, _ = ops.calibrate_hist(*args, T)
    assert torch.equal(plain[0], h[0])
    for kw in (dict(thresholds=[0.2, 0.1]), dict(scales=[(1, 1, 0, 1)]), dict(scales=[(1, 1, 1)]),
               dict(scales=[C.ONES] * 65), dict(hist=torch.zeros(3, dtype=torch.int64, device=DEV))):
        a = dict(thresholds=T, scales=C.SCALES, hist=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.calibrate_hist(*args, a["thresholds"], a["scales"], a["hist"])
    with pytest.raises(ValueError, match="label map"):
        ops.calibrate_hist(args[0], args[2].to(torch.int32), args[2], args[3], T, C.SCALES)


# ---- the closed loop: histogram -> derive == fuse -> scorer ---------------------------------------------------------------
POINTS = [(30, 10, 0), (30, 30, 1), (50, 0, 2), (99, 99, 0), (99, 0, 1), (0, 0, 2), (99, 50, 2), (10, 10, 0), (31, 29, 1),
          (64, 1, 2), (1, 0, 0), (98, 97, 1)]


@pytest.mark.parametrize("C_", [4, 5])
def test_derived_counts_equal_the_scored_fusion(C_):
    from xview2_amd import ops
    from xview2_amd.utils import calibrate
    T = _grid(100)
    assert T[30] == np.float32(0.3) and T[10] == np.float32(0.1)
    tl = C.tiles(300 + C_, 3, 65, 67, T, C_)
    loc, dmg, lt, dt = (_dev(np.stack(x)) for x in zip(*tl))
    h, bad = ops.calibrate_hist(loc, dmg, lt, dt, T, C.SCALES)
    assert int(bad) == 0
    counts = calibrate.derive(h.cpu().numpy())
    for i, j, s in POINTS:
        pre, post = ops.postprocess(loc, dmg, loc_threshold=float(T[i]), dmg_threshold=float(T[j]), class_scale=C.SCALES[s])
        rows = ops.xview2_counts(pre, post, lt, dt).sum(dim=0).cpu().numpy()
        assert rows[15] == 0 and counts[s, i, j].tolist() == rows[:15].tolist(), (i, j, s)
    assert counts[0, 30, 10].tolist() == C.brute(*zip(*tl), 0.3, 0.1, None)


# ---- the parameterised fusion -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases():
    c = R.cases()
    return {k: c[k] for k in ("thresholds", "buildings_4ch", "buildings_5ch", "vote_ties")}


@pytest.mark.parametrize("mode", ["plain", "components", "rate3"])
@pytest.mark.parametrize("name", ["thresholds", "buildings_4ch", "buildings_5ch", "vote_ties"])
def test_the_default_parameters_are_inert(name, mode):
    from xview2_amd import ops
    loc, dmg = (_dev(x)[None] for x in _cases()[name])
    kw = dict(components=mode == "components", rate=3 if mode == "rate3" else 0)
    want = ops.postprocess(loc, dmg, **kw)
    got = ops.postprocess(loc, dmg, loc_threshold=0.3, dmg_threshold=0.1, class_scale=(1, 1, 1, 1), **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    only_a = ops.postprocess(loc, dmg, loc_threshold=0.3, **kw)
    assert torch.equal(only_a[0], want[0]) and torch.equal(only_a[1], want[1])


@pytest.mark.parametrize("a,b,scale", [(0.5, 0.2, None), (0.42, 0.42, (1.0, 2.0, 1.0, 0.5)), (0.7, 0.0, (1.0, 3.0, 0.25, 7.0)),
                                       (0.3, 0.1, (1.0, 2.0, 1.0, 0.5)), (0.05, -1.0, None)])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_the_fusion_at_other_points_equals_the_restatement(kind, a, b, scale):
    if kind == 2:
        scale = None      # a label map takes no scales (an argument error, covered without a GPU): the thresholds alone
    T = np.array(sorted({np.float32(b), np.float32(a)}), dtype=np.float32)
    B, H, W = 3, 65, 67
    loc = np.stack([C.edge_loc(40 + k, (H, W), T) for k in range(B)])      # loc exactly at a, at b, and at their neighbours
    assert (loc == np.float32(a)).any() and (loc == np.nextafter(np.float32(a), np.float32(4))).any()
    dmg = (np.stack([R.hash_int(60 + k, (H, W), 5) for k in range(B)]) if kind == 2
           else np.stack([C.tie_dmg(60 + k, (H, W), 4 + kind) for k in range(B)]))
    pre, post, status = _ex_call(loc, dmg, a, b, scale)
    assert status == 0
    for k in range(B):
        wpre, wpost = C.fuse(loc[k], dmg[k], a, b, scale)
        assert np.array_equal(pre[k], wpre) and np.array_equal(post[k], wpost), k
    if kind != 2:       # the vote and the dilation behind the parameterised fusion are the ones behind the fixed one
        cpre, cpost, _ = _ex_call(loc, dmg, a, b, scale, components=True, rate=3)
        for k in range(B):
            wpre, wpost = C.fuse(loc[k], dmg[k], a, b, scale)
            assert np.array_equal(cpre[k], R.dilate(wpre, 3)) and np.array_equal(cpost[k], R.dilate(R.vote(wpost), 3)), k


def test_post_process_tiles_applies_the_parameters_to_the_fusing_pass_only():
    from xview2_amd.utils.post_process import post_process_tiles
    T = np.array([0.2, 0.6], dtype=np.float32)
    loc, dmg = C.edge_loc(3, (70, 90), T), C.tie_dmg(4, (70, 90))
    pre, post = post_process_tiles(_dev(loc), _dev(dmg), loc_threshold=0.6, dmg_threshold=0.2, class_scale=C.SCALES[1])
    wpre, wpost = C.fuse(loc, dmg, 0.6, 0.2, C.SCALES[1])
    assert np.array_equal(pre.cpu().numpy(), wpre) and np.array_equal(post.cpu().numpy(), wpost)
    # min_area = 1 drops nothing: the second pass (components over the 0/1 map) must vote on exactly the fused buildings
    pre2, post2 = post_process_tiles(_dev(loc), _dev(dmg), components=True, min_area=1, loc_threshold=0.6, dmg_threshold=0.2,
                                     class_scale=C.SCALES[1])
    assert np.array_equal(pre2.cpu().numpy(), wpre) and np.array_equal(post2.cpu().numpy(), R.vote(wpost))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _write_results(root):
    from PIL import Image
    os.makedirs(os.path.join(root, "probs"))
    os.makedirs(os.path.join(root, "targets"))
    tiles = []
    for k in range(4):
        cls = R.buildings(700 + k, 128, 128, 14)
        truth = np.roll(cls, 2, axis=1)
        truth = np.where(R.hash_int(710 + k, cls.shape, 9) == 0, np.where(truth > 0, 1 + truth % 4, 0), truth).astype(np.uint8)
        # soft localization: a wide band of doubt around 0.3, so that the threshold matters
        loc = (R.hash_unit(720 + k, cls.shape) * np.float32(0.5) + np.where(cls > 0, np.float32(0.25), np.float32(0))).astype(np.float32)
        dmg = R.probs_from_classes(730 + k, cls, 4)
        dmg[1] *= np.float32(0.75)             # an under-confident class: scales have something to mend
        lt, dt = (truth > 0).astype(np.uint8), truth
        np.save(os.path.join(root, "probs", "test_localization_%05d.npy" % k), loc)
        np.save(os.path.join(root, "probs", "test_damage_%05d.npy" % k), dmg)
        Image.fromarray(lt).save(os.path.join(root, "targets", "test_localization_%05d_target.png" % k))
        Image.fromarray(dt).save(os.path.join(root, "targets", "test_damage_%05d_target.png" % k))
        tiles.append((loc, dmg, lt, dt))
    return tiles


def test_end_to_end(tmp_path):
    from PIL import Image
    from xview2_amd.utils import calibrate, post_process
    root = str(tmp_path / "results")
    tiles = _write_results(root)
    cols = list(zip(*tiles))
    scales = "1,1,1,1;1,2,1,0.5;1,1.5,1,1"
    argv = ["--results", root, "--class_scales", scales, "--batch", "3", "--table", str(tmp_path / "table.npy")]
    doc = calibrate.run(calibrate.get_parser().parse_args(argv))
    first = open(os.path.join(root, "calibration.json"), "rb").read()
    assert json.loads(first) == doc and (doc["tiles"], doc["pixels"], doc["bad"]) == (4, 4 * 128 * 128, 0)
    want_default = C.brute(*cols, 0.3, 0.1, None)
    assert doc["default"]["counts"] == want_default and doc["default"]["scores"] == R.score([want_default])
    assert doc["default"]["grid_index"] == [30, 10]
    b = doc["best"]
    assert b["scores"]["score"] >= doc["default"]["scores"]["score"]
    assert b["counts"] == C.brute(*cols, b["loc_threshold"], b["loc_threshold_dmg"], b["class_scale"])
    assert b["scores"] == R.score([b["counts"]])
    # without post-processing flags the real pipeline gives the swept numbers exactly
    for key in ("default", "best"):
        assert doc["verified"][key]["counts"] == doc[key]["counts"] and doc["verified"][key]["scores"] == doc[key]["scores"]
    table = np.load(str(tmp_path / "table.npy"))
    s, i, j = b["index"]
    assert table.shape == (3, 100, 100) and table[s, i, j] >= np.nanmax(table) - 1e-12 and np.isnan(table[0, 0, 1])
    assert abs(table[0, 30, 10] - doc["default"]["scores"]["score"]) < 1e-12
    # utils.post_process --calibration writes the best point's maps
    post_process.run(post_process.get_parser().parse_args(["--results", root, "--calibration", os.path.join(root, "calibration.json")]))
    for k, (loc, dmg, _, _) in enumerate(tiles):
        wpre, wpost = C.fuse(loc, dmg, b["loc_threshold"], b["loc_threshold_dmg"],
                             None if tuple(b["class_scale"]) == C.ONES else b["class_scale"])
        pre = np.asarray(Image.open(os.path.join(root, "predictions", "test_localization_%05d_prediction.png" % k)))
        post = np.asarray(Image.open(os.path.join(root, "predictions", "test_damage_%05d_prediction.png" % k)))
        assert np.array_equal(pre, wpre) and np.array_equal(post, wpost), k
    # the same bytes on a second run
    calibrate.run(calibrate.get_parser().parse_args(argv))
    assert open(os.path.join(root, "calibration.json"), "rb").read() == first
    # --components can move the numbers: the report shows both, and says which flags it verified with
    doc2 = calibrate.run(calibrate.get_parser().parse_args(argv + ["--components", "--out", str(tmp_path / "c.json")]))
    assert doc2["best"] == doc["best"] and doc2["verified"]["flags"]["components"] is True
    os.remove(os.path.join(root, "targets", "test_damage_00002_target.png"))
    with pytest.raises(FileNotFoundError, match="test_damage_00002_target.png"):
        calibrate.run(calibrate.get_parser().parse_args(argv))
