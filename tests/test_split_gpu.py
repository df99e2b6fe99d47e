"""Splitting touching buildings on the MI355X (csrc/split.hip through xv2_edt_sq, xv2_split_seed / _grow / _finish,
ops.split_buildings and utils/split.py) against the host restatement of tests/split_ref.py.  Every value is an integer, so
every comparison is np.array_equal / torch.equal.  Each direct call runs between canary stretches around out, labels, d2,
pending and the workspace, and its inputs are compared with their copies afterwards."""
import functools

import numpy as np
import pytest
import torch

import buildings_ref as R
import split_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of out (uint8), labels (int32), d2 (uint16) and pending (int32)
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = 0x5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, fill=FILL):
    buf = torch.full((2 * CAN + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, what, fill=FILL, can=CAN):
    assert bool((buf[:can] == fill).all()) and bool((buf[-can:] == fill).all()), what + ": canary overwritten"


def _edt(masks, cap):
    """xv2_edt_sq on a caller-owned d2 between canaries; masks uint8 [B,H,W] (numpy) -> numpy int64 [B,H,W]"""
    from xview2_amd import _capi
    m = _dev(masks)
    keep = m.clone()
    B, H, W = m.shape
    buf, d2 = _guarded(B * H * W, torch.int16)        # (the same 16 bits; the canary compare runs on int16)
    torch.cuda.synchronize()
    _capi.call("xv2_edt_sq", m, B, H, W, cap, d2)
    torch.cuda.synchronize()
    _intact(buf, "d2")
    assert torch.equal(m, keep), "the mask was written"
    return d2.cpu().numpy().view(np.uint16).astype(np.int64).reshape(B, H, W)


def _split(masks, r2, sweeps=8, max_calls=4000):
    """seed, grow until pending is 0, finish, on caller-owned buffers -> numpy (out [B,H,W], L [B,H,W], grow calls)"""
    from xview2_amd import _capi
    m = _dev(masks)
    keep = m.clone()
    B, H, W = m.shape
    need = int(_capi.query("xv2_split_workspace", B, H, W))
    assert need > 0
    ws_buf = torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws_buf[CAN_WS:CAN_WS + need]
    out_buf, out = _guarded(B * H * W, torch.uint8)
    lab_buf, lab = _guarded(B * H * W, torch.int32)
    pen_buf, pending = _guarded(1, torch.int32)
    torch.cuda.synchronize()
    _capi.call("xv2_split_seed", m, B, H, W, r2, ws)
    calls = 0
    while True:
        _capi.call("xv2_split_grow", m, B, H, W, sweeps, ws, pending)
        calls += 1
        if int(pending.item()) == 0:
            break
        assert calls < max_calls, "the growth does not converge"
    _capi.call("xv2_split_finish", m, B, H, W, ws, out, lab)
    torch.cuda.synchronize()
    for buf, what in ((out_buf, "out"), (lab_buf, "labels"), (pen_buf, "pending")):
        _intact(buf, what)
    _intact(ws_buf, "workspace", 0xA5, CAN_WS)
    assert torch.equal(m, keep), "the mask was written"
    # a NULL labels gives the same out
    out2_buf, out2 = _guarded(B * H * W, torch.uint8)
    _capi.call("xv2_split_finish", m, B, H, W, ws, out2, None)
    torch.cuda.synchronize()
    _intact(out2_buf, "out")
    assert torch.equal(out, out2)
    return out.cpu().numpy().reshape(B, H, W), lab.cpu().numpy().reshape(B, H, W), calls


@functools.lru_cache(maxsize=None)
def _want(key, r2):
    """the restatement of every tile of a named batch, computed once: (out [B,H,W], L [B,H,W], rounds per tile)"""
    res = [S.split(t, r2) for t in _batch(key)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), [r[2] for r in res]


def _check_split(key, r2, sweeps=8):
    masks = _batch(key)
    out, L, calls = _split(masks, r2, sweeps)
    want_out, want_L, _ = _want(key, r2)
    assert np.array_equal(L, want_L), "L differs in %d pixels" % int((L != want_L).sum())
    assert np.array_equal(out, want_out), "out differs in %d pixels" % int((out != want_out).sum())
    return out, L, calls


# ---- masks ---------------------------------------------------------------------------------------------------------------
def _corner_zero(H, W):
    m = np.ones((4, H, W), dtype=np.uint8)
    m[0, 0, 0] = m[1, 0, W - 1] = m[2, H - 1, 0] = m[3, H - 1, W - 1] = 0
    return m


def _three_and_none():
    """three bodies joined by two necks (three seeds at r2 = 4), and one pixel away a long bar two pixels wide (no seed)"""
    m = np.zeros((40, 80), dtype=np.uint8)
    for k in range(3):
        m[3:17, 3 + 24 * k:17 + 24 * k] = 1
    m[9:11, 17:27] = 1
    m[8:12, 41:51] = 1
    m[20:22, 2:78] = 7
    return m[None]


def _staircase():
    """a body in the first block region and one in the region diagonally below, joined by a staircase three pixels wide that
    crosses the region borders at y = 64 and x = 64 several times; and a blob field of the same size"""
    m = np.zeros((140, 140), dtype=np.uint8)
    m[20:40, 20:40] = 1
    m[100:120, 100:125] = 1
    y, x = 38, 40
    while y < 100:
        m[y:y + 3, x:x + 9] = 1          # a step to the right ...
        m[y:y + 9, x + 6:x + 9] = 1      # ... and one down
        y, x = y + 6, x + 6
    m[y:y + 3, x - 3:x + 3] = 1
    return np.stack([m, S.blob_mask(31, 140, 140), m.T.copy()])


@functools.lru_cache(maxsize=None)
def _batch(key):
    if key.startswith("dumbbells"):
        return np.stack([S.dumbbell(n, int(key[-1]))[0] for n in range(1, 7)])
    if key == "blobs":
        return np.stack([S.blob_mask(seed, 90, 70) for seed in (11, 12, 13, 14)])
    if key == "values":
        return np.stack([S.blob_mask(seed, 67, 93, values=True) for seed in (21, 22)])
    if key == "three_and_none":
        return _three_and_none()
    if key == "staircase":
        return _staircase()
    if key == "serpentine":
        return S.serpentine()[None]
    raise KeyError(key)


# ---- distance ------------------------------------------------------------------------------------------------------------
def _edt_cases():
    one = np.ones((1, 63, 65), dtype=np.uint8)
    big = np.ones((1, 193, 191), dtype=np.uint8)      # a few zeros far apart: distances up to the largest cap
    big[0][R._hash(5, (193, 191), 3000) == 0] = 0
    return {
        "1x1": np.array([[[1]], [[0]]], dtype=np.uint8),
        "row_150": np.stack([S.blob_mask(1, 1, 150), _corner_zero(1, 150)[1]]),
        "col_150": np.stack([S.blob_mask(2, 150, 1), _corner_zero(150, 1)[2]]),
        "63x65": np.concatenate([S.blob_mask(3, 63, 65)[None], one, 0 * one, _corner_zero(63, 65)]),
        "3x70x130": np.stack([S.blob_mask(seed, 70, 130) for seed in (6, 7, 8)]),
        "193x191": big,                  # wider and taller than a block's 64 x 64 region plus its halo, at every cap
    }


@pytest.mark.parametrize("cap", [1, 2, 5, 64])
@pytest.mark.parametrize("name", sorted(_edt_cases()))
def test_edt(name, cap):
    masks = _edt_cases()[name]
    got = _edt(masks, cap)
    for b, m in enumerate(masks):
        want = S.edt_sq(m, cap)
        assert np.array_equal(got[b], want), "tile %d: %d pixels differ" % (b, int((got[b] != want).sum()))
    if name == "63x65":
        assert np.all(got[1] == cap * cap) and np.all(got[2] == 0)       # all ones: the tile edge is no background
        assert got[3][0, 0] == 0 and got[3][0, 1] == min(1, cap * cap) and got[6][62, 64] == 0


def test_edt_through_ops():
    from xview2_amd import ops
    m = S.blob_mask(9, 50, 77)
    d2 = ops.edt_sq(_dev(m[None]), 4)
    assert d2.dtype == torch.uint16 and np.array_equal(d2[0].cpu().numpy().astype(np.int64), S.edt_sq(m, 4))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="cap"):
            ops.edt_sq(_dev(m[None]), bad)


# ---- split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", [1, 2, 4, 5, 8, 9])
@pytest.mark.parametrize("neck_len", [6, 7])
def test_dumbbells_are_cut_iff_half_the_neck_fits_the_radius(neck_len, r2):
    key = "dumbbells%d" % neck_len
    out, _, _ = _check_split(key, r2)
    for n in range(1, 7):
        m, col, top = S.dumbbell(n, neck_len)
        want = m.copy()
        if ((n + 1) // 2) ** 2 <= r2:
            want[top:top + n, col + (neck_len + 1) // 2] = 0
        assert np.array_equal(out[n - 1], want), "neck width %d" % n


@pytest.mark.parametrize("r2", [1, 2, 4, 5, 9])
def test_random_blobs(r2):
    out, L, _ = _check_split("blobs", r2)
    assert int((out != _batch("blobs")).sum()) > 20 and len(np.unique(L)) > 20


@pytest.mark.parametrize("r2", [2, 4])
def test_mask_values_are_kept(r2):
    out, _, _ = _check_split("values", r2)
    m = _batch("values")
    assert m.max() > 200 and np.all((out == m) | (out == 0)) and int((out != m).sum()) > 0


def test_a_component_without_a_seed_next_to_one_with_three():
    out, L, _ = _check_split("three_and_none", 4)
    m = _batch("three_and_none")
    assert len(np.unique(L[0, :18])) == 4 and not L[0, 18:].any()            # three labels and 0; the bar has none
    assert np.array_equal(out[0, 18:], m[0, 18:]) and int((out != m).sum()) == 2 + 4


def test_growth_crosses_region_borders_in_both_axes():
    out, L, _ = _check_split("staircase", 4)
    m = _batch("staircase")
    assert [int((out[b] != m[b]).sum()) for b in (0, 2)] == [3, 3] and len(np.unique(L[0])) == 3
    assert len(np.unique(L[1])) > 50


def test_serpentine_converges_whatever_the_sweeps_per_call():
    from xview2_amd import ops
    assert _want("serpentine", 4)[2][0] > 1000
    out8, L8, calls8 = _check_split("serpentine", 4, sweeps=8)
    out1, L1, calls1 = _check_split("serpentine", 4, sweeps=1)
    assert np.array_equal(out1, out8) and np.array_equal(L1, L8)
    assert calls1 > 9 and 8 * (calls8 - 1) < calls1 <= 8 * calls8
    m = _dev(_batch("serpentine"))
    a, ca = ops.split_buildings(m, 4)
    b, cb, lab = ops.split_buildings(m, 4, return_labels=True)
    assert ca == cb == calls8 and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), out8)
    assert np.array_equal(lab.cpu().numpy(), L8)
    c, cc = ops.split_buildings(m, 4, sweeps_per_call=1)
    assert cc == calls1 and torch.equal(a, c)


# ---- contract ------------------------------------------------------------------------------------------------------------
def _two_squares():
    """loc fp32 and a damage label map: a 12 x 12 square of class 2 and a 16 x 16 one of class 3, joined by a neck 2 wide"""
    pre = np.zeros((30, 50), dtype=np.uint8)
    dmg = np.zeros((30, 50), dtype=np.int32)
    pre[8:20, 4:16] = 1
    dmg[8:20, 4:16] = 2
    pre[6:22, 24:40] = 1
    dmg[6:22, 24:40] = 3
    pre[13:15, 16:24] = 1
    dmg[13:15, 16:20] = 2
    dmg[13:15, 20:24] = 3
    return pre, dmg


def test_split_zero_changes_nothing():
    from xview2_amd import ops
    from xview2_amd.utils.post_process import post_process_tiles
    loc = _dev(R.loc_for(5, (3, 70, 90)))
    loc = torch.nan_to_num(loc, nan=0.0, posinf=1.0, neginf=0.0)
    dmg = torch.rand((3, 4, 70, 90), device=DEV)
    for comp, dilate in ((False, False), (True, False), (True, True)):
        want = ops.postprocess(loc, dmg, components=comp, rate=3 if dilate else 0)
        got = post_process_tiles(loc, dmg, comp, dilate, 3, split=0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        got = post_process_tiles(loc, dmg, comp, dilate, 3)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_components_vote_per_split_piece():
    from xview2_amd.utils.post_process import post_process_tiles
    pre, dmg = _two_squares()
    loc = _dev(pre.astype(np.float32))
    one_pre, one_post = post_process_tiles(loc, _dev(dmg), components=True)
    assert np.array_equal(one_pre.cpu().numpy(), pre)
    assert np.array_equal(one_post.cpu().numpy(), 3 * pre)                   # one building, one class: the larger square's
    two_pre, two_post = post_process_tiles(loc, _dev(dmg), components=True, split=1)
    want_pre = S.split(pre, 1)[0]
    assert np.array_equal(two_pre.cpu().numpy(), want_pre) and int((want_pre != pre).sum()) == 2
    want_post = dmg.astype(np.uint8) * want_pre
    assert np.array_equal(two_post.cpu().numpy(), want_post)                 # two buildings with their own classes
    assert set(np.unique(want_post).tolist()) == {0, 2, 3}
    raw_pre, raw_post = post_process_tiles(loc, _dev(dmg), components=False, split=1)
    assert np.array_equal(raw_pre.cpu().numpy(), want_pre) and np.array_equal(raw_post.cpu().numpy(), want_post)
    # batched input, and a dilation that comes before the split
    b_pre, b_post = post_process_tiles(torch.stack([loc, loc]), torch.stack([_dev(dmg)] * 2), True, True, 3, split=2)
    dil = R.ndimage.maximum_filter(pre, size=3, mode="constant")
    assert np.array_equal(b_pre[1].cpu().numpy(), S.split(dil, 4)[0]) and torch.equal(b_pre[0], b_pre[1])
    assert torch.equal(b_post[0], b_post[1])


def test_building_table_of_the_split_maps():
    from xview2_amd.utils import buildings
    from xview2_amd.utils.split import split_maps
    masks = _batch("blobs")
    dmgs = np.stack([R.dmg_for(40 + b, masks[b].shape) for b in range(len(masks))])
    pre2, post2 = split_maps(_dev(masks), _dev(dmgs), 2)
    want_pre = _want("blobs", 4)[0]
    assert np.array_equal(pre2.cpu().numpy(), want_pre) and np.array_equal(post2.cpu().numpy(), dmgs * (want_pre != 0))
    tables = buildings.building_table(pre2, post2)
    for b, rows in enumerate(tables):
        want = R.table(want_pre[b], dmgs[b] * (want_pre[b] != 0))
        assert len(want) > len(R.table(masks[b], dmgs[b])) and np.array_equal(rows, want)
    single = split_maps(_dev(masks[0]), _dev(dmgs[0]), 2)
    assert torch.equal(single[0], pre2[0]) and torch.equal(single[1], post2[0])


def test_bad_arguments_are_refused():
    from xview2_amd import _capi, ops
    m = _dev(np.ones((1, 8, 8), dtype=np.uint8))
    ws = torch.empty(int(_capi.query("xv2_split_workspace", 1, 8, 8)), dtype=torch.uint8, device=DEV)
    d2 = torch.empty((1, 8, 8), dtype=torch.int16, device=DEV)
    pending = torch.zeros(1, dtype=torch.int32, device=DEV)
    for r2 in (0, 4096):
        with pytest.raises(RuntimeError, match="r2"):
            _capi.call("xv2_split_seed", m, 1, 8, 8, r2, ws)
        with pytest.raises(ValueError, match="r2"):
            ops.split_buildings(m, r2)
    for cap in (0, 65):
        with pytest.raises(RuntimeError, match="cap"):
            _capi.call("xv2_edt_sq", m, 1, 8, 8, cap, d2)
    with pytest.raises(RuntimeError, match="sweeps"):
        _capi.call("xv2_split_grow", m, 1, 8, 8, 0, ws, pending)
    with pytest.raises(ValueError, match="sweeps"):
        ops.split_buildings(m, 4, sweeps_per_call=0)
    q = lambda *a: int(_capi.query("xv2_split_workspace", *a))
    assert q(1, 8, 8) > 0 and q(1, 1 << 15, 1 << 15) == 0 and q(65536, 8, 8) == 0 and q(0, 8, 8) == 0
    out, calls = ops.split_buildings(m, 4095)            # the largest radius, on a tile smaller than its window
    assert torch.equal(out, m) and calls == 1


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_split_command_line(tmp_path):
    from PIL import Image
    from xview2_amd.utils import split
    pre = S.blob_mask(17, 75, 110)
    post = (R.dmg_for(18, pre.shape) % 5).astype(np.uint8) * pre
    names = [str(tmp_path / n) for n in ("pre.png", "post.png", "out_pre.png", "out_post.png")]
    Image.fromarray(pre).save(names[0])
    Image.fromarray(post).save(names[1])
    want = S.split(pre, 9)[0]
    assert split.main(names + ["--radius", "3"]) == int((want != pre).sum()) > 0
    assert np.array_equal(np.asarray(Image.open(names[2])), want)
    assert np.array_equal(np.asarray(Image.open(names[3])), post * (want != 0))


def test_split_targets_turns_one_miss_into_two_hits(tmp_path):
    from PIL import Image
    from xview2_amd.utils import building_metrics as BM
    pred, targ = tmp_path / "pred", tmp_path / "targ"
    pred.mkdir()
    targ.mkdir()
    bell, col, _ = S.dumbbell(2, 6)                  # two labelled buildings that touch through a neck two pixels wide
    target = np.zeros((1024, 1024), dtype=np.uint8)  # (the scorer's tile size)
    target[500:500 + bell.shape[0], 620:620 + bell.shape[1]] = bell
    found = target.copy()
    found[:, 620 + col:620 + col + 6] = 0            # the prediction: the two bodies, apart
    for d, name, a in ((pred, "test_localization_00000_prediction.png", found), (pred, "test_damage_00000_prediction.png", found),
                       (targ, "test_localization_00000_target.png", target), (targ, "test_damage_00000_target.png", target)):
        Image.fromarray(a).save(str(d / name))
    plain = BM.compute_score(str(pred), str(targ), str(tmp_path / "a.json"))
    assert (plain["totals"]["TP"], plain["totals"]["FP"], plain["totals"]["FN"]) == (0, 2, 1)
    cut = BM.compute_score(str(pred), str(targ), str(tmp_path / "b.json"), split_targets=1)
    assert (cut["totals"]["TP"], cut["totals"]["FP"], cut["totals"]["FN"]) == (2, 0, 0)
    both = BM.compute_score(str(pred), str(targ), str(tmp_path / "c.json"), split=1, split_targets=1)
    assert both["totals"] == cut["totals"]           # the prediction has nothing to cut


def test_post_process_command_line_writes_everything_from_the_split_maps(tmp_path):
    import os
    import postproc_ref as P
    from PIL import Image
    from xview2_amd.utils import buildings, post_process
    os.makedirs(str(tmp_path / "probs"))
    pairs = []
    for k, seed in enumerate((61, 67)):
        cls = np.where(S.blob_mask(seed, 70, 90) != 0, 1 + R._hash(seed + 1, (70, 90), 4), 0)
        pairs.append((P.loc_from_mask(seed + 2, cls > 0), P.probs_from_classes(seed + 3, cls, 4)))
        np.save(str(tmp_path / "probs" / ("test_localization_%05d.npy" % k)), pairs[-1][0])
        np.save(str(tmp_path / "probs" / ("test_damage_%05d.npy" % k)), pairs[-1][1])
    plain = post_process.get_parser().parse_args(["--results", str(tmp_path)])
    assert post_process.run(plain) == 2
    name = lambda kind, k: str(tmp_path / "predictions" / ("test_%s_%05d_prediction.png" % (kind, k)))
    before = [(np.asarray(Image.open(name("localization", k))), np.asarray(Image.open(name("damage", k)))) for k in range(2)]
    args = post_process.get_parser().parse_args(["--results", str(tmp_path), "--split", "2", "--components", "--buildings"])
    assert post_process.run(args) == 2
    for k, (loc, _) in enumerate(pairs):
        pre, post = np.asarray(Image.open(name("localization", k))), np.asarray(Image.open(name("damage", k)))
        want_pre = S.split(before[k][0], 4)[0]
        assert np.array_equal(pre, want_pre) and int((want_pre != before[k][0]).sum()) > 0
        assert np.array_equal(post != 0, pre != 0)
        rows = R.table(pre, post, loc)
        assert all(len(np.unique(post[m])) == 1 for m in (R.label_min_index(pre) == r + 1 for r in rows[:, 0]))   # one class a piece
        assert buildings.read_csv(str(tmp_path / "buildings" / ("test_buildings_%05d.csv" % k))) == buildings.to_records(rows, 70, 90)
        csv = str(tmp_path / ("again_%d.csv" % k))                      # the table of the written PNGs is the same table
        assert buildings.main([name("localization", k), name("damage", k), csv]) == len(rows)
        drop = lambda recs: [{f: v for f, v in r.items() if f != "confidence"} for r in recs]
        assert buildings.read_csv(csv) == drop(buildings.to_records(rows, 70, 90))
