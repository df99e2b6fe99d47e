"""Filling holes and dropping small buildings on the MI355X (csrc/clean.hip through xv2_clean_buildings, ops.clean_buildings
and utils/clean.py) against the host restatement of tests/clean_ref.py.  Every value is an integer, so every comparison is
np.array_equal / torch.equal.  Each direct call runs between canary stretches around pre_out, post_out, stats and the
workspace, the workspace pre-filled with 0xA5, and its inputs are compared with their copies afterwards."""
import functools

import numpy as np
import pytest
import torch

import clean_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of pre_out, post_out (uint8) and stats (int64)
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = 0x5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, fill=FILL):
    buf = torch.full((2 * CAN + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, what, fill=FILL, can=CAN):
    assert bool((buf[:can] == fill).all()) and bool((buf[-can:] == fill).all()), what + ": canary overwritten"


def _call(pre, post, A, M):
    """one xv2_clean_buildings on caller-owned buffers; pre, post uint8 [B,H,W] (numpy; post may be None) -> numpy
    (pre_out, post_out or None, stats [B,4])"""
    from xview2_amd import _capi
    p = _dev(pre)
    q = _dev(post) if post is not None else None
    keep_p, keep_q = p.clone(), (q.clone() if q is not None else None)
    B, H, W = p.shape
    need = int(_capi.query("xv2_clean_workspace", B, H, W))
    assert need >= 20 * B * H * W
    ws_buf = torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws_buf[CAN_WS:CAN_WS + need]
    po_buf, po = _guarded(B * H * W, torch.uint8)
    qo_buf, qo = _guarded(B * H * W, torch.uint8)
    st_buf, st = _guarded(B * 4, torch.int64)
    torch.cuda.synchronize()
    _capi.call("xv2_clean_buildings", p, q, B, H, W, int(A), int(M), ws, po, qo if q is not None else None, st)
    torch.cuda.synchronize()
    _intact(po_buf, "pre_out")
    _intact(qo_buf, "post_out")
    _intact(st_buf, "stats")
    _intact(ws_buf, "workspace", 0xA5, CAN_WS)
    assert torch.equal(p, keep_p) and (q is None or torch.equal(q, keep_q)), "an input was written"
    if q is None:
        assert bool((qo == FILL).all()), "post_out written without a post"
    return (po.cpu().numpy().reshape(B, H, W), qo.cpu().numpy().reshape(B, H, W) if q is not None else None,
            st.cpu().numpy().reshape(B, 4))


def _check(pre, post, A, M):
    """the kernels against the restatement, tile by tile, with and without post; returns the stats [B,4]"""
    pre = np.ascontiguousarray(pre, dtype=np.uint8)
    if pre.ndim == 2:
        pre, post = pre[None], post[None]
    out, pout, stats = _call(pre, post, A, M)
    for b in range(pre.shape[0]):
        want, wpost, wstats = C.clean(pre[b], post[b], A, M)
        assert np.array_equal(out[b], want), "tile %d (A=%d M=%d): pre differs in %d pixels" % (b, A, M, int((out[b] != want).sum()))
        assert np.array_equal(pout[b], wpost), "tile %d (A=%d M=%d): post differs in %d pixels" % (b, A, M, int((pout[b] != wpost).sum()))
        assert stats[b].tolist() == wstats.tolist(), "tile %d (A=%d M=%d): stats" % (b, A, M)
    out2, none, stats2 = _call(pre, None, A, M)
    assert none is None and np.array_equal(out2, out) and np.array_equal(stats2, stats)
    return stats


def _posts(pre, seed=0):
    """a post map with every value 0..6 for the pre map(s)"""
    return np.random.RandomState(1000 + seed).randint(0, 7, size=pre.shape).astype(np.uint8)


# ---- random masks at degenerate and region-edge sizes --------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (3, 3), (63, 63), (64, 64), (65, 65), (130, 67)])
def test_random_masks(H, W):
    pairs = [C.random_pair(7 * H + W + k, H, W, d) for k, d in enumerate((0.1, 0.5, 0.9))]
    pre, post = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for A, M in ((1, 0), (0, 1), (2, 0), (0, 3), (3, 2), (6, 40), (H * W, H * W), (H * W + 1, 1 << 40)):
        _check(pre, post, A, M)


def test_zero_and_zero_copies():
    pre, post = C.random_pair(5, 70, 90, 0.5)
    out, pout, stats = _call(pre[None], post[None], 0, 0)
    assert np.array_equal(out[0], pre) and np.array_equal(pout[0], post) and not stats.any()


# ---- diagonal joins across region borders --------------------------------------------------------------------------------
def _diagonals():
    """a solid tile with six holes of two pixels that meet only diagonally: across the corner shared by four regions both
    ways, across a vertical and a horizontal region edge both ways"""
    m = np.ones((130, 130), dtype=np.uint8)
    for a, b in (((63, 63), (64, 64)), ((20, 63), (21, 64)), ((25, 64), (26, 63)), ((63, 20), (64, 21)), ((64, 25), (63, 26)),
                 ((127, 64), (128, 63))):
        m[a] = m[b] = 0
    n = np.ones((130, 130), dtype=np.uint8)
    n[63, 64] = n[64, 63] = 0
    return np.stack([m, n])


def test_holes_that_meet_diagonally_across_region_corners_and_edges():
    pre = _diagonals()
    post = _posts(pre)
    assert _check(pre, post, 0, 1)[:, :2].tolist() == [[0, 0], [0, 0]]          # areas of two: the halves are one hole each
    assert _check(pre, post, 0, 2)[:, :2].tolist() == [[6, 12], [1, 2]]


def test_a_diagonal_step_to_the_frame_is_a_way_out():
    m = np.ones((70, 70), dtype=np.uint8)
    m[1, 1] = m[0, 2] = 0            # reaches the frame through a diagonal step: no hole
    m[68, 68] = m[69, 69] = 0
    m[64, 1] = m[63, 0] = 0          # the same across a region edge
    m[1, 64] = m[0, 63] = 0
    m[1, 10] = 0                     # one pixel inside the frame: holes
    m[30, 68] = m[68, 30] = m[40, 1] = 0
    stats = _check(m, _posts(m), 0, 9)
    assert stats[0, :2].tolist() == [4, 4]
    _check(m, _posts(m), 3, 1)


# ---- islands, nesting and thresholds -------------------------------------------------------------------------------------
def _nested(H=80, W=80, y=58, x=58):
    """a 9 x 9 building (32 pixels) around a ring hole of 40 pixels around an island of 8 pixels with its own hole of one
    pixel, laid across the region borders at 64; and a speck"""
    pre = np.zeros((H, W), dtype=np.uint8)
    pre[y:y + 9, x:x + 9] = 1
    pre[y + 1:y + 8, x + 1:x + 8] = 0
    pre[y + 3:y + 6, x + 3:x + 6] = 2
    pre[y + 4, x + 4] = 0
    pre[5, 5] = 9
    post = np.where(pre == 1, 3, np.where(pre == 2, 4, 0)).astype(np.uint8)
    post[0, 0] = 2                   # a class on background stays where it is
    return pre, post


@pytest.mark.parametrize("A,M,stats", [(0, 1, [1, 1, 0, 0]), (0, 39, [1, 1, 0, 0]), (0, 40, [2, 41, 0, 0]), (2, 0, [0, 0, 1, 1]),
                                       (10, 1, [1, 1, 2, 10]), (9, 1, [1, 1, 1, 1]), (10, 40, [2, 41, 1, 1]),
                                       (81, 40, [2, 41, 1, 1]), (82, 40, [2, 41, 2, 82]), (33, 0, [0, 0, 3, 41])])
def test_island_and_nested_holes(A, M, stats):
    pre, post = _nested()
    assert _check(pre, post, A, M)[0].tolist() == stats


def test_only_the_outer_hole():
    """M between the two areas the other way round: an inner hole larger than the ring around its island"""
    pre = np.zeros((40, 90), dtype=np.uint8)
    pre[2:38, 40:88] = 1
    pre[4:36, 42:86] = 0             # outer hole ...
    pre[5:35, 43:85] = 1             # ... a ring one pixel wide: 32 * 44 - 30 * 42 = 148
    pre[8:32, 46:82] = 0             # the island's own hole: 24 * 36 = 864
    post = _posts(pre, 3)
    assert _check(pre, post, 0, 148)[0].tolist() == [1, 148, 0, 0]
    assert _check(pre, post, 0, 147)[0].tolist() == [0, 0, 0, 0]
    assert _check(pre, post, 0, 864)[0].tolist() == [2, 1012, 0, 0]


def test_thresholds_hold_at_equality():
    pre = np.zeros((12, 20), dtype=np.uint8)
    pre[1:7, 1:8] = 1
    pre[2:4, 2:4] = 0                # a hole of 4
    pre[2:4, 5:7] = 0
    pre[4, 5] = 0                    # a hole of 5
    pre[9, 1:4] = 1                  # a building of 3
    pre[9, 6:10] = 1                 # a building of 4
    post = _posts(pre, 1)
    assert _check(pre, post, 4, 4)[0].tolist() == [1, 4, 1, 3]
    assert _check(pre, post, 3, 5)[0].tolist() == [2, 9, 0, 0]
    assert _check(pre, post, 5, 3)[0].tolist() == [0, 0, 2, 7]


def test_owner_vote():
    pre = np.zeros((3, 9, 9), dtype=np.uint8)
    pre[:, 2:7, 2:7] = 1
    pre[:, 4, 4] = 0
    post = np.zeros_like(pre)
    post[0, 2, 2:7] = 4              # a tie between 4 and 2 (five each) over three pixels of 3: the smaller class
    post[0, 6, 2:7] = 2
    post[0, 3, 2:5] = 3
    post[0, 4, 4] = 1                # the hole's own value does not vote
    post[1][pre[1] != 0] = 0         # an owner without a class: 0 and values above 4
    post[1, 2, 2:5] = 5
    post[1, 3, 2] = 255
    post[1, 0, 0] = 3
    post[2][pre[2] != 0] = 6
    post[2, 5, 5] = 3                # one pixel in 1..4 decides
    out, pout, stats = _call(pre, post, 0, 1)
    assert pout[:, 4, 4].tolist() == [2, 0, 3] and out[:, 4, 4].tolist() == [1, 1, 1]
    _check(pre, post, 0, 1)


# ---- long parent chains, extremes ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spiral(n=130):
    """a path one pixel wide that winds inwards with walls one pixel wide, two pixels inside the frame"""
    m = np.zeros((n, n), dtype=np.uint8)
    inside = lambda y, x: 2 <= y <= n - 3 and 2 <= x <= n - 3
    y, x, dy, dx, turns = 2, 2, 0, 1, 0
    m[y, x] = 1
    while turns < 2:
        v, u, v2, u2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(v, u) and not m[v, u] and not (inside(v2, u2) and m[v2, u2]):
            y, x, turns = v, u, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def test_spiral_hole_and_spiral_building():
    m = _spiral()
    n = int(m.sum())
    assert n > 4000 and len(C.components(m != 0, C.N4)[1]) == 1
    hole = (1 - m).astype(np.uint8)
    assert [len(h) for h in C.holes(hole)] == [n]
    pre = np.stack([hole, m])
    post = _posts(pre, 2)
    assert _check(pre, post, 0, n)[:, :2].tolist() == [[1, n], [0, 0]]
    assert _check(pre, post, 0, n - 1)[:, :2].tolist() == [[0, 0], [0, 0]]
    assert _check(pre, post, n + 1, 0)[1].tolist() == [0, 0, 1, n]
    assert _check(pre, post, n, n)[1, 2:].tolist() == [0, 0]


def test_checkerboard_and_uniform_tiles():
    board = (np.indices((66, 66)).sum(0) % 2).astype(np.uint8)
    pre = np.stack([board, 1 - board, np.zeros((66, 66), np.uint8), np.ones((66, 66), np.uint8)])
    post = _posts(pre, 4)
    stats = _check(pre, post, 2, 5)
    assert stats.tolist() == [[0, 0, 2178, 2178], [0, 0, 2178, 2178], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert _check(pre, post, 66 * 66 + 1, 66 * 66)[3].tolist() == [0, 0, 1, 66 * 66]
    assert _check(pre, post, 66 * 66, 0)[3].tolist() == [0, 0, 0, 0]


# ---- batches and repeatability -------------------------------------------------------------------------------------------
def test_batch_equals_tiles_alone_and_runs_repeat():
    tiles = [C.random_pair(40 + k, 70, 90, d) for k, d in enumerate((0.3, 0.6, 0.8))]
    pre, post = np.stack([t[0] for t in tiles]), np.stack([t[1] for t in tiles])
    out, pout, stats = _call(pre, post, 4, 6)
    assert len({tuple(s) for s in stats.tolist()}) == 3
    for b in range(3):
        o, p, s = _call(pre[b:b + 1], post[b:b + 1], 4, 6)
        assert np.array_equal(o[0], out[b]) and np.array_equal(p[0], pout[b]) and np.array_equal(s[0], stats[b])
    again = _call(pre, post, 4, 6)
    assert all(np.array_equal(a, b) for a, b in zip(again, (out, pout, stats)))
    _check(pre, post, 4, 6)


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    from xview2_amd import _capi, ops
    from xview2_amd.utils import clean
    m = _dev(np.ones((1, 8, 8), dtype=np.uint8))
    ws = torch.empty(int(_capi.query("xv2_clean_workspace", 1, 8, 8)), dtype=torch.uint8, device=DEV)
    o1, o2 = torch.full_like(m, FILL), torch.full_like(m, FILL)
    st = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    for A, M in ((-1, 0), (0, -1)):
        with pytest.raises(RuntimeError, match="negative"):
            _capi.call("xv2_clean_buildings", m, m.clone(), 1, 8, 8, A, M, ws, o1, o2, st)
        with pytest.raises(ValueError, match="negative"):
            ops.clean_buildings(m, None, A, M)
        with pytest.raises(ValueError, match="integer >= 0"):
            clean.clean_maps(m, m.clone(), A, M)
    with pytest.raises(RuntimeError, match="both"):
        _capi.call("xv2_clean_buildings", m, m.clone(), 1, 8, 8, 1, 1, ws, o1, None, st)
    with pytest.raises(RuntimeError, match="both"):
        _capi.call("xv2_clean_buildings", m, None, 1, 8, 8, 1, 1, ws, o1, o2, st)
    with pytest.raises(RuntimeError, match="alias"):
        _capi.call("xv2_clean_buildings", m, None, 1, 8, 8, 1, 1, ws, m, None, st)
    torch.cuda.synchronize()
    assert bool((o1 == FILL).all()) and bool((o2 == FILL).all()) and bool((st == -7).all())      # nothing was launched
    q = lambda *a: int(_capi.query("xv2_clean_workspace", *a))
    assert q(1, 8, 8) > 0 and q(1, 1 << 15, 1 << 15) == 0 and q(65536, 8, 8) == 0 and q(0, 8, 8) == 0
    with pytest.raises(ValueError, match="shape"):
        ops.clean_buildings(m, torch.zeros((1, 8, 9), dtype=torch.uint8, device=DEV), 1, 1)
    with pytest.raises(ValueError, match="workspace"):
        ops.clean_buildings(m, None, 1, 1, workspace=ws[:64])
    pre2, none, stats = ops.clean_buildings(m, None, 1 << 70, 1 << 70, workspace=ws)      # anything large means "all"
    assert none is None and not bool(pre2.any()) and stats.tolist() == [[0, 0, 1, 64]]


# ---- composition ---------------------------------------------------------------------------------------------------------
def test_polygons_of_the_filled_map_have_no_hole_ring():
    from xview2_amd.utils import polygons
    from xview2_amd.utils.clean import clean_maps
    pre, post = C.random_pair(71, 90, 110, 0.7)
    before = polygons.building_polygons(_dev(pre))
    assert sum(len(p["holes"]) for p in before) == len(C.holes(pre)) > 10
    pre2, _ = clean_maps(_dev(pre), _dev(post), 0, 90 * 110)
    after = polygons.building_polygons(pre2)
    assert after and all(p["holes"] == [] for p in after)


def test_building_table_of_the_cleaned_map_has_no_small_row():
    from xview2_amd.utils import buildings
    from xview2_amd.utils.clean import clean_maps
    pre, post = C.random_pair(72, 90, 110, 0.5)
    rows = buildings.building_table(_dev(pre), _dev(post))
    assert int((rows[:, 1] < 5).sum()) > 10
    pre2, post2, stats = clean_maps(_dev(pre), _dev(post), 5, 0, return_stats=True)
    rows2 = buildings.building_table(pre2, post2)
    assert len(rows2) > 0 and int(rows2[:, 1].min()) >= 5 and len(rows2) == len(rows) - int(stats[2])
    want = C.clean(pre, post, 5, 0)
    assert np.array_equal(pre2.cpu().numpy(), want[0]) and np.array_equal(post2.cpu().numpy(), want[1])
    assert stats.cpu().tolist() == want[2].tolist()


def test_post_process_tiles_is_the_stages_assembled_by_hand():
    from xview2_amd import ops
    from xview2_amd.utils.clean import clean_maps
    from xview2_amd.utils.post_process import post_process_tiles
    from xview2_amd.utils.split import split_maps
    g = torch.Generator(device="cpu").manual_seed(9)
    loc = torch.nn.functional.avg_pool2d(torch.rand((2, 1, 76, 96), generator=g), 7, 1)[:, 0]
    loc = ((loc - loc.mean()) * 10).clamp(0, 1).contiguous().to(DEV)       # blobs with specks and pinholes
    dmg = torch.rand((2, 4, 70, 90), generator=g).to(DEV)
    base = ops.postprocess(loc, dmg, components=False, rate=3)
    cleaned = clean_maps(base[0], base[1], 16, 4, return_stats=True)
    assert int(cleaned[2][:, 0].sum()) > 0 and int(cleaned[2][:, 2].sum()) > 0
    cut = split_maps(cleaned[0], cleaned[1], 2)
    want = ops.postprocess(cut[0].float(), cut[1].to(torch.int32), components=True, rate=0)
    got = post_process_tiles(loc, dmg, True, True, 3, None, 2, 16, 4, return_stats=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], cleaned[2])
    # without the split and the vote: the cleaned maps themselves; unbatched input gives unbatched output
    got = post_process_tiles(loc, dmg, False, True, 3, min_area=16, fill_holes=4)
    assert len(got) == 2 and torch.equal(got[0], cleaned[0]) and torch.equal(got[1], cleaned[1])
    one = post_process_tiles(loc[1], dmg[1], False, True, 3, min_area=16, fill_holes=4, return_stats=True)
    assert torch.equal(one[0], cleaned[0][1]) and torch.equal(one[1], cleaned[1][1]) and torch.equal(one[2], cleaned[2][1])
    # and with zeros the call that was made before
    plain = post_process_tiles(loc, dmg, True, True, 3, min_area=0, fill_holes=0)
    want = ops.postprocess(loc, dmg, components=True, rate=3)
    assert torch.equal(plain[0], want[0]) and torch.equal(plain[1], want[1])


def test_clean_command_line(tmp_path):
    from PIL import Image
    from xview2_amd.utils import clean
    pre, post = C.random_pair(73, 75, 110, 0.6)
    names = [str(tmp_path / n) for n in ("pre.png", "post.png", "out_pre.png", "out_post.png")]
    Image.fromarray(pre).save(names[0])
    Image.fromarray(post).save(names[1])
    want = C.clean(pre, post, 4, 3)
    got = clean.main(names + ["--min_area", "4", "--fill_holes", "3"])
    assert [got[k] for k in clean.STAT_KEYS] == want[2].tolist() and min(want[2]) > 0
    assert np.array_equal(np.asarray(Image.open(names[2])), want[0])
    assert np.array_equal(np.asarray(Image.open(names[3])), want[1])


def test_min_area_removes_speck_false_positives_from_the_object_score(tmp_path):
    from PIL import Image
    from xview2_amd.utils import building_metrics as BM
    dirs = {k: tmp_path / k for k in ("pred", "targ", "pred_clean")}
    for d in dirs.values():
        d.mkdir()
    target = np.zeros((1024, 1024), dtype=np.uint8)  # (the scorer's tile size)
    target[100:140, 200:260] = 1
    target[500:530, 620:650] = 2
    target[900, 900] = 3                             # a labelled speck: --min_area_targets drops it
    found = np.where(target > 0, target, 0).astype(np.uint8)
    found[900, 900] = 0
    for y, x in ((10, 10), (300, 700), (640, 64), (1023, 1023)):
        found[y, x] = 1                              # four single-pixel specks
    found[110, 210] = 0                              # and a pinhole
    cleaned = C.clean(found, found, 2, 0)[0]
    assert int((cleaned != found).sum()) == 4
    for d, kind, a in ((dirs["pred"], "prediction", found), (dirs["pred_clean"], "prediction", cleaned), (dirs["targ"], "target", target)):
        Image.fromarray(a).save(str(d / ("test_localization_00000_%s.png" % kind)))
        Image.fromarray(a).save(str(d / ("test_damage_00000_%s.png" % kind)))
    score = lambda p, name, **kw: BM.compute_score(str(dirs[p]), str(dirs["targ"]), str(tmp_path / name), **kw)
    plain = score("pred", "a.json")
    assert (plain["totals"]["TP"], plain["totals"]["FP"], plain["totals"]["FN"]) == (2, 4, 1)
    filtered = score("pred", "b.json", min_area=2)
    assert (filtered["totals"]["TP"], filtered["totals"]["FP"], filtered["totals"]["FN"]) == (2, 0, 1)
    assert filtered == score("pred_clean", "c.json")
    both = score("pred", "d.json", min_area=2, fill_holes=1, min_area_targets=2)
    assert (both["totals"]["TP"], both["totals"]["FP"], both["totals"]["FN"]) == (2, 0, 0)


def test_post_process_command_line_writes_everything_from_the_cleaned_maps(tmp_path):
    import os
    import buildings_ref as R
    import postproc_ref as P
    from PIL import Image
    from xview2_amd.utils import buildings, post_process
    os.makedirs(str(tmp_path / "probs"))
    pairs = []
    for k, seed in enumerate((61, 67)):
        cls = np.where(C.random_pair(seed, 70, 90, 0.55)[0] != 0, 1 + R._hash(seed + 1, (70, 90), 4), 0)
        pairs.append((P.loc_from_mask(seed + 2, cls > 0), P.probs_from_classes(seed + 3, cls, 4)))
        np.save(str(tmp_path / "probs" / ("test_localization_%05d.npy" % k)), pairs[-1][0])
        np.save(str(tmp_path / "probs" / ("test_damage_%05d.npy" % k)), pairs[-1][1])
    assert post_process.run(post_process.get_parser().parse_args(["--results", str(tmp_path)])) == 2
    name = lambda kind, k: str(tmp_path / "predictions" / ("test_%s_%05d_prediction.png" % (kind, k)))
    before = [(np.asarray(Image.open(name("localization", k))), np.asarray(Image.open(name("damage", k)))) for k in range(2)]
    args = post_process.get_parser().parse_args(["--results", str(tmp_path), "--min_area", "5", "--fill_holes", "3", "--buildings"])
    assert post_process.run(args) == 2
    for k, (loc, _) in enumerate(pairs):
        pre, post = np.asarray(Image.open(name("localization", k))), np.asarray(Image.open(name("damage", k)))
        want = C.clean(before[k][0], before[k][1], 5, 3)
        assert min(want[2]) > 0 and np.array_equal(pre, want[0]) and np.array_equal(post, want[1])
        rows = R.table(pre, post, loc)
        assert len(rows) > 0 and int(rows[:, 1].min()) >= 5
        assert buildings.read_csv(str(tmp_path / "buildings" / ("test_buildings_%05d.csv" % k))) == buildings.to_records(rows, 70, 90)
    with pytest.raises(ValueError, match="integer >= 0"):
        post_process.run(post_process.get_parser().parse_args(["--results", str(tmp_path), "--min_area", "-3"]))
