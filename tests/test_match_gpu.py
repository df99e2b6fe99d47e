"""The building match on the MI355X (csrc/match.hip through xv2_building_match, ops.building_match and
utils/building_metrics.py) against the host restatement of tests/match_ref.py.  Every value is an integer, so every
comparison is np.array_equal.  Each direct call runs between canary stretches around match_p, match_t, piece_count and the
workspace, and its inputs are compared with their copies afterwards."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import buildings_ref as R
import match_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of the match rows (int64) and piece_count (int32)
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = -7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(masks, dmgs, max_rows):
    """device (labels [B,H,W], rows [B,max_rows,16], count [B]) of B tiles, through the two existing entry points"""
    from xview2_amd import ops
    labels = ops.label_components(_dev(np.stack(masks)))
    rows, count = ops.building_table(labels, _dev(np.stack(dmgs)), None, max_rows)
    return labels, rows, count


def _call(p, t, iou, max_pieces, stream=None):
    """xv2_building_match on caller-owned buffers; p, t: (labels, rows, count) on the device.  Returns numpy (match_p
    [B,max_rows_p,8], match_t, piece_count [B]); asserts the canaries and that no input was written."""
    from xview2_amd import _capi
    B, H, W = p[0].shape
    rp, rt = int(p[1].shape[1]), int(t[1].shape[1])
    need = int(_capi.query("xv2_building_match_workspace", B, H, W, max_pieces))
    assert need > 0
    bufs = [torch.full((2 * CAN + B * rp * 8,), FILL, dtype=torch.int64, device=DEV),
            torch.full((2 * CAN + B * rt * 8,), FILL, dtype=torch.int64, device=DEV),
            torch.full((2 * CAN + B,), FILL, dtype=torch.int32, device=DEV),
            torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)]
    mp = bufs[0][CAN:CAN + B * rp * 8].view(B, rp, 8)
    mt = bufs[1][CAN:CAN + B * rt * 8].view(B, rt, 8)
    pc = bufs[2][CAN:CAN + B]
    ws = bufs[3][CAN_WS:CAN_WS + need]
    ins = list(p) + list(t)
    keep = [x.clone() for x in ins]
    args = (p[0], p[1], p[2], rp, t[0], t[1], t[2], rt, B, H, W, iou[0], iou[1], max_pieces, ws, mp, mt, pc)
    torch.cuda.synchronize()
    if stream is None:
        _capi.call("xv2_building_match", *args)
        torch.cuda.synchronize()
        got = mp.cpu().numpy(), mt.cpu().numpy(), pc.cpu().numpy()
    else:
        with torch.cuda.stream(stream):      # the copies are ordered by the stream alone: no device-wide wait
            _capi.call("xv2_building_match", *args)
            got = mp.cpu().numpy(), mt.cpu().numpy(), pc.cpu().numpy()
        torch.cuda.synchronize()
    for buf, can, what in zip(bufs, (CAN, CAN, CAN, CAN_WS), ("match_p", "match_t", "piece_count", "workspace")):
        want = 0xA5 if what == "workspace" else FILL
        assert bool((buf[:can] == want).all()) and bool((buf[-can:] == want).all()), what + ": canary overwritten"
    assert all(torch.equal(a, b) for a, b in zip(ins, keep)), "an input was written"
    return got


def _first_diff(got, want, what, b):
    r, c = np.nonzero(got != want)
    return "%s of tile %d: %d cells differ, first row %d col %d: %d != %d\n%s\n%s" % (
        what, b, len(r), r[0], c[0], got[r[0], c[0]], want[r[0], c[0]], got[r[0]], want[r[0]])


def _check(masks_p, dmgs_p, masks_t, dmgs_t, iou=(1, 2), max_pieces=None, spare=3, stream=None, want=None):
    """B tiles of one shape against the restatement (or `want`, a list of its dicts) -> what _call returned"""
    if want is None:
        want = [M.match(*maps, iou) for maps in zip(masks_p, dmgs_p, masks_t, dmgs_t)]
    rows_p = max(1, max(len(w["match_p"]) for w in want)) + spare
    rows_t = max(1, max(len(w["match_t"]) for w in want)) + 2 * spare
    if max_pieces is None:
        max_pieces = max(1, max(w["piece_count"] for w in want))
    p, t = _tables(masks_p, dmgs_p, rows_p), _tables(masks_t, dmgs_t, rows_t)
    mp, mt, pc = _call(p, t, iou, max_pieces, stream)
    assert pc.tolist() == [w["piece_count"] for w in want]
    for b, w in enumerate(want):
        for got, key in ((mp, "match_p"), (mt, "match_t")):
            n = len(w[key])
            assert np.all(got[b, n:] == FILL), "tile %d: %s storage behind row %d was written" % (b, key, n)
            if w["piece_count"] <= max_pieces:
                assert np.array_equal(got[b, :n], w[key]), _first_diff(got[b, :n], w[key], key, b)
    return mp, mt, pc


def _ones(mask):
    return np.ones(mask.shape, dtype=np.uint8)


# ---- planted shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.planted()))
def test_planted_cases(name):
    mask_p, mask_t, want = M.planted()[name]
    mp, mt, pc = _check([mask_p], [_ones(mask_p)], [mask_t], [_ones(mask_t)])
    assert pc.tolist() == [want["piece_count"]]
    assert np.array_equal(mp[0, :len(want["match_p"])], want["match_p"]), mp[0]
    assert np.array_equal(mt[0, :len(want["match_t"])], want["match_t"]), mt[0]
    if name == "u_over_bar":
        assert mp[0, 0, 1] == 6 and pc[0] == 2             # one pair, two pieces: the intersection is their sum
    if name == "crossing_bars":
        assert mp[0, :2, 0].tolist() == [0, 0] and mt[0, :2, 0].tolist() == [0, 0]      # the equal-IoU tie: the smaller root
    if name.startswith("empty") or name == "disjoint":
        assert pc[0] == 0 and not mp[0, :len(want["match_p"]), 4].any()


def test_one_sided_at_a_higher_threshold():
    """at 3/4 the pair at exactly 1/2 no longer passes; partners, I and U do not depend on the threshold"""
    mask_p, mask_t, want = M.planted()["one_sided"]
    mp, mt, _ = _check([mask_p], [_ones(mask_p)], [mask_t], [_ones(mask_t)], iou=(3, 4))
    assert not mp[0, :2, 3].any() and not mt[0, :3, 3].any()
    assert np.array_equal(mp[0, :2, :3], want["match_p"][:, :3]) and np.array_equal(mt[0, :3, 4], want["match_t"][:, 4])


def test_identical_maps_match_every_building():
    mask = R.blobs(3, 65, 65)
    dmg = R.dmg_for(4, mask.shape)
    mp, mt, pc = _check([mask], [dmg], [mask], [dmg], iou=(1, 1))
    area = R.table(mask, dmg)[:, 1]
    n = len(area)
    assert n > 5 and pc[0] == n
    for m in (mp, mt):
        assert m[0, :n, 0].tolist() == list(range(n)) and np.array_equal(m[0, :n, 1], area) and np.array_equal(m[0, :n, 2], area)
        assert np.all(m[0, :n, 3] == 1) and np.all(m[0, :n, 4] == 1)


def test_checkerboard_against_its_shift_and_against_a_full_tile():
    cb = M.checker(64, 64)
    mp, mt, pc = _check([cb], [_ones(cb)], [~cb], [_ones(cb)])
    assert pc[0] == 0 and np.all(mp[0, :2048, 0] == -1) and np.all(mt[0, :2048, 4] == 0)
    full = np.ones((64, 64), dtype=bool)
    # 2048 pieces, 2048 pairs, one labelled building with 2048 partners: the pair table at its designed load
    mp, mt, pc = _check([cb], [_ones(cb)], [full], [_ones(cb)], max_pieces=2048)
    assert pc[0] == 2048 and mt[0, 0].tolist() == [0, 1, 4096, 0, 2048, 0, 0, 0]
    assert np.all(mp[0, :2048, 0] == 0) and np.all(mp[0, :2048, 1] == 1) and np.all(mp[0, :2048, 4] == 1)
    # overflow: the count is still true, the canaries hold (_call) and the rows stay inside their storage (_check)
    mp, mt, pc = _check([cb], [_ones(cb)], [full], [_ones(cb)], max_pieces=100)
    assert pc[0] == 2048


SPANS = {"33x65": (R.blobs(7, 33, 65, thresh=0.45), np.ones((33, 65), dtype=bool)),
         "130x70": (R.spiral(130, 70), np.ones((130, 70), dtype=bool)),
         "130x70_blobs": (R.blobs(8, 130, 70), R.spiral(130, 70)),
         "1x9000": (((np.arange(9000) // 7) % 2 == 0)[None, :], (np.arange(9000) < 8990)[None, :]),
         "9000x1": (((np.arange(9000) // 5) % 3 != 0)[:, None], (np.arange(9000) > 4)[:, None])}


@pytest.mark.parametrize("name", sorted(SPANS))
def test_pieces_and_buildings_that_span_regions_and_chunks(name):
    a, b = SPANS[name]
    dmg = R.dmg_for(11, a.shape)
    _check([a], [dmg], [b], [dmg])
    _check([b], [dmg], [a], [dmg], iou=(2, 3))           # the entry is symmetric in its two sides


def test_full_512_needs_a_64_bit_comparison():
    full = np.ones((512, 512), dtype=bool)
    mp, mt, pc = _check([full], [_ones(full)], [full], [_ones(full)], iou=(1, 1))
    row = [0, 1 << 18, 1 << 18, 1, 1, 0, 0, 0]           # I * U = 2^36
    assert pc.tolist() == [1] and mp[0, 0].tolist() == row and mt[0, 0].tolist() == row


# ---- random maps, batches ----------------------------------------------------------------------------------------------------
SHAPE = (96, 160)


@functools.lru_cache(maxsize=None)
def _random_case():
    masks_p = [R.blobs(21, *SHAPE), np.zeros(SHAPE, dtype=bool), R.blobs(22, *SHAPE, thresh=0.52)]
    masks_t = [R.blobs(31, *SHAPE, thresh=0.48), R.blobs(32, *SHAPE), R.blobs(22, *SHAPE, thresh=0.5)]
    dmgs_p = [R.dmg_for(40 + i, SHAPE) for i in range(3)]
    dmgs_t = [R.dmg_for(50 + i, SHAPE) for i in range(3)]
    want = [M.match(*maps) for maps in zip(masks_p, dmgs_p, masks_t, dmgs_t)]
    return masks_p, dmgs_p, masks_t, dmgs_t, want


def test_batch_of_three_with_an_empty_middle_tile_equals_single_runs():
    masks_p, dmgs_p, masks_t, dmgs_t, want = _random_case()
    mp, mt, pc = _check(masks_p, dmgs_p, masks_t, dmgs_t, want=want)
    assert pc[1] == 0 and pc[0] > 10 and pc[2] > 10
    assert want[2]["match_p"][:, 3].sum() > 3 and (want[0]["match_p"][:, 4] > 1).any()
    for b in range(3):
        m1p, m1t, pc1 = _check([masks_p[b]], [dmgs_p[b]], [masks_t[b]], [dmgs_t[b]], want=[want[b]])
        n_p, n_t = len(want[b]["match_p"]), len(want[b]["match_t"])
        assert pc1[0] == pc[b] and np.array_equal(m1p[0, :n_p], mp[b, :n_p]) and np.array_equal(m1t[0, :n_t], mt[b, :n_t])


def test_five_runs_on_a_side_stream_give_identical_bytes():
    masks_p, dmgs_p, masks_t, dmgs_t, want = _random_case()
    side = torch.cuda.Stream()
    first = _check(masks_p, dmgs_p, masks_t, dmgs_t, want=want, stream=side)
    for _ in range(4):
        again = _check(masks_p, dmgs_p, masks_t, dmgs_t, want=want, stream=side)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def _tile_with(n_components, shape=(40, 60)):
    """a tile with exactly n separate 2 x 2 blocks"""
    mask = np.zeros(shape, dtype=bool)
    k = 0
    for y in range(0, shape[0] - 1, 3):
        for x in range(0, shape[1] - 1, 3):
            if k < n_components:
                mask[y:y + 2, x:x + 2] = True
                k += 1
    assert k == n_components
    return mask


def test_tables_truncated_on_one_tile_leave_the_other_tile_exact():
    masks_p = [_tile_with(37), _tile_with(4)]
    masks_t = [R.blobs(61, 40, 60), R.blobs(62, 40, 60)]
    dmgs = [R.dmg_for(63, (40, 60))] * 2
    want = M.match(masks_p[1], dmgs[1], masks_t[1], dmgs[1])
    n_t = max(len(R.table(m, dmgs[0])) for m in masks_t)
    p, t = _tables(masks_p, dmgs, 5), _tables(masks_t, dmgs, n_t)
    assert p[2].tolist() == [37, 4]
    mp, mt, pc = _call(p, t, (1, 2), 4096)
    assert pc[1] == want["piece_count"]
    assert np.array_equal(mp[1, :4], want["match_p"]) and np.all(mp[1, 4:] == FILL)
    assert np.array_equal(mt[1, :len(want["match_t"])], want["match_t"]) and np.all(mt[1, len(want["match_t"]):] == FILL)
    # tile 0: its five rows hold something, inside their storage (the canaries of _call)
    assert np.all(mp[0] != FILL)
    # and the same with the target's table cut short instead
    p, t = _tables(masks_t, dmgs, n_t), _tables(masks_p, dmgs, 5)
    mp, mt, pc = _call(p, t, (1, 2), 4096)
    assert np.array_equal(mt[1, :4], want["match_p"]) and np.array_equal(mp[1, :len(want["match_t"])], want["match_t"])


def test_labels_from_one_map_with_rows_from_another():
    """rows_t (and count_t) of a map whose right half was cleared, under labels_t of the whole map: buildings of the left
    half keep root and area, buildings across the middle keep their root but have another area in the table, buildings of
    the right half name no row and are dropped"""
    shape = (70, 130)
    mask_p, mask_t = R.blobs(71, *shape), R.blobs(72, *shape)
    cut = mask_t.copy()
    cut[:, 65:] = False
    dmg = R.dmg_for(73, shape)
    n_p, n_cut = len(R.table(mask_p, dmg)), len(R.table(cut, dmg))
    p = _tables([mask_p], [dmg], n_p)
    whole, other = _tables([mask_t], [dmg], n_cut), _tables([cut], [dmg], n_cut)
    assert int(whole[2][0]) > n_cut == int(other[2][0])
    mp, mt, pc = _call(p, (whole[0], other[1], other[2]), (1, 2), 4096)
    lab_t, rows_cut = R.label_min_index(mask_t), R.table(cut, dmg)
    named = np.isin(lab_t - 1, rows_cut[:, 0])
    assert (named & (lab_t > 0)).any() and (~named & (lab_t > 0)).any()
    area = dict(R.table(mask_t, dmg)[:, :2].tolist())
    assert any(r in area and area[r] != a for r, a in rows_cut[:, :2].tolist())      # a named row with another area
    want_p, want_t = M.match_tables(R.label_min_index(mask_p), R.table(mask_p, dmg), np.where(named, lab_t, 0), rows_cut)
    assert np.array_equal(mp[0], want_p), _first_diff(mp[0], want_p, "match_p", 0)
    assert np.array_equal(mt[0], want_t), _first_diff(mt[0], want_t, "match_t", 0)
    assert pc[0] == M.piece_count(R.label_min_index(mask_p), lab_t)          # pieces are counted before any is dropped


@pytest.mark.parametrize("long_side", ["p", "t"])
def test_a_pair_that_passes_the_threshold_without_being_mutual_is_not_matched(long_side):
    """M.two_halves: column 3 needs the mutual-best condition, not the threshold alone"""
    labels_of, rows_of, short, want = M.two_halves()
    dmg = _ones(short)
    lab, other = _tables([labels_of], [dmg], 1), _tables([rows_of], [dmg], 1)
    assert int(other[1][0, 0, 0]) == int(lab[1][0, 0, 0]) and int(other[1][0, 0, 1]) == 4 and int(lab[1][0, 0, 1]) == 5
    long_, short_ = (lab[0], other[1], other[2]), _tables([short], [dmg], 2)
    if long_side == "p":
        m_long, m_short, pc = _call(long_, short_, (1, 2), 16)
    else:
        m_short, m_long, pc = _call(short_, long_, (1, 2), 16)
    assert pc.tolist() == [2]
    assert np.array_equal(m_long[0], want["long"]), m_long[0]
    assert np.array_equal(m_short[0], want["short"]), m_short[0]
    assert 2 * m_short[0, 1, 1] >= m_short[0, 1, 2] and m_short[0, 1, 3] == 0        # passes 1/2, partner's best is another


# ---- the wrappers --------------------------------------------------------------------------------------------------------------
def test_ops_wrapper_checks_its_arguments():
    from xview2_amd import ops
    mask = R.blobs(3, 20, 30)
    p = _tables([mask], [_ones(mask)], 8)
    mp, mt, pc = ops.building_match(*p, *p)
    assert mp.shape == (1, 8, 8) and mt.shape == (1, 8, 8) and mp.dtype == torch.int64 and pc.dtype == torch.int32
    with pytest.raises(ValueError, match="iou"):
        ops.building_match(*p, *p, iou=(1, 3))
    with pytest.raises(ValueError, match="labels_t"):
        ops.building_match(*p, p[0][:, :10], p[1], p[2])
    with pytest.raises(ValueError, match="rows_p"):
        ops.building_match(p[0], p[1][:, :, :8], p[2], *p)
    with pytest.raises(ValueError, match="count_t"):
        ops.building_match(*p, p[0], p[1], p[2].long())
    with pytest.raises(ValueError, match="max_pieces"):
        ops.building_match(*p, *p, max_pieces=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.building_match(p[0].cpu(), p[1], p[2], *p)


def test_match_maps_runs_once_more_when_the_pieces_exceed_the_first_capacity(monkeypatch):
    from xview2_amd import ops
    from xview2_amd.utils import building_metrics as BM
    masks_p, dmgs_p, masks_t, dmgs_t, want = _random_case()
    calls = []
    real = ops.building_match
    monkeypatch.setattr(ops, "building_match", lambda *a: calls.append(a[-1]) or real(*a))
    maps = [_dev(np.stack(x).astype(np.uint8)) for x in (masks_p, dmgs_p, masks_t, dmgs_t)]
    most = max(w["piece_count"] for w in want)

    def same(tms):
        for tm, w in zip(tms, want):
            for key in ("table_p", "table_t", "match_p", "match_t"):
                assert np.array_equal(getattr(tm, key), w[key]), key

    same(BM.match_maps(*maps))
    assert calls == [BM.first_capacity(*SHAPE)]                  # the first capacity sufficed: one run
    del calls[:]
    same(BM.match_maps(*maps, max_pieces=4))
    assert calls == [4, most]
    del calls[:]
    monkeypatch.setattr(BM, "first_capacity", lambda H, W: 7)
    same(BM.match_maps(*maps))
    assert calls == [7, most]
    one = BM.match_maps(*(m[0] for m in maps))                   # unbatched input: one TileMatch
    assert np.array_equal(one.match_p, want[0]["match_p"]) and np.array_equal(one.match_t, want[0]["match_t"])


def _class_blocks(seed, shape, cell=64):
    """values 1..4, constant on cell x cell blocks"""
    coarse = R._hash(seed, (shape[0] // cell, shape[1] // cell), 4) + 1
    return np.kron(coarse, np.ones((cell, cell), dtype=np.int64)).astype(np.uint8)


def test_compute_score_on_a_directory_of_four_tiles(tmp_path):
    from PIL import Image
    from xview2_amd.utils import building_metrics as BM
    pred, targ = tmp_path / "pred", tmp_path / "targ"
    pred.mkdir()
    targ.mkdir()
    shape, counts, wants = (1024, 1024), [], []
    for i in range(4):
        # about 300 rectangular buildings per tile; the prediction moves every edge by up to 3 pixels and leaves some out
        pre_t, pre_p = M.town(100 + i, *shape), M.town(100 + i, *shape, jitter=500 + i)
        post_t = _class_blocks(200 + i, shape) * pre_t
        post_p = np.where(R._hash(300 + i, shape, 8) == 0, _class_blocks(400 + i, shape), _class_blocks(200 + i, shape)) * pre_p
        tile = "%05d" % (7 * i)
        for d, name, a in ((pred, "test_localization_%s_prediction.png", pre_p), (pred, "test_damage_%s_prediction.png", post_p),
                           (targ, "test_localization_%s_target.png", pre_t), (targ, "test_damage_%s_target.png", post_t)):
            Image.fromarray(np.ascontiguousarray(a).astype(np.uint8)).save(str(d / (name % tile)))
        w = M.match(pre_p.astype(np.uint8), post_p.astype(np.uint8), pre_t.astype(np.uint8), post_t.astype(np.uint8))
        wants.append(w)
        counts.append(M.tile_counts(w["table_p"], w["table_t"], w["match_p"], w["match_t"]))
    want = M.score(counts)
    assert want["totals"]["TP"] > 500 and want["totals"]["FP"] > 20 and want["totals"]["FN"] > 20 and want["totals"]["merged"] > 5
    out, csvs = str(tmp_path / "o.json"), str(tmp_path / "csv")
    got = BM.compute_score(str(pred), str(targ), out, per_building=csvs)
    assert got == want and json.load(open(out)) == want
    first = open(out, "rb").read()
    names = sorted(os.listdir(csvs))
    assert names == ["test_buildings_%05d_match.csv" % (7 * i) for i in range(4)]
    first_csv = [open(os.path.join(csvs, n), "rb").read() for n in names]
    for n, w in zip(names, wants):
        recs = BM.read_csv(os.path.join(csvs, n))
        assert recs == BM.to_records(BM.TileMatch(w["table_p"], w["table_t"], w["match_p"], w["match_t"]))
    assert BM.compute_score(str(pred), str(targ), out, per_building=csvs) == want
    assert open(out, "rb").read() == first
    assert [open(os.path.join(csvs, n), "rb").read() for n in names] == first_csv
    with pytest.raises(ValueError, match="0-4"):
        Image.fromarray(np.full(shape, 5, np.uint8)).save(str(pred / "test_damage_00000_prediction.png"))
        BM.compute_score(str(pred), str(targ), out)
