"""The building match without a GPU: the restatement (tests/match_ref.py) against a brute-force dense version and the
hand-derived planted cases, the score arithmetic of xview2_amd/utils/building_metrics.py on hand-written match arrays, the
--iou parser, the ABI declaration, the workspace query and every argument check of the entry point."""
import ctypes
import json

import numpy as np
import pytest

import buildings_ref as R
import match_ref as M

TINY = [(1, 1), (1, 7), (7, 1), (5, 9), (12, 12)]
DENSITY = (35, 50, 65, 80, 100, 0)


# ---- the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TINY)
def test_restatement_equals_dense_brute_force(shape):
    dmg = np.ones(shape, np.uint8)
    for sp in range(6):
        for st in range(6):                      # densities 100 and 0: full and empty maps on either side and on both
            mask_p = R._hash(10 * sp + shape[0], shape, 100) < DENSITY[sp]
            mask_t = R._hash(977 + 10 * st + shape[1], shape, 100) < DENSITY[st]
            for iou in ((1, 2), (3, 4), (1, 1)):
                got = M.match(mask_p, dmg, mask_t, dmg, iou)
                mp, mt, pieces = M.dense_match(mask_p, mask_t, iou)
                assert np.array_equal(got["match_p"], mp), (shape, sp, st, iou, got["match_p"], mp)
                assert np.array_equal(got["match_t"], mt), (shape, sp, st, iou, got["match_t"], mt)
                assert got["piece_count"] == pieces
                assert got["match_p"][:, 3].sum() == got["match_t"][:, 3].sum()
                assert got["match_p"][:, 4].sum() == got["match_t"][:, 4].sum() <= pieces      # pairs <= pieces


def test_planted_cases_have_their_hand_derived_answers():
    for name, (mask_p, mask_t, want) in M.planted().items():
        dmg = np.ones(mask_p.shape, np.uint8)
        got = M.match(mask_p, dmg, mask_t, dmg, (1, 2))
        assert np.array_equal(got["match_p"], want["match_p"]), (name, got["match_p"])
        assert np.array_equal(got["match_t"], want["match_t"]), (name, got["match_t"])
        assert got["piece_count"] == want["piece_count"], name
        mp, mt, pieces = M.dense_match(mask_p, mask_t, (1, 2))
        assert np.array_equal(mp, want["match_p"]) and np.array_equal(mt, want["match_t"]) and pieces == want["piece_count"]


def test_mutual_best_decides_only_with_a_table_from_another_map():
    labels_of, rows_of, short, want = M.two_halves()
    dmg = np.ones(short.shape, np.uint8)
    lab_long, rows_long = R.label_min_index(labels_of), R.table(rows_of, dmg)
    lab_short, rows_short = R.label_min_index(short), R.table(short, dmg)
    assert rows_long[:, :2].tolist() == [[21, 4]] and rows_short[:, :2].tolist() == [[21, 2], [24, 2]]
    mp, mt = M.match_tables(lab_long, rows_long, lab_short, rows_short)
    assert np.array_equal(mp, want["long"]) and np.array_equal(mt, want["short"])
    mp, mt = M.match_tables(lab_short, rows_short, lab_long, rows_long)
    assert np.array_equal(mp, want["short"]) and np.array_equal(mt, want["long"])
    assert M.piece_count(lab_long, lab_short) == want["piece_count"]
    # with the labels' own table (area 5) neither pair reaches 1/2: I = 2, U = 5
    own = M.match(labels_of, dmg, short, dmg)
    assert own["match_p"].tolist() == [[0, 2, 5, 0, 2, 0, 0, 0]] and not own["match_t"][:, 3].any()
    # and on genuine labellings a pair that passes the threshold is always mutual (the argument of M.two_halves)
    for sp in range(6):
        for st in range(6):
            got = M.match(R.blobs(sp, 24, 40, box=3), np.ones((24, 40), np.uint8), R.blobs(50 + st, 24, 40, box=3),
                          np.ones((24, 40), np.uint8))
            for m in (got["match_p"], got["match_t"]):
                assert np.array_equal(m[:, 3], ((m[:, 0] >= 0) & (2 * m[:, 1] >= m[:, 2])).astype(np.int64))


def test_labels_that_name_no_row_are_dropped_by_the_restatement():
    mask_p, mask_t = R.blobs(5, 20, 30), R.blobs(6, 20, 30)
    dmg = np.ones((20, 30), np.uint8)
    full = M.match(mask_p, dmg, mask_t, dmg)
    keep = full["table_t"][::2]                                   # every other labelled building loses its row
    zeroed = np.where(np.isin(full["labels_t"] - 1, keep[:, 0]), full["labels_t"], 0)
    a = M.match_tables(full["labels_p"], full["table_p"], full["labels_t"], keep)
    b = M.match_tables(full["labels_p"], full["table_p"], zeroed, keep)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].shape[0] == keep.shape[0]


# ---- the score arithmetic --------------------------------------------------------------------------------------------------
def _table(classes, areas=None):
    t = np.zeros((len(classes), 16), dtype=np.int64)
    t[:, 0] = 10 * np.arange(len(classes))
    t[:, 1] = 4 if areas is None else areas
    t[:, 13] = classes
    return t


#          partner I  U  matched partners
MATCH_P = [[0, 4, 4, 1, 1, 0, 0, 0],      # p0 (class 1) <-> t0 (class 1)
           [2, 3, 5, 1, 2, 0, 0, 0],      # p1 (class 2) <-> t2 (class 4); p1 also touches t1: a merge
           [-1, 0, 4, 0, 0, 0, 0, 0],     # p2 (class 2): spurious
           [3, 1, 7, 0, 1, 0, 0, 0]]      # p3 (class 0): touches t3, below the threshold
MATCH_T = [[0, 4, 4, 1, 1, 0, 0, 0],
           [1, 1, 7, 0, 1, 0, 0, 0],
           [1, 3, 5, 1, 1, 0, 0, 0],
           [3, 1, 7, 0, 1, 0, 0, 0],
           [-1, 0, 4, 0, 0, 0, 0, 0]]


def _hand_tile():
    from xview2_amd.utils import building_metrics as BM
    return BM.TileMatch(_table([1, 2, 2, 0]), _table([1, 3, 4, 4, 3]), np.array(MATCH_P, dtype=np.int64),
                        np.array(MATCH_T, dtype=np.int64))


def test_tile_counts_and_score_on_hand_written_matches(tmp_path):
    from xview2_amd.utils import building_metrics as BM
    tm = _hand_tile()
    c = BM.tile_counts(tm)
    conf = [[0] * 5 for _ in range(5)]
    conf[1][1] = 1
    conf[4][2] = 1
    assert c == {"TP": 2, "FP": 2, "FN": 3, "confusion": conf, "pred_per_class": [1, 1, 2, 0, 0],
                 "targ_per_class": [0, 1, 0, 2, 2], "merged": 1, "split": 0}
    assert all(type(v) is int for k in ("TP", "FP", "FN", "merged", "split") for v in [c[k]])
    assert sum(sum(r) for r in c["confusion"]) == c["TP"]
    assert c == M.tile_counts(*tm)
    tot = BM.sum_counts([c, c, c])
    assert tot["TP"] == 6 and tot["confusion"][4][2] == 3 and tot["pred_per_class"] == [3, 3, 6, 0, 0]
    d = BM.score_dict(tot, (1, 2), 3)
    assert d["object_localization_precision"] == 6 / 12 and d["object_localization_recall"] == 6 / 15
    assert d["object_localization_f1"] == (2 * 0.5 * 0.4) / (0.5 + 0.4)
    # class 1: TP 3, FP 0, FN 0 -> 1.0; class 2: TP 0 -> 0; class 3: TP 0; class 4: TP 0 (the matched class-4 label was called 2)
    assert [d["object_damage_f1_" + k] for k in BM.CLASS_KEYS] == [1.0, 0, 0, 0]
    assert d["object_damage_f1"] == 4 / sum((x + 1e-6) ** -1 for x in (1.0, 0, 0, 0))
    assert d["totals"]["predicted"] == 12 and d["totals"]["labelled"] == 15 and d["totals"]["tiles"] == 3 and d["iou"] == [1, 2]
    assert d == M.score([c, c, c], (1, 2))
    assert json.loads(json.dumps(d, sort_keys=True)) == d
    # per-building records and their CSV
    recs = BM.to_records(tm)
    assert len(recs) == 9 and [r["side"] for r in recs] == ["p"] * 4 + ["t"] * 5
    assert recs[1] == {"side": "p", "id": 2, "y0": 0, "x0": 0, "y1": 0, "x1": 0, "area": 4, "damage": 2, "partner": 3,
                       "intersection": 3, "union": 5, "matched": 1, "partners": 2}
    assert recs[2]["partner"] == 0 and recs[8]["partner"] == 0
    path = str(tmp_path / "m.csv")
    BM.write_csv(path, recs)
    first = open(path, "rb").read()
    assert first.split(b"\n")[0] == b"side,id,y0,x0,y1,x1,area,damage,partner,intersection,union,matched,partners"
    assert first.split(b"\n")[2] == b"p,2,0,0,0,0,4,2,3,3,5,1,2"
    assert BM.read_csv(path) == recs
    BM.write_csv(path, BM.to_records(tm))
    assert open(path, "rb").read() == first


def test_zero_buildings_give_zeros_and_no_division_error():
    from xview2_amd.utils import building_metrics as BM
    e16, e8 = np.zeros((0, 16), np.int64), np.zeros((0, 8), np.int64)
    lone = np.array([[-1, 0, 4, 0, 0, 0, 0, 0]], dtype=np.int64)
    for tm in (BM.TileMatch(e16, e16, e8, e8), BM.TileMatch(_table([1]), e16, lone, e8), BM.TileMatch(e16, _table([3]), e8, lone)):
        c = BM.tile_counts(tm)
        assert c["TP"] == 0 and c == M.tile_counts(*tm) and sum(sum(r) for r in c["confusion"]) == 0
        d = BM.score_dict(BM.sum_counts([c]), (1, 2), 1)
        assert d["object_localization_precision"] == 0 and d["object_localization_recall"] == 0
        assert d["object_localization_f1"] == 0 and all(d["object_damage_f1_" + k] == 0 for k in BM.CLASS_KEYS)
        assert d["object_damage_f1"] == 4 / sum((x + 1e-6) ** -1 for x in (0, 0, 0, 0)) and d == M.score([c], (1, 2))
    d = BM.score_dict(BM.sum_counts([]), (3, 4), 0)                 # no tile at all
    assert d["object_localization_f1"] == 0 and d["totals"]["tiles"] == 0 and d["iou"] == [3, 4]
    with pytest.raises(ValueError, match="match rows"):
        BM.tile_counts(BM.TileMatch(_table([1]), e16, e8, e8))


def test_iou_parsing():
    from xview2_amd.utils import building_metrics as BM
    assert BM.parse_iou("1/2") == (1, 2) and BM.parse_iou("0.5") == (1, 2) and BM.parse_iou("0.75") == (3, 4)
    assert BM.parse_iou("2/4") == (1, 2) and BM.parse_iou("1") == (1, 1) and BM.parse_iou("0.55") == (11, 20)
    for bad in ("1/3", "0", "0.49", "1.5", "3/2", "1/0", "abc", "0.123456789", "-1/2", "inf", "Infinity", "nan", "1/2/3"):
        with pytest.raises(ValueError):
            BM.parse_iou(bad)
    p = BM.get_parser()
    a = p.parse_args(["P", "T", "o.json"])
    assert a.iou == (1, 2) and a.per_building is None and a.batch == 16
    a = p.parse_args(["P", "T", "o.json", "--iou", "0.75", "--per_building", "D"])
    assert a.iou == (3, 4) and a.per_building == "D"
    for bad in ("1/3", "inf"):
        with pytest.raises(SystemExit):
            p.parse_args(["P", "T", "o.json", "--iou", bad])
    import inspect
    assert inspect.signature(BM.BuildingMetrics.compute_score).parameters["batch"].default == 16
    assert "touch" in BM.__doc__ and "minimum-area" in BM.__doc__ and "georeferencing" in BM.__doc__


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_match_and_its_workspace_query():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    rt, argt = protos["xv2_building_match"]
    assert rt is ctypes.c_int and len(argt) == 19
    assert [i for i, t in enumerate(argt) if t is ctypes.c_int] == [3, 7, 8, 9, 10, 11, 12, 13]
    rt, argt = protos["xv2_building_match_workspace"]
    assert rt is ctypes.c_size_t and argt == [ctypes.c_int] * 4
    assert "match.hip" in _lib.SOURCES
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "xv2.h")).read()
    assert "#define XV2_MATCH_COLS 8" in hdr
    from xview2_amd import ops
    assert ops.MATCH_COLS == 8


def test_workspace_query():
    from xview2_amd import _capi, _lib
    _lib.build()
    q = lambda *a: _capi.query("xv2_building_match_workspace", *a)
    n = q(2, 100, 70, 500)
    # mask + piece labels + the piece table's workspace + piece rows + a pair table of >= 2 * max_pieces slots (key + sum)
    assert n >= 5 * 2 * 100 * 70 + _capi.query("xv2_building_table_workspace", 2, 100, 70) + 2 * 500 * 128 + 2 * 1000 * 16
    assert n % 256 == 0
    assert q(1, 1, 1, 1) > 0 and q(65535, 1, 1, 1) > 0
    assert q(0, 4, 4, 1) == 0 and q(1, 0, 4, 1) == 0 and q(1, 4, 0, 1) == 0 and q(1, 4, 4, 0) == 0
    assert q(1, 1 << 15, 1 << 15, 1) == 0 and q(65536, 4, 4, 1) == 0
    assert q(1, 64, 64, 1 << 30) == q(1, 64, 64, 2048)      # a tile of 4096 pixels has at most 2048 pieces
    assert q(1, 64, 64, 2048) > q(1, 64, 64, 100)


def test_every_argument_check_is_reachable_without_a_gpu():
    from xview2_amd import _capi, _lib
    _lib.build()
    f = _capi._func("xv2_building_match")
    one = ctypes.c_void_p(8)

    def args(**kw):
        a = dict(labels_p=one, rows_p=one, count_p=one, max_rows_p=1, labels_t=one, rows_t=one, count_t=one, max_rows_t=1,
                 B=1, H=4, W=4, num=1, den=2, max_pieces=1, ws=one, match_p=one, match_t=one, piece_count=one, stream=None)
        a.update(kw)
        return tuple(a.values())

    cases = [(dict(B=0), b"positive"), (dict(H=0), b"positive"), (dict(W=-1), b"positive"),
             (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"),
             (dict(max_rows_p=0), b"max_rows"), (dict(max_rows_t=0), b"max_rows"), (dict(max_pieces=0), b"max_pieces"),
             (dict(num=0), b"iou_num"), (dict(num=3, den=2), b"iou_num"), (dict(num=40000, den=65537), b"iou_num"),
             (dict(num=1, den=3), b"below 1/2"), (dict(num=32767, den=65535), b"below 1/2")]
    cases += [({k: None}, b"null") for k in ("labels_p", "rows_p", "count_p", "labels_t", "rows_t", "count_t", "ws", "match_p",
                                             "match_t", "piece_count")]
    for kw, msg in cases:
        assert f(*args(**kw)) == 1 and msg in _lib.lib().xv2_last_error(), (kw, _lib.lib().xv2_last_error())
        assert b"building_match" in _lib.lib().xv2_last_error()
