"""The per-building table without a GPU: the scipy restatement (tests/buildings_ref.py) against a brute-force flood fill,
the record / CSV / summary helpers of xview2_amd/utils/buildings.py on hand-written rows, the ABI declaration and the
command-line flags."""
import ctypes
import json

import numpy as np
import pytest

import buildings_ref as R


# ---- the restatement itself ----------------------------------------------------------------------------------------------
TINY = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (12, 12), (11, 12), (12, 3)]


@pytest.mark.parametrize("shape", TINY)
def test_restatement_equals_flood_fill(shape):
    for seed in range(6):
        mask = R._hash(10 * seed + shape[0], shape, 100) < (35, 50, 65, 80, 100, 0)[seed]
        dmg = R.dmg_for(seed + 50, shape)
        loc = R.loc_for(seed + 70, shape)
        a, b = R.table(mask, dmg, loc), R.flood_table(mask, dmg, loc)
        assert a.shape == b.shape and np.array_equal(a, b), (shape, seed, a, b)
        a0 = R.table(mask, dmg, None)
        assert np.array_equal(a0[:, :14], a[:, :14]) and not a0[:, 14].any() and not a[:, 15].any()
        assert np.all(np.diff(a[:, 0]) > 0)                      # ascending roots: scipy's numbering
        lab = R.label_min_index(mask)
        assert np.array_equal(np.unique(lab[lab > 0]) - 1, a[:, 0])


def test_restatement_on_the_named_shapes():
    cases = R.shape_cases()
    assert R.table(cases["checker_64"], np.ones((64, 64), np.uint8)).shape == (2048, 16)
    assert R.table(cases["checker_128x96"], np.ones((128, 96), np.uint8)).shape == (6144, 16)
    assert R.table(cases["empty_70"], np.zeros((70, 70), np.uint8)).shape == (0, 16)
    t = R.table(cases["spiral_130x70"], np.full((130, 70), 3, np.uint8))
    assert t.shape[0] == 1 and t[0, 0] == 0 and t[0, 2:6].tolist() == [0, 0, 129, 69] and t[0, 13] == 3
    u = R.table(cases["u_around_block"], np.ones((40, 90), np.uint8))
    assert u.shape[0] == 2 and u[0, 2] <= u[1, 2] and u[0, 3] <= u[1, 3] and u[0, 4] >= u[1, 4] and u[0, 5] >= u[1, 5]
    d = R.table(cases["diagonals"], np.ones((9, 70), np.uint8))
    assert d.shape[0] == int(cases["diagonals"].sum()) and np.all(d[:, 1] == 1)
    # the sums of a full 2100 x 2100 tile need 64 bits (closed form: no 4.4 M-pixel labelling in a CPU test)
    assert 2100 * (2100 * 2099 // 2) == 4628295000 > 2 ** 32


def test_quantiser_ties_and_specials():
    q = R.quantise(np.array([np.nan, np.inf, -np.inf, -1, 2, 0, 1, 0.5], dtype=np.float32))
    assert q.tolist() == [0, 65535, 0, 0, 65535, 0, 65535, 32768]
    h = R.halfway_values()
    prod = (h * np.float32(65535)).astype(np.float64)
    assert len(h) == 9 and np.all(prod - np.floor(prod) == 0.5)
    fl = np.floor(prod).astype(np.int64)
    want = np.where(fl % 2 == 0, fl, fl + 1)                    # ties to the even integer
    assert np.array_equal(R.quantise(h), want)
    assert (fl % 2 == 0).sum() >= 4 and (fl % 2 == 1).sum() >= 4


def test_vote_tie_rule():
    assert R.vote([[3, 3, 0, 0], [1, 5, 0, 5], [0, 0, 0, 0], [0, 0, 0, 1], [2, 2, 2, 2]]).tolist() == [1, 2, 0, 4, 1]


# ---- records, CSV, summary -------------------------------------------------------------------------------------------------
#        root area y0 x0 y1 x1   sy   sx n1 n2 n3 n4 no cls       q  -
ROWS = [[3, 4, 0, 3, 1, 4, 2, 14, 2, 2, 0, 0, 0, 1, 4 * 65535, 0],
        [40, 3, 2, 0, 2, 2, 6, 3, 0, 0, 0, 0, 3, 0, 0, 0],
        [77, 7, 3, 17, 5, 19, 29, 127, 1, 2, 0, 2, 2, 2, 100000, 0],
        [2 ** 21, 2100 * 2100, 0, 0, 2099, 2099, 4628295000, 4628295000, 0, 0, 0, 2100 * 2100, 0, 4, 65535 * 2100 * 1050, 0]]


def test_records_csv_and_summary(tmp_path):
    from xview2_amd.utils import buildings as B
    recs = B.to_records(np.array(ROWS, dtype=np.int64), 2100, 2100)
    assert [r["id"] for r in recs] == [1, 2, 3, 4]
    assert recs[0] == {"id": 1, "y0": 0, "x0": 3, "y1": 1, "x1": 4, "area": 4, "cy": 0.5, "cx": 3.5, "damage": 1, "n1": 2,
                       "n2": 2, "n3": 0, "n4": 0, "n_other": 0, "confidence": 1.0}
    assert recs[1]["damage"] == 0 and recs[1]["confidence"] == 0.0 and recs[1]["cy"] == 2.0 and recs[1]["cx"] == 1.0
    assert recs[2]["cy"] == 29 / 7 and recs[2]["cx"] == 127 / 7 and recs[2]["confidence"] == 100000 / (65535 * 7)
    assert recs[3]["cy"] == 1049.5 and recs[3]["cx"] == 1049.5 and recs[3]["confidence"] == 0.5
    assert all(type(r[k]) is float for r in recs for k in ("cy", "cx", "confidence"))
    assert all(type(r[k]) is int for r in recs for k in r if k not in ("cy", "cx", "confidence"))
    path = str(tmp_path / "b.csv")
    B.write_csv(path, recs)
    lines = open(path).read().split("\n")
    assert lines[0] == "id,y0,x0,y1,x1,area,cy,cx,damage,n1,n2,n3,n4,n_other,confidence" and len(lines) == 6 and lines[5] == ""
    assert lines[3] == "3,3,17,5,19,7,%r,%r,2,1,2,0,2,2,%r" % (29 / 7, 127 / 7, 100000 / (65535 * 7))
    assert B.read_csv(path) == recs                              # repr round-trips every float
    first = open(path, "rb").read()
    B.write_csv(path, B.to_records(np.array(ROWS, dtype=np.int64), 2100, 2100))
    assert open(path, "rb").read() == first
    # no localization probabilities: no confidence, in the records and in the file
    bare = B.to_records(ROWS[:3], 2100, 2100, confidence=False)
    assert all("confidence" not in r for r in bare)
    B.write_csv(path, bare)
    assert open(path).readline().strip().endswith("n_other") and B.read_csv(path) == bare
    B.write_csv(path, [])
    assert open(path).read() == "id,y0,x0,y1,x1,area,cy,cx,damage,n1,n2,n3,n4,n_other\n"
    s = B.summary(recs)
    assert s == {"buildings": 4, "buildings_per_damage": [1, 1, 1, 0, 1],
                 "pixels_per_damage": [5, 3, 4, 0, 2 + 2100 * 2100]}
    assert sum(s["buildings_per_damage"]) == s["buildings"]
    assert sum(s["pixels_per_damage"]) == sum(r["area"] for r in recs)
    B.write_summary(str(tmp_path / "b.json"), recs)
    assert json.load(open(str(tmp_path / "b.json"))) == s
    with pytest.raises(ValueError, match="no building"):
        B.to_records([[0, 0] + [0] * 14], 4, 4)
    assert B.first_capacity(64, 64) == 1024 and B.first_capacity(2100, 2100) == 2100 * 2100 // 256


# ---- ABI and flags -----------------------------------------------------------------------------------------------------------
def test_header_declares_the_table_and_its_workspace_query():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    rt, argt = protos["xv2_building_table"]
    assert rt is ctypes.c_int and len(argt) == 11
    rt, argt = protos["xv2_building_table_workspace"]
    assert rt is ctypes.c_size_t and argt == [ctypes.c_int] * 3
    assert "buildings.hip" in _lib.SOURCES
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "xv2.h")).read()
    assert "#define XV2_BUILDING_COLS 16" in hdr
    _lib.build()
    q = lambda *a: _capi.query("xv2_building_table_workspace", *a)
    n = q(2, 100, 70)
    assert n >= 4 * 2 * 100 * 70 + 4 * 2 * 2 and n % 256 == 0
    assert q(0, 4, 4) == 0 and q(1, 1 << 15, 1 << 15) == 0 and q(65536, 4, 4) == 0 and q(1, 1, 1) > 0
    # argument checks are reachable without a GPU
    f = _capi._func("xv2_building_table")
    one = ctypes.c_void_p(8)
    for args, msg in (((one, one, None, 0, 4, 4, 1, one, one, one, None), b"positive"),
                      ((one, one, None, 1, 1 << 15, 1 << 15, 1, one, one, one, None), b"2^30"),
                      ((one, one, None, 1, 4, 4, 0, one, one, one, None), b"max_rows"),
                      ((None, one, None, 1, 4, 4, 1, one, one, one, None), b"null"),
                      ((one, None, None, 1, 4, 4, 1, one, one, one, None), b"null"),
                      ((one, one, None, 1, 4, 4, 1, None, one, one, None), b"null"),
                      ((one, one, None, 1, 4, 4, 1, one, None, one, None), b"null"),
                      ((one, one, None, 1, 4, 4, 1, one, one, None, None), b"null")):
        assert f(*args) == 1 and msg in _lib.lib().xv2_last_error(), (args, _lib.lib().xv2_last_error())


def test_cli_flags_default_off():
    from xview2_amd import predict
    from xview2_amd.utils import post_process
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o"])
    assert a.buildings is False
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--buildings"]).buildings is True
    b = post_process.get_parser().parse_args([])
    assert b.buildings is False and post_process.get_parser().parse_args(["--buildings"]).buildings is True
    assert post_process._buildings_name("/r/probs/test_localization_00012.npy") == "test_buildings_00012.csv"


def test_scene_predict_pair_takes_buildings():
    import inspect
    from xview2_amd import scene
    p = inspect.signature(scene.predict_pair).parameters
    assert p["buildings"].default is False
