"""The building outlines without a GPU: the sequential restatement (tests/polygons_ref.py) against the properties the
contract of include/xv2.h states and against the building table's restatement, the WKT / GeoJSON / xBD writers of
xview2_amd/utils/polygons.py on hand-written polygons, the ABI declaration and the command-line flags."""
import ctypes
import json

import numpy as np
import pytest

import buildings_ref as BR
import polygons_ref as R


# ---- the restatement itself ----------------------------------------------------------------------------------------------
def _five_checks(mask):
    """the contract's properties on one tile, and agreement with the building table"""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    lab = R.labels_of(mask)
    rings, verts, n_edges = R.trace_tile(lab)                    # (asserts that every walk stays on unvisited boundary edges)
    # 1. every cycle closes: the rings partition the boundary edges
    assert int(rings[:, 5].sum()) == n_edges == len(R.boundary_edges(lab))
    assert int(rings[:, 2].sum()) == len(verts)
    # 2. even-odd rasterisation of the rings at pixel centres gives back the mask
    assert np.array_equal(R.rasterise(rings, verts, H, W), mask)
    # 3. exterior leaders are exactly {4 root}
    roots = np.unique(lab[lab > 0]).astype(np.int64) - 1
    ext = rings[rings[:, 4] > 0]
    assert np.array_equal(ext[:, 1], 4 * roots) and np.array_equal(ext[:, 0], roots)
    assert np.all(rings[rings[:, 4] <= 0][:, 1] != 4 * rings[rings[:, 4] <= 0][:, 0]) and np.all(rings[:, 4] != 0)
    # 4. every ring has an even number of vertices, at least 4
    assert np.all(rings[:, 2] % 2 == 0) and np.all(rings[:, 2] >= 4)
    # 5. the number of rings
    assert len(rings) == R.expected_ring_count(mask)
    assert np.all(np.diff(rings[:, 1]) > 0) and not rings[:, 6:].any()
    # the building table: the 2A of a component's rings sum to twice its area; the exterior's extent is its box
    table = BR.table(mask, np.zeros((H, W), np.uint8))
    assert np.array_equal(table[:, 0], roots)
    for row in table:
        mine = rings[rings[:, 0] == row[0]]
        assert int(mine[:, 4].sum()) == 2 * row[1]
        e = mine[mine[:, 1] == 4 * row[0]]
        assert len(e) == 1
        pts = verts[e[0, 3]:e[0, 3] + e[0, 2]]
        assert [pts[:, 1].min(), pts[:, 0].min(), pts[:, 1].max(), pts[:, 0].max()] == [row[2], row[3], row[4] + 1, row[5] + 1]
    return rings, verts, n_edges


@pytest.mark.parametrize("name", sorted(R.shape_cases()))
def test_restatement_on_the_case_table(name):
    _five_checks(R.shape_cases()[name])


def test_restatement_on_the_batch_case_and_a_sweep_of_random_masks():
    for m in R.batch_case():
        _five_checks(m)
    for shape in R.SWEEP_SHAPES:
        for k, pc in enumerate(R.SWEEP_PERCENT):
            _five_checks(R.random_mask(100 + 7 * shape[0] + k, shape[0], shape[1], pc))


def test_named_cases_have_the_stated_rings():
    c = R.shape_cases()
    t = lambda m: R.trace_tile(R.labels_of(m))       # noqa: E731
    rings, verts, ne = t(c["one_fg"])
    assert ne == 4 and rings.tolist() == [[0, 0, 4, 0, 2, 4, 0, 0]] and verts.tolist() == [[1, 0], [1, 1], [0, 1], [0, 0]]
    rings, verts, ne = t(c["one_bg"])
    assert ne == 0 and rings.shape == (0, 8) and verts.shape == (0, 2)
    for n in (126, 127, 128):
        rings, verts, ne = t(c["row_%d" % n])
        assert ne == 2 * n + 2 and rings[:, 5].tolist() == [2 * n + 2] and rings[0, 2] == 4 and rings[0, 4] == 2 * n
    rings, verts, ne = t(c["full_65x63"])
    assert rings.tolist() == [[0, 0, 4, 0, 2 * 65 * 63, 2 * (65 + 63), 0, 0]]
    assert verts.tolist() == [[63, 0], [63, 65], [0, 65], [0, 0]]
    rings, verts, ne = t(c["checker_8"])
    assert len(rings) == 32 and ne == 128 and np.all(rings[:, 2] == 4) and np.all(rings[:, 4] == 2)
    rings, verts, ne = t(c["serpentine_96"])
    assert len(rings) == 1 and ne == 9314 and rings[0, 2] == 194 and rings[0, 5] == 9314
    # two hole pixels that touch at a corner: one hole ring of 8 vertices through (2, 2) twice
    rings, verts, ne = t(c["diagonal_holes"])
    assert len(rings) == 2 and rings[:, 2].tolist() == [4, 8] and rings[:, 4].tolist() == [32, -4]
    assert verts[4:].tolist().count([2, 2]) == 2
    # two buildings that touch at a corner stay two rings; both pass (1, 1)
    rings, verts, ne = t(c["corner_touch"])
    assert len(rings) == 2 and rings[:, 4].tolist() == [2, 2] and verts.tolist().count([1, 1]) == 2
    rings, verts, ne = t(c["nested_17"])
    assert rings[:, 0].tolist() == [18, 18, 90, 90] and [int(np.sign(a)) for a in rings[:, 4]] == [1, -1, 1, -1]
    assert rings[:, 4].tolist() == [2 * 225, -2 * 121, 2 * 49, -2 * 9]
    # the batched form: tile-major rows, vertex offsets into one array
    counts, rings, verts, rc = R.trace(np.stack([R.labels_of(m) for m in R.batch_case()]))
    assert rc.tolist() == [2, 0, 3] and counts[1].tolist() == [0, 0] and rings[:, 6].tolist() == [0, 0, 2, 2, 2]
    assert rings[:, 3].tolist() == np.concatenate([[0], np.cumsum(rings[:, 2])[:-1]]).tolist()
    assert int(counts[:, 1].sum()) == len(verts) and len(verts) // 4 >= len(rings)


# ---- the writers ------------------------------------------------------------------------------------------------------------
POLY = {"root": 9, "exterior": [[6, 1], [6, 7], [1, 7], [1, 1]],
        "holes": [[[2, 2], [2, 3], [3, 3], [3, 2]], [[4, 4], [4, 6], [5, 6], [5, 4]]]}
SMALL = {"root": 70, "exterior": [[9, 8], [9, 9], [8, 9], [8, 8]], "holes": []}


def _record(i, y0, x0, y1, x1, damage):
    return {"id": i, "y0": y0, "x0": x0, "y1": y1, "x1": x1, "area": 7, "cy": 29 / 7, "cx": 0.5, "damage": damage, "n1": 1,
            "n2": 2, "n3": 0, "n4": 2, "n_other": 2, "confidence": 100000 / (65535 * 7)}


RECORDS = [_record(1, 1, 1, 6, 5, 3), _record(2, 8, 8, 8, 8, 0)]


def test_wkt_of_a_polygon_with_two_holes():
    from xview2_amd.utils import polygons as P
    assert P.to_wkt(POLY) == ("POLYGON ((6 1, 6 7, 1 7, 1 1, 6 1), (2 2, 2 3, 3 3, 3 2, 2 2), (4 4, 4 6, 5 6, 5 4, 4 4))")
    assert P.to_wkt(SMALL) == "POLYGON ((9 8, 9 9, 8 9, 8 8, 9 8))"


def test_geojson_and_xbd_json_are_byte_stable_and_carry_the_records(tmp_path):
    from xview2_amd.utils import polygons as P
    g, x = str(tmp_path / "b.geojson"), str(tmp_path / "scene_7.json")
    P.write_geojson(g, [POLY, SMALL], RECORDS)
    P.write_xbd_json(x, [POLY, SMALL], RECORDS)
    first = open(g, "rb").read(), open(x, "rb").read()
    P.write_geojson(g, [dict(POLY), dict(SMALL)], [dict(r) for r in RECORDS])
    P.write_xbd_json(x, [dict(POLY), dict(SMALL)], [dict(r) for r in RECORDS])
    assert (open(g, "rb").read(), open(x, "rb").read()) == first
    assert b"\r" not in first[0] + first[1] and first[0].endswith(b"]}\n") and first[1].endswith(b"]}}\n")
    doc = json.loads(first[0])
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 2
    f0 = doc["features"][0]
    assert f0["type"] == "Feature" and f0["geometry"]["type"] == "Polygon"
    assert f0["geometry"]["coordinates"] == [r + r[:1] for r in [POLY["exterior"]] + POLY["holes"]]
    assert f0["properties"] == dict(RECORDS[0], damage_name="major-damage")
    assert list(f0["properties"])[:6] == ["id", "y0", "x0", "y1", "x1", "area"]          # the record's own key order
    assert doc["features"][1]["properties"]["damage_name"] == "un-classified"
    assert ('"cy": %r' % (29 / 7)).encode() in first[0]                                   # floats as repr
    xbd = json.loads(first[1])
    assert list(xbd) == ["features"] and list(xbd["features"]) == ["xy"]
    assert xbd["features"]["xy"][0] == {"properties": {"feature_type": "building", "subtype": "major-damage",
                                                       "uid": "scene_7-1"}, "wkt": P.to_wkt(POLY)}
    assert xbd["features"]["xy"][1]["properties"]["subtype"] == "un-classified"
    assert P.DAMAGE_NAMES == ("un-classified", "no-damage", "minor-damage", "major-damage", "destroyed")
    # without records: id and root
    P.write_geojson(g, [POLY, SMALL])
    assert [f["properties"] for f in json.load(open(g))["features"]] == [{"id": 1, "root": 9}, {"id": 2, "root": 70}]
    P.write_geojson(g, [])
    assert open(g).read() == '{"type": "FeatureCollection", "features": [\n]}\n'
    P.write_xbd_json(x, [], [])
    assert json.load(open(x)) == {"features": {"xy": []}}


def test_records_that_do_not_match_raise(tmp_path):
    from xview2_amd.utils import polygons as P
    g = str(tmp_path / "b.geojson")
    with pytest.raises(ValueError, match="2 polygons but 1 building records"):
        P.write_geojson(g, [POLY, SMALL], RECORDS[:1])
    with pytest.raises(ValueError, match="order"):
        P.write_geojson(g, [POLY, SMALL], RECORDS[::-1])
    with pytest.raises(ValueError, match="order"):
        P.write_xbd_json(g, [POLY, SMALL], RECORDS[::-1])
    with pytest.raises(ValueError, match="records"):
        P.write_xbd_json(g, [POLY], None)


def test_grouping_rings_by_root():
    from xview2_amd.utils import polygons as P
    lab = R.labels_of(R.shape_cases()["nested_17"])
    rings, verts, _ = R.trace_tile(lab)
    polys = P.group_rings(rings, verts)
    assert polys == R.polygons(rings, verts) and [p["root"] for p in polys] == [18, 90]
    assert [len(p["holes"]) for p in polys] == [1, 1] and polys[0]["exterior"] == [[16, 1], [16, 16], [1, 16], [1, 1]]
    # a later tile of a batch (offsets into a shared vertex array, given as a list), and rings without their exterior
    shared = [[0, 0]] * 100 + verts.tolist()
    assert P.group_rings(rings + np.array([0, 0, 0, 100, 0, 0, 0, 0]), shared) == polys
    with pytest.raises(ValueError, match="no exterior"):
        P.group_rings(rings[1:], verts)
    assert P.group_rings(np.zeros((0, 8), np.int64), np.zeros((0, 2), np.int32)) == []


# ---- ABI, flags, no GPU -----------------------------------------------------------------------------------------------------
def test_header_declares_the_two_calls_and_their_workspace_queries():
    from xview2_amd import _capi, _lib
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    protos = _capi._parse_header()
    assert protos["xv2_polygon_count"] == (I, [P, I, I, I, P, P, P])
    assert protos["xv2_polygon_trace"] == (I, [P, I, I, I, I64, I64, P, P, P, P, P, P])
    assert protos["xv2_polygon_count_workspace"] == (ctypes.c_size_t, [I, I, I])
    assert protos["xv2_polygon_trace_workspace"] == (ctypes.c_size_t, [I, I, I, I64])
    assert "polygons.hip" in _lib.SOURCES
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "xv2.h")).read()
    assert "#define XV2_POLYGON_RING_COLS 8" in hdr
    _lib.build()
    qc = lambda *a: _capi.query("xv2_polygon_count_workspace", *a)     # noqa: E731
    qt = lambda *a: _capi.query("xv2_polygon_trace_workspace", *a)     # noqa: E731
    assert qc(2, 100, 70) >= 8 * 2 * 7 and qc(2, 100, 70) % 256 == 0 and qc(1, 1, 1) > 0
    assert qc(0, 4, 4) == 0 and qc(1, 1 << 15, 1 << 15) == 0 and qc(65536, 4, 4) == 0
    assert qt(0, 4, 4, 4) == 0 and qt(1, 1 << 15, 1 << 15, 4) == 0 and qt(65536, 4, 4, 4) == 0
    assert qt(1, 4, 4, -1) == 0 and qt(1, 4, 4, 1 << 31) == 0 and qt(1, 4, 4, 0) > 0
    assert qt(2, 100, 70, 5000) >= 4 * 2 * 100 * 70 + 64 * 5000 and qt(2, 100, 70, 5000) % 256 == 0
    assert qt(2, 100, 70, 5000) > qt(2, 100, 70, 4000)
    # argument checks are reachable without a GPU
    one = ctypes.c_void_p(8)
    err = _lib.lib().xv2_last_error
    f = _capi._func("xv2_polygon_count")
    for args, msg in (((one, 0, 4, 4, one, one, None), b"positive"),
                      ((one, 1, 1 << 15, 1 << 15, one, one, None), b"2^30"),
                      ((one, 65536, 4, 4, one, one, None), b"too large"),
                      ((None, 1, 4, 4, one, one, None), b"null"),
                      ((one, 1, 4, 4, None, one, None), b"null"),
                      ((one, 1, 4, 4, one, None, None), b"null")):
        assert f(*args) == 1 and msg in err(), (args, err())
    f = _capi._func("xv2_polygon_trace")
    for args, msg in (((one, 1, 0, 4, 4, 4, one, one, one, one, one, None), b"positive"),
                      ((one, 1, 4, 4, -1, 0, one, one, one, one, one, None), b"total_edges"),
                      ((one, 1, 4, 4, 1 << 31, 4, one, one, one, one, one, None), b"total_edges"),
                      ((one, 1, 4, 4, 4, 8, one, one, one, one, one, None), b"total_vertices"),
                      ((None, 1, 4, 4, 4, 4, one, one, one, one, one, None), b"null"),
                      ((one, 1, 4, 4, 4, 4, None, one, one, one, one, None), b"null"),
                      ((one, 1, 4, 4, 4, 4, one, None, one, one, one, None), b"null"),
                      ((one, 1, 4, 4, 4, 4, one, one, None, one, one, None), b"null"),
                      ((one, 1, 4, 4, 4, 4, one, one, one, None, one, None), b"null"),
                      ((one, 1, 4, 4, 4, 4, one, one, one, one, None, None), b"null")):
        assert f(*args) == 1 and msg in err(), (args, err())


def test_a_missing_gpu_is_a_loud_error():
    import torch
    from xview2_amd import ops
    from xview2_amd.utils import polygons as P
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.building_polygons(torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polygon_count(torch.zeros((1, 4, 4), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polygon_trace(torch.zeros((1, 4, 4), dtype=torch.int32), 0, 0)


def test_cli_flags_and_argument_errors():
    from xview2_amd import predict
    from xview2_amd.utils import polygons as P
    from xview2_amd.utils import post_process
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o"])
    assert a.polygons is False and a.buildings is False
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--polygons"])
    assert a.polygons is True
    assert post_process.get_parser().parse_args([]).polygons is False
    assert post_process.get_parser().parse_args(["--polygons"]).polygons is True
    for argv in ([], ["a.png", "b.png"], ["a.png", "b.png", "c.geojson", "d"]):
        with pytest.raises(SystemExit, match="usage: python -m xview2_amd.utils.polygons PRE.png POST.png OUT.geojson"):
            P.main(argv)
    import inspect
    from xview2_amd.utils import buildings
    assert inspect.signature(buildings.building_table).parameters["return_labels"].default is False
