"""The rule of the tolerance simplification (include/xv2.h xv2_polygon_simplify) on the host restatement of
tests/simplify_ref.py, over the whole case table at every q of it, and the host layers of the feature: the quantised
tolerance, the relaxed record match, the files and the command-line flags.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

import polygons_ref as R
import simplify_ref as S

CASES = sorted(S.cases())


def _rings_of(rows, verts):
    v = np.asarray(verts).tolist()
    return [[tuple(p) for p in v[r[3]:r[3] + r[2]]] for r in np.asarray(rows).tolist()]


def _is_subsequence_from_first(kept, pts):
    it = iter(pts)
    return (not pts and not kept) or (kept[:1] == pts[:1] and all(any(k == p for p in it) for k in kept))


def _within_tolerance(pts, kept, q):
    """every input vertex lies within T of some segment of the output ring: first the segment that spans it in ring order,
    which is the one the rule dropped it for, then any"""
    closed = kept + kept[:1]
    segs = list(zip(closed, closed[1:]))
    j = 0
    for p in pts:
        if j + 1 < len(kept) and p == kept[j + 1]:
            j += 1
        if p == kept[j] or S.within(segs[j][0], segs[j][1], p, q):
            continue
        if not any(S.within(a, b, p, q) for a, b in segs):
            return False
    return True


@pytest.mark.parametrize("q", S.QS)
@pytest.mark.parametrize("name", CASES)
def test_the_restatement_keeps_the_rules_promises(name, q):
    rings, verts, traced = S.cases()[name]
    out_r, out_v, total = S.expected(name, q)
    assert total == len(out_v) == int(out_r[:, 2].sum()) and len(out_r) == len(rings)
    assert np.array_equal(out_r[:, [0, 1, 5, 6]], rings[:, [0, 1, 5, 6]])
    assert np.array_equal(out_r[:, 3], np.cumsum(out_r[:, 2]) - out_r[:, 2])
    for row, pts, kept in zip(out_r.tolist(), _rings_of(rings, verts), _rings_of(out_r, out_v)):
        n, flag = len(pts), row[7]
        assert _is_subsequence_from_first(kept, pts)
        ext = max(max(p[0] for p in pts) - min(p[0] for p in pts), max(p[1] for p in pts) - min(p[1] for p in pts)) if n else 0
        assert (flag == 2) == (ext > S.EXT_MAX)
        assert len(kept) >= 3 or flag == 1
        if flag:
            assert kept == pts
        if n < 3 or len(set(pts)) == 1:
            assert flag in (1, 2)
        assert row[4] == R.shoelace(kept)
        assert (row[4] > 0) == (R.shoelace(pts) > 0) and (row[4] < 0) == (R.shoelace(pts) < 0)
        assert _within_tolerance(pts, kept, q)
        if traced and q == 0:
            assert kept == pts and flag == 0


def test_traced_tables_are_unchanged_at_q_0():
    for name in CASES:
        rings, verts, traced = S.cases()[name]
        if traced:
            out_r, out_v, total = S.expected(name, 0)
            assert np.array_equal(out_r, rings) and np.array_equal(out_v, verts) and total == len(verts)


def test_named_cases_do_what_they_are_there_for():
    flags = lambda name, q: S.expected(name, q)[0][:, 7].tolist()      # noqa: E731
    assert flags("tiny", 16) == [1, 1, 1, 0, 1, 1] and flags("tiny", 64) == [1] * 6      # the triangle collapses at T = 4
    assert flags("extent", 16) == [0, 2, 2, 0, 2]
    assert S.expected("extent", 8)[0][:, 2].tolist() == [6, 7, 7, 6, 7] and S.expected("extent", 16)[0][:, 2].tolist() == [4, 7, 7, 4, 7]
    # the tie: the lowest index goes first, and at T = 4 that decides what survives
    assert S.simplify_ring(S.tie_ring(), 64)[0] == [(0, 0), (3, 6), (60, 0), (30, -40)]
    assert S.simplify_ring(S.tie_ring(), 64, tie_high=True)[0] == S.tie_ring()
    # the zigzag needs about n rounds in the level-synchronous form, the circle about log n
    assert S.simplify_ring(S.zigzag(300), 16)[2] == 298 and S.simplify_ring(S.circle(5000, 16000, 7), 16)[2] < 30
    assert len(S.square_spiral(200)) == 200 and len(S.zigzag(300)) == 300
    assert S.simplify_ring(S.zigzag_linear(1100), 64)[1:] == (0, 1098)
    # the sizes on either side of both path thresholds
    assert S.cases()["thresholds"][0][:, 2].tolist() == [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025]
    assert len(S.cases()["mixed"][0]) > 300 and set(S.cases()["mixed"][0][:, 6].tolist()) == {0, 2, 3, 5}
    # the rotated, round and jagged rings do get simpler
    assert S.expected("circle_5000", 16)[2] < 4000 and S.expected("circle_5000", 64)[2] < 1300
    assert S.expected("mixed", 16)[2] < len(S.cases()["mixed"][1])


@pytest.mark.parametrize("name", S.TRANSLATED)
@pytest.mark.parametrize("q", S.QS)
def test_a_translated_table_gives_the_translated_result(name, q):
    near, far = S.expected(name, q), S.expected(name + "_far", q)
    assert np.array_equal(far[1], near[1] + S.FAR) and far[2] == near[2]
    assert np.array_equal(far[0][:, [2, 3, 7]], near[0][:, [2, 3, 7]])


def test_the_key_is_the_squared_distance_to_the_segment_times_its_scale():
    A, B = (0, 0), (10, 0)
    assert S.key_scale(A, B, (4, 3)) == (900, 100)                      # 3^2 * 100: beside the segment
    assert S.key_scale(A, B, (-3, 4)) == (2500, 100)                    # before A: 5^2 * 100
    assert S.key_scale(A, B, (13, -4)) == (2500, 100)                   # past B
    assert S.key_scale(A, A, (3, 4)) == (25, 1)                         # both ends one point
    assert S.key_scale(A, B, A) == (0, 100) and S.key_scale(A, B, B) == (0, 100)
    # key > (q^2 scale) >> 8 is dist > q / 16: at distance 3, T = 3 keeps nothing and T just below 3 does
    assert S.within(A, B, (4, 3), 48) and not S.within(A, B, (4, 3), 47)


# ---- the host layers -------------------------------------------------------------------------------------------------------
def test_quantise_tolerance():
    from xview2_amd.utils import polygons as P
    assert [P.quantise_tolerance(t) for t in (0, 0.0, 0.03, 0.5, 1, 1.5, 2, 4, 4095.9)] == [0, 0, 0, 8, 16, 24, 32, 64, 65534]
    assert P.quantise_tolerance(0.03125) == 1 and P.quantise_tolerance(4095.99) == 65535
    for bad in (-0.1, 4096, 1e9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="0 <= T < 4096"):
            P.quantise_tolerance(bad)


def _record(i, y0, x0, y1, x1):
    return {"id": i, "y0": y0, "x0": x0, "y1": y1, "x1": x1, "area": 1, "cy": 0.0, "cx": 0.0, "damage": 1}


def test_the_record_match_allows_a_simplified_exterior_to_fall_short_by_ceil_T():
    from xview2_amd.utils import polygons as P
    rec = [_record(1, 10, 20, 29, 49)]                                    # the box of corners y 10..30, x 20..50
    poly = lambda x0, y0, x1, y1, **kw: dict({"root": 5, "exterior": [[x0, y0], [x1, y0], [x1, y1], [x0, y1]], "holes": []}, **kw)  # noqa: E731
    assert P._match([poly(20, 10, 50, 30)], rec) == rec
    assert P._match([poly(20, 10, 50, 30, simplified=24)], rec) == rec
    # T = 1.5 (q = 24): up to 2 pixels short on any side, not 3, and never outside
    assert P._match([poly(22, 12, 48, 28, simplified=24)], rec) == rec
    for bad in (poly(23, 10, 50, 30, simplified=24), poly(20, 13, 50, 30, simplified=24), poly(20, 10, 47, 30, simplified=24),
                poly(20, 10, 50, 27, simplified=24), poly(19, 10, 50, 30, simplified=24), poly(20, 9, 50, 30, simplified=24),
                poly(20, 10, 51, 30, simplified=24), poly(20, 10, 50, 31, simplified=24)):
        with pytest.raises(ValueError, match="order"):
            P._match([bad], rec)
    # q = 16 is exactly one pixel; a polygon without the key is held to the box itself
    assert P._match([poly(21, 11, 49, 29, simplified=16)], rec) == rec
    for bad in (poly(22, 10, 50, 30, simplified=16), poly(21, 10, 50, 30), poly(20, 10, 50, 29)):
        with pytest.raises(ValueError, match="order"):
            P._match([bad], rec)


def test_geojson_of_simplified_polygons_has_closed_rings_of_at_least_4_positions(tmp_path):
    from xview2_amd.utils import polygons as P
    rings, verts, _ = S.cases()["shape_random_33x47_p50"]
    polys = S.polygons_of(rings, verts, 24)
    assert len(polys) == len(R.polygons(rings, verts)) and all(p["simplified"] == 24 for p in polys)
    assert sum(len(p["exterior"]) for p in polys) < sum(len(p["exterior"]) for p in R.polygons(rings, verts))
    g = str(tmp_path / "s.geojson")
    P.write_geojson(g, polys)
    doc = json.load(open(g))
    assert len(doc["features"]) == len(polys)
    for f, p in zip(doc["features"], polys):
        coords = f["geometry"]["coordinates"]
        assert len(coords) == 1 + len(p["holes"]) and coords[0][:-1] == [list(v) for v in p["exterior"]]
        for ring in coords:
            assert len(ring) >= 4 and ring[0] == ring[-1]
    assert "simplified" not in doc["features"][0]["properties"]
    assert P.to_wkt(polys[0]).startswith("POLYGON ((")


def test_the_three_parsers_know_simplify():
    from xview2_amd import predict
    from xview2_amd.utils import polygons as P
    from xview2_amd.utils import post_process
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o"]).simplify == 0.0
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--polygons", "--simplify", "1.5"]).simplify == 1.5
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--simplify", "1"]).polygons is False      # implies nothing
    assert post_process.get_parser().parse_args([]).simplify == 0.0
    assert post_process.get_parser().parse_args(["--polygons", "--simplify", "0.5"]).simplify == 0.5
    a = P.get_parser().parse_args(["a.png", "b.png", "c.geojson"])
    assert (a.pre, a.post, a.out, a.simplify) == ("a.png", "b.png", "c.geojson", 0.0)
    assert P.get_parser().parse_args(["a.png", "b.png", "c.geojson", "--simplify", "2"]).simplify == 2.0
    with pytest.raises(SystemExit, match=r"usage: python -m xview2_amd.utils.polygons PRE.png POST.png OUT.geojson \[--simplify T\]"):
        P.main(["a.png", "b.png", "c.geojson", "--simplify"])
    with pytest.raises(ValueError, match="0 <= T < 4096"):
        P.main(["a.png", "b.png", "c.geojson", "--simplify", "-1"])
    import inspect
    assert inspect.signature(P.building_polygons).parameters["simplify"].default == 0.0


def test_header_declares_the_call_and_its_workspace_query():
    from xview2_amd import _capi, _lib
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    protos = _capi._parse_header()
    assert protos["xv2_polygon_simplify"] == (I, [P, P, I64, I64, I, P, P, P, P, P])
    assert protos["xv2_polygon_simplify_workspace"] == (ctypes.c_size_t, [I64, I64])
    assert "simplify.hip" in _lib.SOURCES
    _lib.build()
    qs = lambda *a: _capi.query("xv2_polygon_simplify_workspace", *a)     # noqa: E731
    assert qs(0, 0) > 0 and qs(10, 100) >= 44 * 100 + 24 * 10 and qs(10, 200) > qs(10, 100) and qs(1000, 100) >= qs(1, 100) + 24 * 999 - 1024
    assert qs(-1, 4) == 0 and qs(1, -4) == 0 and qs(1 << 31, 4) == 0 and qs(1, 1 << 31) == 0
    # argument checks are reachable without a GPU: nothing is enqueued
    one = ctypes.c_void_p(8)
    err = _lib.lib().xv2_last_error
    f = _capi._func("xv2_polygon_simplify")
    for args, msg in (((one, one, -1, 4, 16, one, one, one, one, None), b"outside 0 .. 2^31 - 1"),
                      ((one, one, 1, 1 << 31, 16, one, one, one, one, None), b"outside 0 .. 2^31 - 1"),
                      ((one, one, 1, 4, -1, one, one, one, one, None), b"q=-1"),
                      ((one, one, 1, 4, 65536, one, one, one, one, None), b"q=65536"),
                      ((one, one, 1, 4, 16, None, one, one, one, None), b"null"),
                      ((one, one, 1, 4, 16, one, one, one, None, None), b"null"),
                      ((None, one, 1, 4, 16, one, one, one, one, None), b"null"),
                      ((one, None, 1, 4, 16, one, one, one, one, None), b"null"),
                      ((one, one, 1, 4, 16, one, None, one, one, None), b"null"),
                      ((one, one, 1, 4, 16, one, one, None, one, None), b"null"),
                      ((one, ctypes.c_void_p(12), 1, 4, 16, one, one, one, one, None), b"8-byte aligned")):
        assert f(*args) == 1 and msg in err(), (args, err())


def test_a_missing_gpu_is_a_loud_error():
    import torch
    from xview2_amd import ops
    from xview2_amd.utils import polygons as P
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.building_polygons(torch.zeros((4, 4), dtype=torch.uint8), simplify=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polygon_simplify(torch.zeros((1, 8), dtype=torch.int64), torch.zeros((4, 2), dtype=torch.int32), 1, 16)
