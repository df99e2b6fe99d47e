"""Polygons -> masks on the host: the two restatements of the contract against each other (tests/rasterize_ref.py), the WKT /
xBD / GeoJSON readers, the rounding rules, the packing of utils/rasterize.py, the round trip label map -> rings -> raster on
the host, and the C ABI's new entry points.  Every comparison is ==."""
import ctypes
import json

import numpy as np
import pytest

import polygons_ref as PR
import rasterize_ref as R

SMALL = [(24, 24), (17, 23)]


def _rz():
    from xview2_amd.utils import rasterize
    return rasterize


# ---- ref == brute force ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,off", R.SAMPLINGS)
@pytest.mark.parametrize("H,W", SMALL)
def test_ref_equals_brute_force_on_every_case(H, W, k, off):
    rz = _rz()
    for name, tiles in R.cases(H, W, k, off).items():
        T = rz.pack_rings(tiles, H, W, k, off)
        got, want = R.ref(T, H, W), R.brute(tiles, H, W, k, off)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())
        if name == "outside":
            assert T.n_features == 0 and T.n_work == 0 and not want.any()
        elif name == "whole_tile":
            assert (want == 7).all()
        elif name == "empty_middle":
            assert want[0].any() and not want[1].any() and want[2].any()
        else:
            assert want.any(), name
    c = R.cases(H, W, k, off)
    assert np.array_equal(R.brute(c["ring_cw"], H, W, k, off), R.brute(c["ring_ccw"], H, W, k, off))
    bow = R.brute(c["bow_tie"], H, W, k, off)[0]              # the two lobes beside the crossing, not above or below it
    assert bow[H // 2, 3] != 0 and bow[H // 2, W - 5] != 0 and bow[3, W // 2] == 0 and bow[H - 5, W // 2] == 0


def test_ref_equals_brute_force_on_the_special_rings():
    rz = _rz()
    for tiles, H, W, k, off in [(R.painter_overlap(), 40, 44, 1, 1), (R.painter_twins(), 36, 36, 1, 1),
                                (R.window_boxes(), 40, 70, 1, 1), (R.far_triangle(0, 0), 24, 24, 0, 0),
                                (R.far_triangle(1, 1), 24, 24, 1, 1), (R.painter_pixels(300, 12, 80), 12, 80, 1, 1)]:
        T = rz.pack_rings(tiles, H, W, k, off)
        assert np.array_equal(R.ref(T, H, W), R.brute(tiles, H, W, k, off))
    over = R.brute(R.painter_overlap(), 40, 44, 1, 1)[0]
    assert over[3, 3] == 3 and over[10, 12] == 255 and over[15, 12] == 1 and over[25, 35] == 255 and over[0, 0] == 0
    assert set(np.unique(R.brute(R.painter_twins(), 36, 36, 1, 1))) == {0, 200}
    far = R.brute(R.far_triangle(0, 0), 24, 24, 0, 0)[0]
    assert far.any() and not far.all()


@pytest.mark.parametrize("n_edges", [255, 256, 257, 513])
def test_ref_equals_brute_force_on_the_stage_size_rings(n_edges):
    """the device test compares these rings with ref, which shares the packing with the call; the brute force shares nothing"""
    tiles = R.comb(n_edges)
    T = _rz().pack_rings(tiles, 64, 64, 8, 128)
    assert T.n_edges == n_edges
    assert np.array_equal(R.ref(T, 64, 64), R.brute(tiles, 64, 64, 8, 128))


# ---- readers -----------------------------------------------------------------------------------------------------------------
def test_parse_wkt():
    rz = _rz()
    p = rz.parse_wkt("POLYGON ((0 0, 4 0, 4 3, 0 0))")
    assert p == {"exterior": [[0.0, 0.0], [4.0, 0.0], [4.0, 3.0]], "holes": []}
    p = rz.parse_wkt("polygon((0 0,10 0,10 10,0 10,0 0),(2 2,4 2,4 4,2 2), (5 5, 6 5, 6 6, 5 6))")
    assert len(p["exterior"]) == 4 and p["holes"] == [[[2.0, 2.0], [4.0, 2.0], [4.0, 4.0]],
                                                      [[5.0, 5.0], [6.0, 5.0], [6.0, 6.0], [5.0, 6.0]]]
    assert rz.parse_wkt("POLYGON EMPTY") is None
    p = rz.parse_wkt("POLYGON ((1.5e2 -2.5E-1, 3e0 4, .5 6.25, 1.5e2 -2.5E-1))")
    assert p["exterior"] == [[150.0, -0.25], [3.0, 4.0], [0.5, 6.25]]
    for bad in ("MULTIPOLYGON (((0 0, 1 0, 1 1, 0 0)))", "POINT (1 2)", "POLYGON ((0 0, 1 1, 0 0))", "POLYGON ((0 0, 1 x, 2 2))",
                "POLYGON (((0 0, 1 0, 1 1)))", "POLYGON ()", "LINESTRING (0 0, 1 1)", ""):
        with pytest.raises(ValueError) as e:
            rz.parse_wkt(bad)
        assert repr(bad) in str(e.value)


def test_rounding_rules():
    rz = _rz()
    assert rz.quantise([0.5, 1.5, 2.5, -0.5, -1.5, 2.49, 2.51], "reference").tolist() == [0, 2, 2, 0, -2, 2, 3]
    # 1/256 px: 3 / 512 is half a unit above 1 (-> 2, even), 1 / 512 half a unit above 0 (-> 0), 5 / 512 -> 2
    assert rz.quantise([1.0, 3 / 512, 1 / 512, 5 / 512, 0.3, -7.25], "exact").tolist() == [256, 2, 0, 2, 77, -1856]
    assert rz.quantise([[3, 4], [0, 7]], "corner").tolist() == [[6, 8], [0, 14]]
    with pytest.raises(ValueError, match="integer corner"):
        rz.quantise([1.25], "corner")
    with pytest.raises(ValueError, match="unknown rule"):
        rz.pack([[]], 8, 8, "nearest")


def _scene():
    import buildings_ref as BR
    mask = BR.blobs(61, 40, 52, thresh=0.5)
    post = np.where(mask, 1 + BR._hash(62, (40, 52), 4), 0).astype(np.uint8)
    return mask.astype(np.uint8), post


def _polys_records(pre, post):
    import buildings_ref as BR
    from xview2_amd.utils import buildings
    _, rings, verts, _ = PR.trace(PR.labels_of(pre)[None])
    return PR.polygons(rings, verts), buildings.to_records(BR.table(pre, post), pre.shape[0], pre.shape[1], confidence=False)


def test_readers_take_what_the_writers_write(tmp_path):
    from xview2_amd.utils import polygons
    rz = _rz()
    pre, post = _scene()
    polys, records = _polys_records(pre, post)
    assert len(polys) > 3 and sum(len(p["holes"]) for p in polys) > 0
    polygons.write_geojson(str(tmp_path / "a.geojson"), polys, records)
    polygons.write_xbd_json(str(tmp_path / "a.json"), polys, records)
    want = [({"exterior": [[float(x), float(y)] for x, y in p["exterior"]],
              "holes": [[[float(x), float(y)] for x, y in h] for h in p["holes"]]}, r["damage"]) for p, r in zip(polys, records)]
    assert rz.read_geojson(str(tmp_path / "a.geojson")) == want
    sub = {0: 255, 1: 1, 2: 2, 3: 3, 4: 4}
    assert rz.read_xbd_json(str(tmp_path / "a.json"), "post") == [(p, sub[v]) for p, v in want]
    assert rz.read_xbd_json(str(tmp_path / "a.json"), "pre") == [(p, 1) for p, _ in want]
    # without records the GeoJSON has no damage property: every feature paints 1
    polygons.write_geojson(str(tmp_path / "b.geojson"), polys)
    assert rz.read_geojson(str(tmp_path / "b.geojson")) == [(p, 1) for p, _ in want]


def test_xbd_subtypes_and_their_errors(tmp_path):
    rz = _rz()
    names = ["no-damage", "minor-damage", "major-damage", "destroyed", "un-classified"]
    feats = [{"properties": {"feature_type": "building", "subtype": s, "uid": "u%d" % i},
              "wkt": "POLYGON ((%d 1, %d 1, %d 5, %d 1))" % (i, i + 3, i + 3, i)} for i, s in enumerate(names)]
    feats.insert(2, {"properties": {"subtype": "destroyed", "uid": "none"}, "wkt": "POLYGON EMPTY"})
    path = str(tmp_path / "x_post_disaster.json")
    json.dump({"features": {"lng_lat": [], "xy": feats}, "metadata": {}}, open(path, "w"))
    assert [v for _, v in rz.read_xbd_json(path, "post")] == [1, 2, 3, 4, 255]
    assert [v for _, v in rz.read_xbd_json(path, "pre")] == [1] * 5
    for props in ({"uid": "abc-7"}, {"uid": "abc-7", "subtype": "flattened"}):
        json.dump({"features": {"xy": [{"properties": props, "wkt": "POLYGON ((0 0, 1 0, 1 1, 0 0))"}]}}, open(path, "w"))
        with pytest.raises(ValueError) as e:
            rz.read_xbd_json(path, "post")
        assert path in str(e.value) and "abc-7" in str(e.value)
        assert len(rz.read_xbd_json(path, "pre")) == 1          # pre files carry no subtype
    # the CLI's reader: a file without any subtype is a pre-disaster file and paints 1 into both maps; one unknown subtype is an error
    json.dump({"features": {"xy": [{"properties": {"uid": "abc-7"}, "wkt": "POLYGON ((0 0, 1 0, 1 1, 0 0))"}]}}, open(path, "w"))
    pre, post, is_xbd = rz.read_features(path)
    assert is_xbd and pre == post and [v for _, v in post] == [1]
    json.dump({"features": {"xy": feats}}, open(path, "w"))
    pre, post, is_xbd = rz.read_features(path)
    assert is_xbd and [v for _, v in pre] == [1] * 5 and [v for _, v in post] == [1, 2, 3, 4, 255]


# ---- packing -----------------------------------------------------------------------------------------------------------------
def test_pack_boxes_windows_and_tile_order():
    rz = _rz()
    H, W = 70, 90
    sq = lambda x0, y0, x1, y1: {"exterior": [[x0, y0], [x1, y0], [x1, y1], [x0, y1]], "holes": [[[x0 + 1, y0 + 1], [x0 + 2, y0 + 1],
                                                                                                 [x0 + 2, y0 + 2]]]}
    tiles = [[(sq(-10, -5, 40.4, 33.6), 1), (sq(200, 5, 230, 9), 2), (sq(50, 60, 300, 300), 3)], [],
             [(sq(0, 0, 90, 70), 4), (sq(3.5, 4.5, 3.5, 4.5), 5), (sq(10, -9, 20, -2), 6)]]
    for rule in ("reference", "corner", "exact"):
        if rule == "corner":
            with pytest.raises(ValueError, match="integer corner"):
                rz.pack(tiles, H, W, rule)
            ts = [[({"exterior": np.floor(p["exterior"]).tolist(), "holes": [np.floor(h).tolist() for h in p["holes"]]}, v)
                   for p, v in t] for t in tiles]
        else:
            ts = tiles
        T = rz.pack(ts, H, W, rule)
        k, off, holes = rz.RULES[rule]
        assert (T.frac_bits, T.off, T.B) == (k, off, 3) and T.tables.dtype == np.int32
        assert T.tables.size == 4 * T.n_edges + 8 * T.n_features + 4 * T.n_work
        f = T.features
        # the features outside the tile are dropped, the rest keep tile and file order
        assert f[:, 1].tolist() == [1, 3, 4, 5] and f[:, 0].tolist() == [0, 0, 2, 2]
        assert (f[:, 3] == (7 if holes else 4)).all()
        assert (f[:, 4] >= 0).all() and (f[:, 5] >= 0).all() and (f[:, 6] < W).all() and (f[:, 7] < H).all()
        assert (f[:, 4] <= f[:, 6]).all() and (f[:, 5] <= f[:, 7]).all()
        # the box is the pixels whose sample lies in the extent of the feature's own edges
        for row in f.tolist():
            e = T.edges[row[2]:row[2] + row[3]].astype(np.int64)
            xs, ys = e[:, [0, 2]], e[:, [1, 3]]
            px = [x for x in range(W) if xs.min() <= (x << k) + off <= xs.max()]
            py = [y for y in range(H) if ys.min() <= (y << k) + off <= ys.max()]
            assert row[4:] == [px[0], py[0], px[-1], py[-1]]
        # every pixel of every clipped box lies in exactly one window of its feature
        for i, row in enumerate(f.tolist()):
            cnt = np.zeros((H, W), dtype=int)
            for _, wx, wy, zero in T.work[T.work[:, 0] == i].tolist():
                assert zero == 0 and row[4] <= wx <= row[6] and row[5] <= wy <= row[7]
                cnt[wy:min(wy + 32, row[7] + 1), wx:min(wx + 32, row[6] + 1)] += 1
            want = np.zeros((H, W), dtype=int)
            want[row[5]:row[7] + 1, row[4]:row[6] + 1] = 1
            assert np.array_equal(cnt, want)
        assert (np.diff(T.work[:, 0]) >= 0).all()
    assert rz.pack([[], []], 8, 8, "exact").tables.size == 0
    with pytest.raises(ValueError, match="2\\^24"):
        rz.pack([[(sq(0, 0, 70000, 5), 1)]], 8, 8, "exact")
    with pytest.raises(ValueError, match="0..255"):
        rz.pack([[(sq(0, 0, 7, 5), 256)]], 8, 8, "exact")


# ---- the round trip on the host ------------------------------------------------------------------------------------------------
def _round_trip(mask):
    rz = _rz()
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    _, rings, verts, _ = PR.trace(PR.labels_of(mask)[None])
    polys = PR.polygons(rings, verts)
    T = rz.pack([[(p, 1) for p in polys]], H, W, "corner")
    return R.ref(T, H, W)[0], len(polys)


@pytest.mark.parametrize("name", sorted(PR.shape_cases()))
def test_label_map_to_rings_to_raster_is_the_identity(name):
    mask = PR.shape_cases()[name]
    got, _ = _round_trip(mask)
    assert np.array_equal(got, mask.astype(np.uint8))


def test_round_trip_of_a_random_mask_with_holes():
    mask = PR.random_mask(77, 40, 52, 55)
    got, n = _round_trip(mask)
    assert n > 20 and np.array_equal(got, mask.astype(np.uint8))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_built_and_bounded():
    from xview2_amd import _capi, _lib
    names = _lib.declared_symbols()
    assert "xv2_rasterize_polygons" in names and "xv2_rasterize_workspace" in names
    lib = ctypes.CDLL(_lib.build())
    assert hasattr(lib, "xv2_rasterize_polygons") and hasattr(lib, "xv2_rasterize_workspace")
    assert "rasterize.hip" in _lib.SOURCES
    q = lambda *a: int(_capi.query("xv2_rasterize_workspace", *a))
    assert q(1, 1, 1) == 4 and q(3, 37, 53) == 4 * 3 * 37 * 53 and q(65535, 8, 8) == 4 * 65535 * 64
    assert q(32, 1024, 1024) == 4 * 32 * 1024 * 1024
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (65536, 8, 8), (1, 1 << 15, 1 << 15), (1, 1 << 30, 1)):
        assert q(*bad) == 0, bad
    assert q(1, (1 << 15) - 1, 1 << 15) > 0


def test_tables_are_rejected_before_anything_runs():
    """the validation of the host copy needs no device: every call here returns XV2_EINVAL before a launch"""
    from xview2_amd import _capi, _lib
    rz = _rz()
    T = rz.pack_rings(R.painter_overlap(), 40, 44, 1, 1)
    f = _capi._func("xv2_rasterize_polygons")

    import torch
    spare = np.zeros(64, dtype=np.int64)

    def rc(tables, ne=T.n_edges, nf=T.n_features, nw=T.n_work, k=1, off=1, B=1, H=40, W=44):
        host = np.ascontiguousarray(tables, dtype=np.int32)
        if torch.cuda.is_available():
            # with a device present a call that were wrongly accepted would launch: give it real buffers of the sizes it names
            px = max(B, 1) * max(H, 1) * max(W, 1)
            dev, ws = torch.from_numpy(host).cuda(), torch.empty(4 * px, dtype=torch.uint8, device="cuda")
            out = torch.empty(px, dtype=torch.uint8, device="cuda")
            ptrs = dev.data_ptr(), ws.data_ptr(), out.data_ptr()
        else:
            # no device: nothing can be launched, the pointers only have to be non-null and aligned
            ptrs = (spare.ctypes.data // 16 * 16 + 16,) * 3
        code = f(ptrs[0], host.ctypes.data, ne, nf, nw, k, off, B, H, W, ptrs[1], ptrs[2], None)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        return code, _lib.lib().xv2_last_error().decode()

    def edit(part, row, col, value):
        t = T.tables.copy()
        base = {"edges": 0, "features": 4 * T.n_edges, "work": 4 * T.n_edges + 8 * T.n_features}[part]
        t[base + row * {"edges": 4, "features": 8, "work": 4}[part] + col] = value
        return t
    bad = [(edit("edges", 1, 2, (1 << 24) + 1), "coordinate"), (edit("edges", 0, 1, -(1 << 24) - 1), "coordinate"),
           (edit("features", 0, 0, 1), "tile"), (edit("features", 2, 0, -1), "tile"), (edit("features", 1, 1, 256), "value"),
           (edit("features", 1, 1, -1), "value"), (edit("features", 2, 2, T.n_edges - 1), "edges"),
           (edit("features", 0, 3, -4), "edges"), (edit("features", 0, 6, 44), "box"), (edit("features", 0, 7, 40), "box"),
           (edit("features", 0, 4, -1), "box"), (edit("features", 1, 5, 39), "box"), (edit("work", 0, 0, 3), "names feature"),
           (edit("work", 0, 0, -1), "names feature"), (edit("work", 1, 1, 43), "window"), (edit("work", 1, 2, 0), "window"),
           (edit("work", 0, 3, 1), "last column")]
    for tables, word in bad:
        code, msg = rc(tables)
        assert code == 1 and word in msg, (word, code, msg)
    two = rz.pack_rings([R.painter_overlap()[0], R.painter_twins()[0]], 40, 44, 1, 1)
    assert two.features[:, 0].tolist() == [0, 0, 0, 1, 1]
    t = two.tables.copy()
    t[4 * two.n_edges + 8 * 1] = 1                       # tiles 0, 1, 0, 1, 1
    code, msg = rc(t, ne=two.n_edges, nf=two.n_features, nw=two.n_work, B=2)
    assert code == 1 and "sorted by tile" in msg, msg
    for kw, word in [(dict(k=9, off=256), "frac_bits"), (dict(k=1, off=2), "off="), (dict(k=0, off=1), "off="),
                     (dict(k=-1, off=0), "frac_bits"), (dict(k=8, off=128, H=1, W=(1 << 16) + 1), "2^24"),
                     (dict(nw=-1), "n_work"), (dict(B=0), "positive"), (dict(B=65536), "too large")]:
        code, msg = rc(T.tables, **kw)
        assert code == 1 and word in msg, (kw, code, msg)
