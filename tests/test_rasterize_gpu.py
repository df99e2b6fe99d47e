"""Polygons -> masks on the MI355X (csrc/rasterize.hip through the C ABI, ops.rasterize_polygons, utils/rasterize.py,
utils/convert2png.py and the CLIs) against the restatements of tests/rasterize_ref.py.  Every value is an integer, so every
comparison is np.array_equal.  Each call runs between canary stretches around out and the workspace, and the device tables
are compared with their host copy afterwards."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import buildings_ref as BR
import polygons_ref as PR
import rasterize_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary bytes on either side of out
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = 0xEE


def _rz():
    from xview2_amd.utils import rasterize
    return rasterize


def _call(tables, ne, nf, nw, k, off, B, H, W, stream=None):
    """xv2_rasterize_polygons on caller-owned buffers -> (out uint8 [B,H,W] numpy, error text or None); a rejected call must
    leave out and the workspace as they were"""
    from xview2_amd import _capi
    need = int(_capi.query("xv2_rasterize_workspace", B, H, W))
    assert need == 4 * B * H * W
    obuf = torch.full((2 * CAN + B * H * W,), FILL, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)
    out, ws = obuf[CAN:CAN + B * H * W], wbuf[CAN_WS:CAN_WS + need]
    host = np.ascontiguousarray(tables, dtype=np.int32)
    dev = torch.from_numpy(host).to(DEV) if host.size else None
    torch.cuda.synchronize()

    def run():
        try:
            _capi.call("xv2_rasterize_polygons", dev, host.ctypes.data if host.size else None, ne, nf, nw, k, off, B, H, W, ws, out)
        except RuntimeError as e:
            return None, str(e)
        return out.cpu().numpy().reshape(B, H, W), None
    if stream is None:
        got, err = run()
    else:
        with torch.cuda.stream(stream):          # the copy back is ordered by the stream alone: no device-wide wait
            got, err = run()
    torch.cuda.synchronize()
    assert bool((obuf[:CAN] == FILL).all()) and bool((obuf[-CAN:] == FILL).all()), "out: canary overwritten"
    assert bool((wbuf[:CAN_WS] == 0xA5).all()) and bool((wbuf[-CAN_WS:] == 0xA5).all()), "workspace: canary overwritten"
    if dev is not None:
        assert np.array_equal(dev.cpu().numpy(), host), "the tables were written"
    if err is not None:
        assert bool((out == FILL).all()) and bool((ws == 0xA5).all()), "a rejected call wrote something"
    return got, err


def _run(T, H, W, stream=None):
    got, err = _call(T.tables, T.n_edges, T.n_features, T.n_work, T.frac_bits, T.off, T.B, H, W, stream)
    assert err is None, err
    return got


def _diff(got, want):
    return np.argwhere(got != want)[:5].tolist()


@functools.lru_cache(maxsize=None)
def _brute_cases(H, W, k, off):
    return {name: R.brute(tiles, H, W, k, off) for name, tiles in R.cases(H, W, k, off).items()}


# ---- the case table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,off", R.SAMPLINGS)
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_case_table_equals_ref_and_brute_force(H, W, k, off):
    rz = _rz()
    brute = _brute_cases(H, W, k, off)
    got = {}
    for name, tiles in R.cases(H, W, k, off).items():
        T = rz.pack_rings(tiles, H, W, k, off)
        got[name] = _run(T, H, W)
        assert np.array_equal(got[name], R.ref(T, H, W)), (name, _diff(got[name], R.ref(T, H, W)))
        assert np.array_equal(got[name], brute[name]), (name, _diff(got[name], brute[name]))
    assert np.array_equal(got["ring_cw"], got["ring_ccw"]) and got["ring_cw"].any()
    assert (got["whole_tile"] == 7).all() and not got["outside"].any()
    assert rz.pack_rings(R.cases(H, W, k, off)["outside"], H, W, k, off).n_features == 0
    assert got["empty_middle"][0].any() and not got["empty_middle"][1].any() and got["empty_middle"][2].any()
    assert got["collinear"].sum() == 7 * 5                       # a zero-area ring covers the sample points on it, no more


@pytest.mark.parametrize("n_edges", [255, 256, 257, 513])
def test_rings_around_the_stage_size(n_edges):
    rz = _rz()
    T = rz.pack_rings(R.comb(n_edges), 64, 64, 8, 128)
    assert T.n_edges == n_edges and T.n_features == 1 and T.n_work == 4
    got = _run(T, 64, 64)
    want = R.ref(T, 64, 64)
    assert np.array_equal(got, want), _diff(got, want)
    assert np.array_equal(got, R.brute(R.comb(n_edges), 64, 64, 8, 128))      # (shares no packing with the call)
    assert 0 < (got != 0).sum() < 64 * 64


@pytest.mark.parametrize("k,off", R.SAMPLINGS)
def test_cross_products_beyond_32_bits(k, off):
    rz = _rz()
    tiles = R.far_triangle(k, off)
    T = rz.pack_rings(tiles, 64, 64, k, off)
    got = _run(T, 64, 64)
    want = R.brute(tiles, 64, 64, k, off)                         # Python integers: no width to overflow
    assert np.array_equal(got, want), _diff(got, want)
    assert want.any() and not want.all()                          # the slanted edge crosses the tile


# ---- painting ------------------------------------------------------------------------------------------------------------------
def test_painter_last_feature_wins():
    rz = _rz()
    tiles = R.painter_overlap()
    got = _run(rz.pack_rings(tiles, 40, 44, 1, 1), 40, 44)
    assert np.array_equal(got, R.brute(tiles, 40, 44, 1, 1))
    assert got[0, 3, 3] == 3 and got[0, 10, 12] == 255 and got[0, 15, 12] == 1 and got[0, 25, 35] == 255
    tiles = R.painter_twins()
    got = _run(rz.pack_rings(tiles, 36, 36, 1, 1), 36, 36)
    assert np.array_equal(got, R.brute(tiles, 36, 36, 1, 1)) and set(np.unique(got)) == {0, 200}


def test_painter_5000_one_pixel_features():
    rz = _rz()
    tiles = R.painter_pixels(5000, 96, 80)
    T = rz.pack_rings(tiles, 96, 80, 1, 1)
    assert T.n_features == 5000 and T.n_work == 5000
    got = _run(T, 96, 80)
    want = np.zeros((96, 80), dtype=np.uint8)
    for i in range(5000):                                          # one-pixel squares: the painter's rule, stated directly
        p = (i * 37) % 3000
        want[p // 80, p % 80] = 1 + i % 4
    assert np.array_equal(got[0], want), _diff(got[0], want)
    assert (want != 0).sum() == 3000


def test_windows_cut_by_the_box_and_by_the_tile():
    rz = _rz()
    tiles = R.window_boxes()
    T = rz.pack_rings(tiles, 40, 70, 1, 1)
    f = T.features
    assert (f[:, 6] - f[:, 4] + 1).tolist() == [65, 33, 20] and (f[:, 7] - f[:, 5] + 1).tolist() == [1, 31, 15]
    assert T.n_work == 3 + 2 + 1
    got = _run(T, 40, 70)
    assert np.array_equal(got, R.ref(T, 40, 70)) and np.array_equal(got, R.brute(tiles, 40, 70, 1, 1))
    assert (got[0, 5, 3:68] == 6).all() and (got[0] == 6).sum() == 65


def test_quarter_pixel_vertices_under_rule_exact():
    rz = _rz()
    polys = [({"exterior": [[3.3, 2.71], [48.12, 9.5], [40.77, 33.333], [7.5, 30.0009]],
               "holes": [[[12.25, 10.125], [30.6, 12.4], [22.01, 25.99]]]}, 4),
             ({"exterior": [[20.5, 15.5], [52.9, 36.2], [30.5, 36.999]], "holes": []}, 2)]
    T = rz.pack([polys], 37, 53, "exact")
    assert (T.frac_bits, T.off) == (8, 128) and (T.edges % 256 != 0).any()
    got = _run(T, 37, 53)
    tiles = [[([rz.quantise(r, "exact").tolist() for r in [p["exterior"]] + p["holes"]], v) for p, v in polys]]
    assert np.array_equal(got, R.ref(T, 37, 53)) and np.array_equal(got, R.brute(tiles, 37, 53, 8, 128))
    assert set(np.unique(got)) == {0, 2, 4}
    # ... and the module's own entry gives the same map
    assert np.array_equal(rz.rasterize([polys], 37, 53, "exact").cpu().numpy(), got)


# ---- behaviour -----------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_equal_bits():
    rz = _rz()
    T = rz.pack_rings([R.painter_overlap()[0], R.cases(40, 44, 1, 1)["hole"][0], R.painter_twins()[0]], 40, 44, 1, 1)
    a = _run(T, 40, 44)
    b = _run(T, 40, 44)
    c = _run(T, 40, 44, stream=torch.cuda.Stream())
    assert a.tobytes() == b.tobytes() == c.tobytes() and np.array_equal(a, R.ref(T, 40, 44))


def test_rejected_tables_return_einval_and_write_nothing():
    rz = _rz()
    T = rz.pack_rings(R.painter_overlap(), 40, 44, 1, 1)
    fo, wo = 4 * T.n_edges, 4 * T.n_edges + 8 * T.n_features

    def edited(index, value):
        t = T.tables.copy()
        t[index] = value
        return t
    bad = [(edited(6, (1 << 24) + 1), "coordinate"), (edited(fo, 1), "tile"), (edited(fo + 8 + 1, 256), "value"),
           (edited(fo + 16 + 2, T.n_edges - 1), "edges"), (edited(fo + 3, -4), "edges"), (edited(fo + 6, 44), "box"),
           (edited(fo + 7, 40), "box"), (edited(fo + 4, -1), "box"), (edited(wo, 3), "names feature"),
           (edited(wo + 4 + 1, 43), "window"), (edited(wo + 4 + 2, 0), "window"), (edited(wo + 3, 1), "last column")]
    for tables, word in bad:
        got, err = _call(tables, T.n_edges, T.n_features, T.n_work, 1, 1, 1, 40, 44)
        assert got is None and word in err, (word, err)
    two = rz.pack_rings([R.painter_overlap()[0], R.painter_twins()[0]], 40, 44, 1, 1)
    t = two.tables.copy()
    t[4 * two.n_edges + 8] = 1                                     # tiles 0, 1, 0, 1, 1
    got, err = _call(t, two.n_edges, two.n_features, two.n_work, 1, 1, 2, 40, 44)
    assert got is None and "sorted by tile" in err
    for k, off, word in [(9, 256, "frac_bits"), (1, 2, "off="), (0, 1, "off=")]:
        got, err = _call(T.tables, T.n_edges, T.n_features, T.n_work, k, off, 1, 40, 44)
        assert got is None and word in err, (k, off, err)
    got, err = _call(np.zeros(0, dtype=np.int32), 0, 0, 0, 8, 128, 1, 1, (1 << 16) + 1)
    assert got is None and "2^24" in err
    # the unedited tables pass, and so do no features at all and features without work
    assert np.array_equal(_run(T, 40, 44), R.ref(T, 40, 44))
    got, err = _call(np.zeros(0, dtype=np.int32), 0, 0, 0, 1, 1, 2, 40, 44)
    assert err is None and got.shape == (2, 40, 44) and not got.any()
    got, err = _call(T.tables[:wo], T.n_edges, T.n_features, 0, 1, 1, 1, 40, 44)
    assert err is None and not got.any()


def test_ops_binding_checks_and_kernel_names():
    from tests.test_f16x2_gpu import _prof
    from xview2_amd import ops
    rz = _rz()
    T = rz.pack_rings(R.painter_overlap(), 40, 44, 1, 1)
    with _prof() as pr:
        out = ops.rasterize_polygons(T.tables, T.n_edges, T.n_features, T.n_work, 1, 1, 1, 40, 44)
        names = pr.names()
    assert "rs_cover_kernel" in names and "rs_resolve_kernel" in names, names
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 40, 44) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), R.ref(T, 40, 44))
    with pytest.raises(ValueError, match="int32"):
        ops.rasterize_polygons(T.tables.astype(np.int64), T.n_edges, T.n_features, T.n_work, 1, 1, 1, 40, 44)
    with pytest.raises(ValueError, match="table words"):
        ops.rasterize_polygons(T.tables[:-1], T.n_edges, T.n_features, T.n_work, 1, 1, 1, 40, 44)
    with pytest.raises(ValueError, match="supported sizes"):
        ops.rasterize_polygons(T.tables, T.n_edges, T.n_features, T.n_work, 1, 1, 65536, 40, 44)
    with pytest.raises(RuntimeError, match="names tile"):
        ops.rasterize_polygons(_with(T.tables, 4 * T.n_edges, 5), T.n_edges, T.n_features, T.n_work, 1, 1, 1, 40, 44)


def _with(tables, index, value):
    t = tables.copy()
    t[index] = value
    return t


# ---- the device round trip -----------------------------------------------------------------------------------------------------
def _vote_painted(mask, seed):
    """(pre, post) uint8: post holds one class 1..4 per 4-connected building, so the building table's vote is that class"""
    labels = PR.labels_of(mask)
    cls = 1 + BR._hash(seed, (int(labels.max()) + 1,), 4)
    return (labels != 0).astype(np.uint8), np.where(labels != 0, cls[labels], 0).astype(np.uint8)


@pytest.mark.parametrize("name", ["blobs_192x256", "diagonal_holes", "nested"])
def test_label_map_to_polygons_to_raster_is_the_identity_on_the_device(name):
    from xview2_amd.utils import buildings, polygons
    rz = _rz()
    mask = {"blobs_192x256": lambda: BR.blobs(91, 192, 256), "diagonal_holes": PR.diagonal_holes, "nested": PR.nested}[name]()
    pre, post = _vote_painted(mask, 92)
    H, W = pre.shape
    pre_d, post_d = torch.from_numpy(pre).to(DEV), torch.from_numpy(post).to(DEV)
    polys = polygons.building_polygons(pre_d)
    got = rz.rasterize([[(p, 1) for p in polys]], H, W, "corner").cpu().numpy()
    assert np.array_equal(got[0], pre), _diff(got[0], pre)
    table = buildings.building_table(pre_d, post_d)
    assert len(table) == len(polys) and (table[:, 13] > 0).all()
    got = rz.rasterize([[(p, int(v)) for p, v in zip(polys, table[:, 13].tolist())]], H, W, "corner").cpu().numpy()
    assert np.array_equal(got[0], post), _diff(got[0], post)
    if name == "blobs_192x256":
        assert len(polys) > 10 and sum(len(p["holes"]) for p in polys) > 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _label_tree(root, size=128):
    """four label files (two pre / post pairs) of rotated quads with float vertices, and the images build_index reads"""
    from PIL import Image
    names = ["no-damage", "minor-damage", "major-damage", "destroyed", "un-classified"]
    os.makedirs(os.path.join(root, "labels"))
    os.makedirs(os.path.join(root, "images"))
    for t in range(2):
        feats = []
        for i in range(9):
            h = BR._hash(100 * t + i, (6,), 1000).astype(np.float64) / 1000.0
            cx, cy, a, b, th = 10 + 108 * h[0], 10 + 108 * h[1], 4 + 14 * h[2], 3 + 9 * h[3], np.pi * h[4]
            pts = [(cx + c * a * np.cos(th) - s * b * np.sin(th), cy + c * a * np.sin(th) + s * b * np.cos(th))
                   for c, s in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            wkt = "POLYGON ((%s))" % ", ".join("%r %r" % (float(x), float(y)) for x, y in pts + pts[:1])
            feats.append({"properties": {"feature_type": "building", "subtype": names[(i + t) % 5], "uid": "t%d-%d" % (t, i)},
                          "wkt": wkt})
        for mode in ("pre", "post"):
            stem = "scene_%08d_%s_disaster" % (t, mode)
            xy = [dict(f, properties={k: v for k, v in f["properties"].items() if mode == "post" or k != "subtype"}) for f in feats]
            with open(os.path.join(root, "labels", stem + ".json"), "w") as f:
                json.dump({"features": {"lng_lat": [], "xy": xy}, "metadata": {"width": size, "height": size}}, f)
            Image.fromarray(BR._hash(t, (size, size, 3), 256).astype(np.uint8)).save(os.path.join(root, "images", stem + ".png"))
    return names


def test_convert2png_writes_the_targets_the_loaders_read(tmp_path):
    from PIL import Image
    from xview2_amd.data_loading.pytorch_loader import load_data, read_index
    from xview2_amd.utils import convert2png
    rz = _rz()
    root = str(tmp_path / "data")
    _label_tree(root)
    index = str(tmp_path / "index.csv")
    args = convert2png.parser.parse_args(["--data", root, "--n_jobs", "-1", "--size", "128", "--batch", "3", "--index", index])
    conv = convert2png.Converter(args)
    assert conv.threads == 16 and convert2png.threads_for(4) == 4 and convert2png.threads_for(400) == 16
    assert conv.run() == 4
    seen = set()
    for mode in ("pre", "post"):
        for t in range(2):
            stem = "scene_%08d_%s_disaster" % (t, mode)
            im = Image.open(os.path.join(root, "targets", stem + ".png"))
            assert im.mode == "L" and im.size == (128, 128)
            feats = rz.read_xbd_json(os.path.join(root, "labels", stem + ".json"), mode)
            assert len(feats) == 9
            want = R.ref(rz.pack([feats], 128, 128, "reference"), 128, 128)[0]
            assert np.array_equal(np.asarray(im), want), (stem, _diff(np.asarray(im), want))
            seen |= set(np.unique(want).tolist()) if mode == "post" else set()
            if mode == "pre":
                assert set(np.unique(want).tolist()) == {0, 1}
    assert 255 in seen and {1, 2, 3, 4} & seen
    imgs, lbls = load_data(root, "post")
    assert len(imgs) == len(lbls) == 2
    assert sorted(read_index(index)) == ["1", "2", "3", "4", "idx"]


def test_cli_reproduces_the_png_pair_its_geojson_came_from(tmp_path):
    from PIL import Image
    from xview2_amd.utils import polygons
    rz = _rz()
    pre, post = _vote_painted(BR.blobs(71, 70, 90, thresh=0.5), 72)
    Image.fromarray(pre).save(str(tmp_path / "pre.png"))
    Image.fromarray(post).save(str(tmp_path / "post.png"))
    geo = str(tmp_path / "out.geojson")
    n = polygons.main([str(tmp_path / "pre.png"), str(tmp_path / "post.png"), geo])
    assert n > 3
    assert rz.main([geo, str(tmp_path / "pre2.png"), str(tmp_path / "post2.png"), "--size", "70", "90"]) == n
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "pre2.png"))), pre)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "post2.png"))), post)


def test_cli_on_xbd_label_files_pre_and_post(tmp_path):
    """a post-disaster label file gives the pair; a pre-disaster one carries no subtype and paints 1 into both maps"""
    from PIL import Image
    rz = _rz()
    root = str(tmp_path / "data")
    _label_tree(root)
    for mode in ("pre", "post"):
        src = os.path.join(root, "labels", "scene_00000001_%s_disaster.json" % mode)
        a, b = str(tmp_path / (mode + "_a.png")), str(tmp_path / (mode + "_b.png"))
        assert rz.main([src, a, b, "--size", "128", "128"]) == 9
        want_pre = R.ref(rz.pack([rz.read_xbd_json(src, "pre")], 128, 128, "reference"), 128, 128)[0]
        want_post = R.ref(rz.pack([rz.read_xbd_json(src, "post")], 128, 128, "reference"), 128, 128)[0] if mode == "post" \
            else want_pre
        assert np.array_equal(np.asarray(Image.open(a)), want_pre) and np.array_equal(np.asarray(Image.open(b)), want_post)
        assert (want_post.max() > 1) == (mode == "post")
