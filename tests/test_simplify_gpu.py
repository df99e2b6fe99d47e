"""The tolerance simplification on the MI355X (csrc/simplify.hip through the C ABI, ops.polygon_simplify,
utils/polygons.py and the CLIs) against the recursive restatement of tests/simplify_ref.py.  Every value is an integer, so
every comparison is np.array_equal.  Each call runs between canary stretches around out_rings, out_verts, out_total and the
workspace, the rows of out_verts behind out_total must still hold the fill, and the inputs are compared with their copies
afterwards."""
import json
import os

import numpy as np
import pytest
import torch

import buildings_ref as BR
import polygons_ref as R
import simplify_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of every output
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = -7


def _guarded(n, dtype, can=CAN, fill=FILL):
    buf = torch.full((2 * can + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[can:can + n]


def _intact(bufs):
    for what, buf, can, fill in bufs:
        assert bool((buf[:can] == fill).all()) and bool((buf[-can:] == fill).all()), what + ": canary overwritten"


def _simplify(rings_h, verts_h, q, stream=None):
    """xv2_polygon_simplify on caller-owned buffers -> (out_rings [R, 8], out_verts [V, 2] with FILL behind out_total,
    out_total) as numpy"""
    from xview2_amd import _capi
    n, V = len(rings_h), len(verts_h)
    need = int(_capi.query("xv2_polygon_simplify_workspace", n, V))
    assert need > 0
    rings = torch.from_numpy(np.ascontiguousarray(rings_h)).to(DEV)
    verts = torch.from_numpy(np.ascontiguousarray(verts_h)).to(DEV)
    rbuf, out_rings = _guarded(8 * n, torch.int64)
    vbuf, out_verts = _guarded(2 * V, torch.int32)
    tbuf, out_total = _guarded(1, torch.int64)
    wbuf, ws = _guarded(need, torch.uint8, CAN_WS, 0xA5)
    keep_r, keep_v = rings.clone(), verts.clone()
    torch.cuda.synchronize()

    def run():
        _capi.call("xv2_polygon_simplify", rings if n else None, verts if V else None, n, V, q, ws, out_rings if n else None,
                   out_verts if V else None, out_total)
        return out_rings.cpu().numpy().reshape(-1, 8), out_verts.cpu().numpy().reshape(-1, 2), int(out_total.cpu()[0])
    if stream is None:
        got = run()
    else:
        with torch.cuda.stream(stream):      # the copies are ordered by the stream alone: no device-wide wait
            got = run()
    torch.cuda.synchronize()
    _intact([("out_rings", rbuf, CAN, FILL), ("out_verts", vbuf, CAN, FILL), ("out_total", tbuf, CAN, FILL),
             ("workspace", wbuf, CAN_WS, 0xA5)])
    assert torch.equal(rings, keep_r) and torch.equal(verts, keep_v), "an input was written"
    return got


def _first_diff(got, want):
    r, c = np.nonzero(got != want)
    return "%d cells differ, first row %d col %d: %d != %d\n%s\n%s" % (len(r), r[0], c[0], got[r[0], c[0]], want[r[0], c[0]],
                                                                       got[r[0]], want[r[0]])


def _check(name, q, stream=None):
    rings, verts, _ = S.cases()[name]
    want_r, want_v, want_total = S.expected(name, q)
    out_r, out_v, total = _simplify(rings, verts, q, stream)
    assert total == want_total == int(out_r[:, 2].sum())
    assert np.array_equal(out_r, want_r), _first_diff(out_r, want_r)
    assert np.array_equal(out_v[:total], want_v), _first_diff(out_v[:total], want_v)
    assert np.all(out_v[total:] == FILL), "storage behind vertex %d was written" % total
    return out_r, out_v, total


# ---- the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", S.QS)
@pytest.mark.parametrize("name", sorted(S.cases()))
def test_cases_equal_the_restatement(name, q):
    _check(name, q)


@pytest.mark.parametrize("q", (1, 37, 160, 4000, 65535))
def test_other_tolerances_up_to_the_largest(q):
    """the largest q squares to just under 2^32; with it every ring of the mixed table keeps two anchors and collapses"""
    out_r, _, _ = _check("mixed", q)
    _check("thresholds", q)
    _check("circle_5000", q)
    if q == 65535:
        assert np.all(out_r[:, 7] == 1)


def test_two_runs_and_a_side_stream_give_equal_bits():
    for name in ("mixed", "thresholds", "circle_5000", "zigzag_300"):
        a = _check(name, 16)
        b = _check(name, 16)
        c = _check(name, 16, stream=torch.cuda.Stream())
        for x, y, z in zip(a, b, c):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes()


def test_kernels_are_named_by_the_profiler():
    from tests.test_f16x2_gpu import _prof
    with _prof() as pr:
        _check("thresholds", 16)
        names = pr.names()
    for k in ("simplify", "offsets", "write"):
        assert "sp_%s_kernel" % k in names, names


# ---- the binding ------------------------------------------------------------------------------------------------------------
def test_ops_binding_checks_and_refusals():
    from xview2_amd import ops
    rings_h, verts_h, _ = S.cases()["mixed"]
    want_r, want_v, want_total = S.expected("mixed", 24)
    rings, verts = torch.from_numpy(rings_h).to(DEV), torch.from_numpy(verts_h).to(DEV)
    spare = torch.cat([rings, torch.full((5, 8), FILL, dtype=torch.int64, device=DEV)])      # as polygon_trace sizes its table
    for table in (rings, spare):
        out_r, out_v, total = ops.polygon_simplify(table, verts, len(rings_h), 24)
        assert out_r.dtype == torch.int64 and tuple(out_r.shape) == (len(rings_h), 8)
        assert out_v.dtype == torch.int32 and tuple(out_v.shape) == (len(verts_h), 2)
        assert total.dtype == torch.int64 and tuple(total.shape) == (1,) and int(total) == want_total
        assert np.array_equal(out_r.cpu().numpy(), want_r) and np.array_equal(out_v[:want_total].cpu().numpy(), want_v)
    with pytest.raises(ValueError, match="int64"):
        ops.polygon_simplify(rings.int(), verts, len(rings_h), 24)
    with pytest.raises(ValueError, match="int64"):
        ops.polygon_simplify(rings[:, :7], verts, len(rings_h), 24)
    with pytest.raises(ValueError, match="int32"):
        ops.polygon_simplify(rings, verts.long(), len(rings_h), 24)
    with pytest.raises(ValueError, match="int32"):
        ops.polygon_simplify(rings, verts.reshape(-1), len(rings_h), 24)
    for q in (-1, 65536):
        with pytest.raises(ValueError, match="0..65535"):
            ops.polygon_simplify(rings, verts, len(rings_h), q)
    with pytest.raises(ValueError, match="n_rings"):
        ops.polygon_simplify(rings, verts, len(rings_h) + 1, 24)
    # offsets that are not contiguous from 0, counts that do not sum to the vertex rows: refused before any launch
    gap = rings.clone()
    gap[3:, 3] += 2
    shifted = rings.clone()
    shifted[:, 3] += 1
    swapped = rings.clone()
    swapped[[0, 1]] = rings[[1, 0]]
    negative = rings.clone()
    negative[0, 2] = -negative[0, 2]
    for bad in (gap, shifted, swapped, negative):
        with pytest.raises(ValueError, match="contiguous"):
            ops.polygon_simplify(bad, verts, len(rings_h), 24)
    with pytest.raises(ValueError, match="contiguous"):
        ops.polygon_simplify(rings, verts[:-1], len(rings_h), 24)
    with pytest.raises(ValueError, match="contiguous"):
        ops.polygon_simplify(rings, verts, len(rings_h) - 1, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polygon_simplify(rings.cpu(), verts, len(rings_h), 24)
    # nothing to simplify
    out_r, out_v, total = ops.polygon_simplify(rings[:0], verts[:0], 0, 24)
    assert tuple(out_r.shape) == (0, 8) and tuple(out_v.shape) == (0, 2) and int(total) == 0


# ---- the module ------------------------------------------------------------------------------------------------------------
def _scene(seed, H, W):
    """uint8 pre / post label maps with some tens of buildings, some with holes"""
    mask = BR.blobs(seed, H, W, thresh=0.5)
    pre = mask.astype(np.uint8)
    post = np.where(mask, 1 + BR._hash(seed + 1, (H, W), 4), 0).astype(np.uint8)
    return pre, post


def test_building_polygons_with_a_tolerance_equal_the_restatement_on_the_traced_rings():
    from xview2_amd.utils import polygons
    pre, _ = _scene(61, 96, 80)
    pre_d = torch.from_numpy(pre).to(DEV)
    _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
    plain = polygons.building_polygons(pre_d)
    for T, q in ((0.5, 8), (1, 16), (1.5, 24), (4.0, 64)):
        polys = polygons.building_polygons(pre_d, simplify=T)
        assert polys == S.polygons_of(rings, verts, q) and len(polys) == len(plain) > 3
        assert [p["root"] for p in polys] == [p["root"] for p in plain]
    assert sum(len(p["exterior"]) for p in polys) < sum(len(p["exterior"]) for p in plain)
    # a batch with an empty tile in the middle gives one list per tile
    both = polygons.building_polygons(torch.stack([pre_d, torch.zeros_like(pre_d), pre_d]), simplify=1.5)
    assert both == [S.polygons_of(rings, verts, 24), [], S.polygons_of(rings, verts, 24)]
    assert polygons.building_polygons(torch.zeros_like(pre_d), simplify=1.5) == []
    with pytest.raises(ValueError, match="0 <= T < 4096"):
        polygons.building_polygons(pre_d, simplify=-1)


def test_without_a_tolerance_the_result_is_todays_object_for_object():
    from xview2_amd.utils import polygons
    pre, _ = _scene(61, 96, 80)
    pre_d = torch.from_numpy(pre).to(DEV)
    _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
    want = R.polygons(rings, verts)
    for kw in ({}, {"simplify": 0}, {"simplify": 0.0}, {"simplify": 0.03}):
        got = polygons.building_polygons(pre_d, **kw)
        assert got == want and all("simplified" not in p for p in got)


def test_cli_with_simplify_on_a_png_pair_writes_the_restatements_polygons(tmp_path):
    from PIL import Image
    from xview2_amd.utils import buildings, polygons
    pre, post = _scene(71, 70, 90)
    Image.fromarray(pre).save(str(tmp_path / "pre.png"))
    Image.fromarray(post).save(str(tmp_path / "post.png"))
    out, want, plain = str(tmp_path / "out.geojson"), str(tmp_path / "want.geojson"), str(tmp_path / "plain.geojson")
    n = polygons.main([str(tmp_path / "pre.png"), str(tmp_path / "post.png"), out, "--simplify", "1"])
    _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
    records = buildings.to_records(BR.table(pre, post), 70, 90, confidence=False)
    assert n == len(records) > 3
    polygons.write_geojson(want, S.polygons_of(rings, verts, 16), records)
    assert open(out, "rb").read() == open(want, "rb").read()
    # without the flag, and with --simplify 0, the file is the one the plain trace gives
    polygons.write_geojson(plain, R.polygons(rings, verts), records)
    assert open(plain, "rb").read() != open(want, "rb").read()
    for extra in ([], ["--simplify", "0"]):
        polygons.main([str(tmp_path / "pre.png"), str(tmp_path / "post.png"), out] + extra)
        assert open(out, "rb").read() == open(plain, "rb").read()


def test_cli_post_process_with_simplify_writes_one_feature_per_table_row(tmp_path):
    import postproc_ref as P
    from xview2_amd.utils import buildings, post_process
    os.makedirs(str(tmp_path / "probs"))
    for k, seed in enumerate((81, 85)):
        cls = np.where(BR.blobs(seed, 70, 90, thresh=0.56), 1 + BR._hash(seed + 1, (70, 90), 4), 0)
        np.save(str(tmp_path / "probs" / ("test_localization_%05d.npy" % k)), P.loc_from_mask(seed + 2, cls > 0))
        np.save(str(tmp_path / "probs" / ("test_damage_%05d.npy" % k)), P.probs_from_classes(seed + 3, cls, 4))
    args = post_process.get_parser().parse_args(["--results", str(tmp_path), "--components", "--polygons", "--simplify", "1"])
    assert post_process.run(args) == 2
    from PIL import Image
    for k in range(2):
        rows = buildings.read_csv(str(tmp_path / "buildings" / ("test_buildings_%05d.csv" % k)))
        doc = json.load(open(str(tmp_path / "buildings" / ("test_buildings_%05d.geojson" % k))))
        assert len(doc["features"]) == len(rows) > 1
        assert [f["properties"]["id"] for f in doc["features"]] == [r["id"] for r in rows]
        assert [f["properties"]["area"] for f in doc["features"]] == [r["area"] for r in rows]
        pre = np.asarray(Image.open(str(tmp_path / "predictions" / ("test_localization_%05d_prediction.png" % k))))
        _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
        assert [f["geometry"]["coordinates"] for f in doc["features"]] == [
            [[list(v) for v in r + r[:1]] for r in [p["exterior"]] + p["holes"]] for p in S.polygons_of(rings, verts, 16)]
    with pytest.raises(ValueError, match="0 <= T < 4096"):
        post_process.run(post_process.get_parser().parse_args(["--results", str(tmp_path), "--polygons", "--simplify", "5000"]))
