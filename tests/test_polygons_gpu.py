"""The building outlines on the MI355X (csrc/polygons.hip through the C ABI, ops.polygon_count / ops.polygon_trace,
utils/polygons.py and the CLIs) against the sequential restatement of tests/polygons_ref.py.  Every value is an integer,
so every comparison is np.array_equal.  Each call runs between canary stretches around counts, rings, verts, ring_count
and both workspaces, and the labels are compared with their copy afterwards."""
import json
import os

import numpy as np
import pytest
import torch

import buildings_ref as BR
import polygons_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of every output
CAN_WS = 256        # canary bytes on either side of a workspace
FILL = -7


def _labels(masks):
    from xview2_amd import ops
    return ops.label_components(torch.from_numpy(np.ascontiguousarray(np.stack(masks))).to(DEV))


def _guarded(n, dtype, can=CAN, fill=FILL):
    buf = torch.full((2 * can + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[can:can + n]


def _intact(bufs):
    for what, buf, can, fill in bufs:
        assert bool((buf[:can] == fill).all()) and bool((buf[-can:] == fill).all()), what + ": canary overwritten"


def _count(labels):
    """xv2_polygon_count on caller-owned buffers -> counts int64 [B,2] numpy"""
    from xview2_amd import _capi
    B, H, W = labels.shape
    need = int(_capi.query("xv2_polygon_count_workspace", B, H, W))
    assert need > 0
    cbuf, counts = _guarded(2 * B, torch.int64)
    wbuf, ws = _guarded(need, torch.uint8, CAN_WS, 0xA5)
    _capi.call("xv2_polygon_count", labels, B, H, W, ws, counts)
    torch.cuda.synchronize()
    _intact([("counts", cbuf, CAN, FILL), ("count workspace", wbuf, CAN_WS, 0xA5)])
    return counts.cpu().numpy().reshape(B, 2)


def _trace(labels, E, V, stream=None):
    """xv2_polygon_trace on caller-owned buffers sized by E and V -> (rings [V // 4, 8], verts [V, 2], ring_count [B],
    status, rounds) as numpy, everything behind the written part still FILL"""
    from xview2_amd import _capi
    B, H, W = labels.shape
    need = int(_capi.query("xv2_polygon_trace_workspace", B, H, W, E))
    assert need > 0
    rbuf, rings = _guarded(V // 4 * 8, torch.int64)
    vbuf, verts = _guarded(2 * V, torch.int32)
    nbuf, ring_count = _guarded(B, torch.int32)
    wbuf, ws = _guarded(need, torch.uint8, CAN_WS, 0xA5)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    keep = labels.clone()
    torch.cuda.synchronize()

    def run():
        _capi.call("xv2_polygon_trace", labels, B, H, W, E, V, ws, rings, verts, ring_count, status)
        return (rings.cpu().numpy().reshape(-1, 8), verts.cpu().numpy().reshape(-1, 2), ring_count.cpu().numpy(),
                int(status.cpu()[0]), ws[16:32].cpu().numpy().view(np.int32)[1:3].tolist())
    if stream is None:
        got = run()
    else:
        with torch.cuda.stream(stream):      # the copies are ordered by the stream alone: no device-wide wait
            got = run()
    torch.cuda.synchronize()
    _intact([("rings", rbuf, CAN, FILL), ("verts", vbuf, CAN, FILL), ("ring_count", nbuf, CAN, FILL),
             ("trace workspace", wbuf, CAN_WS, 0xA5)])
    assert torch.equal(labels, keep), "the labels were written"
    return got


def _check(masks, stream=None):
    """B tiles of one shape against the restatement -> (counts, rings, verts, ring_count, rounds)"""
    labels = _labels(masks)
    want_counts, want_rings, want_verts, want_rc = R.trace(labels.cpu().numpy())
    counts = _count(labels)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    E, V = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    rings, verts, rc, status, rounds = _trace(labels, E, V, stream)
    assert status == 0
    assert np.array_equal(rc, want_rc), (rc, want_rc)
    n = len(want_rings)
    assert np.array_equal(rings[:n], want_rings), _first_diff(rings[:n], want_rings)
    assert np.all(rings[n:] == FILL), "storage behind ring row %d was written" % n
    assert np.array_equal(verts, want_verts), _first_diff(verts, want_verts)
    return counts, rings[:n], verts, rc, rounds


def _first_diff(got, want):
    r, c = np.nonzero(got != want)
    return "%d cells differ, first row %d col %d: %d != %d\n%s\n%s" % (len(r), r[0], c[0], got[r[0], c[0]], want[r[0], c[0]],
                                                                       got[r[0]], want[r[0]])


# ---- shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.shape_cases()))
def test_shape_cases_equal_restatement(name):
    mask = R.shape_cases()[name]
    counts, rings, verts, rc, rounds = _check([mask])
    if name == "one_fg":
        assert counts.tolist() == [[4, 4]] and rings.tolist() == [[0, 0, 4, 0, 2, 4, 0, 0]]
    if name == "one_bg":
        assert counts.tolist() == [[0, 0]] and rc.tolist() == [0] and len(verts) == 0
    if name in ("full_64", "full_65x63"):
        H, W = mask.shape                        # the ring runs along the image border: out of the image is background
        assert rings.tolist() == [[0, 0, 4, 0, 2 * H * W, 2 * (H + W), 0, 0]]
        assert verts.tolist() == [[W, 0], [W, H], [0, H], [0, 0]]
    if name.startswith("row_"):
        n = int(name[4:])                        # 254, 256, 258 edges: a power of two and either side of it
        assert counts.tolist() == [[2 * n + 2, 4]] and rings[0, 5] == 2 * n + 2
        assert rounds == [8 if 2 * n + 2 <= 256 else 9] * 2
    if name == "checker_8":
        assert counts.tolist() == [[128, 128]] and rc.tolist() == [32]      # every ring row and vertex slot is used
    if name == "diagonal_holes":
        assert rings[:, 2].tolist() == [4, 8] and rings[1, 4] == -4 and verts[4:].tolist().count([2, 2]) == 2
    if name == "corner_touch":
        assert rc.tolist() == [2] and verts.tolist().count([1, 1]) == 2
    if name == "serpentine_96":
        assert counts.tolist() == [[9314, 194]] and rc.tolist() == [1] and rings[0, 5] == 9314 and rounds == [14, 14]


def test_batch_of_three_with_an_empty_middle_tile_equals_single_runs():
    masks = list(R.batch_case())
    counts, rings, verts, rc, _ = _check(masks)
    assert rc.tolist() == [2, 0, 3] and counts[1].tolist() == [0, 0] and rings[:, 6].tolist() == [0, 0, 2, 2, 2]
    for b in (0, 2):
        c1, r1, v1, n1, _ = _check([masks[b]])
        mine = rings[rings[:, 6] == b]
        assert c1[0].tolist() == counts[b].tolist() and n1[0] == rc[b]
        assert np.array_equal(r1[:, [0, 1, 2, 4, 5]], mine[:, [0, 1, 2, 4, 5]])
        assert np.array_equal(v1, verts[mine[0, 3]:mine[-1, 3] + mine[-1, 2]])


def test_blobs_across_chunks_and_a_batch():
    """130 x 200 pixels are 26 pixel chunks per tile and several edge chunks; two different tiles"""
    _check([BR.blobs(51, 130, 200), BR.blobs(52, 130, 200, thresh=0.45)])


# ---- behaviour -------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_equal_bits():
    masks = [R.random_mask(21, 70, 90, 55), BR.blobs(22, 70, 90)]
    a = _check(masks)
    b = _check(masks)
    c = _check(masks, stream=torch.cuda.Stream())
    for x, y, z in zip(a, b, c):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes()


@pytest.mark.parametrize("de,dv", [(4, 0), (-4, 0), (0, 4), (0, -4), (8, 8), (-4, -4)])
def test_wrong_totals_raise_the_status_and_write_nothing(de, dv):
    labels = _labels([R.random_mask(31, 33, 47, 50)])
    counts = _count(labels)
    E, V = int(counts[0, 0]) + de, int(counts[0, 1]) + dv
    rings, verts, rc, status, _ = _trace(labels, E, V)           # (the canaries behind the given sizes are checked in there)
    assert status == 1 and rc.tolist() == [0]
    assert np.all(rings == FILL) and np.all(verts == FILL)


def test_ops_binding_checks_and_the_exception():
    from xview2_amd import ops
    mask = R.random_mask(41, 33, 47, 50)
    labels = _labels([mask])
    want_counts, want_rings, want_verts, want_rc = R.trace(labels.cpu().numpy())
    counts = ops.polygon_count(labels)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (1, 2) and np.array_equal(counts.cpu().numpy(), want_counts)
    E, V = (int(v) for v in counts[0])
    rings, verts, rc = ops.polygon_trace(labels, E, V)
    assert rings.dtype == torch.int64 and tuple(rings.shape) == (V // 4, 8) and verts.dtype == torch.int32
    assert rc.dtype == torch.int32 and np.array_equal(rc.cpu().numpy(), want_rc)
    assert np.array_equal(rings[:len(want_rings)].cpu().numpy(), want_rings) and np.array_equal(verts.cpu().numpy(), want_verts)
    with pytest.raises(RuntimeError, match="other totals"):
        ops.polygon_trace(labels, E + 4, V)
    with pytest.raises(RuntimeError, match="other totals"):
        ops.polygon_trace(labels, E, V - 2)
    with pytest.raises(ValueError, match="totals"):
        ops.polygon_trace(labels, V - 1, V)
    with pytest.raises(ValueError, match="int32"):
        ops.polygon_count(labels.long())
    with pytest.raises(ValueError, match="int32"):
        ops.polygon_trace(labels[0], E, V)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.polygon_count(labels.cpu())
    # an all-background batch: nothing to trace
    empty = torch.zeros((2, 5, 6), dtype=torch.int32, device=DEV)
    assert ops.polygon_count(empty).cpu().tolist() == [[0, 0], [0, 0]]
    rings, verts, rc = ops.polygon_trace(empty, 0, 0)
    assert tuple(rings.shape) == (0, 8) and tuple(verts.shape) == (0, 2) and rc.cpu().tolist() == [0, 0]


def test_kernels_are_named_by_the_profiler():
    from tests.test_f16x2_gpu import _prof
    from xview2_amd import ops
    labels = _labels([R.shape_cases()["nested_17"]])
    with _prof() as pr:
        counts = ops.polygon_count(labels)
        ops.polygon_trace(labels, int(counts[0, 0]), int(counts[0, 1]))
        names = pr.names()
    for k in ("count", "scan", "tiles", "index", "succ", "min", "cut", "rank", "lcount", "lscan", "rings", "verts"):
        assert "pg_%s_kernel" % k in names, names


# ---- the module ------------------------------------------------------------------------------------------------------------
def _scene(seed, H, W):
    """uint8 pre / post label maps with some tens of buildings, some with holes"""
    mask = BR.blobs(seed, H, W, thresh=0.5)
    pre = mask.astype(np.uint8)
    post = np.where(mask, 1 + BR._hash(seed + 1, (H, W), 4), 0).astype(np.uint8)
    return pre, post


def test_building_polygons_follow_the_building_table():
    from xview2_amd.utils import buildings, polygons
    pre, post = _scene(61, 96, 80)
    pre_d, post_d = torch.from_numpy(pre).to(DEV), torch.from_numpy(post).to(DEV)
    table = buildings.building_table(pre_d, post_d)
    polys = polygons.building_polygons(pre_d)
    assert len(polys) == len(table) > 3 and [p["root"] for p in polys] == table[:, 0].tolist()
    assert sum(len(p["holes"]) for p in polys) > 0
    area2 = [R.shoelace(p["exterior"]) + sum(R.shoelace(h) for h in p["holes"]) for p in polys]
    assert area2 == (2 * table[:, 1]).tolist()
    _, want_rings, want_verts, _ = R.trace(R.labels_of(pre)[None])
    assert polys == R.polygons(want_rings, want_verts)
    # the labels the table was built from give the same polygons; a batch gives one list per tile
    rows, labels = buildings.building_table(pre_d, post_d, return_labels=True)
    assert np.array_equal(rows, table) and polygons.building_polygons(pre_d, labels) == polys
    both = polygons.building_polygons(torch.stack([pre_d, torch.zeros_like(pre_d), pre_d]))
    assert both == [polys, [], polys]
    with pytest.raises(ValueError, match="uint8"):
        polygons.building_polygons(pre_d.int())


def test_cli_on_a_png_pair_equals_the_restatement(tmp_path):
    from PIL import Image
    from xview2_amd.utils import buildings, polygons
    pre, post = _scene(71, 70, 90)
    Image.fromarray(pre).save(str(tmp_path / "pre.png"))
    Image.fromarray(post).save(str(tmp_path / "post.png"))
    out, want = str(tmp_path / "out.geojson"), str(tmp_path / "want.geojson")
    n = polygons.main([str(tmp_path / "pre.png"), str(tmp_path / "post.png"), out])
    _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
    records = buildings.to_records(BR.table(pre, post), 70, 90, confidence=False)
    assert n == len(records) > 3
    polygons.write_geojson(want, R.polygons(rings, verts), records)
    assert open(out, "rb").read() == open(want, "rb").read()
    # the same features as the dataset's own label layout
    polygons.write_xbd_json(str(tmp_path / "scene.json"), polygons.building_polygons(torch.from_numpy(pre).to(DEV)), records)
    xy = json.load(open(str(tmp_path / "scene.json")))["features"]["xy"]
    assert [f["properties"]["uid"] for f in xy] == ["scene-%d" % (i + 1) for i in range(n)]
    assert [f["properties"]["subtype"] for f in xy] == [polygons.DAMAGE_NAMES[r["damage"]] for r in records]


def test_cli_post_process_writes_one_geojson_per_pair(tmp_path):
    import postproc_ref as P
    from xview2_amd.utils import buildings, post_process
    os.makedirs(str(tmp_path / "probs"))
    for k, seed in enumerate((81, 85)):
        cls = np.where(BR.blobs(seed, 70, 90, thresh=0.56), 1 + BR._hash(seed + 1, (70, 90), 4), 0)
        np.save(str(tmp_path / "probs" / ("test_localization_%05d.npy" % k)), P.loc_from_mask(seed + 2, cls > 0))
        np.save(str(tmp_path / "probs" / ("test_damage_%05d.npy" % k)), P.probs_from_classes(seed + 3, cls, 4))
    args = post_process.get_parser().parse_args(["--results", str(tmp_path), "--components", "--polygons"])
    assert post_process.run(args) == 2
    for k in range(2):
        rows = buildings.read_csv(str(tmp_path / "buildings" / ("test_buildings_%05d.csv" % k)))      # implied by --polygons
        doc = json.load(open(str(tmp_path / "buildings" / ("test_buildings_%05d.geojson" % k))))
        assert len(doc["features"]) == len(rows) > 1
        assert [f["properties"]["id"] for f in doc["features"]] == [r["id"] for r in rows]
        assert [f["properties"]["area"] for f in doc["features"]] == [r["area"] for r in rows]


def test_cli_predict_writes_one_feature_per_table_row(tmp_path):
    import main as cli
    from PIL import Image
    from xview2_amd import predict
    from xview2_amd.utils import buildings
    common = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
              "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3", "--exec_mode", "train", "--epochs", "1"]
    cli.main(common + ["--type", "pre", "--loss_str", "dice", "--results", str(tmp_path / "loc")])
    g = torch.Generator().manual_seed(9)
    Image.fromarray(torch.randint(0, 256, (96, 80, 3), generator=g, dtype=torch.uint8).numpy()).save(str(tmp_path / "scene.png"))
    out = str(tmp_path / "out")
    flags = ["--ckpt_loc", str(tmp_path / "loc" / "checkpoints" / "last.ckpt"), "--pre", str(tmp_path / "scene.png"),
             "--window", "64", "--overlap", "16", "--batch", "2", "--precision", "32", "--out", out]
    assert predict.main(flags + ["--polygons"]) == 1
    rows = buildings.read_csv(os.path.join(out, "scene_buildings.csv"))
    doc = json.load(open(os.path.join(out, "scene_buildings.geojson")))
    assert len(doc["features"]) == len(rows)
    assert [f["properties"]["area"] for f in doc["features"]] == [r["area"] for r in rows]
    pre = np.asarray(Image.open(os.path.join(out, "scene_localization_prediction.png")))
    _, rings, verts, _ = R.trace(R.labels_of(pre)[None])
    assert [f["geometry"]["coordinates"] for f in doc["features"]] == [
        [r + r[:1] for r in [p["exterior"]] + p["holes"]] for p in R.polygons(rings, verts)]
