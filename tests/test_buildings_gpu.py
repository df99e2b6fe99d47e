"""The per-building table on the MI355X (csrc/buildings.hip through ops.building_table, utils/buildings.py and the two
CLIs) against the scipy restatement of tests/buildings_ref.py.  Every column is an integer, so every comparison is
np.array_equal.  Each kernel call runs between canary stretches around rows, count and the workspace, and its inputs are
compared with their copies afterwards."""
import json
import os

import numpy as np
import pytest
import torch

import buildings_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of rows (int64) and count (int32)
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = -7


def _labels(mask):
    from xview2_amd import ops
    return ops.label_components(torch.from_numpy(np.ascontiguousarray(mask)).to(DEV))


def _call(labels, dmg, loc, max_rows, stream=None):
    """xv2_building_table on caller-owned buffers -> (rows [B,max_rows,16] numpy, count [B] numpy); asserts the canaries"""
    from xview2_amd import _capi
    B, H, W = labels.shape
    need = int(_capi.query("xv2_building_table_workspace", B, H, W))
    assert need > 0
    rbuf = torch.full((2 * CAN + B * max_rows * 16,), FILL, dtype=torch.int64, device=DEV)
    cbuf = torch.full((2 * CAN + B,), FILL, dtype=torch.int32, device=DEV)
    wbuf = torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)
    rows = rbuf[CAN:CAN + B * max_rows * 16].view(B, max_rows, 16)
    count = cbuf[CAN:CAN + B]
    ws = wbuf[CAN_WS:CAN_WS + need]
    keep = [labels.clone(), dmg.clone(), None if loc is None else loc.clone()]
    torch.cuda.synchronize()
    if stream is None:
        _capi.call("xv2_building_table", labels, dmg, loc, B, H, W, max_rows, ws, rows, count)
        torch.cuda.synchronize()
        got = rows.cpu().numpy(), count.cpu().numpy()
    else:
        with torch.cuda.stream(stream):      # the copies are ordered by the stream alone: no device-wide wait
            _capi.call("xv2_building_table", labels, dmg, loc, B, H, W, max_rows, ws, rows, count)
            got = rows.cpu().numpy(), count.cpu().numpy()
        torch.cuda.synchronize()
    for buf, can, what in ((rbuf, CAN, "rows"), (cbuf, CAN, "count"), (wbuf, CAN_WS, "workspace")):
        want = FILL if buf is not wbuf else 0xA5
        assert bool((buf[:can] == want).all()) and bool((buf[-can:] == want).all()), what + ": canary overwritten"
    assert torch.equal(labels, keep[0]) and torch.equal(dmg, keep[1]), "an input was written"
    if loc is not None:
        assert torch.equal(loc.view(torch.int32), keep[2].view(torch.int32)), "loc was written"
    return got


def _check(masks, dmgs, locs, max_rows=None, stream=None):
    """B tiles of one shape against the restatement -> (rows, count) as returned"""
    masks = np.stack(masks)
    want = [R.table(m, d, None if locs is None else l) for m, d, l in zip(masks, dmgs, locs or [None] * len(masks))]
    labels = _labels(masks)
    dmg = torch.from_numpy(np.stack(dmgs)).to(DEV)
    loc = None if locs is None else torch.from_numpy(np.stack(locs)).to(DEV)
    if max_rows is None:
        max_rows = max(1, max(len(w) for w in want)) + 3
    rows, count = _call(labels, dmg, loc, max_rows, stream)
    assert count.tolist() == [len(w) for w in want]
    for b, w in enumerate(want):
        n = min(len(w), max_rows)
        assert np.array_equal(rows[b, :n], w[:n]), _first_diff(rows[b, :n], w[:n], b)
        assert np.all(rows[b, n:] == FILL), "tile %d: storage behind row %d was written" % (b, n)
    return rows, count


def _first_diff(got, want, b):
    r, c = np.nonzero(got != want)
    return "tile %d: %d cells differ, first row %d col %d: %d != %d\n%s\n%s" % (
        b, len(r), r[0], c[0], got[r[0], c[0]], want[r[0], c[0]], got[r[0]], want[r[0]])


# ---- shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.shape_cases()))
def test_shape_cases_equal_restatement(name):
    mask, dmg, loc = R.case_inputs(name, R.shape_cases()[name])
    rows, count = _check([mask], [dmg], [loc])
    if name == "empty_70":
        assert count.tolist() == [0] and np.all(rows == FILL)
    if name == "checker_64":
        assert count.tolist() == [2048]              # 1024 roots in each 64 x 32 region: the LDS table exactly full
    if name == "checker_128x96":
        assert count.tolist() == [6144]
    if name == "diagonals":
        assert np.all(rows[0, :count[0], 1] == 1)    # pixels that touch only diagonally stay distinct


def test_full_2100_needs_64_bit_sums():
    H = W = 2100
    mask = np.ones((H, W), dtype=bool)
    dmg = np.full((H, W), 4, dtype=np.uint8)
    loc = np.full((H, W), 1.0, dtype=np.float32)
    rows, count = _check([mask], [dmg], [loc], max_rows=2)
    assert count.tolist() == [1]
    s = W * (H * (H - 1) // 2)
    assert s == 4628295000 > 2 ** 32
    assert rows[0, 0].tolist() == [0, H * W, 0, 0, H - 1, W - 1, s, s, 0, 0, 0, H * W, 0, 4, 65535 * H * W, 0]


def test_scan_carries_over_more_than_one_round_of_chunks():
    """2060 x 2100 pixels are 1057 chunks of 4096, more than the 1024 the scan takes per round: the ranks of the roots in
    the last chunks need the carry"""
    H, W = 2060, 2100
    mask = R.blobs(91, H, W, thresh=0.54, box=9)
    rows, count = _check([mask], [R.dmg_for(92, (H, W))], None)
    assert count[0] > 10000 and rows[0, count[0] - 1, 0] > 1024 * 4096


# ---- batch and capacity -------------------------------------------------------------------------------------------------
def test_batch_of_three_with_an_empty_middle_tile_equals_single_runs():
    shape = (70, 130)
    masks = [R.blobs(21, *shape), np.zeros(shape, dtype=bool), R.blobs(22, *shape, thresh=0.52)]
    dmgs = [R.dmg_for(30 + i, shape) for i in range(3)]
    locs = [R.loc_for(40 + i, shape) for i in range(3)]
    rows, count = _check(masks, dmgs, locs, max_rows=200)
    assert count[1] == 0 and count[0] > 1 and count[2] > 1 and count[0] != count[2]
    for b in range(3):
        r1, c1 = _check([masks[b]], [dmgs[b]], [locs[b]], max_rows=200)
        assert c1[0] == count[b] and np.array_equal(r1[0], rows[b])


def _tile_with(n_components):
    """a 40 x 60 tile with exactly n separate 2 x 2 blocks"""
    mask = np.zeros((40, 60), dtype=bool)
    k = 0
    for y in range(0, 39, 3):
        for x in range(0, 59, 3):
            if k < n_components:
                mask[y:y + 2, x:x + 2] = True
                k += 1
    assert k == n_components
    return mask


@pytest.mark.parametrize("max_rows", [5, 1])
def test_capacity_below_the_count(max_rows):
    mask = _tile_with(37)
    dmg, loc = R.dmg_for(5, mask.shape), R.loc_for(6, mask.shape)
    rows, count = _check([mask], [dmg], [loc], max_rows=max_rows)
    assert count.tolist() == [37] and rows.shape == (1, max_rows, 16) and np.all(rows != FILL)


# ---- content ---------------------------------------------------------------------------------------------------------------
def test_damage_values_ties_and_confidence_specials():
    mask = np.zeros((12, 80), dtype=bool)
    dmg = np.zeros((12, 80), dtype=np.uint8)
    loc = np.zeros((12, 80), dtype=np.float32)
    special = np.concatenate([np.array([np.nan, np.inf, -np.inf, -1, 2, 0, 1, 0.5], dtype=np.float32), R.halfway_values()])
    rows_of = {0: [0, 1, 2, 3, 4, 5, 255, 1, 2],          # every kind of value inside one building
               2: [1, 1, 2, 2, 0, 5],                      # n1 == n2                  -> 1
               4: [2, 2, 4, 4, 1, 255],                    # n2 == n4 > n1             -> 2
               6: [0, 5, 255, 0],                          # all four zero             -> 0
               8: [3, 4, 4, 3, 3, 4],                      # n3 == n4                  -> 3
               10: [4] * len(special)}                     # one pixel per special loc value
    for y, vals in rows_of.items():
        mask[y, 1:1 + len(vals)] = True
        dmg[y, 1:1 + len(vals)] = vals
        loc[y, 1:1 + len(vals)] = special[:len(vals)] if y != 10 else special
    dmg[~mask] = 3                                          # background damage must not be counted
    loc[~mask] = 0.75
    rows, count = _check([mask], [dmg], [loc])
    assert rows[0, :6, 13].tolist() == [1, 1, 2, 0, 3, 4]
    assert rows[0, 0, 8:13].tolist() == [2, 2, 1, 1, 3]
    assert rows[0, 5, 14] == int(R.quantise(special).sum())
    # single pixels: the rounding of every special value on its own
    one = np.zeros((2, 2 * len(special)), dtype=bool)
    one[0, ::2] = True
    l1 = np.zeros(one.shape, dtype=np.float32)
    l1[0, ::2] = special
    r1, _ = _check([one], [np.ones(one.shape, np.uint8)], [l1])
    assert r1[0, :len(special), 14].tolist() == R.quantise(special).tolist()
    assert r1[0, 7, 14] == 32768                            # 0.5f * 65535 = 32767.5 -> even
    # no localization map: column 14 is all 0
    r0, c0 = _check([mask], [dmg], None)
    assert not r0[0, :c0[0], 14].any() and np.array_equal(r0[0, :c0[0], :14], rows[0, :count[0], :14])


# ---- behaviour -------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_equal_bits():
    shape = (130, 200)
    mask, dmg, loc = R.blobs(51, *shape), R.dmg_for(52, shape), R.loc_for(53, shape)
    a, ca = _check([mask], [dmg], [loc])
    b, cb = _check([mask], [dmg], [loc])
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    c, cc = _check([mask], [dmg], [loc], stream=torch.cuda.Stream())
    assert np.array_equal(a, c) and np.array_equal(ca, cc)


def test_kernels_are_named_by_the_profiler():
    from tests.test_f16x2_gpu import _prof
    from xview2_amd import ops
    mask = R.blobs(61, 65, 65)
    labels = _labels(mask[None])
    with _prof() as pr:
        ops.building_table(labels, torch.ones((1, 65, 65), dtype=torch.uint8, device=DEV))
        names = pr.names()
    for k in ("bt_count_kernel", "bt_scan_kernel", "bt_rank_kernel", "bt_accum_kernel", "bt_finish_kernel"):
        assert k in names, names


def test_ops_binding_checks_and_defaults():
    from xview2_amd import ops
    mask = R.blobs(62, 33, 47)
    labels = _labels(mask[None])
    dmg = torch.from_numpy(R.dmg_for(63, (1, 33, 47))).to(DEV)
    rows, count = ops.building_table(labels, dmg)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (1, 1024, 16) and count.dtype == torch.int32
    want = R.table(mask, dmg[0].cpu().numpy())
    assert int(count[0]) == len(want) and np.array_equal(rows[0, :len(want)].cpu().numpy(), want)
    with pytest.raises(ValueError, match="int32"):
        ops.building_table(labels.long(), dmg)
    with pytest.raises(ValueError, match="uint8"):
        ops.building_table(labels, dmg.int())
    with pytest.raises(ValueError, match="uint8"):
        ops.building_table(labels, dmg[:, :5])
    with pytest.raises(ValueError, match="fp32"):
        ops.building_table(labels, dmg, loc=dmg)
    with pytest.raises(ValueError, match="max_rows"):
        ops.building_table(labels, dmg, max_rows=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.building_table(labels.cpu(), dmg)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _pair(seed, H, W):
    import postproc_ref as P
    # thresh 0.56: sparse enough that a 3 x 3 dilation leaves some tens of separate buildings (0.5 dilates into one)
    cls = np.where(R.blobs(seed, H, W, thresh=0.56), 1 + R._hash(seed + 1, (H, W), 4), 0)
    return P.loc_from_mask(seed + 2, cls > 0), P.probs_from_classes(seed + 3, cls, 4)


def test_post_processed_pair_to_table_and_the_retry_path():
    from xview2_amd.utils import buildings
    from xview2_amd.utils.post_process import post_process_tiles
    loc, dmg = _pair(71, 96, 80)
    loc_d = torch.from_numpy(loc).to(DEV)
    pre, post = post_process_tiles(loc_d, torch.from_numpy(dmg).to(DEV), components=True, dilate=True)
    want = R.table(pre.cpu().numpy(), post.cpu().numpy(), loc)
    assert len(want) > 3
    got = buildings.building_table(pre, post, loc_d)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    # a first capacity below the count: one more run with the capacity the count asks for
    assert np.array_equal(buildings.building_table(pre, post, loc_d, capacity=2), want)
    # batched input gives a list; without loc column 14 stays 0
    both = buildings.building_table(torch.stack([pre, torch.zeros_like(pre)]), torch.stack([post, post]))
    assert len(both) == 2 and both[1].shape == (0, 16) and np.array_equal(both[0][:, :14], want[:, :14])
    assert not both[0][:, 14].any()


@pytest.fixture(scope="module")
def predict_flags(tmp_path_factory):
    import main as cli
    from PIL import Image
    tmp = tmp_path_factory.mktemp("buildings_cli")
    common = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
              "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3", "--exec_mode", "train", "--epochs", "1",
              "--ema_decay", "0.9"]
    cli.main(common + ["--type", "pre", "--loss_str", "dice", "--results", str(tmp / "loc")])
    cli.main(common + ["--type", "post", "--dmg_model", "siamese", "--loss_str", "focal+dice", "--results", str(tmp / "dmg")])
    g = torch.Generator().manual_seed(9)
    for name in ("scene_pre.png", "scene_post.png"):
        Image.fromarray(torch.randint(0, 256, (96, 80, 3), generator=g, dtype=torch.uint8).numpy()).save(str(tmp / name))
    return tmp, ["--ckpt_loc", str(tmp / "loc" / "checkpoints" / "last.ckpt"), "--ckpt_dmg",
                 str(tmp / "dmg" / "checkpoints" / "last.ckpt"), "--pre", str(tmp / "scene_pre.png"), "--post",
                 str(tmp / "scene_post.png"), "--window", "64", "--overlap", "16", "--batch", "2", "--precision", "32"]


def test_cli_predict_writes_the_table_of_its_pngs(predict_flags):
    from PIL import Image
    from xview2_amd import predict
    from xview2_amd.utils import buildings
    tmp, flags = predict_flags
    out = str(tmp / "with")
    assert predict.main(flags + ["--out", out, "--components", "--dilate", "--save_probs", "--buildings"]) == 1
    pre = np.asarray(Image.open(os.path.join(out, "scene_pre_localization_prediction.png")))
    post = np.asarray(Image.open(os.path.join(out, "scene_pre_damage_prediction.png")))
    loc = np.load(os.path.join(out, "scene_pre_localization_probs.npy"))[0]
    want = buildings.to_records(R.table(pre, post, loc), 96, 80)
    got = buildings.read_csv(os.path.join(out, "scene_pre_buildings.csv"))
    assert got == want
    s = json.load(open(os.path.join(out, "scene_pre_buildings.json")))
    assert s["buildings"] == len(want) == sum(s["buildings_per_damage"])
    assert sum(s["pixels_per_damage"]) == int((pre != 0).sum())
    # the stand-alone tool on the two PNGs: the same integers, no confidence
    csv2 = str(tmp / "again.csv")
    n = buildings.main([os.path.join(out, "scene_pre_localization_prediction.png"),
                        os.path.join(out, "scene_pre_damage_prediction.png"), csv2])
    assert n == len(want)
    assert buildings.read_csv(csv2) == [{k: v for k, v in r.items() if k != "confidence"} for r in want]


def test_cli_predict_without_the_flag_writes_no_table(predict_flags):
    from xview2_amd import predict
    tmp, flags = predict_flags
    out = str(tmp / "without")
    assert predict.main(flags + ["--out", out, "--components", "--dilate"]) == 1
    assert sorted(os.listdir(out)) == ["scene_pre_damage_prediction.png", "scene_pre_localization_prediction.png"]


def test_cli_post_process_writes_one_csv_per_pair(tmp_path):
    from PIL import Image
    from xview2_amd.utils import buildings, post_process
    os.makedirs(str(tmp_path / "probs"))
    pairs = [_pair(81, 70, 90), _pair(85, 70, 90)]
    for k, (loc, dmg) in enumerate(pairs):
        np.save(str(tmp_path / "probs" / ("test_localization_%05d.npy" % k)), loc)
        np.save(str(tmp_path / "probs" / ("test_damage_%05d.npy" % k)), dmg)
    args = post_process.get_parser().parse_args(["--results", str(tmp_path), "--components", "--buildings"])
    assert post_process.run(args) == 2
    for k, (loc, _) in enumerate(pairs):
        pre = np.asarray(Image.open(str(tmp_path / "predictions" / ("test_localization_%05d_prediction.png" % k))))
        post = np.asarray(Image.open(str(tmp_path / "predictions" / ("test_damage_%05d_prediction.png" % k))))
        want = buildings.to_records(R.table(pre, post, loc), 70, 90)
        assert len(want) > 1
        assert buildings.read_csv(str(tmp_path / "buildings" / ("test_buildings_%05d.csv" % k))) == want
    args = post_process.get_parser().parse_args(["--results", str(tmp_path / "none")])
    os.makedirs(str(tmp_path / "none" / "probs"))
    assert post_process.run(args) == 0 and not os.path.exists(str(tmp_path / "none" / "buildings"))
