"""Registering the post image to the pre image on the MI355X (csrc/align.hip through xv2_align_estimate, xv2_translate_u8,
ops.align_estimate / translate_u8, scene.align_pair and utils/align.py) against the host restatement of tests/align_ref.py.
Every value is an integer, so every comparison is np.array_equal / torch.equal.  Each direct call runs between canary
stretches around all outputs and the workspace, and its inputs are compared with their copies afterwards."""

import numpy as np
import pytest
import torch

import align_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of every output
CAN_WS = 256        # canary bytes on either side of the workspace
FILL = 0x5A

CASES = ([(1, 3, 3, 1, 32)] + [(1, 2 * R + 1, 2 * R + 5, R, 32) for R in (1, 2, 3)] + [(1, 7, W, 3, 32) for W in (7, 8, 9, 10)] +
         [(1, 37, 41, 3, 32), (2, 70, 67, 5, 32), (1, 97, 101, 32, 32), (1, 131, 203, 16, 64), (1, 200, 197, 32, 128),
          (1, 300, 290, 2, 128)])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(n, dtype, fill=FILL):
    buf = torch.full((2 * CAN + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, what, fill=FILL, can=CAN):
    assert bool((buf[:can] == fill).all()) and bool((buf[-can:] == fill).all()), what + ": canary overwritten"


def _estimate(pre, post, R, T, stream=None):
    """xv2_align_estimate on caller-owned buffers between canaries; pre, post uint8 [B,H,W,3] (numpy) -> numpy int64
    (block_sad [B,nby,nbx,D,D], sad [B,D,D], block_shift [B,nby,nbx,2], shift [B,2]) and the device shift"""
    from xview2_amd import _capi
    p, q = _dev(pre), _dev(post)
    kp, kq = p.clone(), q.clone()
    B, H, W, _ = p.shape
    D = 2 * R + 1
    nby, nbx = A.grid(H, W, R, T)
    need = int(_capi.query("xv2_align_workspace", B, H, W, R, T))
    assert need > 0
    ws_buf = torch.full((2 * CAN_WS + need,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = ws_buf[CAN_WS:CAN_WS + need]
    bs_buf, bs = _guarded(B * nby * nbx * D * D, torch.int32)      # (the same 32 bits as uint32; entries stay below 2^22)
    sad_buf, sad = _guarded(B * D * D, torch.int64)
    bsh_buf, bsh = _guarded(B * nby * nbx * 2, torch.int32)
    sh_buf, sh = _guarded(B * 2, torch.int32)
    torch.cuda.synchronize()
    if stream is None:
        _capi.call("xv2_align_estimate", p, q, B, H, W, R, T, ws, bs, sad, bsh, sh)
    else:
        with torch.cuda.stream(stream):
            _capi.call("xv2_align_estimate", p, q, B, H, W, R, T, ws, bs, sad, bsh, sh)
    torch.cuda.synchronize()
    for buf, what in ((bs_buf, "block_sad"), (sad_buf, "sad"), (bsh_buf, "block_shift"), (sh_buf, "shift")):
        _intact(buf, what)
    _intact(ws_buf, "workspace", 0xA5, CAN_WS)
    assert torch.equal(p, kp) and torch.equal(q, kq), "an input was written"
    out = (bs.cpu().numpy().astype(np.int64).reshape(B, nby, nbx, D, D), sad.cpu().numpy().reshape(B, D, D),
           bsh.cpu().numpy().astype(np.int64).reshape(B, nby, nbx, 2), sh.cpu().numpy().astype(np.int64).reshape(B, 2))
    return out, sh.view(B, 2)


def _translate(src, shift_dev):
    """xv2_translate_u8 on a caller-owned out between canaries; src uint8 [B,H,W,C] (numpy), shift a device int32 [B,2]"""
    from xview2_amd import _capi
    s = _dev(src)
    keep, keep_shift = s.clone(), shift_dev.clone()
    B, H, W, C = s.shape
    buf, out = _guarded(B * H * W * C, torch.uint8)
    torch.cuda.synchronize()
    _capi.call("xv2_translate_u8", s, B, H, W, C, shift_dev, out)
    torch.cuda.synchronize()
    _intact(buf, "out")
    assert torch.equal(s, keep) and torch.equal(shift_dev, keep_shift), "an input was written"
    return out.cpu().numpy().reshape(B, H, W, C)


def _reference(pre, post, R, T):
    res = [A.estimate(pre[b], post[b], R, T) for b in range(pre.shape[0])]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def _check(pre, post, R, T, what):
    got, _ = _estimate(pre, post, R, T)
    want = _reference(pre, post, R, T)
    for g, w, name in zip(got, want, ("block_sad", "sad", "block_shift", "shift")):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs in %d entries" % (what, name, int((g != w).sum()))
    return got


# ---- contents ------------------------------------------------------------------------------------------------------------
def _noise(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _ramp(B, H, W):
    """x & 255 in all channels (luma = x & 255): a shift of the row changes nothing, so whole columns of the table tie"""
    img = np.empty((B, H, W, 3), np.uint8)
    img[...] = (np.arange(W) & 255).astype(np.uint8)[None, None, :, None]
    return img


def _planted_patch(seed, H, W, d, y0, x0):
    """post(p + d) = pre(p), except a 32 x 32 patch of post at (y0, x0) that is noise"""
    pre, post = A.planted(seed, H, W, d)
    post = post.copy()
    post[y0:y0 + 32, x0:x0 + 32] = np.random.default_rng(seed + 1).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    return pre, post


# ---- the case table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,R,T", CASES)
def test_tables_and_shifts_equal_the_restatement(B, H, W, R, T):
    _check(_noise(H * W + R, B, H, W), _noise(H * W + R + 1, B, H, W), R, T, "noise")
    ramp = _ramp(B, H, W)
    got = _check(ramp, ramp, R, T, "ramp")
    assert not got[3].any() and not got[2].any()                        # every dy ties at dx = 0: the shortest shift wins
    if T == 128:
        got = _check(np.zeros((B, H, W, 3), np.uint8), np.full((B, H, W, 3), 255, np.uint8), R, T, "0 against 255")
        ny, nx = (H - 2 * R) // T, (W - 2 * R) // T                     # the full tiles
        assert np.all(got[0][:, :ny, :nx] == 255 * 128 * 128) and np.all(got[3] == 0)
        if (H, W) == (300, 290):
            assert (ny, nx) == (2, 2)
    if min(H, W) >= 70:
        d = (-(R // 2) - 1, R)
        pairs = [_planted_patch(H + W + b, H, W, d, H // 2 - 9, W // 2 - 20) for b in range(B)]
        got = _check(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), R, T, "planted")
        assert np.all(got[3] == np.array(d))


@pytest.mark.parametrize("R", [12, 16, 21, 22, 27])
def test_radii_around_the_largest_banded_plan(R):
    """T = 128 asks for the most LDS; up to R = 21 the rows of a tile are split into bands whose sums meet in LDS, from
    R = 22 on a thread walks the whole tile.  Small interiors: the plan depends on R and T only."""
    H, W = 2 * R + 19, 2 * R + 23
    _check(_noise(R, 1, H, W), _noise(R + 100, 1, H, W), R, 128, "noise")


def test_four_way_tie_goes_to_the_smallest_dy():
    """one bright pixel in pre, its four neighbours bright in post: (0, 1), (1, 0), (0, -1) and (-1, 0) tie"""
    pre, post = np.zeros((1, 40, 45, 3), np.uint8), np.zeros((1, 40, 45, 3), np.uint8)
    pre[0, 20, 22] = 255
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        post[0, 20 + dy, 22 + dx] = 255
    got = _check(pre, post, 2, 32, "four-way tie")
    assert got[1][0, 2, 3] == got[1][0, 3, 2] == got[1][0, 2, 1] == got[1][0, 1, 2] == 3 * 255 == got[1].min()
    assert got[3].tolist() == [[-1, 0]]
    shifted = np.roll(_ramp(1, 40, 45), 3, axis=2)                      # the ramp moved: every dy ties at dx = 3
    assert _check(_ramp(1, 40, 45), shifted, 4, 32, "ramp")[3].tolist() == [[0, 3]]


def test_a_patch_of_noise_leaves_the_global_shift_and_one_tile_disagrees():
    from xview2_amd.utils import align
    H, W, R, T, d = 150, 170, 5, 32, (3, -4)
    # the patch covers tile (2, 3) under the shift: post rows R + 64 + dy ..., columns R + 96 + dx ...
    pre, post = _planted_patch(9, H, W, d, R + 64 + d[0], R + 96 + d[1])
    got = _check(pre[None], post[None], R, T, "patch")
    rep = align.summarise(got[0][0], got[1][0], got[2][0], got[3][0], R, T, H, W)
    want = A.estimate(pre, post, R, T)
    assert rep == align.summarise(want[0], want[1], want[2], want[3], R, T, H, W)
    nby, nbx = A.grid(H, W, R, T)
    assert rep["shift"] == list(d) and rep["blocks"]["grid"] == [nby, nbx] and rep["blocks"]["flat"] == 0
    assert rep["blocks"]["agree"] == nby * nbx - 1 and rep["blocks"]["shifts"][2][3] != list(d)
    assert rep["blocks"]["spread"] > 0 and rep["sad_best"] > 0 and rep["at_limit"] is False


# ---- the resampler -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 6])
def test_translate_equals_the_restatement(C):
    rng = np.random.default_rng(40 + C)
    for H, W, shifts in ((37, 41, [(0, 0)]), (37, 41, [(-3, 5)]), (37, 41, [(32, -32)]), (3, 5, [(32, 0)]), (3, 5, [(-32, 7)]),
                         (1, 1, [(5, -5)]), (33, 29, [(4, -9), (-31, 30)])):
        src = rng.integers(0, 256, (len(shifts), H, W, C), dtype=np.uint8)
        got = _translate(src, _dev(np.array(shifts, np.int32)))
        for b, (dy, dx) in enumerate(shifts):
            assert np.array_equal(got[b], A.translate(src[b], dy, dx)), (H, W, C, dy, dx)
    src = rng.integers(0, 256, (1, 4, 6, C), dtype=np.uint8)
    big = 2 ** 31 - 1
    got = _translate(src, _dev(np.array([[big, -big - 1]], np.int32)))
    assert np.array_equal(got[0], A.translate(src[0], big, -big - 1))


def test_estimate_then_translate_without_a_read_back():
    H, W, R, d = 131, 203, 16, (7, -16)
    pre, post = A.planted(1, H, W, d)
    _, shift_dev = _estimate(pre[None], post[None], R, 64)
    aligned = _translate(post[None], shift_dev)[0]
    assert shift_dev.cpu().tolist() == [list(d)]
    assert np.array_equal(aligned[R:H - R, R:W - R], pre[R:H - R, R:W - R])
    assert np.array_equal(aligned, A.translate(post, *d))


def test_the_same_bytes_on_every_run_and_stream():
    pre, post = _noise(70, 2, 131, 140), _noise(71, 2, 131, 140)
    first, _ = _estimate(pre, post, 6, 32)
    again, _ = _estimate(pre, post, 6, 32)
    side, _ = _estimate(pre, post, 6, 32, stream=torch.cuda.Stream())
    for a, b, c in zip(first, again, side):
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- through the modules -------------------------------------------------------------------------------------------------
def test_ops_bindings_and_their_argument_checks():
    from xview2_amd import ops
    pre, post = A.planted(3, 70, 67, (-5, 5))
    bs, sad, bsh, sh = ops.align_estimate(_dev(pre[None]), _dev(post[None]), 5, 32)
    want = A.estimate(pre, post, 5, 32)
    for g, w in zip((bs, sad, bsh, sh), want):
        assert np.array_equal(g[0].cpu().numpy().astype(np.int64), w)
    assert (bs.dtype, sad.dtype, bsh.dtype, sh.dtype) == (torch.int32, torch.int64, torch.int32, torch.int32)
    assert np.array_equal(ops.translate_u8(_dev(post[None]), sh)[0].cpu().numpy(), A.translate(post, -5, 5))
    for bad in (lambda: ops.align_estimate(_dev(pre[None]), _dev(post[None]), 33, 32),
                lambda: ops.align_estimate(_dev(pre[None]), _dev(post[None]), 5, 48),
                lambda: ops.align_estimate(_dev(pre[None]), _dev(post[None, :60]), 5, 32),
                lambda: ops.align_estimate(_dev(pre[None, :10]), _dev(post[None, :10]), 5, 32),
                lambda: ops.align_estimate(_dev(pre), _dev(post), 5, 32),
                lambda: ops.translate_u8(_dev(post[None]), torch.zeros((1, 2), dtype=torch.int32)),
                lambda: ops.translate_u8(_dev(post[None]), sh.long())):
        with pytest.raises(ValueError):
            bad()


def test_alignment_before_scene_prediction():
    """what predict --align does, without a checkpoint: the maps of the aligned pair equal those of the pair that was never
    shifted, on the interior"""
    from xview2_amd import scene
    from xview2_amd.utils import align
    H, W, R, d = 150, 170, 6, (4, -6)
    rng = np.random.default_rng(12)
    pre = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    post0 = (pre.astype(np.int64) + rng.integers(-6, 7, pre.shape)).clip(0, 255).astype(np.uint8)     # the registered post
    post = np.roll(post0, d, (0, 1))

    def model(img):     # logits that depend on the pixel's own six values only: [K, 3, n, n]
        v = img.u8.float()
        return torch.stack([(v[..., 3] - v[..., 0]) / 16.0, (v[..., 4] - v[..., 1]) / 16.0, (v[..., 5] + v[..., 2]) / 128.0 - 2.0],
                           dim=1).contiguous()

    aligned, info = scene.align_pair(_dev(pre), _dev(post), R, 64)
    rep = align.report_of(info, H, W)
    assert rep["shift"] == list(d) and rep["blocks"]["agree"] == 3 * 3 and rep["sad_best"] < rep["sad_zero"]
    predictor = scene.ScenePredictor(model, window=64, overlap=16, kind=scene.SIGMOID, batch=4)
    got = predictor.predict(_dev(pre), aligned)
    want = predictor.predict(_dev(pre), _dev(post0))
    wrong = predictor.predict(_dev(pre), _dev(post))
    assert tuple(got.shape) == (3, H, W)
    assert torch.equal(got[:, R:H - R, R:W - R], want[:, R:H - R, R:W - R])
    assert not torch.equal(wrong[:, R:H - R, R:W - R], want[:, R:H - R, R:W - R])
    assert np.array_equal(aligned.cpu().numpy(), A.translate(post, *d))


def test_command_line_on_pngs(tmp_path):
    from PIL import Image
    from xview2_amd.utils import align
    H, W, R, T, d = 90, 75, 4, 32, (-2, 3)
    pre, post = _planted_patch(21, H, W, d, 40, 30)                  # as read_bgr gives them: stored channel order B, G, R
    Image.fromarray(pre[:, :, ::-1]).save(tmp_path / "pre.png")
    Image.fromarray(post[:, :, ::-1]).save(tmp_path / "post.png")
    out, js = tmp_path / "aligned.png", tmp_path / "report.json"
    assert align.main([str(tmp_path / "pre.png"), str(tmp_path / "post.png"), str(out), "--radius", str(R), "--tile", str(T),
                       "--json", str(js)]) == 1
    want = A.estimate(pre, post, R, T)
    assert js.read_bytes() == align.dumps(align.summarise(want[0], want[1], want[2], want[3], R, T, H, W)).encode()
    assert tuple(want[3]) == d
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB"))[:, :, ::-1], A.translate(post, *d))
    # directories: one entry per pair and the histogram of the shifts
    for k, dk in enumerate(((1, 0), (1, 0), (0, -2))):
        a, b = A.planted(30 + k, 40, 44, dk)
        (tmp_path / "P").mkdir(exist_ok=True)
        (tmp_path / "Q").mkdir(exist_ok=True)
        Image.fromarray(a[:, :, ::-1]).save(tmp_path / "P" / ("s%d.png" % k))
        Image.fromarray(b[:, :, ::-1]).save(tmp_path / "Q" / ("t%d.png" % k))
    assert align.main([str(tmp_path / "P"), str(tmp_path / "Q"), str(tmp_path / "O"), "--radius", "2", "--tile", "32"]) == 3
    import json
    rep = json.loads((tmp_path / "O" / "alignment.json").read_text())
    assert rep["histogram"] == [[0, -2, 1], [1, 0, 2]] and sorted(rep["pairs"]) == ["s0", "s1", "s2"]
    b2 = A.planted(32, 40, 44, (0, -2))[1]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "O" / "t2.png").convert("RGB"))[:, :, ::-1], A.translate(b2, 0, -2))


def test_cli_predict_align_equals_predicting_the_aligned_pair(tmp_path):
    """predict --align R = utils.align, then predict on its output: the same report, the same maps, the same PNG; and without
    the flag no report is written"""
    import os
    import main as cli
    from PIL import Image
    from xview2_amd import predict
    from xview2_amd.utils import align
    cli.main(["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
              "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "2", "--exec_mode", "train", "--epochs", "1",
              "--type", "post", "--dmg_model", "siamese", "--loss_str", "focal+dice", "--results", str(tmp_path / "dmg")])
    H, W, R, d = 96, 80, 5, (2, -4)
    pre, post = A.planted(17, H, W, d)
    Image.fromarray(pre[:, :, ::-1]).save(tmp_path / "scene_pre.png")
    Image.fromarray(post[:, :, ::-1]).save(tmp_path / "scene_post.png")
    flags = ["--ckpt_dmg", str(tmp_path / "dmg" / "checkpoints" / "last.ckpt"), "--pre", str(tmp_path / "scene_pre.png"),
             "--window", "64", "--overlap", "16", "--batch", "2", "--precision", "32", "--save_probs"]
    one, two, off = (str(tmp_path / k) for k in ("one", "two", "off"))
    assert predict.main(flags + ["--post", str(tmp_path / "scene_post.png"), "--out", one, "--align", str(R), "--align_tile", "32"]) == 1
    assert align.main([str(tmp_path / "scene_pre.png"), str(tmp_path / "scene_post.png"), str(tmp_path / "aligned.png"), "--radius",
                       str(R), "--tile", "32"]) == 1
    assert predict.main(flags + ["--post", str(tmp_path / "aligned.png"), "--out", two]) == 1
    assert predict.main(flags + ["--post", str(tmp_path / "scene_post.png"), "--out", off, "--align", "0"]) == 1
    report = open(os.path.join(one, "scene_pre_alignment.json"), "rb").read()
    assert report == (tmp_path / "aligned_alignment.json").read_bytes()
    want = A.estimate(pre, post, R, 32)
    assert report == align.dumps(align.summarise(want[0], want[1], want[2], want[3], R, 32, H, W)).encode() and tuple(want[3]) == d
    names = ["scene_pre_damage_prediction.png", "scene_pre_damage_probs.npy"]
    assert sorted(os.listdir(two)) == sorted(os.listdir(off)) == names
    assert sorted(os.listdir(one)) == sorted(names + ["scene_pre_alignment.json"])
    for name in names:
        assert open(os.path.join(one, name), "rb").read() == open(os.path.join(two, name), "rb").read(), name
    assert not np.array_equal(np.load(os.path.join(one, names[1])), np.load(os.path.join(off, names[1])))
