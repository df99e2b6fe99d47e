"""Scene inference on the GPU (csrc/scene.hip through xview2_amd/scene.py and xview2_amd/predict.py) against the float64
restatement and the bound of tests/scene_ref.py.  Windows of 32 and 64 are the smallest shapes at which these kernels can
go wrong; every axis class of scene_ref.SCENES is on both axes."""
import os

import numpy as np
import pytest
import torch

from tests import scene_ref as R

pytestmark = pytest.mark.gpu

CANARY = 64


def _geom(case):
    return case["H"], case["W"], case["n"], case["overlap"]


def _table(tab):
    return torch.tensor(tab, dtype=torch.int32).reshape(-1, 2).cuda()


def _norm(case):
    from xview2_amd import scene
    H, W, n, overlap = _geom(case)
    return (torch.from_numpy(scene.axis_normaliser(H, n, overlap)).cuda(),
            torch.from_numpy(scene.axis_normaliser(W, n, overlap)).cuda())


def _acc(cout, H, W):
    """zeroed accumulators between two canary stretches -> (buffer, view)"""
    buf = torch.full((2 * CANARY + cout * H * W,), 1234.5, dtype=torch.float32, device="cuda")
    acc = buf[CANARY:CANARY + cout * H * W].view(cout, H, W)
    acc.zero_()
    return buf, acc


def _run_blend(case, x, kind, splits=None, finalize=True):
    from xview2_amd import scene
    H, W, n, overlap = _geom(case)
    tab = _table(R.windows(H, W, n, overlap))
    K = tab.shape[0]
    buf, acc = _acc(1 if kind == R.SIGMOID1 else x.shape[1], H, W)
    xd = x.cuda()
    k0 = 0
    for m in splits or [K]:
        scene.blend(xd[k0:k0 + m].contiguous(), kind, tab[k0:k0 + m], overlap, acc)
        k0 += m
    assert k0 == K
    if finalize:
        scene.finalize(acc, *_norm(case))
    torch.cuda.synchronize()
    assert bool((buf[:CANARY] == 1234.5).all()) and bool((buf[-CANARY:] == 1234.5).all()), "canary overwritten"
    return acc.clone()


def _assert_within(y, ref, what):
    """outside the planted pixels: within the bound.  A planted pixel: NaN, or what the reference says."""
    y = y.detach().cpu().double()
    planted = ref["planted"].unsqueeze(0).expand_as(ref["out"])
    z = torch.zeros_like(ref["out"])
    ratio, where = R.check(torch.where(planted, z, y), torch.where(planted, z, ref["out"]), torch.where(planted, z, ref["bound"]))
    print("%s: worst error / bound %.4f at %d" % (what, ratio, where))
    assert ratio <= 1.0, (what, ratio, where)
    if bool(planted.any()):
        yp, rp, bp = y[planted], ref["out"][planted], ref["bound"][planted]
        ok = torch.isnan(yp) | (yp == rp) | ((yp - rp).abs() <= bp)
        assert bool(ok.all()), (what, yp, rp)


# ---- gather --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.SCENES, ids=R.name)
def test_gather_is_bit_equal_to_the_reference(case):
    from xview2_amd import scene
    H, W, n, overlap = _geom(case)
    pre, post = R.make_scene(case)
    tab = R.windows(H, W, n, overlap)
    assert tab == [tuple(t) for t in scene.scene_windows(H, W, n, overlap).tolist()]
    pre_d, post_d = torch.from_numpy(pre).cuda(), torch.from_numpy(post).cuda()
    for C, pd in ((3, None), (6, post_d)):
        nbytes = len(tab) * n * n * C
        buf = torch.full((2 * CANARY + nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[CANARY:CANARY + nbytes].view(len(tab), n, n, C)
        scene.gather_windows(pre_d, pd, _table(tab), n, out=out)
        torch.cuda.synchronize()
        want = R.gather(pre, post if C == 6 else None, tab, n)
        assert np.array_equal(out.cpu().numpy(), want), (R.name(case), C)
        assert bool((buf[:CANARY] == 0xA5).all()) and bool((buf[-CANARY:] == 0xA5).all()), "canary overwritten"


# ---- blend + finalize ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.SCENES, ids=R.name)
def test_blend_and_finalize_are_within_the_bound(case):
    H, W, n, overlap = _geom(case)
    tab = R.windows(H, W, n, overlap)
    for kind, C in R.KINDS:
        for regime in R.REGIMES:
            x = R.make_logits(case, len(tab), C, regime)
            ref = R.blend(x, kind, tab, n, overlap, H, W)
            if regime != "nonfinite":
                assert not bool(ref["planted"].any())
            _assert_within(_run_blend(case, x, kind), ref, "%s kind %d C %d %s" % (R.name(case), kind, C, regime))


@pytest.mark.parametrize("case", [R.SCENES[8], R.SCENES[11], R.SCENES[12]], ids=R.name)
def test_result_does_not_depend_on_how_the_windows_are_split(case):
    H, W, n, overlap = _geom(case)
    K = len(R.windows(H, W, n, overlap))
    assert K >= 6
    for kind, C in R.KINDS:
        x = R.make_logits(case, K, C, "pm80" if kind == R.SOFTMAX else "position")
        for fin in (False, True):
            whole = _run_blend(case, x, kind, finalize=fin)
            assert torch.equal(whole, _run_blend(case, x, kind, finalize=fin)), "two runs differ"
            assert torch.equal(whole, _run_blend(case, x, kind, [1] * K, finalize=fin)), "one window per call differs"
            assert torch.equal(whole, _run_blend(case, x, kind, [1, 3, K - 4], finalize=fin)), "1 + 3 + rest differs"


# ---- the predictor with a pointwise model ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,C,pair", [(R.SIGMOID1, 2, False), (R.SOFTMAX, 5, True)])
def test_pointwise_model_gives_the_same_function_of_the_whole_scene(kind, C, pair):
    """logits that depend only on the pixel's own value: all windows agree, so any misplacement shows"""
    from xview2_amd import scene
    case = R.SCENES[8]
    H, W, n, overlap = _geom(case)
    assert (H, W) == (49, 81)
    pre, post = R.make_scene(case, post=pair)
    ch = 3 if pair else 0
    g = torch.Generator().manual_seed(77)
    lut = (torch.randn((C, 256), generator=g) * 3.0).float()      # logit of channel c for a stored pixel value
    lut_d = lut.cuda()

    def model(img):
        v = img.u8[..., ch].long()                                  # [K, n, n]
        return lut_d[:, v].permute(1, 0, 2, 3).contiguous()

    both = pre if not pair else np.concatenate([pre, post], axis=2)
    got = scene.ScenePredictor(model, n, overlap, batch=4, kind=kind).predict(
        torch.from_numpy(pre).cuda(), torch.from_numpy(post).cuda() if pair else None)
    tab = R.windows(H, W, n, overlap)
    wins = torch.from_numpy(R.gather(pre, post, tab, n)[..., ch].astype(np.int64))
    ref = R.blend(lut[:, wins].permute(1, 0, 2, 3), kind, tab, n, overlap, H, W)
    whole, _ = R.decode(lut[:, torch.from_numpy(both[..., ch].astype(np.int64))].unsqueeze(0).double(), kind)
    assert float((ref["out"] - whole[0]).abs().max()) < 1e-12      # in float64 the blend of agreeing windows is the function
    ref["out"] = whole[0]
    assert tuple(got.shape) == tuple(whole[0].shape)
    _assert_within(got, ref, "pointwise kind %d" % kind)


# ---- real networks ---------------------------------------------------------------------------------------------------------

def _model(kind):
    import main as cli
    from xview2_amd.lightning import Model
    from xview2_amd.weights import deterministic_init_
    flags = ["--encoder", "resnet50", "--type", "pre", "--loss_str", "dice"] if kind == "loc" else [
        "--encoder", "resnet50", "--type", "post", "--dmg_model", "siamese", "--loss_str", "focal+dice"]
    torch.manual_seed(0)
    m = Model(cli.build_parser().parse_args(flags + ["--results", "."]))
    deterministic_init_(m.model, 1)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def loc_model():
    return _model("loc")


@pytest.fixture(scope="module")
def dmg_model():
    return _model("dmg")


def _scene_u8(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))


@pytest.mark.parametrize("tta", [False, True])
def test_one_window_without_overlap_is_the_model_itself(loc_model, tta):
    """scene = window = 64, overlap 0: every weight is 1, so nothing may round"""
    from xview2_amd import ops, scene
    pre, _ = _scene_u8(64, 64, 3)
    loc_model.args.tta = tta
    try:
        got = scene.ScenePredictor(loc_model, 64, 0, batch=4).predict(pre.cuda())
        with torch.no_grad():
            want = loc_model._decode(loc_model.forward(ops.DeviceImage(pre.cuda().unsqueeze(0))))
    finally:
        loc_model.args.tta = False
    assert tuple(got.shape) == (1, 64, 64) and torch.equal(got, want)


@pytest.mark.parametrize("which", ["loc", "dmg"])
def test_real_network_over_several_windows(loc_model, dmg_model, which):
    from xview2_amd import scene
    H, W, n, overlap = 80, 112, 64, 16
    pre, post = _scene_u8(H, W, 4)
    model = loc_model if which == "loc" else dmg_model
    seen = []

    def recording(img):
        logits = model(img)
        seen.append((img.u8.clone(), logits.clone()))
        return logits

    kind = R.SIGMOID1 if which == "loc" else R.SOFTMAX
    got = scene.ScenePredictor(recording, n, overlap, batch=2, kind=kind).predict(
        pre.cuda(), post.cuda() if which == "dmg" else None)
    tab = R.windows(H, W, n, overlap)
    assert len(tab) == 4 and [s[0].shape[0] for s in seen] == [2, 2]
    wins = torch.cat([s[0] for s in seen]).cpu().numpy()
    assert np.array_equal(wins, R.gather(pre.numpy(), post.numpy() if which == "dmg" else None, tab, n))
    logits = torch.cat([s[1] for s in seen]).float().cpu()
    assert tuple(logits.shape) == (4, 2 if which == "loc" else 4, n, n)      # networks.get_nclass: four damage classes
    ref = R.blend(logits, kind, tab, n, overlap, H, W)
    assert tuple(got.shape) == ((1, H, W) if which == "loc" else (4, H, W))
    _assert_within(got, ref, "network " + which)
    assert scene.ScenePredictor(model, n, overlap, batch=2).kind == kind      # and the default decode is the checkpoint's


def test_predict_pair_is_post_processing_of_the_blended_maps(loc_model, dmg_model):
    from xview2_amd import scene
    from xview2_amd.utils.post_process import post_process_tiles
    H, W = 80, 112
    pre, post = _scene_u8(H, W, 4)
    pre, post = pre.cuda(), post.cuda()
    loc, dmg = scene.ScenePredictor(loc_model, 64, 16, batch=2), scene.ScenePredictor(dmg_model, 64, 16, batch=2)
    for kw in (dict(), dict(components=True, dilate=True, dilation_rate=3)):
        a, b = scene.predict_pair(loc, dmg, pre, post, **kw)
        wa, wb = post_process_tiles(loc.predict(pre)[0], dmg.predict(pre, post), **kw)
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and tuple(a.shape) == (H, W) and tuple(b.shape) == (H, W)
        assert torch.equal(a, wa) and torch.equal(b, wb)
        assert int(a.max()) <= 1 and int(b.max()) <= 4


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_cli_predicts_a_png_pair_from_trained_checkpoints(tmp_path):
    import main as cli
    from PIL import Image
    from xview2_amd import predict
    common = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
              "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3", "--exec_mode", "train", "--epochs", "1",
              "--ema_decay", "0.9"]
    cli.main(common + ["--type", "pre", "--loss_str", "dice", "--results", str(tmp_path / "loc")])
    cli.main(common + ["--type", "post", "--dmg_model", "siamese", "--loss_str", "focal+dice", "--results", str(tmp_path / "dmg")])
    ck_loc = str(tmp_path / "loc" / "checkpoints" / "last.ckpt")
    ck_dmg = str(tmp_path / "dmg" / "checkpoints" / "last.ckpt")
    g = torch.Generator().manual_seed(9)
    for name in ("scene_pre.png", "scene_post.png"):
        Image.fromarray(torch.randint(0, 256, (96, 80, 3), generator=g, dtype=torch.uint8).numpy()).save(str(tmp_path / name))
    out = str(tmp_path / "out")
    flags = ["--ckpt_loc", ck_loc, "--ckpt_dmg", ck_dmg, "--pre", str(tmp_path / "scene_pre.png"), "--out", out,
             "--window", "64", "--overlap", "16", "--batch", "2", "--precision", "32"]
    n = predict.main(flags + ["--post", str(tmp_path / "scene_post.png"), "--tta", "--ema", "--components", "--dilate",
                              "--save_probs"])
    assert n == 1
    loc = np.asarray(Image.open(os.path.join(out, "scene_pre_localization_prediction.png")))
    dmg = np.asarray(Image.open(os.path.join(out, "scene_pre_damage_prediction.png")))
    assert loc.shape == (96, 80) and dmg.shape == (96, 80) and loc.dtype == np.uint8 and loc.max() <= 1 and dmg.max() <= 4
    assert np.load(os.path.join(out, "scene_pre_localization_probs.npy")).shape == (1, 96, 80)
    assert np.load(os.path.join(out, "scene_pre_damage_probs.npy")).shape == (4, 96, 80)
    # a pair of different sizes is an error that names both files
    Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(str(tmp_path / "small_post.png"))
    with pytest.raises(ValueError, match="scene_pre.png.*small_post.png"):
        predict.main(flags + ["--post", str(tmp_path / "small_post.png")])
