"""Scene inference without a GPU: the integer geometry of xview2_amd/scene.py, the float64 restatement and its bound
(tests/scene_ref.py), argument validation of the three entry points, and the command line of xview2_amd/predict.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import scene_ref as R
from xview2_amd import scene


@pytest.mark.parametrize("n", [32, 64])
def test_window_origins_cover_every_position_at_most_three_times(n):
    for overlap in range(0, n // 2 + 1):
        r = scene.ramp(n, overlap)
        for L in range(1, 6 * n + 1):
            o = scene.window_origins(L, n, overlap)
            assert o == sorted(set(o)) and o[0] == 0, (L, overlap, o)
            assert o == R.origins(L, n, overlap)
            assert o[-1] == max(L - n, 0)      # the last window ends at the scene's edge: never padded when L >= n
            cover = np.zeros(L, dtype=np.int64)
            wsum = np.zeros(L, dtype=np.int64)
            for a in o:
                m = min(n, L - a)
                cover[a:a + m] += 1
                wsum[a:a + m] += r[:m]
            assert cover.min() >= 1 and cover.max() <= 3, (L, overlap, o)
            w = scene.axis_normaliser(L, n, overlap)
            assert w.dtype == np.int32 and np.array_equal(w, wsum) and w.min() >= 1


def test_window_parameters_are_validated():
    for n, overlap in [(48, 0), (0, 0), (2080, 0), (32, 17), (32, -1)]:
        with pytest.raises(ValueError):
            scene.window_origins(100, n, overlap)
    assert scene.window_origins(100, 32, 16) == [0, 16, 32, 48, 64, 68]


@pytest.mark.parametrize("case", R.SCENES, ids=R.name)
def test_normaliser_is_the_outer_product_of_the_axis_tables(case):
    H, W, n, overlap = (case[k] for k in ("H", "W", "n", "overlap"))
    r = scene.ramp(n, overlap)
    brute = np.zeros((H, W), dtype=np.int64)
    tab = scene.scene_windows(H, W, n, overlap)
    assert [tuple(t) for t in tab.tolist()] == R.windows(H, W, n, overlap)      # y outer, x inner
    for y0, x0 in tab:
        hh, ww = min(n, H - y0), min(n, W - x0)
        brute[y0:y0 + hh, x0:x0 + ww] += np.outer(r[:hh], r[:ww])
    wy, wx = scene.axis_normaliser(H, n, overlap), scene.axis_normaliser(W, n, overlap)
    assert np.array_equal(np.outer(wy.astype(np.int64), wx.astype(np.int64)), brute)
    assert brute.max() < 2 ** 24


@pytest.mark.parametrize("L,n", [(1, 32), (2, 32), (5, 32), (31, 32), (32, 32), (17, 64), (40, 64)])
def test_tri_is_numpy_reflect_padding(L, n):
    a = np.arange(L)
    want = a if L >= n else (np.zeros(n, dtype=np.int64) if L == 1 else np.pad(a, (0, n - L), mode="reflect"))
    assert np.array_equal(scene.tri(np.arange(max(L, n)), L)[:len(want)], want)
    assert [R.reflect(i, L) for i in range(n)] == list(scene.tri(np.arange(n), L))


@pytest.mark.parametrize("case", R.SCENES, ids=R.name)
def test_reference_gather_is_a_reflect_padded_crop(case):
    H, W, n, overlap = (case[k] for k in ("H", "W", "n", "overlap"))
    pre, post = R.make_scene(case)
    both = np.concatenate([pre, post], axis=2)
    pad = np.pad(both, ((0, max(n - H, 0) if H > 1 else 0), (0, max(n - W, 0) if W > 1 else 0), (0, 0)), mode="reflect")
    if H == 1:
        pad = np.repeat(pad, n, axis=0)
    if W == 1:
        pad = np.repeat(pad, n, axis=1)
    tab = R.windows(H, W, n, overlap)
    got = R.gather(pre, post, tab, n)
    for k, (y0, x0) in enumerate(tab):
        assert np.array_equal(got[k], pad[y0:y0 + n, x0:x0 + n])
    assert np.array_equal(R.gather(pre, None, tab, n), got[..., :3])


def _ratio(y, ref):
    ok = ~ref["planted"].unsqueeze(0).expand_as(ref["out"])
    z = torch.zeros_like(ref["out"])
    return R.check(torch.where(ok, y.double(), z), torch.where(ok, ref["out"], z), torch.where(ok, ref["bound"], z))[0]


@pytest.mark.parametrize("case", R.SCENES, ids=R.name)
def test_bound_admits_the_fp32_arithmetic_of_the_kernels(case):
    H, W, n, overlap = (case[k] for k in ("H", "W", "n", "overlap"))
    tab = R.windows(H, W, n, overlap)
    for kind, C in R.KINDS:
        for regime in R.REGIMES[:2]:
            x = R.make_logits(case, len(tab), C, regime)
            ref = R.blend(x, kind, tab, n, overlap, H, W)
            assert int(ref["count"].max()) <= 9
            ratio = _ratio(R.f32_blend(x, kind, tab, n, overlap, H, W), ref)
            assert ratio <= 1.0, (kind, C, regime, ratio)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_wrong_variant_lands_outside_the_bound(wrong):
    """on at least one case of the table: the GPU test can fail"""
    hit = []
    for case in R.SCENES:
        H, W, n, overlap = (case[k] for k in ("H", "W", "n", "overlap"))
        tab = R.windows(H, W, n, overlap)
        if wrong == "reflect_repeats_edge":
            pre, post = R.make_scene(case)
            if not np.array_equal(R.gather(pre, post, tab, n, wrong), R.gather(pre, post, tab, n)):
                hit.append(R.name(case))
            continue
        x = R.make_logits(case, len(tab), 5, "position")
        ref = R.blend(x, R.SOFTMAX, tab, n, overlap, H, W)
        bad = R.blend(x, R.SOFTMAX, R.windows(H, W, n, overlap, wrong), n, overlap, H, W, wrong)
        if _ratio(bad["out"], ref) > 1.0:
            hit.append(R.name(case))
    assert hit, wrong
    if wrong == "reflect_repeats_edge":      # only scenes shorter than the window are padded at all
        assert set(hit) == {R.name(c) for c in R.SCENES if c["H"] < c["n"] and c["H"] > 1 or c["W"] < c["n"] and c["W"] > 1}


def test_nonfinite_logits_reach_their_own_pixel_only_in_the_reference():
    case = R.SCENES[8]
    H, W, n, overlap = (case[k] for k in ("H", "W", "n", "overlap"))
    tab = R.windows(H, W, n, overlap)
    for kind, C in R.KINDS:
        ref = R.blend(R.make_logits(case, len(tab), C, "nonfinite"), kind, tab, n, overlap, H, W)
        assert 1 <= int(ref["planted"].sum()) <= 2
        assert torch.isfinite(ref["out"][:, ~ref["planted"]]).all()


# ---- the C ABI: validation comes back as XV2_EINVAL with a message, before anything touches the GPU ------------------------

def _rc(fn, *args):
    from xview2_amd import _capi, _lib
    rc = _capi._func(fn)(*args, None)
    return rc, _lib.lib().xv2_last_error()


def test_entry_points_validate_their_arguments_without_a_gpu():
    rc, msg = _rc("xv2_scene_windows_u8", None, None, 100, 100, None, 1, 48, 32, None)
    assert rc == 1 and b"multiples of 32" in msg
    rc, msg = _rc("xv2_scene_blend", None, R.SOFTMAX, 5, None, 1, 48, 48, 0, 100, 100, None)
    assert rc == 1 and b"multiples of 32" in msg
    rc, msg = _rc("xv2_scene_blend", None, R.SOFTMAX, 5, None, 1, 32, 32, 17, 100, 100, None)
    assert rc == 1 and b"overlap=17" in msg
    rc, msg = _rc("xv2_scene_blend", None, 4, 5, None, 1, 32, 32, 16, 100, 100, None)
    assert rc == 1 and b"unknown kind 4" in msg
    for kind, C in [(R.SIGMOID1, 3), (R.SIGMOID1, 1), (R.SOFTMAX, 1), (R.SOFTMAX, 6), (R.SIGMOID, 0), (R.RELU, 6)]:
        rc, msg = _rc("xv2_scene_blend", None, kind, C, None, 1, 32, 32, 16, 100, 100, None)
        assert rc == 1 and b"does not fit kind" in msg, (kind, C)
    for fn, args in [("xv2_scene_windows_u8", (None, None, 32768, 32768, None, 1, 32, 32, None)),
                     ("xv2_scene_blend", (None, R.SOFTMAX, 5, None, 1, 32, 32, 16, 32768, 32768, None)),
                     ("xv2_scene_finalize", (None, 5, 32768, 32768, None, None))]:
        rc, msg = _rc(fn, *args)
        assert rc == 1 and b"2^30" in msg, fn
    rc, msg = _rc("xv2_scene_blend", None, R.SOFTMAX, 5, None, 1025, 32, 32, 16, 100, 100, None)
    assert rc == 1 and b"windows per call" in msg
    rc, msg = _rc("xv2_scene_finalize", None, 5, 100, 100, None, None)
    assert rc == 1 and b"null tensor" in msg
    from xview2_amd import _capi
    assert _capi._parse_header()["xv2_scene_blend"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                        ctypes.c_void_p] + [ctypes.c_int] * 6
                                                        + [ctypes.c_void_p] * 2)
    assert (scene.SIGMOID1, scene.SOFTMAX, scene.SIGMOID, scene.RELU) == (R.SIGMOID1, R.SOFTMAX, R.SIGMOID, R.RELU)


def test_predictor_validates_and_picks_the_decode_of_the_checkpoint():
    from tests.golden.cases import ARGS

    class M:
        def __init__(self, **kw):
            self.args = ARGS(**kw)
    assert scene.ScenePredictor(M(), 64, 16).kind == scene.SIGMOID1
    assert scene.ScenePredictor(M(type="post", loss_str="coral")).kind == scene.SIGMOID
    assert scene.ScenePredictor(M(type="post", loss_str="mse")).kind == scene.RELU
    assert scene.ScenePredictor(M(type="post", loss_str="focal+dice")).kind == scene.SOFTMAX
    with pytest.raises(ValueError):
        scene.ScenePredictor(lambda x: x)
    with pytest.raises(ValueError):
        scene.ScenePredictor(M(), 48, 0)
    with pytest.raises(ValueError):
        scene.ScenePredictor(M(), 64, 33)
    with pytest.raises(ValueError):
        scene.ScenePredictor(M(), 64, 16, batch=0)
    with pytest.raises(ValueError):
        scene.ScenePredictor(M(), 64, 16).predict(torch.zeros((8, 8, 3), dtype=torch.uint8))      # not on the device


def test_decode_damage_matches_the_decode_of_the_model():
    g = torch.Generator().manual_seed(5)
    maps = torch.rand((3, 7, 9), generator=g)
    assert scene.decode_damage(maps, scene.SOFTMAX) is maps
    coral = scene.decode_damage(maps, scene.SIGMOID)
    assert coral.dtype == torch.int32 and torch.equal(coral, ((maps > 0.5).sum(0) + 1).int())
    mse = scene.decode_damage(maps[:1] * 3.0, scene.RELU)
    assert mse.dtype == torch.int32 and torch.equal(mse, (torch.round(maps[0] * 3.0) + 1).int())
    with pytest.raises(ValueError):
        scene.decode_damage(maps, scene.SIGMOID1)


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_cli_parser_parses():
    from xview2_amd import predict
    a = predict.get_parser().parse_args(["--pre", "a.png", "--out", "o"])
    assert (a.window, a.overlap, a.batch, a.precision, a.dilation_rate) == (1024, 256, 4, 16, 3)
    assert a.ckpt_loc is None and a.ckpt_dmg is None and a.post is None
    assert not (a.tta or a.ema or a.components or a.dilate or a.save_probs)
    a = predict.get_parser().parse_args(["--ckpt_loc", "l", "--ckpt_dmg", "d", "--pre", "p", "--post", "q", "--out", "o",
                                         "--window", "512", "--overlap", "128", "--batch", "2", "--tta", "--precision", "32",
                                         "--ema", "--components", "--dilate", "--dilation_rate", "5", "--save_probs"])
    assert (a.ckpt_loc, a.ckpt_dmg, a.pre, a.post, a.out) == ("l", "d", "p", "q", "o")
    assert (a.window, a.overlap, a.batch, a.precision, a.dilation_rate) == (512, 128, 2, 32, 5)
    assert a.tta and a.ema and a.components and a.dilate and a.save_probs
    with pytest.raises(SystemExit):
        predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--precision", "8"])
    with pytest.raises(ValueError):
        predict.main(["--pre", "p", "--out", "o"])                              # no checkpoint at all
    with pytest.raises(ValueError):
        predict.main(["--ckpt_dmg", "d", "--pre", "p", "--out", "o"])            # a damage model needs the post image


def test_directories_are_paired_by_sorted_order(tmp_path):
    from PIL import Image
    from xview2_amd import predict
    pre, post = tmp_path / "pre", tmp_path / "post"
    pre.mkdir()
    post.mkdir()
    img = Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8))
    for stem in ("b", "a", "c"):
        img.save(str(pre / (stem + "_pre.png")))
        img.save(str(post / (stem + "_post.png")))
    (pre / "notes.txt").write_text("not an image")
    pairs = predict.pair_inputs(str(pre), str(post))
    assert [(p.split("/")[-1], q.split("/")[-1]) for p, q in pairs] == [
        ("a_pre.png", "a_post.png"), ("b_pre.png", "b_post.png"), ("c_pre.png", "c_post.png")]
    assert predict.pair_inputs(str(pre / "a_pre.png"), str(post / "c_post.png")) == [
        (str(pre / "a_pre.png"), str(post / "c_post.png"))]
    assert predict.pair_inputs(str(pre)) == [(p, None) for p, _ in pairs]
    (post / "c_post.png").unlink()
    with pytest.raises(ValueError, match="3 pre images .* 2 post images"):
        predict.pair_inputs(str(pre), str(post))
    with pytest.raises(FileNotFoundError):
        predict.pair_inputs(str(tmp_path / "missing.png"))
    rgb = np.arange(60, dtype=np.uint8).reshape(4, 5, 3)
    Image.fromarray(rgb).save(str(tmp_path / "x.png"))
    assert np.array_equal(predict.read_bgr(str(tmp_path / "x.png")), rgb[:, :, ::-1])
