"""The whole-scene resize on the MI355X (csrc/resize.hip through xv2_resize_u8 / xv2_resize_f32, ops.resize_u8 / resize_f32 and
scene.ScenePredictor.predict(scales=...)) against the numpy restatements of tests/resize_ref.py.  Both rules are exact, so
every comparison is torch.equal / np.array_equal.  Each direct call writes between canary stretches (the entry points take no
workspace) and its inputs - image or maps and both tables - are compared with their copies afterwards."""
import numpy as np
import pytest
import torch

from tests import resize_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAN = 64            # canary elements on either side of every output
CASES = R.cases()


def _name(c):
    return "%dx%d-%dx%d" % c


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the product's tables are read-only arrays)


def _guarded(n, dtype, fill):
    buf = torch.full((2 * CAN + n,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, fill):
    assert bool((buf[:CAN] == fill).all()) and bool((buf[-CAN:] == fill).all()), "canary overwritten"


def _launch(stream, name, *args):
    from xview2_amd import _capi
    torch.cuda.synchronize()
    if stream is None:
        _capi.call(name, *args)
    else:
        with torch.cuda.stream(stream):
            _capi.call(name, *args)
    torch.cuda.synchronize()


def _resize_u8(img, h, w, stream=None):
    """xv2_resize_u8 on a caller-owned output between canaries; img uint8 [H, W, C] (numpy) -> numpy [h, w, C]"""
    from xview2_amd import resize
    H, W, C = img.shape
    s, xt, yt = _dev(img), _dev(resize.axis_table_u8(W, w)), _dev(resize.axis_table_u8(H, h))
    keep = [t.clone() for t in (s, xt, yt)]
    buf, out = _guarded(h * w * C, torch.uint8, 0x5A)
    _launch(stream, "xv2_resize_u8", s, H, W, C, xt, yt, h, w, out)
    _intact(buf, 0x5A)
    assert all(torch.equal(a, b) for a, b in zip((s, xt, yt), keep)), "an input was written"
    return out.cpu().numpy().reshape(h, w, C)


def _resize_f32(maps, H, W, mode, k, dst0, stream=None):
    """xv2_resize_f32 onto dst0 (numpy [C, H, W], what dst holds before the call) between canaries -> numpy [C, H, W]"""
    from xview2_amd import resize
    C, Hs, Ws = maps.shape
    s, xt, yt = _dev(maps), _dev(resize.axis_table_f32(Ws, W)), _dev(resize.axis_table_f32(Hs, H))
    keep = [t.clone() for t in (s, xt, yt)]
    buf, out = _guarded(C * H * W, torch.float32, 1234.5)
    out.copy_(_dev(dst0).reshape(-1))
    _launch(stream, "xv2_resize_f32", s, C, Hs, Ws, xt, yt, H, W, mode, k, out)
    _intact(buf, 1234.5)
    assert all(torch.equal(a, b) for a, b in zip((s, xt, yt), keep)), "an input was written"
    return out.cpu().numpy().reshape(C, H, W)


def _image(seed, H, W, C):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if H * W >= 64:                 # flat extremes beside noise: the overshoot of the negative lobes meets the clip
        img[: H // 3] = 255
        img[H // 3: H // 2, : W // 2] = 0
    return img


def _maps(seed, C, H, W):
    rng = np.random.default_rng(seed)
    m = rng.random((C, H, W), dtype=np.float32)
    m[0].flat[::7] = 0.0
    if C > 1:
        m[1] = m[1] * 8.0 - 4.0
    return m


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the kernels against the restatements, over the case table -----------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_name)
def test_resize_u8_equals_the_restatement(case):
    H, W, h, w = case
    for C in (3, 1, 6):
        img = _image(H * 1000 + W + h + C, H, W, C)
        got, want = _resize_u8(img, h, w), R.resize_u8(img, h, w)
        assert got.shape == want.shape and np.array_equal(got, want), (case, C, int((got != want).sum()))


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_resize_f32_equals_the_restatement_in_every_mode(case):
    Hs, Ws, H, W = case
    for C in (1, 5):
        m = _maps(Hs * 31 + W + C, C, Hs, Ws)
        r = R.resize_f32(m, H, W)
        d0 = _maps(Hs + W * 17 + C, C, H, W)
        assert _same_bits(_resize_f32(m, H, W, 0, 1, d0), r), (case, C, "write")
        assert _same_bits(_resize_f32(m, H, W, 1, 1, d0), d0 + r), (case, C, "accumulate")
        assert _same_bits(_resize_f32(m, H, W, 2, 3, d0), (d0 + r) / np.float32(3)), (case, C, "finish")


def test_a_side_stream_gives_the_same_bytes():
    side = torch.cuda.Stream()
    H, W, h, w = 97, 131, 65, 33
    img = _image(5, H, W, 3)
    assert np.array_equal(_resize_u8(img, h, w, stream=side), R.resize_u8(img, h, w))
    m, d0 = _maps(6, 5, h, w), _maps(7, 5, H, W)
    assert _same_bits(_resize_f32(m, H, W, 2, 2, d0, stream=side), (d0 + R.resize_f32(m, H, W)) / np.float32(2))


def test_more_than_one_tile_per_axis_and_a_scene_sized_ratio():
    """several tiles on both axes at the ratios predict uses (0.75 down, 1.5 up): tile seams and the LDS row window"""
    img = _image(11, 200, 150, 3)
    for h, w in ((150, 113), (300, 225), (50, 38)):
        assert np.array_equal(_resize_u8(img, h, w), R.resize_u8(img, h, w)), (h, w)
    m = _maps(12, 2, 150, 113)
    assert _same_bits(_resize_f32(m, 200, 150, 0, 1, np.zeros((2, 200, 150), np.float32)), R.resize_f32(m, 200, 150))
    m = _maps(13, 2, 300, 225)
    assert _same_bits(_resize_f32(m, 200, 150, 0, 1, np.zeros((2, 200, 150), np.float32)), R.resize_f32(m, 200, 150))


# ---- through ops ---------------------------------------------------------------------------------------------------------
def test_ops_bindings_and_their_argument_checks():
    from xview2_amd import ops
    img = _image(21, 37, 53, 3)
    assert np.array_equal(ops.resize_u8(_dev(img), 56, 80).cpu().numpy(), R.resize_u8(img, 56, 80))
    m = _maps(22, 3, 56, 80)
    r = R.resize_f32(m, 37, 53)
    out = ops.resize_f32(_dev(m), 37, 53)
    assert _same_bits(out.cpu().numpy(), r)
    assert ops.resize_f32(_dev(m), 37, 53, out=out, mode="accumulate") is out and _same_bits(out.cpu().numpy(), r + r)
    ops.resize_f32(_dev(m), 37, 53, out=out, mode="finish", k=3)
    assert _same_bits(out.cpu().numpy(), ((r + r) + r) / np.float32(3))
    d = _dev(img)
    for bad in (lambda: ops.resize_u8(d, 37 * 4 + 1, 53), lambda: ops.resize_u8(d, 37, 13), lambda: ops.resize_u8(d, 0, 53),
                lambda: ops.resize_u8(d[:, :, :2], 37, 53), lambda: ops.resize_u8(d.float(), 37, 53), lambda: ops.resize_u8(d[None], 37, 53),
                lambda: ops.resize_f32(_dev(m), 13, 53), lambda: ops.resize_f32(_dev(m), 37, 53, mode="add"),
                lambda: ops.resize_f32(_dev(m), 37, 53, mode="accumulate"), lambda: ops.resize_f32(_dev(m), 37, 53, out=out, mode="finish"),
                lambda: ops.resize_f32(_dev(m), 37, 53, out=out, mode="finish", k=9), lambda: ops.resize_f32(_dev(m), 37, 53, out=out, k=2),
                lambda: ops.resize_f32(_dev(m), 37, 53, out=out[:, :, :50]), lambda: ops.resize_f32(_dev(m).double(), 37, 53),
                lambda: ops.resize_f32(_dev(m)[0], 37, 53)):
        with pytest.raises(ValueError):
            bad()


# ---- scene level: a stub as the model ------------------------------------------------------------------------------------
WINDOW, OVERLAP = 32, 8
SCENES = [(70, 45), (20, 90)]


def _stub(cout, post):
    """logits [K, cout, n, n] from each pixel's own bytes: independent of the window, its position and the batch"""
    def model(img):
        v = img.u8.float()
        a, b = (v[..., 0], v[..., 4]) if post else (v[..., 0], v[..., 1])
        planes = [(a - b) / 32.0, (a + v[..., 2]) / 128.0 - 2.0, (b - 100.0) / 40.0, (v[..., 2] - a) / 64.0]
        return torch.stack(planes[:cout], dim=1).contiguous()
    return model


def _predictor(kind, post, batch):
    from xview2_amd import scene
    cout = {scene.SIGMOID1: 2, scene.SOFTMAX: 4, scene.SIGMOID: 3, scene.RELU: 1}[kind]
    return scene.ScenePredictor(_stub(cout, post), window=WINDOW, overlap=OVERLAP, batch=batch, kind=kind)


def _pair(H, W, post):
    pre = _image(H * 7 + W, H, W, 3)
    return _dev(pre), (_dev(_image(H * 7 + W + 1, H, W, 3)) if post else None)


def _by_hand(p, pre, post, scales):
    """the composition from ops.resize_u8, the plain prediction and the float32 restatement"""
    from xview2_amd import ops, scene
    H, W, _ = pre.shape
    terms = []
    for s in scales:
        if s == 1:
            terms.append(p.predict(pre, post).cpu().numpy())
            continue
        Hs, Ws = scene.scaled_size(H, W, s)
        maps = p.predict(ops.resize_u8(pre, Hs, Ws), ops.resize_u8(post, Hs, Ws) if post is not None else None)
        assert tuple(maps.shape[1:]) == (Hs, Ws)
        terms.append(R.resize_f32(maps.cpu().numpy(), H, W))
    return R.average(terms)


KINDS = [(0, False), (3, False), (1, True), (2, True)]      # SIGMOID1 and RELU on pre alone, SOFTMAX and SIGMOID on the pair


@pytest.mark.parametrize("H,W", SCENES)
@pytest.mark.parametrize("kind,post", KINDS)
def test_scene_scales_equal_the_composition_by_hand(H, W, kind, post):
    from xview2_amd import scene
    pre_d, post_d = _pair(H, W, post)
    keep = pre_d.clone()
    p = _predictor(kind, post, 4)
    plain = p.predict(pre_d, post_d)
    assert torch.equal(p.predict(pre_d, post_d, scales=(1,)), plain) and torch.equal(p.predict(pre_d, post_d, scales=[1.0]), plain)
    got = p.predict(pre_d, post_d, scales=(0.5, 1, 1.5))
    want = _by_hand(p, pre_d, post_d, (0.5, 1, 1.5))
    assert tuple(got.shape) == tuple(plain.shape) and got.dtype == torch.float32
    assert _same_bits(got.cpu().numpy(), want)
    assert not torch.equal(got, plain)
    for batch in (1, 7):
        assert torch.equal(_predictor(kind, post, batch).predict(pre_d, post_d, scales=(0.5, 1, 1.5)), got)
    assert torch.equal(pre_d, keep)
    if kind in (scene.SIGMOID1, scene.SOFTMAX, scene.SIGMOID):      # probabilities stay probabilities
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-6


@pytest.mark.parametrize("scales", [(1, 0.5), (2, 1), (0.75,), (1.25, 0.75), (1, 2, 0.5, 1.5, 0.75, 1.25, 3, 0.6)])
def test_scene_scales_in_other_orders_and_counts(scales):
    """scale 1 first (the predictor's own tensor starts the sum), last (the identity tables finish it), absent; one scale
    (a plain write, no division); eight scales"""
    pre_d, post_d = _pair(40, 44, True)
    p = _predictor(1, True, 3)
    got = p.predict(pre_d, post_d, scales=scales)
    assert _same_bits(got.cpu().numpy(), _by_hand(p, pre_d, post_d, scales))


def test_invalid_scale_lists_raise_before_any_prediction():
    calls = []
    from xview2_amd import scene

    def model(img):
        calls.append(1)
        return _stub(2, False)(img)
    p = scene.ScenePredictor(model, window=WINDOW, overlap=OVERLAP, batch=2, kind=scene.SIGMOID1)
    pre_d, _ = _pair(70, 45, False)
    for bad in ((), (0.2,), (4.5,), (1, 1), (0.5, 1, 0.5), tuple(1 + i / 10 for i in range(9)), 0.5):
        with pytest.raises(ValueError):
            p.predict(pre_d, scales=bad)
    with pytest.raises(ValueError):     # round(45 * 0.25) = 11 and 45 > 4 * 11: outside the resize limit
        p.predict(pre_d, scales=(1, 0.25))
    assert not calls
