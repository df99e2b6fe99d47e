"""The rules of the whole-scene resize on the host (tests/resize_ref.py, xview2_amd/resize.py): the uint8 restatement against
the installed Pillow, the product's vectorised tables against the restatement's, the limits, and the fp32 rule against fp64
under the bound derived in resize_ref.bound_f32.  No GPU."""
import numpy as np
import pytest

from tests import resize_ref as R

CASES = R.cases()


def _name(c):
    return "%dx%d-%dx%d" % c


def _image(seed, H, W, C):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if H * W >= 64:                 # flat extremes beside noise: the overshoot of the negative lobes meets the clip
        img[: H // 3] = 255
        img[H // 3: H // 2, : W // 2] = 0
    return img


def test_the_case_table_covers_what_it_claims():
    assert len(CASES) >= 50 and len(set(CASES)) == len(CASES)
    assert all(R.allowed(H, h) and R.allowed(W, w) for H, W, h, w in CASES)
    taps = {max(R.taps_of(H, h), R.taps_of(W, w)) for H, W, h, w in CASES}
    u8 = {max(int(R.tables_u8(H, h)[:, 1].max()), int(R.tables_u8(W, w)[:, 1].max())) for H, W, h, w in CASES}
    # 4:1 fills the 17 / 9 slots Pillow allocates up to the last one (the windows hold 2 * support taps there)
    assert max(u8) in (R.U8_TAPS - 1, R.U8_TAPS) and max(taps) in (R.F32_TAPS - 1, R.F32_TAPS)
    assert any(H == h and W != w for H, W, h, w in CASES) and any(W == w and H != h for H, W, h, w in CASES)
    assert any(H == 1 or W == 1 for H, W, h, w in CASES) and any(h == 1 or w == 1 for H, W, h, w in CASES)
    # a source narrower than the support: every tap window of the axis is clipped at both borders
    assert any(np.all(R.tables_u8(W, w)[:, 0] == 0) and np.all(R.tables_u8(W, w)[:, 1] == W) and W > 1 for H, W, h, w in CASES)


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_uint8_restatement_equals_pillow(case):
    from PIL import Image
    H, W, h, w = case
    img = _image(H * 1000 + W + h, H, W, 3)
    want = np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC))
    got = R.resize_u8(img, h, w)
    assert got.shape == want.shape and np.array_equal(got, want)
    grey = np.ascontiguousarray(img[:, :, :1])
    want1 = np.asarray(Image.fromarray(grey[:, :, 0]).resize((w, h), Image.BICUBIC))
    assert np.array_equal(R.resize_u8(grey, h, w)[:, :, 0], want1)


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_product_tables_equal_the_restatement(case):
    from xview2_amd import resize
    H, W, h, w = case
    for a, b in ((H, h), (W, w)):
        t8, t32 = resize.axis_table_u8(a, b), resize.axis_table_f32(a, b)
        assert t8.dtype == np.int32 and t8.shape == (b, 2 + R.U8_TAPS) and np.array_equal(t8, R.tables_u8(a, b))
        assert t32.dtype == np.int32 and t32.shape == (b, 2 + R.F32_TAPS) and np.array_equal(t32, R.tables_f32(a, b))
        for t in (t8, t32):         # what the kernels rely on: windows inside the axis, monotonic in the output index
            assert t[:, 0].min() >= 0 and (t[:, 0] + t[:, 1]).max() <= a and t[:, 1].min() >= 1
            assert np.all(np.diff(t[:, 0]) >= 0) and np.all(np.diff(t[:, 0] + t[:, 1]) >= 0)
            # the rows a tile of 32 outputs needs fit the bound the entry points size their LDS by
            base = 2 if t is t8 else 1
            slots = 2 * (-(-base * a // b) if a > b else base) + 1
            assert t[:, 1].max() <= slots <= t.shape[1] - 2
            for o in range(0, b, 32):
                last = min(o + 32, b) - 1
                assert t[last, 0] + t[last, 1] - t[o, 0] <= -(-31 * a // b) + slots + 1


def test_limits_and_scale_lists_raise():
    from xview2_amd import resize, scene
    for a, b in ((1, 5), (5, 1), (100, 24), (24, 100), (0, 1), (1, 0), (-3, 3)):
        for fn in (resize.axis_table_u8, resize.axis_table_f32, resize.check_axis):
            with pytest.raises(ValueError):
                fn(a, b)
        with pytest.raises(ValueError):
            R.check_axis(a, b)
    for a, b in ((1, 4), (4, 1), (100, 25), (25, 100), (7, 7)):
        resize.axis_table_u8(a, b), resize.axis_table_f32(a, b)
    assert scene.scaled_size(1024, 1024, 0.75) == (768, 768) and scene.scaled_size(3, 5, 0.25) == (1, 1)
    assert scene.scaled_size(1, 1, 0.25) == (1, 1) and scene.scaled_size(37, 53, 1.5) == (56, 80)
    assert scene.check_scales([0.5, 1, 2]) == (0.5, 1.0, 2.0) and scene.check_scales((1,)) == (1.0,)
    for bad in ((), (0.2,), (4.5,), (1, 1.0), (0.5, 2, 0.5), tuple(1 + i / 10 for i in range(9)), (float("nan"),), 1.0, None):
        with pytest.raises(ValueError):
            scene.check_scales(bad)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """argument validation is reachable without a GPU: XV2_EINVAL and a message, nothing enqueued"""
    from xview2_amd import _capi, _lib
    _lib.build()
    u8, f32 = _capi._func("xv2_resize_u8"), _capi._func("xv2_resize_f32")
    p = 4096      # any non-null address: nothing is dereferenced before the checks
    for args, msg in (((p, 37, 53, 3, p, p, 149, 53, p, None), b"out <= 4 in"), ((p, 37, 53, 3, p, p, 37, 13, p, None), b"out <= 4 in"),
                      ((p, 37, 53, 2, p, p, 37, 53, p, None), b"C=2"), ((p, 0, 53, 3, p, p, 37, 53, p, None), b"positive"),
                      ((p, 1 << 15, 1 << 15, 3, p, p, 1 << 15, 1 << 15, p, None), b"2^30"),
                      ((p, 37, 53, 3, None, p, 37, 53, p, None), b"null")):
        assert u8(*args) == 1 and msg in _lib.lib().xv2_last_error(), args
    for args, msg in (((p, 1, 37, 53, p, p, 149, 53, 0, 1, p, None), b"out <= 4 in"), ((p, 9, 37, 53, p, p, 37, 53, 0, 1, p, None), b"C=9"),
                      ((p, 1, 37, 53, p, p, 37, 53, 3, 1, p, None), b"mode"), ((p, 1, 37, 53, p, p, 37, 53, 2, 0, p, None), b"k=0"),
                      ((p, 1, 37, 53, p, p, 37, 53, 0, 1, None, None), b"null")):
        assert f32(*args) == 1 and msg in _lib.lib().xv2_last_error(), args


def _maps(seed, C, H, W):
    rng = np.random.default_rng(seed)
    m = rng.random((C, H, W), dtype=np.float32)
    m[0].flat[::7] = 0.0
    if C > 1:
        m[1] = m[1] * 8.0 - 4.0          # a signed plane (mse / logit-like maps)
    return m


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_float32_rule_against_float64_under_the_derived_bound(case):
    Hs, Ws, H, W = case
    m = _maps(Hs * 31 + W, 2, Hs, Ws)
    got, ref = R.resize_f32(m, H, W), R.resize_f64(m, H, W)
    bound = R.bound_f32(m, Hs, Ws, H, W)
    assert got.dtype == np.float32 and got.shape == (2, H, W)
    err = np.abs(got.astype(np.float64) - ref).max()
    print("%s: error %.3e, bound %.3e" % (_name(case), err, bound))
    assert err <= bound
    # weights: non-negative, summing to 1 within the rounding of their fp32 values
    for a, b in ((Hs, H), (Ws, W)):
        t = R.tables_f32(a, b)
        k = t[:, 2:].view(np.float32).astype(np.float64)
        assert k.min() >= 0.0 and np.abs(k.sum(axis=1) - 1.0).max() <= R.F32_TAPS * R.U
    # a convex combination: the range of each plane is kept, and a constant map comes back constant, within the bound
    for c in range(2):
        assert got[c].max() <= m[c].max() + bound and got[c].min() >= m[c].min() - bound
    const = np.full((1, Hs, Ws), 0.7, dtype=np.float32)
    back = R.resize_f32(const, H, W)
    assert np.abs(back.astype(np.float64) - float(np.float32(0.7))).max() <= R.bound_f32(const, Hs, Ws, H, W)
    if Hs == H and Ws == W:
        assert np.array_equal(got, m)


def test_average_is_the_left_to_right_sum_divided_once():
    a, b, c = (_maps(s, 1, 5, 6) for s in (1, 2, 3))
    assert np.array_equal(R.average([a, b, c]), ((a + b) + c) / np.float32(3))
    assert np.array_equal(R.average([a]), a)


def test_command_line_scales_parse_before_any_gpu_work():
    from xview2_amd import predict
    base = ["--pre", "a.png", "--out", "o"]
    p = predict.get_parser()
    assert p.parse_args(base).scales == (1.0,)
    assert p.parse_args(base + ["--scales", "0.75,1,1.25"]).scales == (0.75, 1.0, 1.25)
    assert p.parse_args(base + ["--scales", " 0.6 "]).scales == (0.6,)
    assert predict.parse_scales("2,0.5") == (2.0, 0.5)
    for bad in ("", "1,,2", "a", "0.2", "5", "1,1", "1;2", "1,2,1.0", ",".join(str(1 + i / 10) for i in range(9)), "nan"):
        with pytest.raises(ValueError):
            predict.parse_scales(bad)
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--scales", bad])
