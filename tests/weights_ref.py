"""Bit-level restatement of the derived copies of a convolution weight (include/xv2.h: packed OHWI / IHWO layouts, the three
bf16 planes of F32X3, the recorded maximum and the two scaled fp16 planes of F16X2, the RGB stem's band form), in numpy on
the CPU.  Written from the header's description of the layouts and of the arithmetic, not from the kernels: every function
returns BIT PATTERNS (uint16 for bf16 / fp16 values, fp32 arrays compare through their uint32 view), so the GPU tests that
use it need no tolerance.

numpy has no bf16 type: a bf16 value is the upper half of an fp32 bit pattern, rounded to nearest even here with integer
arithmetic.  fp16 is numpy's float16 (IEEE, round to nearest even, overflow to Inf); fp32 subtraction and the multiplication by
a power of two are numpy float32 operations (IEEE, denormals kept)."""
import numpy as np


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def bits32(x):
    """the uint32 bit patterns of an fp32 array"""
    return f32(x).view(np.uint32)


def from_bits32(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint32)).view(np.float32)


def bf16_bits(x):
    """round-to-nearest-even of fp32 to bf16, as uint16 bit patterns (a finite value above 0x7f7f8000 rounds to Inf; NaN
    stays a quiet NaN)"""
    b = bits32(x).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7fffffff) > 0x7f800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(b16):
    """the fp32 value of bf16 bit patterns"""
    return from_bits32(np.asarray(b16, dtype=np.uint16).astype(np.uint32) << 16)


def f16_bits(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(x).astype(np.float16).view(np.uint16)


def packed(w_oihw, cin_pad, which, bf16=False):
    """w_oihw [Cout][Cin][KH][KW] -> "ohwi": [Cout][KH*KW][cin_pad], "ihwo": [cin_pad][KH*KW][Cout]; channels >= Cin are +0.0;
    fp32 array, or the uint16 bit patterns of the bf16 layout"""
    w = f32(w_oihw)
    Cout, Cin, KH, KW = w.shape
    assert cin_pad >= Cin and which in ("ohwi", "ihwo")
    T = KH * KW
    out = np.zeros((Cout, T, cin_pad), dtype=np.float32)
    for t in range(T):
        out[:, t, :Cin] = w[:, :, t // KW, t % KW]
    if which == "ihwo":
        out = np.ascontiguousarray(out.transpose(2, 1, 0))
    return bf16_bits(out) if bf16 else out


def split3(x):
    """x = h + m + l: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), every rounding to nearest even; bf16 bit patterns"""
    x = f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        h = bf16_bits(x)
        r1 = x - bf16_value(h)
        m = bf16_bits(r1)
        r2 = r1 - bf16_value(m)
        l = bf16_bits(r2)
    return h, m, l


def join3(h, m, l):
    """(h + m) + l in fp32"""
    return (bf16_value(h) + bf16_value(m)) + bf16_value(l)


def _swap_rows():
    r = np.arange(64)
    return ((r >> 3) & 1).astype(bool)


def plane_image(planes):
    """P arrays [rows][T][ctot] (16-bit patterns: the planes of one packed layout) -> the LDS image of a weight stage,
    [rows/64][T][ctot/16][P][64][16], flat: inside a 64-row unit the rows whose bit 3 is set hold the two 8-element halves of
    their 16 channels swapped"""
    planes = [np.asarray(p) for p in planes]
    rows, T, ctot = planes[0].shape
    assert rows % 64 == 0 and ctot % 16 == 0 and all(p.shape == (rows, T, ctot) for p in planes)
    P = len(planes)
    img = np.empty((rows // 64, T, ctot // 16, P, 64, 16), dtype=planes[0].dtype)
    swap = _swap_rows()
    for p, a in enumerate(planes):
        v = a.reshape(rows // 64, 64, T, ctot // 16, 16).transpose(0, 2, 3, 1, 4)      # [unit][tap][slice][row][16]
        v = np.where(swap[None, None, None, :, None], np.concatenate([v[..., 8:], v[..., :8]], axis=-1), v)
        img[:, :, :, p] = v
    return img.reshape(-1)


def plane_image_inverse(image, rows, T, ctot, P):
    """the P planes [rows][T][ctot] of a flat image"""
    img = np.asarray(image).reshape(rows // 64, T, ctot // 16, P, 64, 16)
    swap = _swap_rows()
    out = []
    for p in range(P):
        v = img[:, :, :, p]
        v = np.where(swap[None, None, None, :, None], np.concatenate([v[..., 8:], v[..., :8]], axis=-1), v)
        out.append(np.ascontiguousarray(v.transpose(0, 3, 1, 2, 4)).reshape(rows, T, ctot))
    return out


def amax_bits(x):
    """the largest bit pattern of |x|: what the 64 slots of a tensor hold between them (bit patterns of non-negative floats
    order like their values, Inf and NaN above every finite one; -0.0 counts as 0)"""
    b = bits32(x).reshape(-1) & np.uint32(0x7fffffff)
    return int(b.max()) if b.size else 0


def f16_scale(bits):
    """the power of two s of F16X2 for a recorded maximum: biased exponent clamped to [16, 240], s = 2^(141 - e), so that
    amax * s lies in [2^14, 2^15) wherever the clamp does not bite"""
    e = min(max((int(bits) >> 23) & 0xff, 16), 240)
    return np.float32(2.0 ** (141 - e))


def split2h(x, s):
    """x * s = h + m: h = fp16(fp32(x * s)), m = fp16(fp32(x * s) - h); fp16 bit patterns"""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = f32(x) * np.float32(s)
        h = xs.astype(np.float16)
        m = (xs - h.astype(np.float32)).astype(np.float16)
    return h.view(np.uint16), m.view(np.uint16)


def join2h(h, m, s):
    """(h + m) / s in float64"""
    h = np.asarray(h, dtype=np.uint16).view(np.float16).astype(np.float64)
    m = np.asarray(m, dtype=np.uint16).view(np.float16).astype(np.float64)
    return (h + m) / float(s)


def pad_band(x4, pad_top, pad_left, IHp, IWp, bf16=False):
    """the NHWC4 image [N][H][W][4] inside a frame [N][IHp][IWp][4] at (pad_top, pad_left), +0.0 everywhere else"""
    x = f32(x4)
    N, H, W, C = x.shape
    assert C == 4 and IHp >= H + pad_top and IWp >= W + pad_left
    out = np.zeros((N, IHp, IWp, 4), dtype=np.float32)
    out[:, pad_top:pad_top + H, pad_left:pad_left + W] = x
    return bf16_bits(out) if bf16 else out


def stem_band(w_oihw, bf16=False):
    """the RGB stem's weights [Cout][Cin <= 4][KH][KW <= 8] as [Cout][KH][8 pixels][4 channels], +0.0 for kw >= KW and c >= Cin"""
    w = f32(w_oihw)
    Cout, Cin, KH, KW = w.shape
    assert Cin <= 4 and KW <= 8
    out = np.zeros((Cout, KH, 8, 4), dtype=np.float32)
    out[:, :, :KW, :Cin] = w.transpose(0, 2, 3, 1)
    return bf16_bits(out) if bf16 else out


# ---- data shared by the CPU self-checks and the GPU tests -----------------------------------------------------------------

def edge_values():
    """fp32 values at which a three-way bf16 split can go wrong: signed zeros, denormals, the ends of the normal range below
    0x7f7f8000 (above it bf16(x) is Inf), values that are exact in bf16, and round-to-nearest-even ties of the first and of
    the second level with an even and with an odd retained half"""
    pats = [0x00000000, 0x80000000,                        # +-0
            0x00000001, 0x80000001, 0x00000100, 0x007fffff, 0x00008000, 0x00018000, 0x00400000,      # denormals
            0x00800000, 0x80800000, 0x00800001, 0x00ffffff,                                          # smallest normals
            0x7f7f7fff, 0xff7f7fff, 0x7f7f0000, 0x7f000000, 0x7f7e8000,                              # largest below 0x7f7f8000
            0x3f800000, 0xbf800000, 0x3fc00000, 0x40490000, 0x42fe0000,                              # exact in bf16
            0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,      # first-level ties: even / odd upper half
            0x3f808001, 0x3f807fff, 0x3f818001, 0x3f817fff,      # ... and one ulp either side of them
            0x3f804040, 0x3f8040c0, 0xbf804040, 0xbf8040c0,      # second-level ties: a 9-bit residual, even / odd retained half
            0x3f800080, 0x3f800180, 0x3f810080, 0x3f810180,
            0x3f7fffff, 0x3effffff, 0x477fe000, 0x38800000, 0x33800000]
    return from_bits32(np.array(pats, dtype=np.uint32))


def sprinkle(a, values, rng):
    """`values` written over random positions of the array `a` (in place); returns a"""
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=min(len(values), flat.size), replace=False)
    flat[idx] = values[:len(idx)]
    return a


# shapes of the GPU tests (tests/test_weight_refresh_gpu.py); tests/test_weights_ref_cpu.py holds them against the library's
# xv2_presplit_supported / xv2_presplit_f16_supported rules
PRESPLIT_SHAPES = [(rows, 9, ctot) for rows in (64, 128, 192) for ctot in (32, 64, 96)]      # (rows, T, ctot)
PRESPLIT_F16_SHAPES = [(64, 9, 32), (128, 9, 64), (64, 1, 16), (128, 1, 48)]
PACK_TAPS = (1, 2, 4, 9, 10, 13, 25, 49)
PACK_GEOMS = ((32, 32, 32), (40, 24, 32), (64, 3, 4), (33, 65, 96))      # (Cout, Cin, cin_pad)
AMAX_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 1024 * 1024 + 1)      # float4 counts


def presplit_supported(rows, T, ctot):
    return T == 9 and rows % 64 == 0 and ctot % 32 == 0


def presplit_f16_supported(rows, T, ctot):
    if T == 9:
        return presplit_supported(rows, T, ctot)
    return T == 1 and rows % 64 == 0 and ctot % 16 == 0
