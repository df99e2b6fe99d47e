"""Coefficient tables of the whole-scene resize (csrc/resize.hip; include/xv2.h, "resize a device scene and bring its maps
back").  numpy only, importable without a GPU, and the specification of what the kernels are handed.

Pillow's resampler (libImaging/Resample.c precompute_coeffs) per axis in_size -> out_size:

    scale = in / out, filterscale = max(scale, 1), support = base * filterscale       base 2: bicubic, base 1: bilinear
    center(i) = (i + 0.5) * scale
    start(i)  = max(int(center - support + 0.5), 0)
    count(i)  = min(int(center + support + 0.5), in) - start
    weight(i, j) = filter((start + j - center + 0.5) / filterscale), j < count; summed in index order; divided by that sum

all in float64; ceil(support) * 2 + 1 coefficient slots.  This is data_loading/device_aug.resample_tables without its
"up-scaling only" restriction (that one stays as the training loader's: five slots, a window of the outputs).  Down-scaling
widens the filter - Pillow's antialiasing - so the slots grow with in / out; the kernels hold 17 (bicubic) and 9 (bilinear),
which is what the limit  out <= 4 in  and  in <= 4 out  per axis needs.

A table is int32 [out, 2 + slots]: rows {start, count, k[slots]}, unused slots zero.  uint8 images: k is the weight in 22-bit
fixed point, rounded as Pillow's normalize_coeffs_8bpc does.  fp32 maps: k holds the BITS of the fp32 nearest the float64
weight.  An axis that keeps its size carries the identity table {i, 1, one}: Pillow skips that pass, and a single tap of weight
one returns the source value itself, in either arithmetic."""
import functools

import numpy as np

PRECISION_BITS = 22
U8_TAPS, F32_TAPS = 17, 9           # include/xv2.h XV2_RESIZE_U8_TAPS, XV2_RESIZE_F32_TAPS
MAX_RATIO = 4
MIN_SCALE, MAX_SCALE, MAX_SCALES = 0.25, 4.0, 8


def check_axis(in_size, out_size):
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("resize %d -> %d: sizes must be positive" % (in_size, out_size))
    if out_size > MAX_RATIO * in_size or in_size > MAX_RATIO * out_size:
        raise ValueError("resize %d -> %d: out <= %d in and in <= %d out are required per axis" % (
            in_size, out_size, MAX_RATIO, MAX_RATIO))
    return in_size, out_size


def _bicubic(x):
    """Pillow's bicubic_filter (a = -0.5, support 2), float64, in its order of operations"""
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))


def _bilinear(x):
    """Pillow's bilinear_filter (the triangle, support 1)"""
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def axis_weights(in_size, out_size, filt, base, slots):
    """-> (start int64 [out], count int64 [out], weights float64 [out, slots]) of the whole axis, normalised"""
    in_size, out_size = check_axis(in_size, out_size)
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = base * filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    start = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int): truncation toward zero
    count = np.minimum((center + support + 0.5).astype(np.int64), in_size) - start
    if int(count.max()) > slots or int(count.min()) < 1:
        raise ValueError("resize %d -> %d: %d taps do not fit %d slots" % (in_size, out_size, int(count.max()), slots))
    j = np.arange(slots, dtype=np.int64)[None, :]
    wgt = filt(((j + start[:, None]).astype(np.float64) - center[:, None] + 0.5) * (1.0 / filterscale))
    wgt = np.where(j < count[:, None], wgt, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for jj in range(slots):                       # summed in index order, as the C loop does
        ww = ww + wgt[:, jj]
    wgt = np.where(ww[:, None] != 0.0, wgt / np.where(ww == 0.0, 1.0, ww)[:, None], wgt)
    return start, count, wgt


def _pack(start, count, k):
    tab = np.concatenate((start[:, None].astype(np.int32), count[:, None].astype(np.int32), k.astype(np.int32)), axis=1)
    tab = np.ascontiguousarray(tab)
    tab.setflags(write=False)
    return tab


def _identity(n, slots, one):
    k = np.zeros((n, slots), dtype=np.int32)
    k[:, 0] = one
    return _pack(np.arange(n, dtype=np.int64), np.ones(n, dtype=np.int64), k)


@functools.lru_cache(maxsize=32)
def axis_table_u8(in_size, out_size):
    """int32 [out, 2 + 17], read-only: Pillow's uint8 bicubic resize in_size -> out_size along one axis"""
    in_size, out_size = check_axis(in_size, out_size)
    if in_size == out_size:
        return _identity(out_size, U8_TAPS, 1 << PRECISION_BITS)
    start, count, wgt = axis_weights(in_size, out_size, _bicubic, 2.0, U8_TAPS)
    k = np.where(wgt < 0, -0.5 + wgt * float(1 << PRECISION_BITS), 0.5 + wgt * float(1 << PRECISION_BITS)).astype(np.int64)
    return _pack(start, count, k)


@functools.lru_cache(maxsize=32)
def axis_table_f32(in_size, out_size):
    """int32 [out, 2 + 9], read-only: the bilinear resample in_size -> out_size along one axis; k = the fp32 weights' bits"""
    in_size, out_size = check_axis(in_size, out_size)
    if in_size == out_size:
        return _identity(out_size, F32_TAPS, int(np.float32(1.0).view(np.int32)))
    start, count, wgt = axis_weights(in_size, out_size, _bilinear, 1.0, F32_TAPS)
    return _pack(start, count, wgt.astype(np.float32).view(np.int32))


def scaled_size(H, W, s):
    """the size an H x W scene is predicted at under scale s: data_loading/device_aug.zoomed_size, each side at least 1"""
    return max(int(round(H * s)), 1), max(int(round(W * s)), 1)


def check_scales(scales):
    """-> the scales as a tuple of floats: 1 to 8 of them, each in [0.25, 4], no duplicates; their order is kept (it is the
    summation order of the average)"""
    try:
        out = tuple(float(s) for s in scales)
    except TypeError:
        raise ValueError("scales: a sequence of numbers expected, got %r" % (scales,))
    if not 1 <= len(out) <= MAX_SCALES:
        raise ValueError("scales: %d given, 1 to %d are supported" % (len(out), MAX_SCALES))
    for s in out:
        if not MIN_SCALE <= s <= MAX_SCALE:           # (a NaN fails both comparisons)
            raise ValueError("scales: %r lies outside [%g, %g]" % (s, MIN_SCALE, MAX_SCALE))
    if len(set(out)) != len(out):
        raise ValueError("scales: duplicates in %r" % (out,))
    return out
