"""Numpy restatement of the threshold / class-scale sweep (include/xv2.h xv2_calibrate_hist and xv2_postprocess_ex,
xview2_amd/utils/calibrate.py), written point by point from the rule so that it shares no arithmetic with the vectorised host
code it checks.  numpy only; the scorer and the synthesiser come from postproc_ref."""
import numpy as np

import postproc_ref as R

ONES = (1.0, 1.0, 1.0, 1.0)


def decode_post(dmg, scale=None):
    """post before masking, with per-class factors: the first maximum of the float32 products scale[c] * dmg[c]"""
    if dmg.ndim == 3 and dmg.shape[0] in (4, 5):
        d = dmg[dmg.shape[0] - 4:].astype(np.float32)
        if scale is not None:
            d = np.stack([np.float32(scale[c]) * d[c] for c in range(4)])
            assert d.dtype == np.float32
        return np.argmax(d, axis=0) + 1
    assert scale is None, "a label map has no channels to scale"
    return dmg


def fuse(loc, dmg, a=0.3, b=0.1, scale=None):
    """(pre, post) as int64 maps of the parameterised fusion; the comparisons are float32"""
    post = decode_post(dmg, scale)
    loc = loc.astype(np.float32)
    pre = (loc > np.float32(a)) | ((loc > np.float32(b)) & (post > 1))
    return pre.astype(np.int64), (post * pre).astype(np.int64)


def bins(loc, dmg, lt, dt, thresholds, scale=None):
    """(k, r, t, d, ok) per pixel: k = #{ j : loc > T_j } in float32 (NaN: 0), r = post_raw - 1, t = lt > 0, d = dt; ok is
    False where the pixel goes to `bad` (a target above 4, or a label-map value outside 1..4)"""
    T = np.asarray(thresholds, dtype=np.float32)
    k = (loc.astype(np.float32)[..., None] > T).sum(axis=-1)
    raw = np.asarray(decode_post(dmg, scale)).astype(np.int64)
    ok = (lt <= 4) & (dt <= 4) & (raw >= 1) & (raw <= 4)
    return k, raw - 1, (lt > 0).astype(np.int64), dt.astype(np.int64), ok


def hist(loc, dmg, lt, dt, thresholds, scales=None):
    """(int64 [S, n+1, 4, 2, 5], bad) over a list of tiles (or one tile)"""
    if isinstance(loc, np.ndarray) and loc.ndim == 2:
        loc, dmg, lt, dt = [loc], [dmg], [lt], [dt]
    n = len(thresholds)
    rows = [None] if scales is None else list(scales)
    out = np.zeros((len(rows), n + 1, 4, 2, 5), dtype=np.int64)
    bad = 0
    for s, scale in enumerate(rows):
        for a, b_, c, e in zip(loc, dmg, lt, dt):
            k, r, t, d, ok = bins(a, b_, c, e, thresholds, scale)
            np.add.at(out[s], (k[ok], r[ok], t[ok], d[ok]), 1)
            if s == 0:
                bad += int((~ok).sum())
    return out, bad


def derive(h, i, j):
    """the scorer's 15 counts at (A, B) = (T_i, T_j), j <= i, from one scale vector's histogram h [n+1, 4, 2, 5]"""
    assert j <= i
    Gi, Gj = h[i + 1:].sum(axis=0), h[j + 1:].sum(axis=0)
    pre = Gi.copy()
    pre[1:] += Gj[1:] - Gi[1:]
    every = h.sum(axis=(0, 1))       # [t, d]
    ltp = int(pre[:, 1, :].sum())
    row = [ltp, int(every[1].sum()) - ltp, int(pre[:, 0, :].sum())]
    for c in range(1, 5):
        tp = int(pre[c - 1, :, c].sum())
        fp = int(sum(pre[c - 1, :, d].sum() for d in range(1, 5) if d != c))
        row += [tp, int(every[:, c].sum()) - tp, fp]
    return row


def brute(loc, dmg, lt, dt, a, b, scale=None):
    """the same 15 counts the long way: fuse every tile at (a, b, scale), score it with the scorer's restatement, sum"""
    total = np.zeros(15, dtype=np.int64)
    for l, d, t1, t2 in zip(loc, dmg, lt, dt):
        pre, post = fuse(l, d, a, b, scale)
        total += np.array(R.tile_row(pre, post, t1.astype(np.int64), t2.astype(np.int64)), dtype=np.int64)
    return total.tolist()


def best(h):
    """(score, (s, i, j)) of the maximum over every point with j <= i; the first in the order (s, i, j) among equals"""
    top, arg = None, None
    for s in range(h.shape[0]):
        for i in range(h.shape[1] - 1):
            for j in range(i + 1):
                v = R.score([derive(h[s], i, j)])["score"]
                if top is None or v > top:
                    top, arg = v, (s, i, j)
    return top, arg


# ---- inputs ------------------------------------------------------------------------------------------------------------
def edge_loc(seed, shape, thresholds):
    """loc drawn from every threshold, its two float32 neighbours, NaN, -1 and 2"""
    T = np.asarray(thresholds, dtype=np.float32)
    vals = np.concatenate([T, np.nextafter(T, np.float32(4)), np.nextafter(T, np.float32(-4)),
                           np.array([np.nan, -1.0, 2.0], dtype=np.float32)]).astype(np.float32)
    return vals[R.hash_int(seed, shape, len(vals))]


def tie_dmg(seed, shape, C=4):
    """fp32 [C,H,W] on a grid of quarters, so that products with the scales of SCALES tie exactly and flip the argmax"""
    return (R.hash_int(seed, (C,) + tuple(shape), 5).astype(np.float32) * np.float32(0.25)).astype(np.float32)


# (1, 2, 1, 0.5): 2 * 0.25 == 1 * 0.5 and 0.5 * 1.0 == 1 * 0.5 are exact ties (first maximum wins); (1, 3, 0.25, 7) flips
SCALES = [ONES, (1.0, 2.0, 1.0, 0.5), (1.0, 3.0, 0.25, 7.0)]


def targets(seed, shape, wide=True):
    """(lt, dt) uint8: dt in 0..4 with buildings where lt = 0 too; wide: one pixel in 16 holds 5 or 255 in lt or dt"""
    dt = R.hash_int(seed, shape, 5).astype(np.uint8)
    lt = (R.hash_int(seed + 1, shape, 3) > 0).astype(np.uint8) * (1 + R.hash_int(seed + 2, shape, 4)).astype(np.uint8)
    if wide:
        w = R.hash_int(seed + 3, shape, 16)
        lt = np.where(w == 0, np.uint8(5), lt)
        dt = np.where(w == 1, np.uint8(255), dt)
        lt = np.where(w == 2, np.uint8(255), lt)
        dt = np.where(w == 3, np.uint8(5), dt)
    return lt.astype(np.uint8), dt.astype(np.uint8)


def tiles(seed, count, H, W, thresholds, C=4):
    """count tuples (loc, dmg, lt, dt) with targets in 0..4 only, for the scored paths"""
    out = []
    for k in range(count):
        s = seed + 10 * k
        lt, dt = targets(s + 2, (H, W), wide=False)
        out.append((edge_loc(s, (H, W), thresholds), tie_dmg(s + 1, (H, W), C), (lt > 0).astype(np.uint8), dt))
    return out
