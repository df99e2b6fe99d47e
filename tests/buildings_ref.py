"""Host restatement of the per-building table (include/xv2.h xv2_building_table) with scipy.ndimage, the case table of
tests/test_buildings_gpu.py, and a brute-force flood fill that checks the restatement itself on tiny maps.

scipy.ndimage.label with the 4-connected structure numbers components in raster order of their first pixel, which is
ascending order of column 0 (the root).  Every column is an integer, so the comparison is ==."""
import numpy as np
from scipy import ndimage

COLS = 16
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def quantise(loc):
    """q of the contract: clamp (NaN -> 0), ONE float32 multiplication, round half to even"""
    v = np.asarray(loc, dtype=np.float32)
    return np.rint(np.fmin(np.fmax(v, np.float32(0)), np.float32(1)) * np.float32(65535)).astype(np.int64)


def vote(n4):
    """[n,4] pixel counts of classes 1..4 -> the class with the most pixels, the smaller on ties, 0 when all are 0"""
    n4 = np.asarray(n4, dtype=np.int64).reshape(-1, 4)
    return np.where(n4.max(axis=1) > 0, np.argmax(n4, axis=1) + 1, 0)


def table(mask, dmg, loc=None):
    """int64 [n,16] of one tile: components of mask != 0, dmg uint8 [H,W], loc fp32 [H,W] or None"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=FOUR)
    rows = np.zeros((n, COLS), dtype=np.int64)
    if n == 0:
        return rows
    idx = np.arange(1, n + 1)
    lin = np.arange(H * W, dtype=np.int64).reshape(H, W)
    rows[:, 0] = ndimage.minimum(lin, lab, idx)
    fg = lab > 0
    k = lab[fg].astype(np.int64) - 1
    ys, xs = np.nonzero(fg)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    rows[:, 1] = np.bincount(k, minlength=n)
    rows[:, 2], rows[:, 3] = H, W
    rows[:, 4], rows[:, 5] = -1, -1
    np.minimum.at(rows[:, 2], k, ys)
    np.minimum.at(rows[:, 3], k, xs)
    np.maximum.at(rows[:, 4], k, ys)
    np.maximum.at(rows[:, 5], k, xs)
    np.add.at(rows[:, 6], k, ys)
    np.add.at(rows[:, 7], k, xs)
    d = np.asarray(dmg)[fg].astype(np.int64)
    for c in range(1, 5):
        rows[:, 7 + c] = np.bincount(k[d == c], minlength=n)
    rows[:, 12] = np.bincount(k[(d < 1) | (d > 4)], minlength=n)
    rows[:, 13] = vote(rows[:, 8:12])
    if loc is not None:
        np.add.at(rows[:, 14], k, quantise(np.asarray(loc)[fg]))
    return rows


def flood_table(mask, dmg, loc=None):
    """the same table by a pixel-by-pixel flood fill in raster order (tiny maps only)"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    seen = np.zeros((H, W), dtype=bool)
    out = []
    for y in range(H):
        for x in range(W):
            if not mask[y, x] or seen[y, x]:
                continue
            seen[y, x] = True
            stack, px = [(y, x)], []
            while stack:
                cy, cx = stack.pop()
                px.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            r = [0] * COLS
            r[0] = y * W + x
            r[1] = len(px)
            r[2], r[3] = min(p[0] for p in px), min(p[1] for p in px)
            r[4], r[5] = max(p[0] for p in px), max(p[1] for p in px)
            r[6], r[7] = sum(p[0] for p in px), sum(p[1] for p in px)
            for py, pxx in px:
                d = int(dmg[py, pxx])
                r[7 + d if 1 <= d <= 4 else 12] += 1
                if loc is not None:
                    v = np.float32(loc[py, pxx])
                    c = np.float32(0) if np.isnan(v) else min(max(v, np.float32(0)), np.float32(1))
                    r[14] += int(np.rint(np.float32(c) * np.float32(65535)))
            best = max(r[8:12])
            r[13] = 0 if best == 0 else 1 + r[8:12].index(best)
            out.append(r)
    return np.array(out, dtype=np.int64).reshape(-1, COLS)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _hash(seed, shape, k):
    """integers 0..k-1, splitmix64 of the index (no RNG version enters the cases)"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(k)).astype(np.int64).reshape(shape)


def blobs(seed, H, W, thresh=0.5, box=5):
    """a box-filtered hashed field (box x box mean) thresholded near its mean: irregular blobs of many sizes"""
    u = _hash(seed, (H + box - 1, W + box - 1), 1 << 20).astype(np.float64) / (1 << 20)
    c = np.cumsum(np.cumsum(np.pad(u, ((1, 0), (1, 0))), axis=0), axis=1)
    mean = (c[box:, box:] - c[:-box, box:] - c[box:, :-box] + c[:-box, :-box]) / float(box * box)
    return mean[:H, :W] > thresh


def dmg_for(seed, shape):
    """uint8 damage values 0, 1..4, 5 and 255, mostly 1..4"""
    vals = np.array([1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 0, 5, 255, 2], dtype=np.uint8)
    return vals[_hash(seed, shape, len(vals))]


def halfway_values():
    """float32 values whose float32 product with 65535 is k + 0.5 exactly, so the rounding is a tie: 0.5 (the only one whose
    real product is a tie: 32767.5 -> 32768) and the float32 neighbours of (2k + 1) / 131070 whose ROUNDED product lands on
    the tie, for even and odd k (ties go to the even integer: both directions are met)"""
    k = np.arange(0, 1 << 15, dtype=np.float64)
    c = ((2 * k + 1) / 131070.0).astype(np.float32)
    prod = (c * np.float32(65535)).astype(np.float64)      # the float32 product the kernel forms
    tie = prod - np.floor(prod) == 0.5
    even = c[tie & (np.floor(prod) % 2 == 0)][-4:]
    odd = c[tie & (np.floor(prod) % 2 == 1)][-4:]
    return np.concatenate([[np.float32(0.5)], even, odd]).astype(np.float32)


def loc_for(seed, shape):
    """fp32 with NaN, +-inf, -1, 2, 0, 1, 0.5, further exact half-way products and ordinary values on a 2^-24 grid"""
    special = np.concatenate([np.array([np.nan, np.inf, -np.inf, -1, 2, 0, 1, 0.5], dtype=np.float32), halfway_values()])
    u = (_hash(seed, shape, 1 << 24).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    pick = _hash(seed + 1, shape, 3 * len(special))
    return np.where(pick < len(special), special[pick % len(special)], u).astype(np.float32)


def spiral(H, W):
    """a rectangular spiral wall one pixel wide with one-pixel gaps: one component whose root is far from most pixels"""
    m = np.zeros((H, W), dtype=bool)
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = True
        m[y0:y1 + 1, x1] = True
        m[y1, x0:x1 + 1] = True
        m[y0 + 2:y1 + 1, x0] = True
        if y0 + 2 <= y1 and x0 + 1 <= x1:
            m[y0 + 2, x0 + 1] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return m


def shape_cases():
    """name -> bool mask [H,W]"""
    yy, xx = np.mgrid[0:130, 0:130]
    plus = ((yy == 64) & (np.abs(xx - 64) <= 3)) | ((xx == 64) & (np.abs(yy - 64) <= 3))
    plus |= ((yy == 63) & (np.abs(xx - 63) <= 2)) | ((xx == 63) & (np.abs(yy - 63) <= 2))
    diag = np.zeros((9, 70), dtype=bool)
    for i in range(9):
        diag[i, i] = diag[i, 69 - i] = True          # diagonal chains: every pixel its own component
    diag[3:5, 30:33] = [[1, 0, 1], [0, 1, 0]]
    u = np.zeros((40, 90), dtype=bool)
    u[2:30, 5] = u[2:30, 80] = u[29, 5:81] = True    # a U ...
    u[5:20, 20:60] = True                            # ... around a block: one bounding box inside another
    runs_row = ((np.arange(5000) // 7) % 2 == 0)[None, :]
    runs_col = ((np.arange(5000) // 5) % 2 == 0)[:, None]
    cb = lambda H, W: (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0)
    return {
        "one_fg": np.ones((1, 1), dtype=bool),
        "one_bg": np.zeros((1, 1), dtype=bool),
        "empty_70": np.zeros((70, 70), dtype=bool),
        "full_64": np.ones((64, 64), dtype=bool),
        "blobs_65": blobs(3, 65, 65),
        "blobs_63x130": blobs(4, 63, 130),
        "plus_at_corner": plus,
        "checker_64": cb(64, 64),
        "checker_128x96": cb(128, 96),
        "checker_odd_phase_67": ~cb(67, 67),
        "diagonals": diag,
        "spiral_130x70": spiral(130, 70),
        "u_around_block": u,
        "row_5000": runs_row,
        "col_5000": runs_col,
    }


def case_inputs(name, mask):
    """(mask bool, dmg uint8, loc fp32) of a shape case"""
    s = sum(name.encode()) + 7
    return mask, dmg_for(s, mask.shape), loc_for(s + 100, mask.shape)


def label_min_index(mask):
    """int32 [H,W]: 1 + the smallest linear index of the pixel's 4-connected component, 0 for background (the labels
    xv2_label_components writes), from scipy's labelling"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=FOUR)
    if n == 0:
        return np.zeros((H, W), dtype=np.int32)
    first = ndimage.minimum(np.arange(H * W, dtype=np.int64).reshape(H, W), lab, np.arange(1, n + 1)).astype(np.int64)
    lut = np.concatenate([[0], first + 1])
    return lut[lab].astype(np.int32)
