"""fp64 restatement of the ``wce`` loss term (csrc/wce.hip, csrc/wce_px.h, include/xv2.h "wce"): the border distances by their
per-component definition and by the kernel's streaming rule, the border map, the loss and its gradient, the fixtures that the
CPU and the GPU test share, and the per-element error bounds the kernels are held to.

Distances.  Components are the 4-connected components of label > 0.  For a background pixel p and a component k, delta_k(p) is
the smallest dy^2 + dx^2 <= R^2 from p to a pixel of k; D1 is the smallest delta_k, D2 the second smallest over the
components; NONE = 0xFFFF where there is none, and on building pixels.  ``distances`` takes one exact Euclidean distance
transform per component (scipy; a brute-force minimum where scipy is missing), squares and rounds it (the squares are
integers), caps it at R^2 and keeps the two smallest values per pixel.  ``distances_stream`` is the kernel's rule: one pass
over the disc keeping (d1, L1), (d2, L2) with L1 != L2.

Loss.  l = logsumexp(x) - x[class], w = cw[class] + b, loss = sum w l / sum w, dlogits = gscale w (softmax - onehot) / sum w;
``post``: pixels with label 0 are dropped and the class is label - 1.  sum w == 0: loss 0, gradient 0.

Bounds.  u = 2^-24 is one fp32 rounding; every bound is a running error in the manner of tests/loss_ref.py (whose softmax
bounds are reused): each rounding charged u times the magnitude of what it rounds, incoming errors carried by the derivative.
  border map (wce_px.h, every operation rounded once, nothing fused)
    D1 + D2, D1 D2            exact (integers <= 2^20)
    r = sqrtf(D1 D2)          u r (correctly rounded); 2 r exact
    s = (D1 + D2) + 2 r       u 2 r + u s <= 2 u s
    den = 2 (sigma sigma)     u den (sigma and w0 are the fp32 values handed in: exact inputs)
    q = s / den               (2 + 1 + 1) u q = 4 u q
    e = expf(-q)              e (4 u q + A_EXP u): the argument's absolute error moves exp by that relative amount; expf 2 ulp
    b = w0 e                  b (4 q + A_EXP + 1) u, + TINY for a result in the denormal range, and exact 0 where D2 is NONE
  weight  w = cw + b          e_w = e_b + u w (cw + 0 is exact: e_w = 0 without a border term)
  forward, per pixel (softmax_px as in tests/loss_ref.py)
    l = lse - x_t             e_l = e_lse + u (|x_t| + |m| + log s)
    w l                       w e_l + |l| e_w + u w |l|
  per-thread fp32 accumulation of k = sweeps(total, 1024) pixels: (k - 1) u times the sum of the magnitudes, as in loss_ref;
  the fp64 folds add nothing.  B0, B1: the bounds of sum w l and sum w.
  loss = S0 / S1              B0 / S1 + |S0| B1 / S1^2 + u |L| (the fp32 store) + TINY
  backward (the weight has the forward's own bits; the softmax is evaluated again)
    inv = (float)(1 / S1)     inv (u + B1 / S1)
    wi = w inv                inv e_w + wi (u + B1 / S1) + u wi
    k = gscale wi             + u k                                 (the bound is for gscale = 1 and scales by |gscale|)
    v = p_c - [c == class]    e_p + u |v|
    g = k v                   k e_v + |v| e_k + u |k v| + TINY
The compiler may fuse w l into the accumulation; that removes a rounding and no bound relies on it.
"""
import math

import numpy as np
import torch

from tests.loss_ref import A_EXP, TINY, _softmax_parts, sweeps
from tests.pool_ref import U, check  # noqa: F401

try:
    from scipy import ndimage
except ImportError:      # the brute-force forms below
    ndimage = None

NONE = 0xFFFF
FWD_BLOCKS = 1024

# largest error / bound ratio per operation over every case of tests/test_wce_gpu.py on an MI355X; no bound is tuned from it
WORST = {"map": 0.496, "loss": 0.075, "grad": 0.396, "grad_against_ce": 0.320}


# ---- fixtures ------------------------------------------------------------------------------------------------------------

def rectangles(H, W, seed, n, smin=2, smax=6):
    """uint8 [H, W]: n random rectangles of side smin..smax; overlapping ones fuse into one component"""
    r = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        h, w = r.randint(smin, min(smax, H, W) + 1, 2)
        y, x = r.randint(0, H - h + 1), r.randint(0, W - w + 1)
        m[y:y + h, x:x + w] = 1
    return m


# name -> (mask builder, R).  The random-rectangle fixtures must have D2 != NONE on >= 10 % of their background pixels
# (tests/test_wce_cpu.py asserts it from `distances` alone): an all-NONE kernel cannot pass them.
RANDOM = {
    "37x45_r3": (lambda: rectangles(37, 45, 1, 30), 3),          # odd shape, tile edges cut components
    "37x45_r8": (lambda: rectangles(37, 45, 2, 12), 8),
    "70x67_r32": (lambda: rectangles(70, 67, 3, 6), 32),
}
BIG = (lambda: rectangles(1024, 1024, 4, 600, 4, 24), 15)      # 483 components, D2 on 14.8 % of the background


def _equidistant():
    m = np.zeros((9, 15), np.uint8)
    m[3:6, 2:4] = 1
    m[3:6, 11:13] = 2         # (4, 7) is 4 columns from both
    return m


def _straddle():
    m = np.zeros((70, 70), np.uint8)
    m[28:36, 27:37] = 1       # covers the corner (32, 32) of four 32 x 32 tiles
    m[40:43, 10:60] = 1       # a second one, two tiles wide
    return m


def _small():
    m = np.zeros((5, 4), np.uint8)
    m[1:3, 1:3] = 1
    return m


SPECIAL = {
    "smaller_than_the_window": (_small, 8),      # one component: D2 is NONE everywhere
    "equidistant": (_equidistant, 6),            # D1 == D2 on the middle column
    "straddles_four_tiles": (_straddle, 8),
    "empty": (lambda: np.zeros((40, 33), np.uint8), 5),
    "full": (lambda: np.ones((40, 33), np.uint8), 5),
}


# ---- distances -----------------------------------------------------------------------------------------------------------

def components(m):
    """int32 [H, W] labels 1..k of the 4-connected components of m > 0, and k"""
    if ndimage is not None:
        lab, k = ndimage.label(m > 0)
        return lab.astype(np.int32), int(k)
    H, W = m.shape
    lab = np.zeros((H, W), np.int32)
    k = 0
    for y in range(H):
        for x in range(W):
            if m[y, x] and not lab[y, x]:
                k += 1
                stack = [(y, x)]
                lab[y, x] = k
                while stack:
                    a, b = stack.pop()
                    for c, d in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                        if 0 <= c < H and 0 <= d < W and m[c, d] and not lab[c, d]:
                            lab[c, d] = k
                            stack.append((c, d))
    return lab, k


def _delta(inside):
    """squared distance from every pixel of the crop to the nearest True pixel of `inside` (exact integers)"""
    if ndimage is not None:
        e = ndimage.distance_transform_edt(~inside)
        return np.rint(e * e).astype(np.int64)
    ys, xs = np.nonzero(inside)
    yy, xx = np.mgrid[0:inside.shape[0], 0:inside.shape[1]]
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(-1).astype(np.int64)


def _boxes(lab, k):
    """the bounding box of every component as a pair of slices"""
    if ndimage is not None:
        return ndimage.find_objects(lab)
    out = []
    for i in range(1, k + 1):
        ys, xs = np.nonzero(lab == i)
        out.append((slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1)))
    return out


def distances(m, R):
    """(D1, D2) int64 [H, W] by the definition: one distance transform per component, on the component's bounding box grown by
    R (every pixel within R of the component lies inside it, and so does the whole component)"""
    lab, k = components(m)
    H, W = m.shape
    D1 = np.full((H, W), NONE, np.int64)
    D2 = np.full((H, W), NONE, np.int64)
    boxes = _boxes(lab, k)
    for i in range(1, k + 1):
        sl = boxes[i - 1]
        y0, y1 = max(sl[0].start - R, 0), min(sl[0].stop + R, H)
        x0, x1 = max(sl[1].start - R, 0), min(sl[1].stop + R, W)
        d = _delta(lab[y0:y1, x0:x1] == i)
        d[d > R * R] = NONE
        a1, a2 = D1[y0:y1, x0:x1], D2[y0:y1, x0:x1]
        lo, hi = np.minimum(a1, d), np.maximum(a1, d)
        D1[y0:y1, x0:x1] = lo
        D2[y0:y1, x0:x1] = np.minimum(a2, hi)
    bld = m > 0
    D1[bld] = NONE
    D2[bld] = NONE
    return D1, D2



def disc(R):
    """the offsets (dy, dx) of the disc in the kernel's scan order"""
    return [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * dy + dx * dx <= R * R]


def distances_stream(m, R, order=None):
    """(D1, D2) by the kernel's update rule, one disc offset after the other for all pixels at once.  order: a permutation of
    the disc's offsets (the result does not depend on it)"""
    lab, _ = components(m)
    H, W = m.shape
    pad = np.zeros((H + 2 * R, W + 2 * R), np.int64)
    pad[R:R + H, R:R + W] = lab
    big = np.iinfo(np.int64).max
    d1 = np.full((H, W), big, np.int64)
    d2 = np.full((H, W), big, np.int64)
    L1 = np.zeros((H, W), np.int64)
    L2 = np.zeros((H, W), np.int64)
    for dy, dx in (disc(R) if order is None else order):
        L = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        d = dy * dy + dx * dx
        on = L != 0
        r1 = on & (L == L1)
        r2 = on & ~r1 & (d < d1)
        r3 = on & ~r1 & ~r2 & (L == L2)
        r4 = on & ~r1 & ~r2 & ~r3 & (d < d2)
        d2 = np.where(r2, d1, np.where(r3 | r4, np.minimum(d2, d), d2))
        L2 = np.where(r2, L1, np.where(r4, L, L2))
        d1 = np.where(r1, np.minimum(d1, d), np.where(r2, d, d1))
        L1 = np.where(r2, L, L1)
    bld = m > 0
    D1 = np.where(bld | (d1 == big), NONE, d1)
    D2 = np.where(bld | (d2 == big), NONE, d2)
    return D1, D2


# ---- the border map ------------------------------------------------------------------------------------------------------

def f32(v):
    return float(np.float32(v))


def border_map(D1, D2, w0, sigma):
    """(fp64 map, its bound) for the fp32 values of w0 and sigma; exact 0 with bound 0 where D2 is NONE"""
    w0, sigma = f32(w0), f32(sigma)
    has = np.asarray(D2) != NONE
    a = np.where(has, D1, 0).astype(np.float64)
    b = np.where(has, D2, 0).astype(np.float64)
    q = (np.sqrt(a) + np.sqrt(b)) ** 2 / (2.0 * sigma * sigma)
    out = np.where(has, w0 * np.exp(-q), 0.0)
    bound = np.where(has, out * (4.0 * q + A_EXP + 1.0) * U + TINY, 0.0)
    return out, bound


# ---- loss and gradient ---------------------------------------------------------------------------------------------------

def _targets(labels, C, post, ls):
    y = labels[:, ::ls, ::ls].long()
    cls = y - 1 if post else y
    valid = (cls >= 0) & (cls < C)
    return cls.clamp(0, C - 1), valid


def weights(labels, cw, C, post=False, ls=1, bmap=None):
    """fp64 [N, H, W]: cw[class] + b at the head's pixels, 0 on dropped pixels.  cw: the fp32 values; bmap: full resolution"""
    cls, valid = _targets(labels, C, post, ls)
    w = torch.tensor([f32(v) for v in cw], dtype=torch.float64)[cls]
    if bmap is not None:
        w = w + torch.as_tensor(bmap, dtype=torch.float64)[:, ::ls, ::ls]
    return w * valid, cls, valid


def forward(logits, labels, cw, post=False, ls=1, bmap=None):
    """differentiable fp64 loss, and (S0, S1)"""
    x = logits if logits.dtype == torch.float64 else logits.double()
    w, cls, _ = weights(labels, cw, x.shape[1], post, ls, bmap)
    l = torch.logsumexp(x, 1) - x.gather(1, cls.unsqueeze(1)).squeeze(1)
    S0, S1 = (w * l).sum(), w.sum()
    return (S0 / S1 if float(S1) > 0 else S0 * 0), (S0, S1)


def backward(logits, labels, cw, post=False, ls=1, bmap=None, gscale=1.0):
    """the stated gradient gscale w (softmax - onehot) / S1 in fp64 (zeros when S1 == 0)"""
    x = logits.detach().double()
    C = x.shape[1]
    w, cls, _ = weights(labels, cw, C, post, ls, bmap)
    S1 = w.sum()
    if float(S1) <= 0:
        return torch.zeros_like(x)
    oh = torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).double()
    return f32(gscale) * (w / S1).unsqueeze(1) * (torch.softmax(x, 1) - oh)


def bounds(logits, labels, cw, post=False, ls=1, bmap=None, bmap_bound=None):
    """-> dict: loss (scalar), grad [N, C, H, W] for gscale = 1, and the fp64 values loss64, S0, S1"""
    x = logits.detach().double()
    N, C, H, W = x.shape
    w, cls, valid = weights(labels, cw, C, post, ls, bmap)
    vk = valid.double()
    e_w = torch.zeros_like(w)
    if bmap is not None:
        e_w = (torch.as_tensor(bmap_bound, dtype=torch.float64)[:, ::ls, ::ls] + U * w) * vk
    m, p, Rp, logs, e_logs = _softmax_parts(x)
    xt = x.gather(1, cls.unsqueeze(1)).squeeze(1)
    l = (m + logs) - xt
    e_l = e_logs + U * (m.abs() + logs) + U * (xt.abs() + m.abs() + logs)
    k = sweeps(N * H * W, FWD_BLOCKS)
    term = w * l.abs()
    B0 = (w * e_l + l.abs() * e_w + U * term).sum() + (k - 1) * U * term.sum()
    B1 = e_w.sum() + (k - 1) * U * w.sum()
    S0, S1 = (w * l).sum(), w.sum()
    if float(S1) <= 0:
        return {"loss": 0.0, "grad": torch.zeros_like(x), "loss64": 0.0, "S0": float(S0), "S1": 0.0}
    L = S0 / S1
    bL = B0 / S1 + S0.abs() * B1 / (S1 * S1) + U * L.abs() + TINY
    inv = 1.0 / S1
    wi = w * inv
    e_wi = inv * e_w + wi * (U + B1 / S1) + U * wi
    e_k = (e_wi + U * wi).unsqueeze(1)
    oh = torch.nn.functional.one_hot(cls, C).permute(0, 3, 1, 2).double()
    v = (p - oh).abs()
    e_v = p * Rp * U + TINY + U * v
    kk = wi.unsqueeze(1)
    grad = (kk * e_v + v * e_k + U * kk * v + TINY) * vk.unsqueeze(1)
    return {"loss": float(bL), "grad": grad, "loss64": float(L), "S0": float(S0), "S1": float(S1)}


def case(shape, seed, post=False, absent=None, scale=2.0, lshape=None):
    """fp32 logits of `shape` and uint8 labels [N, H, W] (or lshape)"""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = torch.randn(shape, generator=g) * scale
    ls = (N, H, W) if lshape is None else lshape
    y = torch.randint(0, C + 1 if post else C, ls, generator=g, dtype=torch.uint8)
    if absent is not None:
        y[y == (absent + 1 if post else absent)] = 0
    return x, y


def default_radius(sigma):
    return min(32, max(1, math.ceil(3.0 * sigma)))
