"""Float64 restatement of the pooling, resampling and glue kernels (csrc/pool.hip, the elementwise / gate / layout part of
csrc/pointwise.hip) and the per-element error bounds they are held to.  NHWC tensors in, float64 out, built from
torch.nn.functional on .double() inputs and torch.autograd.grad, as tests/conv_ref.py does for the convolutions.

Every kernel here except max-pool and add-relu is a linear map f(X) with a handful of terms per element, summed serially
in fp32.  The bounds are therefore worst-case counts of roundings, with no calibrated tail factor.  u = 2^-24 (one fp32
rounding: fl(x) = x (1 + d), |d| <= u) and a_i = f(|X|)_i in float64, the sum of the |terms| behind element i:

  avg-pool forward     (k*k + 1) u a_i           at most k*k additions (each rounds a partial sum <= a_i), one division
  avg-pool backward    (T_i + 2) u a_i           T_i windows contain input i (at most ceil(k/s)^2): per term the rounding of
                                                 1 / (dh dw) and of the product, and T_i additions
  adaptive forward     (K_i + 1) u a_i           K_i pixels in the window
  adaptive backward    (B_i + 2) u a_i           B_i bins contain the pixel; as avg-pool backward
  max-pool backward    (T_i + 1) u a_i           T_i <= 4 windows route their gradient to input i: T_i additions
  gate-mul out, dskip  u |y64_i|                 one product
  gate-mul dgate       (C/4 + log2 L + 2) u sum_c |dout skip|     L = head_lanes(C) lanes of C / (4 L) chunks of four
                                                 products each, then log2 L shuffle additions
  axpby                2 u (|alpha a_i| + |beta b_i|)    two products and one addition (fewer where the compiler fuses one
                                                 product into the addition): u |alpha a| + u |beta b| + u |their sum|
  max-pool forward, add-relu, every copy and layout kernel: bit-exact (max-pool and the copies move values; add-relu is one
                                                 correctly rounded fp32 addition, rounded once more by a bf16 store)

Bilinear, align_corners=True.  An output's source coordinate is src = scale * o with scale = fl((I - 1) / (O - 1)): two fp32
roundings, |d src| <= 2 u src <= 2 u I per axis.  The interpolation weight of an input is the tent function 1 - |src - i|,
which is 1-Lipschitz: an error of d src moves every weight by at most |d src|, also where src crosses an integer and the
kernel picks the other corner pair (the tent is continuous there).
  forward   u (6 + 2 (IH + IW)) max_{h,w} |x[n,:,:,c]|: six roundings of the four-term expression (1 - lh, 1 - lw, the
            products, the sums) on at most max|x|, and the weight error 2 u IH + 2 u IW times max|x|.
  backward  dx_i = sum_o wh(oh, ih) ww(ow, iw) dy_o over the nh_i x nw_i outputs whose source lies within one pixel of i.
            Roundings on exact weights: wh * ww, the product with dy, and one addition per term: (nh_i nw_i + 2) u a_i,
            a = f^T(|dy|).  Weight error: every row weight is off by at most eh = u (2 IH + 2) (2 u IH from src, u from
            1 - lh, u where both taps land on the clamped last row and their weights are added), every column weight by
            ew = u (2 IW + 2); first order in u that is
                max_{h,w} |dy[n,:,:,c]| * (eh nh_i cw_i + ew nw_i ch_i),
            ch_i / cw_i the exact column sums of the row / column weights of input i (sum over oh of wh(oh, ih)).  nh_i counts
            the outputs with |src - i| < 1 + 2^-10, so that an output sitting exactly on the edge of the tent, whose exact
            weight is 0 and whose computed one may be eh, is counted.

bf16 storage: the tests round the inputs to bf16 themselves, the kernels compute in fp32, and the only extra term is the
rounding of the result on store, 2^-8 |y64_i| (tests/conv_ref.py).  Max-pool forward stays exact.

Accumulating backward (the kernel adds onto a gradient `old` already in dx): the reference is old + f^T(dy) in float64.
Where ONE addition joins the two (adaptive backward adds old last; the fallback of the pooling nodes adds two finished
tensors) the bound gains u (|old_i| + a_i).  The max-pool and avg-pool kernels load old FIRST and add their T_i terms onto
it, so old is part of every partial sum and each of the T_i additions may round by u (|old_i| + a_i): the term is
max(T_i, 1) u (|old_i| + a_i) there.  (With a single u (|old| + a) an fp32 CPU emulation of that summation order exceeds the
bound at k = 3, s = 1, T = 9: tests/test_pool_ref_cpu.py::test_accumulate_bound_counts_every_addition.)  bf16 storage adds
2^-8 |result_i| for the store; the fallback stores f^T(dy) as bf16 BEFORE the addition, which costs another
2^-8 (1 + 2^-8) |f^T(dy)_i|.

Elements whose bound is 0 (a_i = 0: nothing reaches them) must equal the reference exactly.  check() returns the worst
error / bound ratio and where it is.  WORST records the largest ratio of every operation over the GPU run of
tests/test_pool_glue_gpu.py; the bounds are not tuned from it.
"""
import math

import torch
import torch.nn.functional as F

from tests.conv_ref import lognormal, nchw, nhwc  # noqa: F401  (lognormal: the tests' input distribution)

U = 2.0 ** -24
B16 = 2.0 ** -8

# largest error / bound ratio per operation over every case of tests/test_pool_glue_gpu.py on an MI355X (fp32 and bf16
# storage, in-place and fallback accumulation, strided operands and grid-stride cases included)
WORST = {
    "maxpool_bwd": 0.479, "maxpool_bwd_bf16": 0.996, "maxpool_acc": 0.902, "maxpool_acc_bf16": 0.996,
    "avgpool_fwd": 0.410, "avgpool_fwd_bf16": 0.996, "avgpool_bwd": 0.507, "avgpool_bwd_bf16": 0.996,
    "avgpool_acc": 0.970, "avgpool_acc_bf16": 0.996,
    "adaptive_fwd": 0.395, "adaptive_bwd": 0.591, "adaptive_bwd_acc": 0.989,
    "bilinear_fwd": 0.241, "bilinear_bwd": 0.311,
    "gate_out": 0.9999, "gate_out_bf16": 0.995, "gate_dskip": 0.9998, "gate_dskip_bf16": 0.995,      # (one rounding, at its bound)
    "gate_dgate": 0.666, "gate_dgate_bf16": 0.376,
    "axpby": 0.498,
}      # a bf16 store's error is its half-ulp rounding, an accumulation onto a much larger `old` the rounding of that addition

# ---- case tables (shared by the CPU test of the bounds and the GPU test of the kernels) ----------------------------------
MAXPOOL_SHAPES = [(1, 1, 1, 4), (2, 1, 7, 4), (1, 2, 2, 8), (2, 7, 5, 12), (1, 8, 6, 32), (2, 18, 22, 32)]      # N, H, W, C
# k, s, pad, ceil_mode, count_include_pad: the model's four, then the added ones
AVG_CFGS = [(3, 1, 1, False, True), (3, 2, 1, False, True), (1, 1, 0, True, False), (2, 2, 0, True, False),
            (3, 2, 1, True, True), (3, 2, 1, True, False), (2, 2, 0, False, False), (3, 3, 1, True, True)]
AVG_HW = [(1, 1), (2, 3), (7, 5), (8, 8), (17, 19), (18, 21)]
ADAPTIVE_BINS = [1, 2, 3, 6]
ADAPTIVE_HW = [(1, 1), (2, 2), (2, 5), (4, 4), (6, 6), (7, 5), (18, 22)]
BILINEAR_CASES = [(1, 1, 8, 8), (1, 5, 4, 1), (5, 1, 1, 4), (7, 9, 1, 3), (2, 2, 64, 64), (3, 3, 16, 16), (9, 11, 18, 22),
                  (33, 31, 64, 64), (16, 16, 8, 8), (64, 64, 5, 3), (8, 8, 8, 8)]      # IH, IW, OH, OW
GATE_C = [4, 8, 12, 32, 64, 96, 256, 512]
GATE_PIX = (2, 5, 7)
N_C = (2, 8)      # batch and channels of the avg-pool, adaptive and bilinear cases


def avg_cases():
    """(k, s, pad, ceil, incl, H, W) that torch accepts (it rejects an input smaller than the window minus the padding)"""
    out = []
    for (k, s, pad, ceil, incl) in AVG_CFGS:
        for (H, W) in AVG_HW:
            if H + 2 * pad >= k and W + 2 * pad >= k:
                out.append((k, s, pad, ceil, incl, H, W))
    return out


def tie_heavy(shape, gen, dtype=torch.float32):
    """values from {0, 0.5, 1, 2} and a zeroed 4x4 corner: most windows hold their maximum more than once"""
    v = torch.tensor([0.0, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, shape, generator=gen)]
    v[:, :4, :4, :] = 0.0
    return v.to(dtype)


def head_lanes(C):
    """csrc/head_fuse.h: lanes that share one pixel in gate_mul_bwd_kernel"""
    L = 1
    while L * 2 <= 64 and L * 2 * 4 <= C:
        L *= 2
    return L


def _vjp(f, in_shape, dy):
    """f^T(dy) of a linear map f, float64"""
    x = torch.zeros(in_shape, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(f(x), x, dy.double())
    return dx


# ---- max-pool 3x3 / stride 2 / pad 1 -----------------------------------------------------------------------------------

def maxpool3x3s2_fwd(x):
    """first maximum in scan order; a NaN wins and stays (torch CPU)"""
    return nhwc(F.max_pool2d(nchw(x.double()), 3, 2, 1))


def maxpool3x3s2_bwd(x, dy):
    """dx: every window's gradient goes to its first maximum"""
    xd = nchw(x.double()).contiguous().requires_grad_(True)
    (dx,) = torch.autograd.grad(F.max_pool2d(xd, 3, 2, 1), xd, nchw(dy.double()).contiguous())
    return nhwc(dx)


def maxpool_taps(x):
    """[N, OH, OW, C, 9]: the nine taps of every window in scan order, -inf outside the image"""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((N, 2 * OH + 2, 2 * OW + 2, C), -math.inf, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x.double()
    return torch.stack([xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] for kh in range(3) for kw in range(3)], dim=-1)


def maxpool3x3s2_bwd_rule(x, dy, rule="first"):
    """the backward spelled out over the taps: rule "first" is maxpool3x3s2_bwd, "last" breaks ties towards the last maximum,
    "all" credits every tied tap"""
    N, H, W, C = x.shape
    taps = maxpool_taps(x)
    OH, OW = taps.shape[1], taps.shape[2]
    hit = taps == taps.max(dim=-1, keepdim=True).values
    if rule == "first":
        sel = F.one_hot(hit.to(torch.uint8).argmax(dim=-1), 9).bool()
    elif rule == "last":
        sel = F.one_hot(8 - hit.flip(-1).to(torch.uint8).argmax(dim=-1), 9).bool()
    else:
        sel = hit
    dxp = torch.zeros((N, 2 * OH + 2, 2 * OW + 2, C), dtype=torch.float64)
    t = 0
    for kh in range(3):
        for kw in range(3):
            dxp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += sel[..., t] * dy.double()
            t += 1
    return dxp[:, 1:H + 1, 1:W + 1]


def maxpool_bwd_bound(x, dy):
    """(T_i + 1) u a_i -> (bound, a, T)"""
    a = maxpool3x3s2_bwd(x, dy.double().abs())
    T = maxpool3x3s2_bwd(x, torch.ones_like(dy, dtype=torch.float64))
    return (T + 1) * U * a, a, T


# ---- avg-pool ------------------------------------------------------------------------------------------------------------

def avgpool_out_size(L, k, s, pad, ceil_mode, last_rule=True):
    """torch's pooling output extent: in ceil mode the last window must start inside the input or the left padding"""
    num = L + 2 * pad - k
    o = (-(-num // s) if ceil_mode else num // s) + 1
    if last_rule and ceil_mode and (o - 1) * s >= L + pad:
        o -= 1
    return o


def avgpool_fwd(x, k, s, pad, ceil_mode, count_include_pad, divisor_override=None):
    return nhwc(F.avg_pool2d(nchw(x.double()), k, s, pad, ceil_mode, count_include_pad, divisor_override))


def avgpool_bwd(dy, in_hw, k, s, pad, ceil_mode, count_include_pad, divisor_override=None):
    shape = (dy.shape[0], in_hw[0], in_hw[1], dy.shape[3])
    return _vjp(lambda x: avgpool_fwd(x, k, s, pad, ceil_mode, count_include_pad, divisor_override), shape, dy)


def avgpool_windows(dy_shape, in_hw, k, s, pad, ceil_mode):
    """T_i: the number of windows that contain input i"""
    return avgpool_bwd(torch.ones(dy_shape, dtype=torch.float64), in_hw, k, s, pad, ceil_mode, True, divisor_override=1)


def avgpool_fwd_bound(x, k, s, pad, ceil_mode, count_include_pad):
    return (k * k + 1) * U * avgpool_fwd(x.double().abs(), k, s, pad, ceil_mode, count_include_pad)


def avgpool_bwd_bound(dy, in_hw, k, s, pad, ceil_mode, count_include_pad):
    """-> (bound, a, T)"""
    a = avgpool_bwd(dy.double().abs(), in_hw, k, s, pad, ceil_mode, count_include_pad)
    T = avgpool_windows(dy.shape, in_hw, k, s, pad, ceil_mode)
    return (T + 2) * U * a, a, T


def avg_matrix(L, k, s, pad, ceil_mode, count_include_pad, last_rule=True, full_divisor=False):
    """[O, L]: one axis of the avg-pool spelled out (the 2-d pool is the product of its two axes); last_rule / full_divisor
    switch on the deliberately wrong variants of tests/test_pool_ref_cpu.py"""
    O = avgpool_out_size(L, k, s, pad, ceil_mode, last_rule)
    M = torch.zeros((O, L), dtype=torch.float64)
    for o in range(O):
        st = o * s - pad
        en = min(st + k, L + pad)
        pool = en - st
        lo, hi = max(st, 0), min(en, L)
        d = k if full_divisor else (pool if count_include_pad else hi - lo)
        if hi > lo and d > 0:
            M[o, lo:hi] = 1.0 / d
    return M


# ---- adaptive avg-pool ---------------------------------------------------------------------------------------------------

def adaptive_fwd(x, bins):
    return nhwc(F.adaptive_avg_pool2d(nchw(x.double()), bins))


def adaptive_bwd(dy, in_hw, bins):
    shape = (dy.shape[0], in_hw[0], in_hw[1], dy.shape[3])
    return _vjp(lambda x: adaptive_fwd(x, bins), shape, dy)


def ada_matrix(L, bins, end_floor=False):
    """[bins, L]: window i = [floor(i L / bins), ceil((i + 1) L / bins)); end_floor is the wrong variant"""
    M = torch.zeros((bins, L), dtype=torch.float64)
    for i in range(bins):
        lo = (i * L) // bins
        hi = ((i + 1) * L) // bins if end_floor else -(-((i + 1) * L) // bins)
        if hi > lo:
            M[i, lo:hi] = 1.0 / (hi - lo)
    return M


def _outer(vh, vw):
    """[1, H, W, 1] from per-row and per-column vectors"""
    return (vh[:, None] * vw[None, :])[None, :, :, None]


def adaptive_fwd_bound(x, bins):
    """(K_i + 1) u a_i"""
    H, W = x.shape[1], x.shape[2]
    K = _outer((ada_matrix(H, bins) != 0).sum(1).double(), (ada_matrix(W, bins) != 0).sum(1).double())
    return (K + 1) * U * adaptive_fwd(x.double().abs(), bins)


def adaptive_bwd_bound(dy, in_hw, bins):
    """(B_i + 2) u a_i -> (bound, a)"""
    B = _outer((ada_matrix(in_hw[0], bins) != 0).sum(0).double(), (ada_matrix(in_hw[1], bins) != 0).sum(0).double())
    a = adaptive_bwd(dy.double().abs(), in_hw, bins)
    return (B + 2) * U * a, a


def sep_fwd(x, Mh, Mw):
    """y[n, p, q, c] = sum_hw Mh[p, h] Mw[q, w] x[n, h, w, c]"""
    return torch.einsum("ph,nhwc,qw->npqc", Mh, x.double(), Mw)


def sep_bwd(dy, Mh, Mw):
    return torch.einsum("ph,npqc,qw->nhwc", Mh, dy.double(), Mw)


# ---- bilinear, align_corners=True ----------------------------------------------------------------------------------------

def bilinear_fwd(x, OH, OW, align_corners=True):
    return nhwc(F.interpolate(nchw(x.double()), (OH, OW), mode="bilinear", align_corners=align_corners))


def bilinear_bwd(dy, IH, IW):
    shape = (dy.shape[0], IH, IW, dy.shape[3])
    return _vjp(lambda x: bilinear_fwd(x, dy.shape[1], dy.shape[2]), shape, dy)


def _bil_src(I, O):
    return torch.arange(O, dtype=torch.float64) * ((I - 1) / (O - 1) if O > 1 else 0.0)


def bil_matrix(I, O):
    """[O, I]: the tent weights 1 - |src_o - i| of one axis"""
    return (1.0 - (_bil_src(I, O)[:, None] - torch.arange(I, dtype=torch.float64)[None, :]).abs()).clamp_min(0.0)


def bil_candidates(I, O):
    """bil_range of csrc/pool.hip in its fp32 arithmetic: per input index the [lo, hi] range of outputs the backward kernel visits"""
    f32 = torch.float32
    if O <= 1 or I <= 1:
        return [(0, O - 1)] * I
    scale = (torch.tensor(float(I - 1), dtype=f32) / torch.tensor(float(O - 1), dtype=f32))
    out = []
    for i in range(I):
        lo = int(torch.floor(torch.tensor(float(i - 1), dtype=f32) / scale)) - 1
        hi = int(torch.ceil(torch.tensor(float(i + 1), dtype=f32) / scale)) + 1
        out.append((max(lo, 0), min(hi, O - 1)))
    return out


def bil_matrix_dropped(I, O):
    """the wrong variant: contributions outside [lo + 1, hi - 1] of the candidate range are dropped"""
    M = bil_matrix(I, O).clone()
    for i, (lo, hi) in enumerate(bil_candidates(I, O)):
        M[:lo + 1, i] = 0.0
        M[hi:, i] = 0.0
    return M


def bilinear_fwd_bound(x, OH, OW):
    N, IH, IW, C = x.shape
    m = x.double().abs().amax(dim=(1, 2), keepdim=True)
    return (U * (6 + 2 * (IH + IW)) * m).expand(N, OH, OW, C)


def bilinear_bwd_bound(dy, IH, IW):
    """module docstring -> (bound, a)"""
    N, OH, OW, C = dy.shape
    a = bilinear_bwd(dy.double().abs(), IH, IW)
    near = 1.0 + 2.0 ** -10

    def axis(I, O):
        d = (_bil_src(I, O)[:, None] - torch.arange(I, dtype=torch.float64)[None, :]).abs()
        return (d < near).sum(0).double(), bil_matrix(I, O).sum(0)
    nh, ch = axis(IH, OH)
    nw, cw = axis(IW, OW)
    eh, ew = U * (2 * IH + 2), U * (2 * IW + 2)
    m = dy.double().abs().amax(dim=(1, 2), keepdim=True)
    return (_outer(nh, nw) + 2) * U * a + m * (eh * _outer(nh, cw) + ew * _outer(ch, nw)), a


# ---- gate-mul, add-relu, channel concat / split --------------------------------------------------------------------------

def gate_mul(skip, gate, dout):
    """skip [.., C], gate [.., 1] -> out, dskip, dgate and the scale sum_c |dout skip| of dgate"""
    s, g, d = skip.double(), gate.double(), dout.double()
    return s * g, d * g, (d * s).sum(-1, keepdim=True), (d * s).abs().sum(-1, keepdim=True)


def gate_dgate_bound(C, scale, lanes=None):
    L = head_lanes(C) if lanes is None else lanes
    return (C / 4 + math.log2(L) + 2) * U * scale


def gate_dgate_first_chunk(skip, dout):
    """the wrong variant: only the first 4 L channels are summed"""
    n = 4 * head_lanes(skip.shape[-1])
    return (dout.double()[..., :n] * skip.double()[..., :n]).sum(-1, keepdim=True)


def add_relu(a, b):
    """relu(a + b) as the kernel computes it: one fp32 addition, stored in the operands' type; float64 of those bits"""
    return (a.float() + b.float()).clamp_min(0.0).to(a.dtype).double()


def add_relu_bwd(r, dr):
    return torch.where(r.double() > 0, dr.double(), torch.zeros((), dtype=torch.float64))


def axpby(alpha, a, beta, b=None):
    """-> (alpha a + beta b, its bound); alpha and beta as the fp32 values the kernel receives"""
    al, be = float(torch.tensor(alpha, dtype=torch.float32)), float(torch.tensor(beta, dtype=torch.float32))
    t0 = al * a.double()
    t1 = be * b.double() if b is not None else torch.zeros_like(t0)
    return t0 + t1, 2 * U * (t0.abs() + t1.abs())


def cat_channels(xs):
    return torch.cat([t.double() for t in xs], dim=-1)


def split_channels(d, cs):
    return list(torch.split(d.double(), list(cs), dim=-1))


def pair_cat(t):
    """[2B, H, W, C] (B pre rows, then B post rows) -> [B, H, W, 2C]"""
    B = t.shape[0] // 2
    return torch.cat([t[:B].double(), t[B:].double()], dim=-1)


def pair_split(d):
    C = d.shape[-1] // 2
    return torch.cat([d[..., :C].double(), d[..., C:].double()], dim=0)


# ---- bounds of the storage type and of accumulation, the gate -----------------------------------------------------------

def stored(bound, y64, bf16):
    """the bound of a result that is stored as bf16"""
    return bound + B16 * y64.abs() if bf16 else bound


def accumulated(bound, a, old, adds, result, bf16=False, fallback=False):
    """bound of old + f^T(dy): `bound` and `a` belong to f^T(dy) alone, `adds` additions are made after old joined the sum
    (tensor or number); fallback: two finished tensors are added, bf16: f^T(dy) was stored before that (module docstring)"""
    old = old.double()
    if not torch.is_tensor(adds):
        adds = torch.full_like(a, float(adds))
    b = bound + adds.clamp_min(1.0) * U * (old.abs() + a)
    if bf16:
        b = b + B16 * result.abs()
        if fallback:
            b = b + B16 * (1.0 + B16) * (result - old).abs()
    return b


def check(y, y64, bound):
    """-> (worst error / bound, flat index of that element).  Where the bound is 0 the result must equal the reference; a
    non-finite result or a result of another shape fails (ratio inf)."""
    if tuple(y.shape) != tuple(y64.shape):
        return math.inf, -1
    y, y64 = y.detach().cpu().double(), y64.double()
    if y.numel() == 0:
        return 0.0, -1
    e = (y - y64).abs()
    b = bound.double().expand_as(e) if torch.is_tensor(bound) else torch.full_like(e, float(bound))
    ratio = torch.where(b == 0, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, math.inf)), e / b.clamp_min(1e-300))
    ratio = ratio.nan_to_num(nan=math.inf, posinf=math.inf)
    where = int(torch.argmax(ratio.flatten()).item())
    return float(ratio.flatten()[where]), where
