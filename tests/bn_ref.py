"""Float64 restatement of the BatchNorm kernels (csrc/norm_act.hip, csrc/bn_fold.h) at the op level of include/xv2.h, the
per-element error bounds they are held to, and the shape / path tables shared by tests/test_bn_ref_cpu.py (the gates, without a
GPU) and tests/test_bn_gpu.py (the kernels).  Tensors are [npix, C] (NHWC with the pixels flattened); inputs are rounded to the
storage type by the test before the reference sees them; everything here is float64.

Two kinds of case.  EXACT cases use small integers (and invstd = 0.5), so that every sum a kernel forms is exact in fp32 in any
order as long as npix * max|term| < 2^23: the result must equal the integer reference bit for bit, at every geometry of the
tables below, with no tolerance and no restatement of the kernels' chunking.  REAL-valued cases are held to the bounds below,
u = 2^-24 (one fp32 rounding: fl(x) = x (1 + d), |d| <= u), first order in u, no calibrated factor.

Column sums (xv2_bn_tensor_stats, xv2_bn_act_backward_reduce[_mask], the sums of xv2_bn_rows_backward).  A sum of n fp32 terms,
in ANY order (serial, pairwise, per lane then across lanes, partly in fp64), errs by at most (n - 1) u sum|t|: every addition
rounds a partial sum that is at most sum|t|.  With r roundings inside one term the bound is (n - 1 + r) u sum|t|, sum|t| in
float64.  It is order-free on purpose: a kernel that changes its summation order must still pass.  r per term:
    x - x0             1      (the shifted sums of tensor_stats: x0 = the first row)
    (x - x0)^2         2      ((1 + d)^2; the product itself is contracted into the accumulation.  Uncontracted it would be 3,
                               which matters at n = 1 only, where x - x0 = 0)
    g = dz act'        1      (NONE / ReLU multiply by 1 or 0, exactly; LeakyReLU rounds the product with 0.01f)
    g xhat             3      (y - mean, times invstd, and g; the product g * xhat is contracted into the accumulation)
  Sigmoid's derivative z (1 - z) is itself computed in fp32 (two more roundings, or - in the recomputed form, from
  z = 1 / (1 + expf(-pre)) - the error of z, below): g_of() returns the absolute error g_err of fl(g), and the sums gain what
  it exceeds the one rounding counted above: sum(excess) and sum(excess |xhat|).
  tensor_stats is compared after the un-shift (fp64 in the kernel): bound(sum x) = bound(S1'), bound(sum x^2) = bound(S2') +
  2 |x0| bound(S1').  dgamma / dbeta are the fp32 roundings of the fp64 sums: u |value| more.

xv2_bn_finalize / xv2_bn_reduce_finalize / xv2_bn_eval_coeffs: finalize() restates bn_fold.h in numpy float64 in the same
operation order (contraction is off in the kernel), including var < 0 -> 0 and count == 1 -> unbiased = var, without the fp32
roundings.  m = s1 / count and var = s2 / count - m m are the same IEEE operations on both sides; the bounds still allow for
the cancellation, dvar = 4 * 2^-53 (s2 / count), which moves invstd by invstd dvar / (2 (var + eps)), because fp64 sqrt and
division may differ in the last bit - nothing is required bit for bit.
    mean               u |m|
    invstd             u is + dis,   dis = is dvar / (2 (var + eps))
    scale              fl(g fl(is)):                       2 u |sc| + |g| dis
    shift              b - fl(fl(m) sc):                   5 u |m sc| + u |b| + |g m| dis
                       (fl(m), the two roundings of sc, the product, and the subtraction on |b| + |m sc|)
    running_mean       fl(fl(keep rm) + fl(mom fl(m))), keep = fl(1 - mom):      3 u (|keep rm| + |mom m|)
    running_var        the same on the unbiased variance:                       3 u (|keep rv| + |mom unb|) + mom dvar count / (count - 1)
  eval_coeffs: is = 1 / sqrtf(rv + eps) is three roundings (the sum counts half): 3 u is; scale 4 u |sc|; shift
  6 u |rm sc| + u |b|.

Forward apply, z = act(fma(y, scale, shift) [+ residual]).  u |pre| for the fma; with a residual u (|fma| + |res|) more; ReLU and
LeakyReLU are 1-Lipschitz, so the error of the pre-activation passes through at most unchanged (also where rounding moves it
across 0), and the leaky slope costs one product, u |z|.  Sigmoid: the HIP math documentation (the ulp table of expf) is not
part of the ROCm installation this was written on, so no ulp figure is quoted: sigmoid_rel() measures torch's fp32
1 / (1 + exp(-v)) on the CPU against float64 over the very inputs of the case (and over a fixed sample of the tests' input
distribution and of [-80, 20]: a case of four elements measures little) and takes twice the worst relative error; the
pre-activation's error enters through the derivative z (1 - z) <= 1/4.  A sigmoid far in its tail underflows (expf overflows
at pre < -88, z and z (1 - z) become subnormal), so every sigmoid bound carries the absolute term 2^-126, the smallest normal
fp32 (times |dz| in g).  The mask byte is compared with the kernel's own z:
bit k of byte row * C/4 + j == (z[4j + k] > 0), exactly.

Backward apply, dy = gi (g - sg - xhat sgx), gi = gamma invstd, sg = sums2[:, 0] / count, sgx = sums2[:, 1] / count, with sums2
taken from the float64 reference (an input of the entry point).  Roundings: gi 1; g as above; sg and sgx 3 each ((float) sum,
(float)(1 / count), their product); xhat 2; xhat sgx 1; the two subtractions and the final product.  Collected:
    u |gi| (4 |g| + 7 |sg| + 9 |xhat sgx|) + |gi| g_err      (|g|: both subtractions, gi and the final product)
  eval mode (train = 0): dy = gi g, two products: 2 u |gi g| + |gi| g_err.  dres = g: one product, max(u |g|, g_err).
  xv2_bn_rows_backward uses its OWN fp32 sums (serial over rows <= 64, bounded as column sums with n = rows), so their bounds
  enter dy as |gi| (dsg + |xhat| dsgx) / rows.

The activation masks need no exclusions.  z and the mask are inputs of the backward entry points.  In the recomputed form the sign
of fma(y, scale, shift) is the sign of y.double() * scale.double() + shift.double(): the product of two fp32 values is exact in
fp64 and a correctly rounded sum keeps the sign of the exact one (the tests assert that no real-valued case holds an exact zero
there).

xv2_bn_rows_forward: the kernel takes two-pass fp64 statistics, as rows_forward() does, so mean and invstd carry one fp32
rounding (plus a float64 allowance for the different summation, (rows + 2) 2^-52 relative to |m| and to 1 + |m| / std); scale,
shift and the running statistics as in finalize; z as forward apply with the coefficient errors |y| dsc + dsh added.

bf16 storage: the only extra term is the rounding of a stored tensor, 2^-8 |y64_i| (tests/conv_ref.py).  Statistics have no
bf16 form (the ABI has no dtype there).

check() is tests/pool_ref.check: worst error / bound and where; bound 0 means exact.  WORST holds the largest ratio per operation
over the run of tests/test_bn_gpu.py on an MI355X; the bounds are not tuned from it.
"""
import math

import numpy as np
import torch

from tests.conv_ref import lognormal  # noqa: F401  (the tests' input distribution)
from tests.pool_ref import check  # noqa: F401

U = 2.0 ** -24
B16 = 2.0 ** -8
D53 = 2.0 ** -53
FLOOR = 2.0 ** -126                          # the smallest normal fp32: below it a result carries no relative accuracy
NONE, RELU, LEAKY, SIGMOID = 0, 1, 2, 3      # XV2_ACT_*
ACTS = (NONE, RELU, LEAKY, SIGMOID)
F32, BF16 = 0, 1                             # XV2_F32 / XV2_BF16
SLOPE = float(np.float32(0.01))
SCRATCH_ROWS = 64                            # XV2_BN_SCRATCH_ROWS
RS1_MAX_TILES = 1024                         # norm_act.hip: the one-phase fold up to here, the ticket kernel above

# largest error / bound ratio per operation over every case of tests/test_bn_gpu.py on an MI355X (fp32 and bf16 storage; a bf16
# store's error is its half-ulp rounding, a single fma's or product's its one rounding; the order-free column-sum bounds are
# worst cases over n additions and are met to a few percent)
WORST = {
    "backward_apply": 0.815, "backward_apply_bf16": 0.996, "backward_apply_eval": 0.954, "backward_apply_eval_bf16":
    0.996, "backward_apply_eval_sigmoid": 0.765, "backward_apply_eval_sigmoid_bf16": 0.996, "backward_apply_sigmoid":
    0.645, "backward_apply_sigmoid_bf16": 0.996, "backward_sums": 0.081, "backward_sums_bf16": 0.065, "dbeta": 0.014,
    "dbeta_bf16": 0.015, "dgamma": 0.081, "dgamma_bf16": 0.064, "dres": 0.985, "dres_bf16": 0.928, "dres_sigmoid": 0.849,
    "dres_sigmoid_bf16": 0.996, "eval_scale": 0.480, "eval_shift": 0.375, "finalize_invstd": 0.874, "finalize_mean":
    0.762, "finalize_running_mean": 0.586, "finalize_running_var": 0.408, "finalize_scale": 0.839, "finalize_shift":
    0.488, "forward": 0.999, "forward_bf16": 0.996, "forward_sigmoid": 0.891, "forward_sigmoid_bf16": 0.996,
    "reduce_finalize_invstd": 0.855, "reduce_finalize_mean": 0.681, "reduce_finalize_running_mean": 0.545,
    "reduce_finalize_running_var": 0.495, "reduce_finalize_scale": 0.751, "reduce_finalize_shift": 0.594, "rows_dbeta":
    0.752, "rows_dbeta_sigmoid": 0.655, "rows_dgamma": 0.823, "rows_dgamma_sigmoid": 0.607, "rows_dy": 0.948,
    "rows_dy_sigmoid": 0.724, "rows_invstd": 0.998, "rows_mean": 0.999, "rows_running_mean": 0.744, "rows_running_var":
    0.755, "rows_scale": 0.924, "rows_shift": 0.925, "rows_z": 0.810, "rows_z_sigmoid": 0.643, "stats_finalize_invstd":
    0.013, "stats_finalize_mean": 0.792, "tensor_stats": 0.021,
}

# ---- shape and path tables -----------------------------------------------------------------------------------------------
C_VECTOR = (4, 8, 64, 256)                   # column form with one block row = the whole channel range (cgw == C)
C_GROUPED = (512, 768)                       # 256-channel groups along grid.y
C_GENERIC = (1, 3, 12, 24, 65, 96, 130, 192, 320)      # 64 channel lanes x 4 row lanes; 130: three passes with a tail
C_ALL = C_VECTOR + C_GROUPED + C_GENERIC
TWO_PHASE = (3, 32 * 1030 + 3)               # C, npix: 1031 chunks of the generic form, folded by the ticket kernel
TILES_1PHASE = (1, 2, 31, 32, 33, 255, 256, 257, 1024)
TILES_2PHASE = (1025, 1040, 2049)            # 1025: the last scratch rows own empty tile ranges
C_REDUCE = (1, 31, 32, 33, 100)
ROWS_ROWS = (2, 3, 64)                       # + 1 in eval mode
ROWS_C = (1, 255, 256, 257)
REAL_C = (8, 512, 130, 12)                   # real-valued column sums: vector, grouped, generic scalar, generic float4
EW_SWEEP = (18750, 256)                      # npix, C: 1.2 M float4 items, more than ew_grid's 4096 x 256 lanes


def column_form(C):
    """which column_partials_kernel geometry a channel count takes"""
    return "vector" if C in C_VECTOR else "grouped" if C in C_GROUPED else "generic"


def apply_form(C):
    """which backward-apply kernel: the streaming rows kernel, the generic float4 kernel or the scalar one"""
    return "rows" if C in C_VECTOR + C_GROUPED else "float4" if C % 4 == 0 else "scalar"


def rows_per_pass(C):
    return 1024 // C if C in C_VECTOR else 4


def npix_list(C):
    """1; the odd tail of the two-rows-in-flight loop; exactly one minimal chunk; a second chunk of one row; three chunks and
    a tail"""
    r = rows_per_pass(C)
    return (1, 2 * r + 1, 8 * r, 8 * r + 1, 3 * 8 * r + 5)


def wide_ld(C):
    """operands as channel slices of a wider tensor: (ld, first channel), ld % 4 == 0"""
    return (C + 3) // 4 * 4 + 8, 4


# ---- inputs --------------------------------------------------------------------------------------------------------------

def ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(torch.float32)


def real(npix, C, gen, dtype=torch.float32, offset=0.0):
    """log-normal magnitudes (tests/conv_ref.lognormal) rounded to the storage type"""
    return (lognormal((1, npix, 1, C), gen).reshape(npix, C).double() + offset).to(dtype)


def coeffs(C, gen):
    """mean, invstd, gamma, beta of a layer: fp32 vectors"""
    mean = torch.randn(C, generator=gen, dtype=torch.float64).float()
    invstd = (0.25 + 2.0 * torch.rand(C, generator=gen, dtype=torch.float64)).float()
    gamma = (1.0 + 0.5 * torch.randn(C, generator=gen, dtype=torch.float64)).float()
    beta = (0.3 * torch.randn(C, generator=gen, dtype=torch.float64)).float()
    return mean, invstd, gamma, beta


def fold(mean, invstd, gamma, beta):
    """fp32 (scale, shift) as bn_fold.h folds them"""
    sc = (gamma * invstd) if gamma is not None else invstd.clone()
    sh = (beta if beta is not None else torch.zeros_like(mean)) - mean * sc
    return sc, sh


def negative_var_sums():
    """(s1, s2, count) of a constant column whose fp64 variance s2 / count - (s1 / count)^2 comes out below 0 by one rounding"""
    v = float(np.float32(1000.1))
    for n in range(2, 400):
        s1, s2 = n * v, n * (v * v)
        m = s1 / n
        if s2 / n - m * m < 0.0:
            return s1, s2, float(n)
    raise AssertionError("no count gives a negative variance")


# ---- activation ----------------------------------------------------------------------------------------------------------

def act(v, a):
    v = v.double()
    if a == RELU:
        return v.clamp_min(0.0)
    if a == LEAKY:
        return torch.where(v > 0, v, SLOPE * v)
    if a == SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    return v


def act_grad_out(z, a):
    """the derivative through the activation's OUTPUT (z > 0 also decides where z was stored as a mask bit)"""
    z = z.double()
    if a == RELU:
        return (z > 0).double()
    if a == LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))
    if a == SIGMOID:
        return z * (1.0 - z)
    return torch.ones_like(z)


def _sigmoid_err(v64):
    v32 = v64.float()
    z32 = 1.0 / (1.0 + torch.exp(-v32))
    z64 = 1.0 / (1.0 + torch.exp(-v32.double()))
    ok = z64 >= 64.0 * FLOOR      # (the underflowing tail has the absolute term FLOOR instead)
    return float(((z32.double() - z64).abs() / z64)[ok].max()) if bool(ok.any()) else 0.0


_SIGMOID_SAMPLE = []


def sigmoid_rel(v64):
    """twice the worst relative error of torch's fp32 CPU 1 / (1 + exp(-v)) against float64 over the inputs of the case and - a
    case of four elements measures little - over a fixed sample of the tests' input distribution and of [-80, 20]"""
    if not _SIGMOID_SAMPLE:
        g = torch.Generator().manual_seed(20240229)
        _SIGMOID_SAMPLE.append(max(_sigmoid_err(real(4096, 64, g).double()), _sigmoid_err(torch.linspace(-80.0, 20.0, 1 << 18).double())))
    return 2.0 * max(_sigmoid_err(v64), _SIGMOID_SAMPLE[0])


def g_of(dz, a, z=None, pre=None):
    """g = dz act' in float64 and the absolute error of the fp32 g: 0 where the derivative is 1 or 0, u |g| for the product with
    the leaky slope, 3 u |g| for sigmoid's z (1 - z) from z (two roundings and the product), and from the pre-activation the
    error of z as well.  The derivative comes from the output z, or (z None) from `pre` (float64, its sign exact)."""
    dz = dz.double()
    if z is not None or a != SIGMOID:
        g = dz * act_grad_out(z if z is not None else pre, a)
        return g, {NONE: 0.0, RELU: 0.0, LEAKY: U, SIGMOID: 3.0 * U}[a] * g.abs() + (FLOOR * dz.abs() if a == SIGMOID else 0.0)
    zz = act(pre, SIGMOID)
    d = zz * (1.0 - zz)
    dzz = sigmoid_rel(pre) * zz + d * U * pre.abs()      # the error of z: expf, the sum, the division; the fma behind pre
    g = dz * d
    return g, dz.abs() * (dzz + 2.0 * U * d + FLOOR) + U * g.abs()      # |1 - 2z| <= 1 carries dzz into z (1 - z); its two roundings


def _excess(g, ge):
    """what g's error exceeds the one rounding that the column sums' r already counts"""
    return (ge - U * g.abs()).clamp_min(0.0)


# ---- column sums ---------------------------------------------------------------------------------------------------------

def sum_bound(t, r, extra=None):
    """(n - 1 + r) u sum|t| per channel (+ the summed excess errors of the terms)"""
    n = t.shape[0]
    b = (n - 1 + r) * U * t.abs().sum(0)
    return b if extra is None else b + extra.sum(0)


def tensor_stats(x):
    """-> sums [C, 2] = (sum x, sum x^2) and their bounds [C, 2]"""
    x = x.double()
    x0 = x[0]
    t = x - x0
    n = float(x.shape[0])
    s1, s2 = t.sum(0), (t * t).sum(0)
    b1, b2 = sum_bound(t, 1), sum_bound(t * t, 2)
    sums = torch.stack([s1 + n * x0, s2 + 2.0 * x0 * s1 + n * x0 * x0], 1)
    return sums, torch.stack([b1, b2 + 2.0 * x0.abs() * b1], 1)


def xhat(y, mean, invstd):
    return (y.double() - mean.double()) * invstd.double()


def backward_sums(dz, y, mean, invstd, a, z=None, pre=None):
    """-> sums2 [C, 2] = (sum g, sum g xhat), bounds [C, 2], and (g, g_err, xh) for the apply pass"""
    g, ge = g_of(dz, a, z, pre)
    xh = xhat(y, mean, invstd)
    t = g * xh
    sums = torch.stack([g.sum(0), t.sum(0)], 1)
    bound = torch.stack([sum_bound(g, 1, _excess(g, ge)), sum_bound(t, 3, _excess(g, ge) * xh.abs())], 1)
    return sums, bound, (g, ge, xh)


def f32_of(v64, bound):
    """the fp32 copy of a float64 sum (dgamma, dbeta): one more rounding"""
    return bound + U * v64.abs()


# ---- coefficients --------------------------------------------------------------------------------------------------------

def finalize(sums, count, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """bn_fold.h in numpy float64, same operation order.  sums [C, 2] float64; gamma / beta / running_* fp32 arrays or None.
    -> dict name -> (value, bound) for mean, invstd, scale, shift (and running_mean, running_var)"""
    s = np.asarray(sums, dtype=np.float64)
    C = s.shape[0]
    count = float(count)
    g = np.ones(C) if gamma is None else np.asarray(gamma, dtype=np.float32).astype(np.float64)
    b = np.zeros(C) if beta is None else np.asarray(beta, dtype=np.float32).astype(np.float64)
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    m = s[:, 0] / count
    mm = m * m
    var = s[:, 1] / count - mm
    var = np.where(var < 0.0, 0.0, var)
    inv = 1.0 / np.sqrt(var + eps)
    sc = g * inv
    msc = m * sc
    sf = b - msc
    dvar = 4.0 * D53 * np.abs(s[:, 1] / count)
    dis = inv * dvar / (2.0 * (var + eps))
    out = {"mean": (m, U * np.abs(m)), "invstd": (inv, U * inv + dis),
           "scale": (sc, 2.0 * U * np.abs(sc) + np.abs(g) * dis),
           "shift": (sf, 5.0 * U * np.abs(msc) + U * np.abs(b) + np.abs(g * m) * dis)}
    if running_mean is not None:
        rm = np.asarray(running_mean, dtype=np.float32).astype(np.float64)
        rv = np.asarray(running_var, dtype=np.float32).astype(np.float64)
        unb = var * count / (count - 1.0) if count > 1.0 else var
        keep = 1.0 - mom
        dunb = dvar * (count / (count - 1.0) if count > 1.0 else 1.0)
        out["running_mean"] = (keep * rm + mom * m, 3.0 * U * (np.abs(keep * rm) + np.abs(mom * m)))
        out["running_var"] = (keep * rv + mom * unb, 3.0 * U * (np.abs(keep * rv) + np.abs(mom * unb)) + mom * dunb)
    return {k: (torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(e))) for k, (v, e) in out.items()}


def eval_coeffs(gamma, beta, running_mean, running_var, eps):
    C = running_mean.shape[0]
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    inv = 1.0 / torch.sqrt(running_var.double() + float(np.float32(eps)))
    sc = g * inv
    msc = running_mean.double() * sc
    return {"scale": (sc, 4.0 * U * sc.abs()), "shift": (b - msc, 6.0 * U * msc.abs() + U * b.abs())}


# ---- apply passes --------------------------------------------------------------------------------------------------------

def forward(y, scale, shift, a, res=None, bf16=False, dsc=None, dsh=None):
    """-> z64, bound, pre64 (the pre-activation, residual included).  dsc / dsh: error bounds of the coefficients the kernel
    used where they are not the inputs given here (xv2_bn_rows_forward)"""
    y = y.double()
    fma = y * scale.double() + shift.double()
    dpre = U * fma.abs()
    if dsc is not None:
        dpre = dpre + y.abs() * dsc + dsh
    pre = fma
    if res is not None:
        pre = fma + res.double()
        dpre = dpre + U * (fma.abs() + res.double().abs())
    z = act(pre, a)
    if a == SIGMOID:
        bound = sigmoid_rel(pre) * z + z * (1.0 - z) * dpre + FLOOR
    elif a == LEAKY:
        bound = dpre + U * z.abs()
    else:
        bound = dpre
    return z, (bound + B16 * z.abs() if bf16 else bound), pre


def amax_bits(t):
    """the bit pattern of max |t| as fp32: what the 64 F16X2 slots must hold as their maximum"""
    return int(t.detach().float().abs().max().cpu().view(torch.int32).item())


def mask_bytes(z):
    """[npix, C / 4] uint8: bit k of byte j = (z[4 j + k] > 0)"""
    npix, C = z.shape
    bits = (z.reshape(npix, C // 4, 4) > 0).to(torch.int32)
    return (bits * torch.tensor([1, 2, 4, 8], dtype=torch.int32)).sum(-1).to(torch.uint8)


def backward_apply(parts, sums2, count, invstd, gamma, train=1, bf16=False, dsums=None):
    """parts = (g, g_err, xh) of backward_sums(); sums2 [C, 2] float64 as handed to the kernel.  -> dy64, its bound, dres64 = g,
    its bound.  dsums [C, 2]: error bounds of the sums where the kernel formed them itself (xv2_bn_rows_backward)"""
    g, ge, xh = parts
    gi = invstd.double() if gamma is None else gamma.double() * invstd.double()
    if train:
        sg, sgx = sums2[:, 0].double() / count, sums2[:, 1].double() / count
        t = xh * sgx
        dy = gi * (g - sg - t)
        b = U * gi.abs() * (4.0 * g.abs() + 7.0 * sg.abs() + 9.0 * t.abs()) + gi.abs() * ge
        if dsums is not None:
            b = b + gi.abs() * (dsums[:, 0] + xh.abs() * dsums[:, 1]) / count
    else:
        dy = gi * g
        b = 2.0 * U * dy.abs() + gi.abs() * ge
    bres = torch.maximum(U * g.abs(), ge)
    if bf16:
        b, bres = b + B16 * dy.abs(), bres + B16 * g.abs()
    return dy, b, g, bres


# ---- BatchNorm over a handful of rows (xv2_bn_rows_*) --------------------------------------------------------------------

def rows_forward(y, rows, parts, gamma, beta, eps, momentum, running_mean, running_var, train, a):
    """y [parts * rows, C] fp32.  -> dict of (value, bound): mean / invstd / scale / shift [parts, C], z, and the running
    statistics after all parts (train)"""
    C = y.shape[1]
    yd = y.double().reshape(parts, rows, C)
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    eps, mom = float(np.float32(eps)), float(np.float32(momentum))
    keep = 1.0 - mom
    out = {k: [] for k in ("mean", "invstd", "scale", "shift", "z")}
    rm = None if running_mean is None else running_mean.double()
    rv = None if running_var is None else running_var.double()
    brm = torch.zeros(C, dtype=torch.float64)
    brv = torch.zeros(C, dtype=torch.float64)
    for s in range(parts):
        if train:
            m = yd[s].mean(0)
            var = ((yd[s] - m) ** 2).mean(0)
            slop = (rows + 2) * 2.0 ** -52
        else:
            m, var, slop = rm, rv, 0.0
        inv = 1.0 / torch.sqrt(var + eps)
        dm = U * m.abs() + slop * yd[s].abs().mean(0)
        dis = U * inv + inv * slop * (1.0 + m.abs() * inv)
        sc = g * inv
        msc = m * sc
        dsc = 2.0 * U * sc.abs() + g.abs() * (dis - U * inv)
        dsh = 5.0 * U * msc.abs() + U * b.abs() + (g * m).abs() * (dis - U * inv) + sc.abs() * (dm - U * m.abs())
        z, bz, _ = forward(yd[s], sc, b - msc, a, dsc=dsc, dsh=dsh)
        for k, v in (("mean", (m, dm)), ("invstd", (inv, dis)), ("scale", (sc, dsc)), ("shift", (b - msc, dsh)), ("z", (z, bz))):
            out[k].append(v)
        if train and rm is not None:
            unb = var * rows / (rows - 1.0) if rows > 1 else var
            brm = brm + 3.0 * U * ((keep * rm).abs() + (mom * m).abs()) + mom * (dm - U * m.abs())
            brv = brv + 3.0 * U * ((keep * rv).abs() + (mom * unb).abs()) + mom * unb * 2.0 * slop * (1.0 + m.abs() * inv)
            rm, rv = keep * rm + mom * m, keep * rv + mom * unb
    res = {k: (torch.stack([v[0] for v in vs]), torch.stack([v[1] for v in vs])) for k, vs in out.items()}
    res["z"] = (res["z"][0].reshape(parts * rows, C), res["z"][1].reshape(parts * rows, C))
    if train and rm is not None:
        res["running_mean"], res["running_var"] = (rm, brm), (rv, brv)
    return res


def rows_backward(dz, z, y, mean, invstd, gamma, rows, parts, a, train):
    """mean / invstd [parts, C] fp32 as handed to the kernel.  -> dict of (value, bound): dy, dgamma, dbeta"""
    C = y.shape[1]
    dys, bys = [], []
    tg = tb = btg = btb = atg = atb = torch.zeros(C, dtype=torch.float64)
    for s in range(parts):
        sl = slice(s * rows, (s + 1) * rows)
        sums, bs, p = backward_sums(dz[sl], y[sl], mean[s], invstd[s], a, z=z[sl])
        # (sg * invn and xh * sgx * invn: the reciprocal of rows and one more product each - 6 |sg| and 8 |xhat sgx| where
        #  backward_apply() counts 7 and 9)
        dy, by, _, _ = backward_apply(p, sums, float(rows), invstd[s], gamma, train, dsums=bs)
        dys.append(dy)
        bys.append(by)
        tb, tg = tb + sums[:, 0], tg + sums[:, 1]
        atb, atg = atb + sums[:, 0].abs(), atg + sums[:, 1].abs()
        btb, btg = btb + bs[:, 0], btg + bs[:, 1]
    add = (parts - 1) * U
    return {"dy": (torch.cat(dys), torch.cat(bys)), "dgamma": (tg, btg + add * atg), "dbeta": (tb, btb + add * atb)}
