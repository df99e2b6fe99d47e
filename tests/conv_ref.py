"""Float64 restatement of the convolutions the HIP kernels compute (NHWC activations, OIHW weights, the layouts of
include/xv2.h) and the per-element error bounds the kernels are held to.

Every operation here is a bilinear map f(A, B) of two operands (forward: image and weights; backward-data: output
gradient and weights; backward-weight: image and output gradient).  Next to the float64 result y64 = f(A, B) the error
scales come from the same map, also in float64:

    a_i = f(|A|, |B|)_i              the sum of |products| behind element i
    s_i = sqrt(f(A^2, B^2)_i)        their root sum of squares

and K = the number of products per element (channels x taps; pixels for a weight gradient).

Bounds, u = 2^-24 (one fp32 rounding):

  - accumulation, every mode: the K products are summed in fp32; each addition rounds by at most u times the partial sum,
    and |partial sum| <= a_i.  The roundings of a long sum behave as a random walk, so the per-element bound is
    EL * u * (1 + sqrt(K)) * a_i, EL a tail factor calibrated on the GPU.
  - F32 (exact fp32 MFMA) and F32X3 (three bf16 planes): every product is exact to u (the dropped cross
    terms of F32X3 are below 2^-24 |a||b|), which the "1 +" above covers.
  - F16X2 (two scaled fp16 planes, include/xv2.h): an operand keeps 22 significant bits when it lies within 2^18 of its
    tensor's maximum, and an absolute error of 2^-39 of that maximum below; the dropped m*m term is below 2^-22 |a||b|.  Per
    product that is 3 * 2^-22 |a||b| + 2^-38 (max|A| |b| + |a| max|B|), so the bound gains 12 u a_i and
    2^-38 K max|A| max|B|.
  - bf16 storage: the tests round the operands to bf16 themselves, so products are exact and the only extra term is the
    rounding of the fp32 result to bf16 on store: 2^-8 |y64_i| (8 significant bits, round to nearest even: half an ulp is
    at most 2^-8 of the value).

Two gates per result tensor (check()):

  - per element: |y - y64|_i <= bound_i.  Elements with a_i = 0 (no product reaches them) must be exactly y64_i.  This catches
    a fault confined to a tile, a border or a low-magnitude region.
  - over the tensor: rms_i((y - y64)_i / s_i) / (u sqrt(K)) <= TAU_RMS[mode] (bf16 storage: (y - bf16(y64)) / s over 2^-8
    instead: a correctly rounded result differs from bf16(y64) only where the fp32 sum lands across a rounding boundary).
    A kernel that lost precision everywhere (one plane short, 16 significant bits) passes the first gate and fails this one.

EL and TAU_RMS were calibrated on an MI355X from passing runs of tests/test_conv_variants_gpu.py; WORST records the largest
ratio (error / bound, rms statistic / TAU_RMS) measured there, per mode.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MODES = ("f32", "f32x3", "f16x2", "bf16")

# per-element tail factor and rms limit per math mode (see the module docstring); "bf16" covers the bf16-storage mode and
# the XV2_MATH_BF16 mode alike (operands rounded to bf16 by the test: exact products, fp32 sums)
EL = {"f32": 3.0, "f32x3": 3.0, "f16x2": 2.0, "bf16": 3.0}
TAU_RMS = {"f32": 0.75, "f32x3": 0.6, "f16x2": 0.5, "bf16": 0.3}
# largest measured ratio to the limits above over every case of the GPU matrix: (per element, rms)
WORST = {"f32": (0.35, 0.50), "f32x3": (0.31, 0.48), "f16x2": (0.14, 0.54), "bf16": (0.996, 0.44)}


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---- the operations, float64, NHWC --------------------------------------------------------------------------------

def conv_fwd(x, w, stride=1, pad=0, dil=1, groups=1, bias=None):
    """y[N,OH,OW,Cout] = conv2d(x[N,H,W,Cin], w[Cout,Cin/groups,KH,KW]) (+ bias)"""
    y = F.conv2d(nchw(x.double()), w.double(), None if bias is None else bias.double(), stride, pad, dil, groups)
    return nhwc(y)


def conv_bwd_data(dy, w, in_hw, stride=1, pad=0, dil=1, groups=1):
    """dx[N,H,W,Cin] of conv2d for the output gradient dy[N,OH,OW,Cout]"""
    shape = (dy.shape[0], w.shape[1] * groups, in_hw[0], in_hw[1])
    dx = torch.nn.grad.conv2d_input(shape, w.double(), nchw(dy.double()), stride, pad, dil, groups)
    return nhwc(dx)


def conv_bwd_weight(x, dy, w_shape, stride=1, pad=0, dil=1, groups=1):
    """dw[Cout,Cin/groups,KH,KW] of conv2d"""
    return torch.nn.grad.conv2d_weight(nchw(x.double()), tuple(w_shape), nchw(dy.double()), stride, pad, dil, groups)


def convT_fwd(x, w):
    """nn.ConvTranspose2d(k=2, s=2, bias=False): x[N,H,W,Cin_T], w[Cin_T,Cout_T,2,2] -> y[N,2H,2W,Cout_T]"""
    return nhwc(F.conv_transpose2d(nchw(x.double()), w.double(), stride=2))


def convT_bwd_data(dy, w):
    """dx[N,H,W,Cin_T] = conv2d(dy[N,2H,2W,Cout_T], w viewed as OIHW, stride 2)"""
    return nhwc(F.conv2d(nchw(dy.double()), w.double(), stride=2))


def convT_bwd_weight(x, dy):
    """dw[Cin_T,Cout_T,2,2]: the weight gradient of the equivalent convolution (input dy, output gradient x)"""
    Cin_T, Cout_T = x.shape[3], dy.shape[3]
    return conv_bwd_weight(dy, x, (Cin_T, Cout_T, 2, 2), stride=2)


# ---- error scales and gates -----------------------------------------------------------------------------------------

def scales(f, A, B):
    """(a, s) of the bilinear map f at (A, B), float64"""
    A, B = A.double(), B.double()
    a = f(A.abs(), B.abs())
    s = f(A * A, B * B).clamp_min(0).sqrt()
    return a, s


def bound(mode, a, K, y64=None, amax=None):
    """per-element bound of one result tensor (module docstring); amax = (max|A|, max|B|) for f16x2, y64 for bf16 stores"""
    b = EL[mode] * U * (1.0 + math.sqrt(K)) * a
    if mode == "f16x2":
        b = b + EL[mode] * (12.0 * U * a + 2.0 ** -38 * K * float(amax[0]) * float(amax[1]))
    if y64 is not None:       # the result is stored as bf16
        b = b + 2.0 ** -8 * y64.abs()
    return b


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def check(y, y64, a, s, K, mode, bf16_out=False, amax=None):
    """both gates for one result: -> dict(el = max error / bound, rms = rms statistic / TAU_RMS, ok = both <= 1, where = flat
    index of the worst element).  `y` is the kernel's result (any float dtype), y64 / a / s from this module."""
    y = y.double()
    y64 = y64.double()
    e = (y - y64).abs()
    b = bound(mode, a, K, y64 if bf16_out else None, amax)
    exact = b == 0
    ratio = torch.where(exact, torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, math.inf)), e / b.clamp_min(1e-300))
    ratio = ratio.nan_to_num(math.inf)
    el = float(ratio.max()) if ratio.numel() else 0.0
    lit = s > 0
    if bf16_out:     # against the rounding of the exact result: an fp32 sum next to a rounding boundary may land one ulp off
        e2 = (y - bf16_round(y64))[lit] / s[lit]
        stat = float(e2.pow(2).mean().sqrt()) / 2.0 ** -8 if e2.numel() else 0.0
    else:
        e2 = (y - y64)[lit] / s[lit]
        stat = float(e2.pow(2).mean().sqrt()) / (U * math.sqrt(K)) if e2.numel() else 0.0
    rms = stat / TAU_RMS[mode] if math.isfinite(stat) else math.inf
    return {"el": el, "rms": rms, "ok": el <= 1.0 and rms <= 1.0, "where": int(torch.argmax(ratio.flatten()).item())}


def lognormal(shape, gen, sigma_pix=1.0, sigma_ch=1.0, dtype=torch.float32):
    """NHWC values with log-normal per-pixel and per-channel magnitudes (as the gradients of a trained network have)"""
    N, H, W, C = shape
    v = torch.randn(shape, generator=gen, dtype=torch.float64)
    v = v * torch.exp(sigma_pix * torch.randn((N, H, W, 1), generator=gen, dtype=torch.float64))
    v = v * torch.exp(sigma_ch * torch.randn((1, 1, 1, C), generator=gen, dtype=torch.float64))
    return v.to(dtype)
