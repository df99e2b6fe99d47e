"""Float64 restatement of the scene-inference kernels (csrc/scene.hip: scene_windows_kernel, scene_blend_kernel,
scene_finalize_kernel), the per-element error bound the blended maps are held to, an fp32 transcription of the kernels' order
of operations for the CPU test of that bound, and the case tables the CPU and the GPU test share.  Written from the geometry
in the docstring of xview2_amd/scene.py, with its own loops instead of that module's helpers.

  origins along an axis of length L, window side n: [0] when L <= n, else range(0, L - n, n - overlap) + [L - n]
  windows of a scene: the product grid, y outer, x inner - the summation order
  reflect(i, L): period 2 (L - 1), the edge not repeated, reflect(i, 1) = 0
  ramp r(i) = min(i + 1, n - i, overlap + 1); window pixel (iy, ix) weighs w = r(iy) r(ix), an integer below 2^21
  out[c, y, x] = sum_k w_k p_k[c] / sum_k w_k over the windows k that hold (y, x), p the decode of window k's logits there

Bound.  u = 2^-24 is one fp32 rounding, fl(x) = x (1 + d), |d| <= u; the style is tests/loss_ref.py's: a running error, every
rounding charged u times the magnitude of what it rounds, nothing relative to the result.
  decode, absolute error e_p of one probability (constants of tests/loss_ref.py: A_EXP = 4, expf within 2 ulp)
    sigmoid   1 / (1 + expf(-x)): expf moves the sum by A_EXP u e / (1 + e) = A_EXP u (1 - p) relative, the sum and the
              division round once each: e_p = p (A_EXP (1 - p) + 2) u
    softmax   loss_ref._softmax_parts: e_p = p R_c u, R_c = |d_c| + A_EXP + R_s + 2 (the maximum is subtracted first)
    relu      exact
    TINY = 2^-126 is added where a result in the denormal range can be reached (a sigmoid of -80 and below)
  blend       a pixel covered by m <= 9 windows runs m fused multiply-adds acc = fl(w p + acc); the weights are exact, so
              each rounds once, a partial sum of magnitude at most S = sum_k w_k |p_k|: m u S.  The bound charges one more,
              (m + 1) u S, which also covers a first product that the compiler does not fuse into its addition; the decode
              errors arrive weighted, E = sum_k w_k e_p,k
  finalize    N = wy[y] wx[x] is an exact fp32 integer (below 2^24); the division rounds once: u S / N
  out         ((m + 2) u S + E) / N + TINY
Elements whose bound is 0 must equal the reference exactly (a relu map of zeros).  check() is tests/pool_ref.check.
The compiler may or may not fuse; no bound relies on either.  The largest error / bound ratio over the GPU run of
tests/test_scene_gpu.py on an MI355X is 0.80 (softmax, C = 4, the +-80 regime); the bound is not tuned from it.

`wrong=` selects a deliberately wrong variant of the restatement (tests/test_scene_cpu.py shows that each lands outside the
bound on at least one case of the table, i.e. that the GPU test can fail):
  origin_last_not_shifted        the last window of an axis continues the stride instead of moving back to L - n
  ramp_flat                      every weight 1
  reflect_repeats_edge           np.pad's "symmetric" instead of "reflect"
  normaliser_from_first_window   the weight of the first window covering a pixel instead of the sum over all of them
"""
import math

import numpy as np
import torch

from tests.loss_ref import A_EXP, TINY, _softmax_parts
from tests.pool_ref import U, check  # noqa: F401

SIGMOID1, SOFTMAX, SIGMOID, RELU = 0, 1, 2, 3
WRONG = ["origin_last_not_shifted", "ramp_flat", "reflect_repeats_edge", "normaliser_from_first_window"]
KINDS = [(SIGMOID1, 2), (SOFTMAX, 5), (SOFTMAX, 4), (SIGMOID, 3), (RELU, 1)]      # decode, channels of the logits


# ---- geometry ------------------------------------------------------------------------------------------------------------

def origins(L, n, overlap, wrong=None):
    if L <= n:
        return [0]
    step = n - overlap
    out = []
    o = 0
    while o < L - n:
        out.append(o)
        o += step
    out.append(out[-1] + step if wrong == "origin_last_not_shifted" else L - n)
    return out


def windows(H, W, n, overlap, wrong=None):
    """[(y0, x0)] in summation order"""
    return [(y, x) for y in origins(H, n, overlap, wrong) for x in origins(W, n, overlap, wrong)]


def reflect(i, L, wrong=None):
    if wrong == "reflect_repeats_edge":
        m = i % (2 * L)
        return m if m < L else 2 * L - 1 - m
    if L == 1:
        return 0
    p = 2 * (L - 1)
    m = i % p
    return m if m < L else p - m


def ramp(n, overlap, wrong=None):
    if wrong == "ramp_flat":
        return torch.ones(n, dtype=torch.float64)
    return torch.tensor([min(i + 1, n - i, overlap + 1) for i in range(n)], dtype=torch.float64)


# ---- gather --------------------------------------------------------------------------------------------------------------

def gather(pre, post, table, n, wrong=None):
    """pre / post: uint8 numpy [H, W, 3] (post may be None) -> uint8 numpy [K, n, n, 3 | 6]"""
    H, W, _ = pre.shape
    src = pre if post is None else np.concatenate([pre, post], axis=2)
    out = np.empty((len(table), n, n, src.shape[2]), dtype=np.uint8)
    for k, (y0, x0) in enumerate(table):
        rows = [reflect(y0 + i, H, wrong) for i in range(n)]
        cols = [reflect(x0 + i, W, wrong) for i in range(n)]
        out[k] = src[rows][:, cols]
    return out


# ---- blend + finalize ----------------------------------------------------------------------------------------------------

def decode(x, kind):
    """x float64 [K, C, n, n] -> (p [K, Cout, n, n], absolute error bound of the fp32 decode)"""
    if kind == SIGMOID1:
        x = x[:, 1:2]
    if kind in (SIGMOID1, SIGMOID):
        p = torch.sigmoid(x)
        return p, p * (A_EXP * (1.0 - p) + 2.0) * U + TINY
    if kind == SOFTMAX:
        _, p, Rp, _, _ = _softmax_parts(x)
        return p, p * Rp * U + TINY
    p = torch.relu(x)
    return p, torch.zeros_like(p)


def blend(logits, kind, table, n, overlap, H, W, wrong=None):
    """logits [K, C, n, n] of the windows at `table` -> dict(out float64 [Cout, H, W], bound, count [H, W], planted [H, W]:
    pixels that a non-finite logit reaches)"""
    x = logits.double()
    p, e = decode(x, kind)
    bad = ~torch.isfinite(x).all(dim=1)
    r = ramp(n, overlap, wrong)
    wgt = r.view(n, 1) * r.view(1, n)
    cout = p.shape[1]
    acc = torch.zeros((cout, H, W), dtype=torch.float64)
    S, E = torch.zeros_like(acc), torch.zeros_like(acc)
    N, cnt = torch.zeros((H, W), dtype=torch.float64), torch.zeros((H, W), dtype=torch.float64)
    planted = torch.zeros((H, W), dtype=torch.bool)
    for k, (y0, x0) in enumerate(table):
        hh, ww = min(n, H - y0), min(n, W - x0)      # positions at or past H / W are padding: dropped
        sl = (slice(y0, y0 + hh), slice(x0, x0 + ww))
        wk = wgt[:hh, :ww]
        acc[(slice(None),) + sl] += wk * p[k, :, :hh, :ww]
        S[(slice(None),) + sl] += wk * p[k, :, :hh, :ww].abs()
        E[(slice(None),) + sl] += wk * e[k, :, :hh, :ww]
        if wrong == "normaliser_from_first_window":
            N[sl] = torch.where(cnt[sl] == 0, wk, N[sl])
        else:
            N[sl] += wk
        cnt[sl] += 1
        planted[sl] |= bad[k, :hh, :ww]
    assert float(cnt.min()) >= 1, "every scene pixel is covered"
    return {"out": acc / N, "bound": ((cnt + 2.0) * U * S + E) / N + TINY, "count": cnt, "planted": planted, "norm": N}


def f32_blend(logits, kind, table, n, overlap, H, W):
    """the kernels' arithmetic in fp32 on the CPU: decode, one fused multiply-add per covering window in table order (the
    product of an integer weight below 2^21 and an fp32 is exact in float64, and so is the sum before its one rounding,
    up to a double rounding far below the bound), then the division"""
    x = logits.float()
    if kind == SIGMOID1:
        p = 1.0 / (1.0 + torch.exp(-x[:, 1:2]))
    elif kind == SIGMOID:
        p = 1.0 / (1.0 + torch.exp(-x))
    elif kind == SOFTMAX:
        m = x.amax(1, keepdim=True)
        ex = torch.exp(x - m)
        s = ex[:, 0:1]
        for c in range(1, x.shape[1]):
            s = s + ex[:, c:c + 1]
        p = ex * (torch.ones_like(s) / s)
    else:
        p = torch.where(x < 0, torch.zeros_like(x), x)
    r = ramp(n, overlap)
    wgt = r.view(n, 1) * r.view(1, n)
    acc = torch.zeros((p.shape[1], H, W), dtype=torch.float32)
    N = torch.zeros((H, W), dtype=torch.float64)
    for k, (y0, x0) in enumerate(table):
        hh, ww = min(n, H - y0), min(n, W - x0)
        sl = (slice(None), slice(y0, y0 + hh), slice(x0, x0 + ww))
        acc[sl] = (wgt[:hh, :ww] * p[k, :, :hh, :ww].double() + acc[sl].double()).float()
        N[sl[1:]] += wgt[:hh, :ww]
    return acc / N.float()


# ---- case tables ---------------------------------------------------------------------------------------------------------

# axis lengths at window 32, overlap 16: 1 single source index, 5 many-fold reflection, 31, 32 exact fit, 33 origins 0 1,
# 48 origins 0 16, 49 origins 0 16 17 (triple cover), 81; every class on both axes, (5, 49) and (49, 5) among them
SCENES = [dict(H=H, W=W, n=32, overlap=16) for H, W in
          [(1, 81), (5, 49), (31, 48), (32, 33), (33, 32), (48, 31), (49, 5), (81, 1), (49, 81)]]
SCENES += [dict(H=64, W=65, n=32, overlap=0), dict(H=65, W=64, n=32, overlap=0),      # no overlap: exact tiling, and + 1
           dict(H=94, W=94, n=32, overlap=1),                                          # odd stride 31
           dict(H=70, W=130, n=64, overlap=32)]                                        # window 64 at the largest overlap
REGIMES = ["position", "pm80", "nonfinite"]


def name(case):
    return "%dx%d-n%d-o%d" % (case["H"], case["W"], case["n"], case["overlap"])


def _gen(case, salt):
    return torch.Generator().manual_seed(1000003 * salt + 8191 * case["H"] + 131 * case["W"] + 7 * case["n"] + case["overlap"])


def make_scene(case, post=True):
    """uint8 numpy [H, W, 3] pre (and post)"""
    g = _gen(case, 1)
    pre = torch.randint(0, 256, (case["H"], case["W"], 3), generator=g, dtype=torch.uint8).numpy()
    if not post:
        return pre, None
    return pre, torch.randint(0, 256, (case["H"], case["W"], 3), generator=g, dtype=torch.uint8).numpy()


def make_logits(case, K, C, regime):
    """fp32 [K, C, n, n].  position: a function of the window index and the window-local position (a wrong origin or ramp
    shows); pm80: |logit| up to 80 with tied channels; nonfinite: random logits with one NaN and one +Inf planted"""
    n = case["n"]
    g = _gen(case, 2 + REGIMES.index(regime) + 10 * C)
    if regime == "position":
        k = torch.arange(K, dtype=torch.float64).view(K, 1, 1, 1)
        c = torch.arange(C, dtype=torch.float64).view(1, C, 1, 1)
        iy = torch.arange(n, dtype=torch.float64).view(1, 1, n, 1)
        ix = torch.arange(n, dtype=torch.float64).view(1, 1, 1, n)
        return (3.0 * torch.sin(0.9 * k + 1.7 * c + 0.23 * iy + 0.31 * ix) + 0.5 * torch.cos(1.3 * k - 0.4 * c)).float()
    x = torch.randn((K, C, n, n), generator=g, dtype=torch.float64) * 2.0
    if regime == "pm80":
        pick = torch.randint(0, 4, x.shape, generator=g)
        x = torch.where(pick == 0, torch.full_like(x, 80.0), x)
        x = torch.where(pick == 1, torch.full_like(x, -80.0), x)
        x = torch.where(pick == 2, x * 40.0, x).clamp(-80.0, 80.0)
        x[:, :, ::3, 1::2] = x[:, :1, ::3, 1::2]      # tied channels
        return x.float()
    x = x.float()
    x[K - 1, C - 1, n // 2, n // 3] = math.nan
    x[0, C - 1, 0, 0] = math.inf
    return x
