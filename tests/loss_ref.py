"""Float64 restatement of the loss kernels (csrc/loss.hip: loss_fwd_kernel, loss_finish_kernel, loss_bwd_kernel,
loss_aux_fwd_kernel, loss_aux_bwd_kernel; csrc/loss_px.h: softmax_px, label_at), the per-element error bounds they are
held to, an fp32 transcription of the kernels' order of operations for the CPU test of those bounds, and the case tables
that the CPU and the GPU test share.

The composed loss, on NCHW logits and uint8 labels [N, H ls, W ls] read at [:, ::ls, ::ls]; under `post` the pixels with
label 0 are masked out and the class is label - 1:
  per class c: I_c = sum p_c [y == c], G_c = sum [y == c], P_c = sum p_c (p = softmax over channels)
  F = sum -(1 - p_t)^2 log p_t, E = sum -log p_t, n = number of counted pixels
  dice  = mean over c0 <= c < C of 1 - (2 I_c + 1e-5) / (G_c + P_c + 1e-5), c0 = 1 at C == 2 (no background), else 0
  focal = F / n, ce = E / n;  mse (C = 1) = sum (relu(x) - y)^2 / n;  coral (C = 3) = -sum_k [k < y] logsig(x_k) +
  [k >= y] (logsig(x_k) - x_k), over n.  acc = [I_0..3, G_0..3, P_0..3, F, E, n]; mse and coral use acc[12] and acc[14].

Bounds.  u = 2^-24 is one fp32 rounding, fl(x) = x (1 + d), |d| <= u.  Every bound is a running error: the kernel's
expression walked operation by operation, each rounding charged u times the MAGNITUDE of what it rounds and every incoming
error carried through by the derivative's magnitude.  Nothing is relative to the result, so cancellation (m + log s in the
confident regime, 1 - p_t, a common offset of 1e4 on all channels) is covered by the same formulas: the bound of log p_t
holds u (|l_t| + 2 |m| + 2 log s) whatever log p_t itself is.  The constants, in units of u unless said otherwise:

  A_EXP, A_LOG, A_LOG1P = 4   expf, logf, log1pf: 2 ulp, and one ulp is at most 2 u of the result
  softmax_px, channel c, d_c = l_c - m (m itself is exact: a maximum)
    e_c = expf(d_c)             |d_c| + A_EXP          the subtraction's rounding u |d_c| moves exp by that relative amount
    s = sum e_c                 R_s = w + A_EXP + C - 1,  w = sum_c e_c |d_c| / s   (the e_c errors weighted, C - 1 additions)
    p_c = e_c * (1 / s)         R_c = |d_c| + A_EXP + R_s + 2                      (the division and the product)
    log s                       absolute u (A_LOG log s + R_s)
    lse = m + log s             + u (|m| + log s)
  forward, per pixel
    lt = l_t - lse              e_lt = the above + u (|l_t| + |m| + log s)
    pt = expf(lt)               e_pt = pt (e_lt + A_EXP u)
    q = 1 - pt                  e_q = e_pt + u q
    f = -(q q) lt               2 q |lt| e_q + q^2 e_lt + 2 u q^2 |lt|             (two products)
    I_c, P_c terms              p_c R_c u;  E term  e_lt;  G_c, n  exact (counts below 2^24)
  per-thread fp32 accumulation: a thread adds the terms of k = ceil(total / threads) pixels, threads = 256 min(ceil(total / 256),
    1024); the first addition onto 0 is exact, each later one rounds a partial sum that the thread's sum of |terms| bounds:
    (k - 1) u sum |terms| over all threads (coral adds three levels per pixel: 3 k - 1).  k = 1 for every shape below 2^18
    pixels.  The fp64 folds across lanes, waves and blocks and the fp64 loss arithmetic add 2^-53 per operation: nothing.
  loss: first-order propagation of the acc bounds through the composition, and u |L| for the store as fp32.
  backward (it recomputes the softmax and takes the acc of the forward launch, whose bounds carry over)
    dI_c, dP_c (fp64, stored fp32)   |dI| (u + bP / den), |dP| (u + 2 bI / (2 I + eps) + 2 bP / den)
    dp_c = dI_c [y == c] + dP_c      + u (|dI_c| [y == c] + |dP_c|)
    dot = sum_c dp_c p_c             carried errors + (2 C - 1) u sum |dp_c| p_c      (C products, C - 1 additions)
    lt = logf(pt), pt lt             e_pt (|lt| + 1) + A_LOG u |pt lt|               (d(p log p) = (log p + 1) dp)
    focal: (2 q pt lt - q q) / n     2 |pt lt| e_q + 2 q e(pt lt) + 2 u |2 q pt lt| + 2 q e_q + u q^2, the subtraction's
                                     u (|2 q pt lt| + q^2), and 2 u of the sum for 1 / n and the product with it
    ce: -1 / n                       u / n, and u (|focal part| + 1 / n) where it is added to focal
    g_c = p_c (dp_c - dot) + dlt ([y == c] - p_c)   the subtraction, the product, [y == c] - p_c (absolute p_c R_c u + u |.|:
                                     1 - p_t is accurate to a few u of p_t, not of itself), the product, the sum
    dlogits = (gscale weight) g      2 u more; the whole bound scales by |gscale weight|, so gscale = 0 demands exact zeros
  mse     forward 3 u d^2 (d = relu(x) - y: the subtraction enters twice, then the square); backward K = 5: gscale weight,
          (float)(1 / n), their product, x - y, the last product (the factor 2 is exact)
  coral   forward per level: expf(-|x|), log1pf of it (A_LOG1P u of the result + A_EXP u ex / (1 + ex)), min(x, 0) - that,
          and - x where the level is not reached; backward sg = 1 / (1 + expf(-x)): relative A_EXP (1 - sg) + 2, then
          sg - level (u) and four roundings of the scale (gscale weight, 1 / n, their product, the last product)
  TINY = 2^-126 is added to every bound that a result in the denormal range can reach (p_t underflows at +-80).

The compiler may fuse a product into the following addition; that removes a rounding and no bound relies on it.
check() is tests/pool_ref.check: worst error / bound ratio and its flat index; where a bound is 0 the result must be equal.
WORST holds the largest ratio per operation over the GPU run of tests/test_loss_gpu.py; no bound is tuned from it.
"""
import torch
import torch.nn.functional as F

from tests.pool_ref import U, check  # noqa: F401

DICE, FOCAL, CE, MSE, CORAL = 1, 2, 4, 8, 16
EPS = 1e-5
TINY = 2.0 ** -126
A_EXP = 4.0      # expf: 2 ulp, each at most 2 u of the result
A_LOG = 4.0      # logf: the same
A_LOG1P = 4.0    # log1pf: the same
K_MSE_FWD = 3.0  # d = relu(x) - y rounds once and enters d * d twice; the product rounds once
K_MSE_BWD = 5.0  # gscale * weight, (float)(1 / n), their product, x - y, the last product
K_SCALE = 2.0    # gscale * weight and the product with g
K_CORAL_SCALE = 4.0   # gscale * weight, (float)(1 / n), their product, the product with sg - level
FWD_BLOCKS, BWD_BLOCKS, THREADS = 1024, 4096, 256      # the caps of the grid-stride loops

# largest error / bound ratio per operation over every case of tests/test_loss_gpu.py on an MI355X (profiles/loss_ref_ratios.md)
WORST = {
    "c2_acc": 0.1633, "c2_loss": 0.3473, "c2_grad": 0.4504, "c4_acc": 0.2262, "c4_loss": 0.2107, "c4_grad": 0.5005,
    "mse_acc": 0.1336, "mse_loss": 0.1840, "mse_grad": 0.5344, "coral_acc": 0.1127, "coral_loss": 0.0977, "coral_grad": 0.7352,
    "composed_loss": 0.0947, "composed_grad": 0.3573, "ds_loss": 0.0442, "ds_grad": 0.2921,
}      # sums over many pixels sit far below a worst-case bound; the one-pixel and 182-pixel cases set these figures


def sweeps(total, cap):
    """pixels per thread of a grid-stride loop over `total` pixels with at most `cap` blocks of 256"""
    threads = min(-(-total // THREADS), cap) * THREADS
    return -(-total // threads)


def aux(terms):
    return terms in (MSE, CORAL)


def channels(terms, C):
    return {MSE: 1, CORAL: 3}.get(terms, C)


# ---- labels: label_at and the building mask ------------------------------------------------------------------------------

def targets(labels, shape, post, ls=1, wrong=None, cap=FWD_BLOCKS):
    """-> (t [N, H, W] long class index, mask [N, H, W] bool counted pixels).  `wrong` selects a deliberately wrong variant
    (tests/test_loss_ref_cpu.py); cap: the block cap of the loop that the dropped-pixel variants refer to."""
    N, _, H, W = shape
    if wrong in ("label_hw_swapped", "label_no_row_stride"):
        n = torch.arange(N).view(N, 1, 1)
        h = torch.arange(H).view(1, H, 1)
        w = torch.arange(W).view(1, 1, W)
        if wrong == "label_hw_swapped":
            idx = (n * W * ls + h * ls) * (H * ls) + w * ls
        else:
            idx = (n * H * ls + h) * (W * ls) + w * ls
        y = labels.reshape(-1).long()[idx % labels.numel()]
    else:
        y = labels[:, ::ls, ::ls].long()
    assert tuple(y.shape) == (N, H, W)
    if post:
        mask = y > 0
        t = y if wrong == "post_no_shift" else y - 1
    else:
        mask = torch.ones_like(y, dtype=torch.bool)
        t = y
    i = torch.arange(N * H * W).view(N, H, W)
    if wrong == "drop_partial_block":
        mask = mask & (i < (N * H * W) // THREADS * THREADS)
    if wrong == "drop_second_sweep":
        mask = mask & (i < cap * THREADS)
    return torch.where(mask, t, torch.zeros_like(t)), mask


def _onehot(t, mask, C):
    return (t.unsqueeze(1) == torch.arange(C).view(1, C, 1, 1)) & mask.unsqueeze(1)


def _pick(x, t):
    """x[n, t, h, w]; a class outside the channels reads channel 0, as the kernels do"""
    C = x.shape[1]
    return x.gather(1, torch.where(t < C, t, torch.zeros_like(t)).unsqueeze(1)).squeeze(1)


def _zero(x):
    return torch.zeros((), dtype=x.dtype)


# ---- forward -------------------------------------------------------------------------------------------------------------

def compose(acc, terms, C, wrong=None):
    """loss_finish_kernel: the scalar loss from the 15 sums (float64)"""
    n = acc[14]
    if aux(terms):
        return acc[12] / n
    L = 0.0
    if terms & DICE:
        c0 = 1 if (C == 2 and wrong != "dice_bg_c2") else 0
        f = 0.0
        for c in range(c0, C):
            f = f + 1.0 - (2.0 * acc[c] + EPS) / (acc[4 + c] + acc[8 + c] + EPS)
        L = L + f / (C if wrong == "dice_div_C" else C - c0)
    if terms & FOCAL:
        L = L + acc[12] / n
    if terms & CE:
        L = L + acc[13] / n
    return L


def forward(logits, labels, terms, post, label_stride=1, wrong=None):
    """-> (acc [15] float64, loss 0-d float64); differentiable in `logits` when that is a float64 leaf"""
    x = logits.double()
    N, C, H, W = x.shape
    t, mask = targets(labels, x.shape, post, label_stride, wrong, FWD_BLOCKS)
    z = _zero(x)
    acc = [z] * 15
    acc[14] = mask.double().sum()
    if wrong == "n_all_post":
        acc[14] = torch.tensor(float(N * H * W), dtype=torch.float64)
    if terms == MSE:
        d = x[:, 0].clamp_min(0.0) - t.double()
        acc[12] = torch.where(mask, d * d, z).sum()
    elif terms == CORAL:
        k = torch.arange(3).view(1, 3, 1, 1)
        reached = (k <= t.unsqueeze(1)) if wrong == "coral_levels" else (k < t.unsqueeze(1))
        lsg = F.logsigmoid(x)
        acc[12] = torch.where(mask.unsqueeze(1), -torch.where(reached, lsg, lsg - x), z).sum()
    else:
        lp = torch.log_softmax(x, 1)
        p = lp.exp()
        oh = _onehot(t, mask, C)
        I, G = torch.where(oh, p, z).sum((0, 2, 3)), oh.double().sum((0, 2, 3))
        P = torch.where(mask.unsqueeze(1), p, z).sum((0, 2, 3))
        for c in range(C):
            acc[c], acc[4 + c], acc[8 + c] = I[c], G[c], P[c]
        lt = _pick(lp, t)
        pt = lt.exp()
        acc[12] = torch.where(mask, -(1.0 - pt) ** 2 * lt, z).sum()
        acc[13] = torch.where(mask, -lt, z).sum()
    acc = torch.stack(acc)
    return acc, compose(acc, terms, C, wrong)


# ---- backward: the closed form in the header of loss_bwd_kernel ----------------------------------------------------------

def dice_coeffs(acc, terms, C, wrong=None):
    """dL/dI_c = -2 / den_c / K and dL/dP_c = (2 I_c + eps) / den_c^2 / K, den = G + P + eps, K classes averaged"""
    dI, dP = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    if terms & DICE and not aux(terms):
        c0 = 1 if (C == 2 and wrong != "dice_bg_c2") else 0
        K = C if wrong == "dice_div_C" else C - c0
        for c in range(c0, C):
            den = acc[4 + c] + acc[8 + c] + EPS
            dI[c] = -2.0 / den / K
            dP[c] = (2.0 * acc[c] + (0.0 if wrong == "dP_no_eps" else EPS)) / (den * den) / K
    return dI, dP


def backward(logits, labels, terms, post, label_stride=1, gscale=1.0, weight=1.0, wrong=None):
    """gscale * weight * dLoss/dlogits in float64, analytically; gscale and weight as the fp32 values the kernel receives"""
    x = logits.detach().double()
    N, C, H, W = x.shape
    acc, _ = forward(x, labels, terms, post, label_stride, wrong)
    t, mask = targets(labels, x.shape, post, label_stride, wrong, BWD_BLOCKS)
    gs = float(torch.tensor(gscale, dtype=torch.float32)) * (1.0 if wrong == "weight_ignored" else
                                                              float(torch.tensor(weight, dtype=torch.float32)))
    z = _zero(x)
    inv_n = 1.0 / acc[14]
    if terms == MSE:
        on = torch.ones_like(mask) if wrong == "mse_grad_at_nonpositive" else x[:, 0] > 0
        g = torch.where(on, 2.0 * (x[:, 0] - t.double()) * inv_n, z).unsqueeze(1)
    elif terms == CORAL:
        k = torch.arange(3).view(1, 3, 1, 1)
        reached = (k <= t.unsqueeze(1)) if wrong == "coral_levels" else (k < t.unsqueeze(1))
        g = (torch.sigmoid(x) - reached.double()) * inv_n
    else:
        p = torch.softmax(x, 1)
        oh = _onehot(t, mask, C).double()
        dI, dP = dice_coeffs(acc, terms, C, wrong)
        dp = dI.view(1, C, 1, 1) * oh + dP.view(1, C, 1, 1)
        dot = (dp * p).sum(1, keepdim=True)
        pt = _pick(p, t)
        lt = pt.clamp_min(1e-300).log()
        dlt = torch.zeros_like(pt)
        if terms & FOCAL:
            extra = z if wrong == "focal_bwd_term" else 2.0 * (1.0 - pt) * pt * lt
            dlt = dlt + (extra - (1.0 - pt) ** 2) * inv_n
        if terms & CE:
            dlt = dlt - inv_n
        g = p * (dp - dot) + dlt.unsqueeze(1) * (oh - p)
    return gs * torch.where(mask.unsqueeze(1), g, z)


# ---- bounds --------------------------------------------------------------------------------------------------------------

def _softmax_parts(x):
    """module docstring, softmax_px -> m, p, R_c (units of u), log s, the absolute error of log s"""
    C = x.shape[1]
    m = x.amax(1, keepdim=True)
    d = x - m
    e = d.exp()
    s = e.sum(1, keepdim=True)
    w = (e * d.abs()).sum(1, keepdim=True) / s
    Rs = w + A_EXP + (C - 1)
    Rp = d.abs() + A_EXP + Rs + 2.0
    logs = s.log()
    return m.squeeze(1), e / s, Rp, logs.squeeze(1), U * (A_LOG * logs + Rs).squeeze(1)


def bounds(logits, labels, terms, post, label_stride=1):
    """-> dict: acc [15] and loss (forward), grad [N, C, H, W] for gscale * weight = 1 (scale it by |gscale * weight|)"""
    x = logits.detach().double()
    N, C, H, W = x.shape
    total = N * H * W
    kf = sweeps(total, FWD_BLOCKS)
    acc, L = forward(x, labels, terms, post, label_stride)
    t, mask = targets(labels, x.shape, post, label_stride)
    mk, mk1 = mask.double(), mask.unsqueeze(1).double()
    n = acc[14]
    b = torch.zeros(15, dtype=torch.float64)
    if terms == MSE:
        d2 = (x[:, 0].clamp_min(0.0) - t.double()) ** 2 * mk
        b[12] = (K_MSE_FWD * U * d2 + TINY * mk).sum() + (kf - 1) * U * d2.sum()
        val = torch.where(x[:, 0] > 0, 2.0 * (x[:, 0] - t.double()) / n, _zero(x)) * mk
        grad = (K_MSE_BWD * U * val.abs() + TINY * mk).unsqueeze(1)
    elif terms == CORAL:
        reached = (torch.arange(3).view(1, 3, 1, 1) < t.unsqueeze(1))
        ex = (-x.abs()).exp()
        l1 = torch.log1p(ex)
        lsg = x.clamp_max(0.0) - l1
        term = torch.where(reached, lsg, lsg - x)
        e = U * (A_LOG1P * l1 + A_EXP * ex / (1.0 + ex)) + U * lsg.abs() + torch.where(reached, _zero(x), U * term.abs()) + TINY
        b[12] = (e * mk1).sum() + (3 * kf - 1) * U * (term.abs() * mk1).sum()
        sg = torch.sigmoid(x)
        v = sg - reached.double()
        e_v = sg * (A_EXP * (1.0 - sg) + 2.0) * U + U * v.abs()
        grad = ((e_v + K_CORAL_SCALE * U * v.abs()) / n + TINY) * mk1
    else:
        m, p, Rp, logs, e_logs = _softmax_parts(x)
        oh = _onehot(t, mask, C).double()
        e_p = p * Rp * U + TINY
        bI = (oh * e_p).sum((0, 2, 3)) + (kf - 1) * U * acc[0:C]
        bP = (mk1 * e_p).sum((0, 2, 3)) + (kf - 1) * U * acc[8:8 + C]
        b[0:C], b[8:8 + C] = bI, bP
        xt = _pick(x, t)
        e_lse = e_logs + U * (m.abs() + logs)
        lt = xt - (m + logs)
        e_lt = e_lse + U * (xt.abs() + m.abs() + logs)
        pt = lt.exp()
        e_pt = pt * (e_lt + A_EXP * U) + TINY
        q = 1.0 - pt
        e_q = e_pt + U * q
        f = q * q * lt.abs()
        e_f = 2.0 * q * lt.abs() * e_q + q * q * e_lt + 2.0 * U * f + TINY
        b[12] = (e_f * mk).sum() + (kf - 1) * U * (f * mk).sum()
        b[13] = (e_lt * mk).sum() + (kf - 1) * U * (lt.abs() * mk).sum()
        # ---- backward
        dI, dP = dice_coeffs(acc, terms, C)
        den = acc[4:4 + C] + acc[8:8 + C] + EPS
        e_dI = dI.abs() * (U + bP / den)
        e_dP = dP.abs() * (U + 2.0 * bI / (2.0 * acc[0:C] + EPS) + 2.0 * bP / den)
        v4 = lambda a: a.view(1, C, 1, 1)      # noqa: E731
        mag_dp = v4(dI.abs()) * oh + v4(dP.abs())
        e_dp = v4(e_dI) * oh + v4(e_dP) + U * mag_dp
        mag_dot = (mag_dp * p).sum(1, keepdim=True)
        e_dot = (e_dp * p + mag_dp * e_p).sum(1, keepdim=True) + (2 * C - 1) * U * mag_dot
        ptb = _pick(p, t)
        e_ptb = _pick(e_p, t)
        ltb = ptb.clamp_min(1e-300).log()
        qb = 1.0 - ptb
        e_qb = e_ptb + U * qb
        mag_dlt, e_dlt = torch.zeros_like(ptb), torch.zeros_like(ptb)
        if terms & FOCAL:
            g = (ptb * ltb).abs()
            e_g = e_ptb * (ltb.abs() + 1.0) + A_LOG * U * g
            A1 = 2.0 * qb * g
            e_A1 = 2.0 * g * e_qb + 2.0 * qb * e_g + 2.0 * U * A1
            B1 = qb * qb
            e_B1 = 2.0 * qb * e_qb + U * B1
            mag_dlt = (A1 + B1) / n
            e_dlt = (e_A1 + e_B1 + U * (A1 + B1)) / n + 2.0 * U * mag_dlt
        if terms & CE:
            e_dlt = e_dlt + U / n + (U * (mag_dlt + 1.0 / n) if terms & FOCAL else 0.0)
            mag_dlt = mag_dlt + 1.0 / n
        mag_t1 = mag_dp + mag_dot
        e_t1 = e_dp + e_dot + U * mag_t1
        mag_t2 = p * mag_t1
        e_t2 = p * e_t1 + e_p * mag_t1 + U * mag_t2
        t3 = (oh - p).abs()
        e_t3 = e_p + U * t3
        mag_t4 = mag_dlt.unsqueeze(1) * t3
        e_t4 = mag_dlt.unsqueeze(1) * e_t3 + e_dlt.unsqueeze(1) * t3 + U * mag_t4
        grad = (e_t2 + e_t4 + U * (mag_t2 + mag_t4) + K_SCALE * U * (mag_t2 + mag_t4) + TINY) * mk1
    # ---- loss: first order through compose(), and the fp32 store
    if aux(terms):
        bL = b[12] / n
    else:
        bL = 0.0
        if terms & DICE:
            c0 = 1 if C == 2 else 0
            for c in range(c0, C):
                den = acc[4 + c] + acc[8 + c] + EPS
                bL = bL + (2.0 * b[c] / den + (2.0 * acc[c] + EPS) / (den * den) * b[8 + c]) / (C - c0)
        if terms & FOCAL:
            bL = bL + b[12] / n
        if terms & CE:
            bL = bL + b[13] / n
    return {"acc": b, "loss": bL + U * abs(L) + TINY, "grad": grad, "acc64": acc, "loss64": L}


def scale(gscale, weight):
    """|gscale * weight| of the fp32 values, for the gradient bound"""
    return abs(float(torch.tensor(gscale, dtype=torch.float32)) * float(torch.tensor(weight, dtype=torch.float32)))


# ---- the kernels' arithmetic in fp32 on the CPU (tests/test_loss_ref_cpu.py: the bounds admit a correct fp32 kernel) --------

def _thread_sums(terms, cap):
    """terms [total, L] fp32 (zero where a pixel is skipped): every thread adds the L terms of its pixels in sweep order in
    fp32; float64 from there on"""
    total, L = terms.shape
    T = min(-(-total // THREADS), cap) * THREADS
    k = -(-total // T)
    v = torch.zeros((k * T, L), dtype=torch.float32)
    v[:total] = terms
    v = v.view(k, T, L)
    a = torch.zeros(T, dtype=torch.float32)
    for j in range(k):
        for i in range(L):
            a = a + v[j, :, i]
    return a.double().sum()


def _softmax_f32(x):
    C = x.shape[1]
    m = x.amax(1, keepdim=True)
    e = (x - m).exp()
    s = e[:, 0:1]
    for c in range(1, C):
        s = s + e[:, c:c + 1]
    inv = torch.ones_like(s) / s
    return e * inv, (m + s.log()).squeeze(1)


def f32_forward(logits, labels, terms, post, label_stride=1):
    """-> (acc [15] float64, loss fp32) in the kernels' order of operations"""
    x = logits.float()
    N, C, H, W = x.shape
    t, mask = targets(labels, x.shape, post, label_stride)
    z = torch.zeros((), dtype=torch.float32)
    acc = torch.zeros(15, dtype=torch.float64)

    def tsum(v):      # [N, H, W] or [N, L, H, W]
        v = v.unsqueeze(1) if v.dim() == 3 else v
        return _thread_sums(v.permute(0, 2, 3, 1).reshape(N * H * W, -1), FWD_BLOCKS)
    acc[14] = tsum(mask.float())
    if terms == MSE:
        d = x[:, 0].clamp_min(0.0) - t.float()
        acc[12] = tsum(torch.where(mask, d * d, z))
    elif terms == CORAL:
        reached = torch.arange(3).view(1, 3, 1, 1) < t.unsqueeze(1)
        lsg = x.clamp_max(0.0) - torch.log1p((-x.abs()).exp())
        acc[12] = -tsum(torch.where(mask.unsqueeze(1), torch.where(reached, lsg, lsg - x), z))
    else:
        p, lse = _softmax_f32(x)
        oh = _onehot(t, mask, C)
        for c in range(C):
            acc[c] = tsum(torch.where(oh[:, c], p[:, c], z))
            acc[4 + c] = tsum(oh[:, c].float())
            acc[8 + c] = tsum(torch.where(mask, p[:, c], z))
        lt = _pick(x, t) - lse
        pt = lt.exp()
        acc[12] = tsum(torch.where(mask, (-(1.0 - pt)) * (1.0 - pt) * lt, z))
        acc[13] = tsum(torch.where(mask, -lt, z))
    return acc, compose(acc, terms, C).float()


def f32_backward(logits, labels, terms, post, label_stride, acc, gscale=1.0, weight=1.0):
    x = logits.float()
    N, C, H, W = x.shape
    t, mask = targets(labels, x.shape, post, label_stride)
    z = torch.zeros((), dtype=torch.float32)
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float64).float()      # noqa: E731
    gs = f32(gscale) * f32(weight)
    inv_n = f32(1.0 / acc[14])
    if terms == MSE:
        g = torch.where(x[:, 0] <= 0, z, (gs * inv_n) * 2.0 * (x[:, 0] - t.float())).unsqueeze(1)
    elif terms == CORAL:
        reached = torch.arange(3).view(1, 3, 1, 1) < t.unsqueeze(1)
        sg = 1.0 / (1.0 + (-x).exp())
        g = (gs * inv_n) * (sg - reached.float())
    else:
        p, _ = _softmax_f32(x)
        oh = _onehot(t, mask, C).float()
        dI, dP = dice_coeffs(acc, terms, C)
        dp = dI.float().view(1, C, 1, 1) * oh + dP.float().view(1, C, 1, 1)
        dot = torch.zeros_like(p[:, 0:1])
        for c in range(C):
            dot = dot + dp[:, c:c + 1] * p[:, c:c + 1]
        pt = _pick(p, t)
        lt = pt.clamp_min(1e-45).log()
        dlt = torch.zeros_like(pt)
        if terms & FOCAL:
            dlt = dlt + (2.0 * (1.0 - pt) * pt * lt - (1.0 - pt) * (1.0 - pt)) * inv_n
        if terms & CE:
            dlt = dlt + (-inv_n)
        g = gs * (p * (dp - dot) + dlt.unsqueeze(1) * (oh - p))
    return torch.where(mask.unsqueeze(1), g, z)


# ---- case tables: data, tensors are made from the seeds -------------------------------------------------------------------

# kernel templates: name -> (C, post, every term of the template)
TEMPLATES = {"c2": (2, 0, 7), "c4post": (4, 1, 7), "c4": (4, 0, 7), "c2post": (2, 1, 7), "mse": (1, 1, MSE), "coral": (3, 1, CORAL)}
SHAPES = [(1, 1, 1, 1), (2, 7, 13, 1), (1, 15, 256, 1), (1, 16, 256, 1), (1, 17, 256, 1), (3, 17, 31, 1),
          (2, 9, 14, 2), (2, 9, 14, 4)]      # N, H, W, label stride: one pixel, under a block, nblocks 15 / 16 / 17, a partial
#                                              last block with N = 3, label strides
BIG = (1, 1025, 1024, 1)      # the only size at which both capped grids take a second sweep
LABELS = ["mix", "absent", "only", "one_pixel", "image0_background"]
REGIMES = ["randn2", "right12", "wrong12", "pm80", "equal", "offset1e4", "quarters"]
SCALES = [(1.0, 1.0), (0.5, 1.0), (0.0, 1.0), (1.0, 0.25), (0.5, 0.25), (0.0, 0.25)]      # gscale, weight


def _case(tpl, shape, terms=None, labels="mix", regime="randn2", scales=None, big=False):
    C, post, full = TEMPLATES[tpl]
    terms = full if terms is None else terms
    N, H, W, ls = shape
    name = "%s-t%d-%dx%dx%d-ls%d-%s-%s%s" % (tpl, terms, N, H, W, ls, labels, regime, "-scales" if scales else "")
    return dict(name=name, tpl=tpl, C=C, post=post, terms=terms, N=N, H=H, W=W, ls=ls, labels=labels, regime=regime,
                scales=scales or SCALES[:1], big=big)


def _cases():
    out = []
    for tpl in ("c2", "c4post", "mse", "coral"):
        for shape in SHAPES:
            out.append(_case(tpl, shape, scales=SCALES if shape[:3] == (3, 17, 31) else None))
    for tpl in ("c2", "c4post"):
        for terms in range(1, 7):
            out.append(_case(tpl, (2, 7, 13, 1), terms))
    for tpl in ("c4", "c2post"):
        out.append(_case(tpl, (2, 7, 13, 1)))
        out.append(_case(tpl, (2, 9, 14, 2)))
    for tpl in TEMPLATES:
        post = TEMPLATES[tpl][1]
        for lab in LABELS[1:]:
            if lab in ("one_pixel", "image0_background") and not post:
                continue
            out.append(_case(tpl, (2, 7, 13, 1), labels=lab))
    for tpl in ("c2", "c4post"):
        for regime in REGIMES[1:]:
            out.append(_case(tpl, (3, 17, 31, 1), regime=regime))
        for terms in (FOCAL, CE, DICE):      # the confident regimes per term
            for regime in ("right12", "wrong12", "pm80"):
                out.append(_case(tpl, (2, 7, 13, 1), terms, regime=regime))
    out.append(_case("mse", (3, 17, 31, 1), regime="mse_edges"))
    out.append(_case("coral", (3, 17, 31, 1), regime="coral_edges"))
    for tpl in ("c2", "c4post", "mse", "coral"):
        out.append(_case(tpl, BIG, big=True))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()
SMALL = [c for c in CASES if not c["big"]]


def _seed(case):
    s = 0
    for ch in case["name"]:
        s = (s * 131 + ord(ch)) % 1000003
    return s


def make_labels(case, gen):
    N, H, W, ls, C, post = (case[k] for k in ("N", "H", "W", "ls", "C", "post"))
    classes = {"mse": 4, "coral": 4}.get(case["tpl"], C)      # class values 0 .. classes - 1 (label = class + post)
    LH, LW = H * ls, W * ls
    y = torch.randint(0, classes, (N, LH, LW), generator=gen)
    kind = case["labels"]
    if kind == "absent":
        y = torch.where(y == classes - 1, torch.zeros_like(y), y)
    elif kind == "only":
        y = torch.full_like(y, classes - 1)
    y = y + post
    if post and kind in ("mix", "absent"):
        y = torch.where(torch.rand((N, LH, LW), generator=gen) < 0.4, torch.zeros_like(y), y)
        y[0, 0, 0] = max(int(y[0, 0, 0]), 1)      # never an empty mask
    if kind == "one_pixel":
        keep = int(y[N - 1, (H - 1) * ls, (W // 2) * ls])
        y = torch.zeros_like(y)
        y[N - 1, (H - 1) * ls, (W // 2) * ls] = keep
    if kind == "image0_background":
        y[0] = 0
    return y.to(torch.uint8)


def make_logits(case, labels, gen):
    N, H, W, ls, C, post = (case[k] for k in ("N", "H", "W", "ls", "C", "post"))
    C = channels(case["terms"], C)
    regime = case["regime"]
    x = torch.randn((N, C, H, W), generator=gen, dtype=torch.float64) * 2.0
    if regime == "mse_edges":      # negative values, exact zeros, values above 4
        x = x * 2.0 + 1.0
        x[:, :, ::3, ::2] = 0.0
        x[:, :, 1::4, 1::3] += 6.0
        return x.float()
    if regime == "coral_edges":
        pick = torch.randint(0, 4, x.shape, generator=gen)
        x = torch.where(pick == 0, torch.zeros_like(x), x)
        x = torch.where(pick == 1, torch.full_like(x, 50.0), x)
        x = torch.where(pick == 2, torch.full_like(x, -50.0), x)
        return x.float()
    if aux(case["terms"]) or regime == "randn2":
        return x.float()
    t, _ = targets(labels, x.shape, post, ls)
    oh = _onehot(t, torch.ones_like(t, dtype=torch.bool), C).double()
    other = _onehot((t + 1) % C, torch.ones_like(t, dtype=torch.bool), C).double()
    sign = torch.where(torch.rand(x.shape, generator=gen) < 0.5, -1.0, 1.0).double()
    made = {"right12": x + 12.0 * oh, "wrong12": x + 12.0 * other, "pm80": 80.0 * sign, "equal": x[:, :1].expand_as(x),
            "offset1e4": x + 1e4}
    if regime == "quarters":
        quarter = (torch.arange(N * H * W).view(N, 1, H, W) % 4).expand_as(x)
        out = x.clone()
        for i, r in enumerate(("right12", "wrong12", "pm80")):
            out = torch.where(quarter == i + 1, made[r], out)
        return out.float()
    return made[regime].float().contiguous()


def make(case):
    """-> (logits fp32 [N, C, H, W], labels uint8 [N, H ls, W ls])"""
    gen = torch.Generator().manual_seed(_seed(case))
    labels = make_labels(case, gen)
    return make_logits(case, labels, gen), labels


# the empty building mask (`post` without a building pixel), pinned to the reference's behaviour: 0.0 for dice alone, NaN
# for every mask with focal or ce, for mse and for coral; the gradient is all zeros.  (terms, C)
EMPTY_MASK = [(DICE, 4), (FOCAL, 4), (CE, 4), (DICE | FOCAL, 4), (7, 4), (DICE, 2), (7, 2), (MSE, 1), (CORAL, 3)]
