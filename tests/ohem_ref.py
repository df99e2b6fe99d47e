"""fp64 restatement of the ``ohem_hard`` loss term (csrc/ohem.hip) and numpy models of its select stage.

Per image i, with l = logsumexp(x) - x[y] per pixel: positives are the pixels with label > 0, negatives those with label 0,
Cp / Cn their counts, k = min(Cn, max(Cn // 4, 5, 2 Cp)).  The loss is the sum over the batch of (sum of l over positives +
sum of the k largest negative l), divided by sum_i (Cp + k).  With t the k-th largest negative loss, c_gt / c_eq the number
of negatives above / at t and r = k - c_gt, a negative's weight is 1 above t, r / c_eq at t, 0 below (the mean over every
valid choice of the tied subset); positives weigh 1.  Deep supervision samples the labels with ``label_stride``."""
import numpy as np
import torch

SIGN = np.uint32(0x80000000)


def k_int(cn, cp):
    return min(cn, max(cn // 4, 5, 2 * cp))


def k_float(cn, cp):
    """the float form: int(max((Cn / 4).clamp_min(5), 2 * Cp)) entries requested, the slice [:k] of Cn values gives min(Cn, .)"""
    cn_t, cp_t = torch.tensor(cn), torch.tensor(cp)
    want = int(torch.max((cn_t / 4).clamp_min(5), 2 * cp_t))
    return len(range(cn)[:want])


def pixel_ce(logits, labels, label_stride=1):
    """fp64 [N, H*W] cross-entropy and the [N, H*W] labels a head sees"""
    x = logits.double()
    n, c = x.shape[:2]
    y = labels[:, ::label_stride, ::label_stride].long().reshape(n, -1)
    x = x.reshape(n, c, -1)
    return torch.logsumexp(x, 1) - torch.gather(x, 1, y.clamp(max=c - 1).unsqueeze(1)).squeeze(1), y


def weights(l, y):
    """per-pixel weights [N, M] (fp64) and the per-image (Cp, Cn, k, t, c_gt, c_eq, r) of the rule above"""
    w = torch.zeros_like(l)
    info = []
    for i in range(l.shape[0]):
        pos = y[i] > 0
        cp, cn = int(pos.sum()), int((~pos).sum())
        k = k_int(cn, cp)
        w[i][pos] = 1.0
        if k == 0:
            info.append((cp, cn, 0, None, 0, 0, 0))
            continue
        neg = l[i][~pos]
        order = torch.sort(neg, descending=True).values
        # NaN is the largest loss: torch sorts it first in descending order
        t = order[k - 1]
        if torch.isnan(t):
            gt, eq = torch.zeros_like(neg, dtype=torch.bool), torch.isnan(neg)
        else:
            gt, eq = (neg > t) | torch.isnan(neg), neg == t
        c_gt, c_eq = int(gt.sum()), int(eq.sum())
        r = k - c_gt
        wn = torch.zeros_like(neg)
        wn[gt] = 1.0
        wn[eq] = r / c_eq
        w[i][~pos] = wn
        info.append((cp, cn, k, float(t), c_gt, c_eq, r))
    return w, info


def ohem_hard(logits, labels, label_stride=1):
    """fp64 loss; differentiable in `logits` (the weights are constants, as in the kernels)"""
    l, y = pixel_ce(logits, labels, label_stride)
    w, info = weights(l.detach(), y)
    count = sum(cp + k for cp, _, k, *_ in info)
    # 0 * NaN would poison images that dropped a pixel; dropped pixels are excluded, not multiplied
    return torch.where(w > 0, w * l, torch.zeros_like(l)).sum() / count


def boundary_gap(logits, labels, label_stride=1):
    """smallest fp64 distance, over the images, between the k-th and the (k+1)-th largest negative loss (inf where every
    negative is kept)"""
    l, y = pixel_ce(logits, labels, label_stride)
    gap = float("inf")
    for i in range(l.shape[0]):
        neg = torch.sort(l[i][y[i] == 0], descending=True).values
        k = k_int(neg.numel(), int((y[i] > 0).sum()))
        if 0 < k < neg.numel():
            gap = min(gap, float(neg[k - 1] - neg[k]))
    return gap


def select_record(bits, k, cp=0):
    """numpy model of one row of the select stage on fp32 bit patterns (uint32): the record Cp, Cn, k, bits(t), c_gt,
    c_eq, r, 0.  Entries with the sign bit set are skipped, except -0.0, which is a zero.  k is clamped to 0..Cn."""
    keys = bits.astype(np.uint32).copy()
    keys[keys == SIGN] = 0
    cand = keys[keys < SIGN]
    cn = int(cand.size)
    k = min(max(int(k), 0), cn)
    if k == 0:
        return [cp, cn, 0, 0, 0, 0, 0, 0]
    t = np.sort(cand)[cn - k]
    c_gt, c_eq = int((cand > t).sum()), int((cand == t).sum())
    return [cp, cn, k, int(t.view(np.int32)), c_gt, c_eq, k - c_gt, 0]


def forward_record(px_bits):
    """the record of one image from its px_loss row (uint32 bit patterns; positives hold a value with the sign bit set)"""
    cn = int((px_bits < SIGN).sum())
    cp = int(px_bits.size) - cn
    return select_record(px_bits, k_int(cn, cp), cp)
