"""fp64 restatement of the ``lovasz`` loss term (csrc/lovasz.hip), written from Berman et al., "The
Lovasz-Softmax loss" (CVPR 2018), Algorithm 1, with classes = "present" and per_image = False, in two independent forms,
and numpy models of the kernels' key encoding and of what they read out of a sorted row.

For a class c over the M considered pixels (``post``: the pixels with label > 0, whose class is label - 1; otherwise every
pixel, class = label): fg_i = (class_i == c), e_i = 1 - p_i(c) if fg_i else p_i(c), p the channel softmax, G = #fg.

(i)  ``lovasz_sorted``: errors sorted descending, J_j = 1 - (G - F_j) / (G + B_j) with F_j / B_j the foreground / background
     entries among the first j, loss_c = sum_j e_(j) (J_j - J_(j-1)); differentiated by autograd through the sort.
(ii) ``lovasz_ranked``: loss_c = sum_i e_i w_i with constant weights from rank counts alone (B_>(v) / b: background errors
     > v / == v; F_>=(v): foreground errors >= v):
        foreground:  w = 1 / (G + B_>(e))
        background:  w = (G - F_>=(e)) (1 / (G + B_>(e)) - 1 / (G + B_>(e) + b)) / b
     i.e. among equal errors the foreground comes first and tied background entries share their telescoped sum equally.
The term is the mean of loss_c over the classes of ``class_mask`` with G > 0; 0 when there is none."""
import numpy as np
import torch

SIGN = np.uint32(0x80000000)
SKIP = np.uint32(0xFFFFFFFF)
NAN = np.uint32(0x7FC00000)
LOW = np.uint32(0x7FFFFFFF)


def class_mask(C, post):
    return 0b10 if (C == 2 and not post) else (1 << C) - 1


def errors(logits, labels, post=False, label_stride=1):
    """fp64 errors e [C, M], fg [C, M] (bool), valid [M] (bool), p [C, M]; M = N*H*W in the kernels' order (n, h, w)"""
    x = logits.double()
    n, c = x.shape[:2]
    y = labels[:, ::label_stride, ::label_stride].long().reshape(-1)
    p = torch.softmax(x.reshape(n, c, -1), 1).permute(1, 0, 2).reshape(c, -1)
    valid = (y > 0) if post else torch.ones_like(y, dtype=torch.bool)
    cls = y - 1 if post else y
    fg = (cls.unsqueeze(0) == torch.arange(c).unsqueeze(1)) & valid.unsqueeze(0)
    return torch.where(fg, 1 - p, p), fg, valid, p


def _mean(losses, x):
    if not losses:
        return x.double().sum() * 0
    return sum(losses) / len(losses)


def lovasz_sorted(logits, labels, post=False, label_stride=1, mask=None):
    """form (i); differentiable in `logits`"""
    e, fg, valid, _ = errors(logits, labels, post, label_stride)
    C = e.shape[0]
    mask = class_mask(C, post) if mask is None else mask
    losses = []
    for c in range(C):
        f = fg[c][valid].double()
        G = f.sum()
        if not (mask >> c) & 1 or G == 0:
            continue
        es, perm = torch.sort(e[c][valid], descending=True)
        fs = f[perm]
        jac = 1 - (G - fs.cumsum(0)) / (G + (1 - fs).cumsum(0))
        losses.append((es * torch.cat([jac[:1], jac[1:] - jac[:-1]])).sum())
    return _mean(losses, logits)


def rank_weights(e, f):
    """the weights of form (ii) for one class: e fp64 [M] errors, f bool [M] foreground flags (numpy), G > 0"""
    G = int(f.sum())
    fgs, bgs = np.sort(e[f]), np.sort(e[~f])
    Nb = bgs.size
    w = np.zeros(e.shape, dtype=np.float64)
    w[f] = 1.0 / (G + Nb - np.searchsorted(bgs, e[f], "right"))
    v = e[~f]
    lo, hi = np.searchsorted(bgs, v, "left"), np.searchsorted(bgs, v, "right")
    bgt, b = Nb - hi, hi - lo
    fge = G - np.searchsorted(fgs, v, "left")
    w[~f] = (G - fge) * (1.0 / (G + bgt) - 1.0 / (G + bgt + b)) / b
    return w


def lovasz_ranked(logits, labels, post=False, label_stride=1, mask=None):
    """form (ii); differentiable in `logits` (the weights are constants, as in the kernels)"""
    e, fg, valid, _ = errors(logits, labels, post, label_stride)
    C = e.shape[0]
    mask = class_mask(C, post) if mask is None else mask
    losses = []
    for c in range(C):
        f = fg[c][valid].numpy()
        if not (mask >> c) & 1 or not f.any():
            continue
        ev = e[c][valid]
        losses.append((ev * torch.from_numpy(rank_weights(ev.detach().numpy(), f))).sum())
    return _mean(losses, logits)


def min_fg_bg_gap(logits, labels, post=False, label_stride=1, mask=None):
    """smallest fp64 distance between a foreground and a background error of one included class: above the fp32 error
    of an error, the fp32 and the fp64 evaluation order the two sets against each other alike"""
    e, fg, valid, _ = errors(logits, labels, post, label_stride)
    C = e.shape[0]
    mask = class_mask(C, post) if mask is None else mask
    gap = float("inf")
    for c in range(C):
        f = fg[c][valid].numpy()
        if not (mask >> c) & 1 or not f.any() or f.all():
            continue
        ev = e[c][valid].numpy()
        bgs = np.sort(ev[~f])
        at = np.searchsorted(bgs, ev[f])
        near = np.minimum(np.abs(bgs[np.clip(at, 0, bgs.size - 1)] - ev[f]), np.abs(bgs[np.clip(at - 1, 0, bgs.size - 1)] - ev[f]))
        gap = min(gap, float(near.min()))
    return gap


# ---- numpy models of the kernels' integer side ------------------------------------------------------------------------

def encode_keys(e32, fg, valid):
    """keys of one class from fp32 errors: bits(e) | fg << 31 with e canonical (everything not > 0 is +0, NaN is 0x7fc00000),
    skipped entries 0xFFFFFFFF"""
    e = np.asarray(e32, dtype=np.float32).copy()
    nan = np.isnan(e)
    e[~(e > 0)] = 0.0
    bits = e.view(np.uint32).copy()
    bits[nan] = NAN
    keys = bits | (np.asarray(fg).astype(np.uint32) << np.uint32(31))
    keys[~np.asarray(valid)] = SKIP
    return keys


def decode_keys(keys):
    """(e fp32, fg bool, valid bool) of a key row"""
    valid = keys != SKIP
    return (keys & LOW).view(np.float32), ((keys >> np.uint32(31)) == 1) & valid, valid


def segments(sorted_row):
    """(background error bits ascending, foreground error bits ascending, skipped count) of an ascending key row"""
    nb = int(np.searchsorted(sorted_row, SIGN, "left"))
    end = int(np.searchsorted(sorted_row, SKIP, "left"))
    return sorted_row[:nb], sorted_row[nb:end] & LOW, int(sorted_row.size) - end


def key_weights(keys, sorted_row):
    """signed fp64 weights d loss_c / d p(c) per entry of `keys` (-w foreground, +w background, 0 skipped) read out of the
    class's sorted row by integer comparisons alone, as the backward kernel does"""
    bg, fgk, _ = segments(sorted_row)
    G, Nb = fgk.size, bg.size
    w = np.zeros(keys.shape, dtype=np.float64)
    if G == 0:
        return w
    valid = keys != SKIP
    isfg = valid & (keys >= SIGN)
    isbg = valid & (keys < SIGN)
    w[isfg] = -1.0 / (G + Nb - np.searchsorted(bg, keys[isfg] & LOW, "right"))
    v = keys[isbg]
    lo, hi = np.searchsorted(bg, v, "left"), np.searchsorted(bg, v, "right")
    bgt, b = Nb - hi, hi - lo
    fge = G - np.searchsorted(fgk, v, "left")
    w[isbg] = (G - fge) / ((G + bgt).astype(np.float64) * (G + bgt + b))
    return w


def sorted_loss(sorted_row):
    """loss_c of one class from its sorted row: sum of e |w| over the row's entries in fp64 (0 when G == 0)"""
    row = sorted_row[sorted_row != SKIP]
    e = (row & LOW).view(np.float32).astype(np.float64)
    return float(np.sum(e * np.abs(key_weights(row, sorted_row))))


def records(keys, mask):
    """records [C, 4] of a key tensor [C, M]: G, Nb, skipped, included-and-present"""
    out = []
    for c in range(keys.shape[0]):
        skipped = int((keys[c] == SKIP).sum())
        G = int((keys[c] >= SIGN).sum()) - skipped
        out.append([G, keys.shape[1] - G - skipped, skipped, int(bool((mask >> c) & 1) and G > 0)])
    return np.array(out, dtype=np.int32)


def lattice_logits(shape, seed):
    """C = 2 logits whose building-class probabilities are p = 0.05 + 0.9 (k + 0.3) / n for a permutation k of 0 .. n - 1:
    all distinct, and no foreground error 1 - p(k) equals a background error p(k') (that needs k + k' + 0.6 = n)"""
    N, C, H, W = shape
    assert C == 2
    n = N * H * W
    k = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).double()
    p = 0.05 + 0.9 * (k + 0.3) / n
    x = torch.zeros(N, 2, H, W, dtype=torch.float64)
    x[:, 1] = torch.log(p / (1 - p)).reshape(N, H, W)
    return x.float()


def lattice_inputs(shape, seed, pos=0.3):
    N, C, H, W = shape
    y = (torch.rand(N, H, W, generator=torch.Generator().manual_seed(seed + 1000)) < pos).to(torch.uint8)
    return lattice_logits(shape, seed), y
