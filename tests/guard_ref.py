"""Float64 CPU restatement of the gradient guard (include/xv2.h xv2_grad_guard): the flat sum of squares of every
gradient element, torch.nn.utils.clip_grad_norm_'s coefficient, then the skip rule.  Written from the formulas; the
CPU test holds it against torch's own clip_grad_norm_ in float64."""
import math

import torch


def guard(gs, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False):
    """gs: gradient tensors (any dtype; summed in float64).  Returns (norm, coef, skip): norm = grad_scale * sqrt(sum of
    squares), coef = min(max_norm / (norm + 1e-6), 1) (1 when max_norm == 0; a NaN stays a NaN), skip = skip_nonfinite and
    the norm is not finite."""
    total = 0.0
    for g in gs:
        total += float((g.detach().double().flatten() ** 2).sum())
    norm = grad_scale * math.sqrt(total)          # (sqrt keeps an Inf and a NaN)
    coef = 1.0
    if max_norm > 0.0:
        coef = max_norm / (norm + 1e-6)
        if coef > 1.0:
            coef = 1.0
    return norm, coef, bool(skip_nonfinite) and not math.isfinite(norm)


def clipped(gs, coef):
    """the gradients the rule then sees (float64)"""
    return [g.detach().double() * coef for g in gs]
