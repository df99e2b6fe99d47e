"""Float64 CPU restatement of the eight --optimizer update rules (model/plt.py:150-161) with the constructor defaults
the reference leaves in place, one plain function per rule, written from the update formulas (apex and torch_optimizer
are not dependencies of this project).

Every rule takes lists of per-tensor parameters `ps` (updated in place) and gradients `gs` (already multiplied by the
gradient scale), a state dict {name: [per-tensor tensor]} it fills on first use, the learning rate of this step and
the 1-based step `t`.  The state names are the flat optimizers' (xview2_amd.optim)."""
import math

import torch
import torch.nn.functional as F


def _state(st, name, ps, scalar=False):
    if name not in st:
        st[name] = [torch.zeros((), dtype=p.dtype) if scalar else torch.zeros_like(p) for p in ps]
    return st[name]


def sgd(ps, gs, st, lr, t, momentum=0.0):
    """apex FusedSGD(lr, momentum): dampening 0, no Nesterov, no weight decay"""
    if momentum == 0.0:
        for p, g in zip(ps, gs):
            p.sub_(lr * g)
        return
    bufs = _state(st, "momentum_buffer", ps)
    for p, g, b in zip(ps, gs, bufs):
        if t == 1:
            b.copy_(g)
        else:
            b.mul_(momentum).add_(g)
        p.sub_(lr * b)


def _moments(m, v, g, b1, b2):
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)


def adamw(ps, gs, st, lr, t, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.AdamW; apex FusedAdam with its default adam_w_mode=True is the same update"""
    b1, b2 = betas
    ms, vs = _state(st, "exp_avg", ps), _state(st, "exp_avg_sq", ps)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    for p, g, m, v in zip(ps, gs, ms, vs):
        p.mul_(1 - lr * wd)
        _moments(m, v, g, b1, b2)
        p.sub_(lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps))


adam = adamw


def radam(ps, gs, st, lr, t, wd, betas=(0.9, 0.999), eps=1e-8):
    """torch_optimizer RAdam: decoupled decay, rectified step once rho_t >= 5"""
    b1, b2 = betas
    ms, vs = _state(st, "exp_avg", ps), _state(st, "exp_avg_sq", ps)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    rho_inf = 2 / (1 - b2) - 1
    rho_t = rho_inf - 2 * t * b2 ** t / bc2
    for p, g, m, v in zip(ps, gs, ms, vs):
        p.mul_(1 - lr * wd)
        _moments(m, v, g, b1, b2)
        if rho_t >= 5:
            rt = math.sqrt(bc2 * (rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t))
            p.sub_(lr * rt / bc1 * m / (v.sqrt() + eps))
        else:
            p.sub_(lr / bc1 * m)


def adabelief(ps, gs, st, lr, t, wd, betas=(0.9, 0.999), eps=1e-3):
    """torch_optimizer AdaBelief: eps 1e-3, L2 decay, eps kept in the variance state"""
    b1, b2 = betas
    ms, ss = _state(st, "exp_avg", ps), _state(st, "exp_avg_var", ps)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    for p, g, m, s in zip(ps, gs, ms, ss):
        g = g + wd * p
        m.mul_(b1).add_((1 - b1) * g)
        s.mul_(b2).add_((1 - b2) * (g - m) ** 2)
        s.add_(eps)
        p.sub_(lr / bc1 * m / (s.sqrt() / math.sqrt(bc2) + eps))


def adabound(ps, gs, st, lr, t, wd, base_lr, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8):
    """torch_optimizer AdaBound: L2 decay, the step clamped between bounds that follow lr / base_lr"""
    b1, b2 = betas
    ms, vs = _state(st, "exp_avg", ps), _state(st, "exp_avg_sq", ps)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    alpha = lr * math.sqrt(bc2) / bc1
    f = final_lr * lr / base_lr
    lo, hi = f * (1 - 1 / (gamma * t + 1)), f * (1 + 1 / (gamma * t))
    for p, g, m, v in zip(ps, gs, ms, vs):
        g = g + wd * p
        _moments(m, v, g, b1, b2)
        p.sub_((alpha / (v.sqrt() + eps)).clamp(lo, hi) * m)


def adamp_view(p, g, delta=0.1, eps=1e-8):
    """AdamP's projection decision for one tensor: 0 none, 1 channel view (rows = dim 0), 2 layer view"""
    if p.dim() < 2:
        return 0
    for code, rows in ((1, p.shape[0]), (2, 1)):
        pv, gv = p.reshape(rows, -1), g.reshape(rows, -1)
        cos = F.cosine_similarity(gv, pv, dim=1, eps=eps).abs()
        if float(cos.max()) < delta / math.sqrt(pv.shape[1]):
            return code
    return 0


def adamp(ps, gs, st, lr, t, wd, betas=(0.9, 0.999), eps=1e-8, delta=0.1, wd_ratio=0.1):
    """torch_optimizer AdamP (nesterov off); returns the per-tensor decision of `adamp_view`"""
    b1, b2 = betas
    ms, vs = _state(st, "exp_avg", ps), _state(st, "exp_avg_sq", ps)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    decisions = []
    for p, g, m, v in zip(ps, gs, ms, vs):
        _moments(m, v, g, b1, b2)
        u = m / (v.sqrt() / math.sqrt(bc2) + eps)
        code = adamp_view(p, g, delta, eps)
        wdr = 1.0
        if code:
            rows = p.shape[0] if code == 1 else 1
            pv = p.reshape(rows, -1)
            pn = pv / (pv.norm(dim=1, keepdim=True) + eps)
            u = (u.reshape(rows, -1) - pn * (pn * u.reshape(rows, -1)).sum(dim=1, keepdim=True)).reshape(p.shape)
            wdr = wd_ratio
        decisions.append(code)
        p.mul_(1 - lr * wd * wdr)
        p.sub_(lr / bc1 * u)
    return decisions


def novograd(ps, gs, st, lr, t, wd, betas=(0.9, 0.999), eps=1e-8):
    """apex FusedNovoGrad defaults: per-tensor blended L2 norm (the first norm at t = 1), grad averaging, bias
    correction, decay outside the moment"""
    b1, b2 = betas
    ms, ns = _state(st, "exp_avg", ps), _state(st, "exp_avg_norm", ps, scalar=True)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    for p, g, m, nv in zip(ps, gs, ms, ns):
        n = g.norm()
        nv.copy_(n if t == 1 else torch.sqrt(b2 * nv * nv + (1 - b2) * n * n))
        m.mul_(b1).add_((1 - b1) * g)
        p.sub_(lr * ((m / bc1) / (nv / math.sqrt(bc2) + eps) + wd * p))


RULES = ("sgd", "adam", "adamw", "radam", "adabelief", "adabound", "adamp", "novograd")


def step(name, ps, gs, st, lr, t, wd=0.0, momentum=0.0, base_lr=None):
    """one step of the --optimizer choice `name` with the hyperparameters model/plt.py:150-161 passes; returns AdamP's
    decisions (None for the other rules)"""
    if name == "sgd":
        return sgd(ps, gs, st, lr, t, momentum)
    if name == "adabound":
        return adabound(ps, gs, st, lr, t, wd, base_lr)
    return globals()[name](ps, gs, st, lr, t, wd)
