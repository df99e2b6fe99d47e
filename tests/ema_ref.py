"""float64 restatement of the weight average (include/xv2.h xv2_ema_update_dev, csrc/optim.hip ema_update_kernel).

Update t (from 0) uses d_t = min(D, (1 + t) / (10 + t)) under warm-up, D otherwise, in double; the kernel multiplies by
om = float32(1 - d_t), and so does the restatement; the update itself, e + om * (p - e), is taken in float64 from the
float32 inputs.

The bound per finite element is derived, not measured.  The kernel rounds the difference once (relative 2^-24) and the
fused multiply-add once (relative 2^-24 of the result); the device's double division may land one double ulp beside the
host's, which can move om by one float32 ulp (relative 2^-23 of om * |p - e|).  Together: at most
(2^-24 + 2^-23) * om * |p - e| + 2^-24 * |e_new| (1 + 2^-22), and the bound used is the next power-of-two envelope,

    2^-22 * om * |p - e|  +  2^-23 * |e_new|.

Non-finite results are compared by class and sign."""
import numpy as np
import torch


def decay_at(decay, t, warmup=True):
    """d_t, in double"""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def om32(decay, t, warmup=True):
    """1 - d_t formed in double, rounded once to the float32 the kernel multiplies by (returned as a Python float)"""
    return float(np.float32(1.0 - decay_at(decay, t, warmup)))


def update(ema, param, om):
    """float64 e + om * (p - e) from float32 (or float64) tensors"""
    e, p = ema.detach().double().cpu(), param.detach().double().cpu()
    return e + om * (p - e)


def bound(ema, param, new, om):
    e, p = ema.detach().double().cpu(), param.detach().double().cpu()
    return 2.0 ** -22 * om * (p - e).abs() + 2.0 ** -23 * new.abs()


def check(got, ema, param, om):
    """asserts the device's float32 result against the restatement fed with the device's previous average; returns the
    largest error / bound ratio over the finite elements (0 when the errors are all zero)"""
    new = update(ema, param, om)
    got = got.detach().double().cpu()
    assert got.shape == new.shape
    fin = torch.isfinite(new)
    assert torch.equal(torch.isfinite(got), fin), "finite / non-finite classes differ"
    assert torch.equal(torch.isnan(got), torch.isnan(new)), "NaN positions differ"
    inf = torch.isinf(new)
    assert torch.equal(got[inf], new[inf]), "infinities differ in sign"
    err = (got - new).abs()[fin]
    bnd = bound(ema, param, new, om)[fin]
    assert bool((err <= bnd).all()), "largest error %.3e at bound %.3e" % (
        float(err[(err - bnd).argmax()]), float(bnd[(err - bnd).argmax()]))
    nz = err > 0
    return float((err[nz] / bnd[nz]).max()) if bool(nz.any()) else 0.0
