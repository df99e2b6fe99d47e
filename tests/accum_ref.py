"""Host restatement of gradient accumulation (include/xv2.h xv2_grad_accumulate, csrc/optim.hip grad_accumulate_kernel).

Every mode is at most one IEEE fp32 addition per element, and a correctly rounded addition has one answer: torch's CPU fp32
`+` is that addition, so the device's result is compared with `same_bits`, never with a tolerance."""
import torch

OPEN, ADD, CLOSE = 0, 1, 2


def _f32(t):
    assert t.dtype == torch.float32 and t.device.type == "cpu"
    return t


def apply(mode, acc, grad):
    """(acc, grad) after one call of `mode` on CPU fp32 tensors; the inputs stay as they are"""
    acc, grad = _f32(acc), _f32(grad)
    if mode == OPEN:
        return grad.clone(), grad.clone()
    if mode == ADD:
        return acc + grad, grad.clone()
    if mode == CLOSE:
        return acc.clone(), acc + grad
    raise ValueError("mode %r" % (mode,))


def group_sum(gs):
    """((g1 + g2) + g3 ... ) + gm: the left-to-right fp32 sum of a group's micro-gradients (one tensor each)"""
    total = _f32(gs[0]).clone()
    for g in gs[1:]:
        total = total + _f32(g)
    return total


def same_bits(a, b):
    """equal int32 views wherever neither is NaN, and NaN in the same places (a NaN's payload is not pinned)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])
