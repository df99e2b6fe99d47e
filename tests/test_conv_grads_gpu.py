"""The host side of the convolution nodes (xview2_amd/ops.py): the one gradient tail `_conv_grads` that ConvBnActFn, ConvBnActHeadFn,
BottleneckTailFn and ConvFn end in, and the hand-off of the global average pool's column sums from bn0's apply pass to the
split-attention tail (`want_gap`), whose claim on the shared scratch must go stale when anything else is handed the scratch."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (N, H, W, C) of encoders.SplAtConv2d(C, C): the smallest shape of test_splat_fused_gpu.py's lists that can tell stale pool sums
# from fresh ones.  (1, 5, 7, 64) is smaller and takes the same launches, but with ONE row bn1 normalises every channel to zero and
# neither the output nor a gradient depends on the pool any more; (2, 16, 16, 64[, 32]) is the next.
SPLAT = (2, 16, 16, 64)


def _kernels(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, " ".join(e.key for e in prof.key_averages())


def _producer(blk, x, **kw):
    from xview2_amd import nn as xnn, ops
    return xnn.conv_bn_act(blk.conv, blk.bn0, x, act=ops.ACT_RELU, **kw)


def _tail(blk, z):
    """the second half of encoders.SplAtConv2d.forward"""
    from xview2_amd import nn as xnn, ops
    bn1, f1, f2 = blk.bn1, blk.fc1, blk.fc2
    xnn.bump_bn_counter(bn1)
    bs = ops.BnState(bn1, xnn.SYNC_BN)
    return ops.SplitAttentionFn.apply(z, f1.weight, f1.bias, bs.weight, bs.bias, f2.weight, f2.bias, bs, bn1.training)


def _results(blk, x, out, dy):
    """output, input gradient and every parameter gradient of one block after its backward"""
    from xview2_amd import ops
    out.backward(dy)
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    return [("out", out.detach()), ("x", x.grad)] + [(k, p.grad) for k, p in blk.named_parameters()]


@pytest.fixture(scope="module")
def splat():
    """blocks A and B of one shape with different weights and inputs; the reference is A(x) run on its own"""
    from xview2_amd import encoders
    N, H, W, C = SPLAT
    torch.manual_seed(11)
    A = encoders.SplAtConv2d(C, C, 1, 1).to(DEV).train()
    B = encoders.SplAtConv2d(C, C, 1, 1).to(DEV).train()
    x = torch.randn(N, H, W, C, device=DEV)
    xb = torch.randn(N, H, W, C, device=DEV) * 3 + 1
    dy = torch.randn(N, H, W, C, device=DEV)
    ref_blk = copy.deepcopy(A)
    xr = x.clone().requires_grad_(True)
    out, names = _kernels(lambda: ref_blk(xr))
    # the grouped layer call took the shape and its apply pass left the pool's sums: the tail ran no column-sum launch of its own
    assert "bn_act_colsum_kernel" in names and "splat_colsum_kernel" not in names, names
    return dict(A=A, B=B, x=x, xb=xb, dy=dy, ref=_results(ref_blk, xr, out, dy))


def _same_as_reference(got, ref):
    for (k, a), (kr, r) in zip(got, ref):
        assert k == kr and a is not None and r is not None, (k, kr)
        assert torch.equal(a, r), (k, float((a.float() - r.float()).abs().max()))


@pytest.mark.parametrize("between", ["forward", "backward"])
def test_pool_sums_of_another_block_in_between_are_not_consumed(splat, between):
    """A's conv + bn0 + ReLU with want_gap, then a whole B(xb) (or B's backward) that uses the same scratch, then A's tail: A's
    output and gradients are bit for bit those of A run on its own - the tail saw that its claim was stale and took the sums
    again (the trace names the column-sum launch)"""
    A, B = copy.deepcopy(splat["A"]), copy.deepcopy(splat["B"])
    x = splat["x"].clone().requires_grad_(True)
    xb = splat["xb"].clone().requires_grad_(True)
    if between == "backward":
        yb = B(xb)
    z = _producer(A, x, want_gap=True)
    assert getattr(z, "_xv2_gap_part", None) is not None
    if between == "forward":
        B(xb)
    else:
        yb.backward(torch.ones_like(yb))
    out, names = _kernels(lambda: _tail(A, z))
    assert "splat_colsum_kernel" in names, names
    _same_as_reference(_results(A, x, out, splat["dy"]), splat["ref"])


def test_undisturbed_hand_off_and_no_request(splat):
    """producer and tail back to back: the claim holds (no column-sum launch).  Without the keyword the producer leaves no claim
    on its output, the tail takes the sums itself, and the result is bit for bit the claimed one"""
    A = copy.deepcopy(splat["A"])
    x = splat["x"].clone().requires_grad_(True)
    z = _producer(A, x, want_gap=True)
    out, names = _kernels(lambda: _tail(A, z))
    assert "splat_colsum_kernel" not in names, names
    _same_as_reference(_results(A, x, out, splat["dy"]), splat["ref"])
    A2 = copy.deepcopy(splat["A"])
    x2 = splat["x"].clone().requires_grad_(True)
    z2 = _producer(A2, x2)
    assert getattr(z2, "_xv2_gap_part", None) is None
    out2, names2 = _kernels(lambda: _tail(A2, z2))
    assert "splat_colsum_kernel" in names2, names2
    _same_as_reference(_results(A2, x2, out2, splat["dy"]), splat["ref"])


# ------------------------------------------------------------------------------------------------
# pass-through gradients through _conv_grads, 3x3 stride-1 layer.  The kernels take channel counts in multiples of 32 only (N = 2,
# 9 x 7 pixels, C0 = 24 + C1 = 8 -> 32 is refused before any launch), so the shape is the smallest 3x3 / stride-1 two-source one
# of test_conv_variants_gpu.py, its case "bf16s-fwd-stats-dual": N = 2, 7 x 9 pixels, C0 = 64 (+ C1 = 32), Cout = 64 - 126 rows,
# no multiple of a tile.  The one-source and the grouped case drop C1.
PT_SHAPE = (2, 7, 9, 64, 32, 64)      # N, H, W, C0, C1, Cout
PT_CASES = {"one_source_epilogue": (False, 1, 1), "grouped_added_afterwards": (False, 2, 1), "two_sources": (True, 1, 3)}      # second source, groups, passthrough


def _pt_layer(two, groups, dtype):
    N, H, W, C0, C1, Co = PT_SHAPE
    C1 = C1 if two else 0
    g = torch.Generator().manual_seed(100 * C1 + groups)
    t = lambda *s: torch.randn(*s, generator=g)
    d = dict(w=t(Co, (C0 + C1) // groups, 3, 3) * 0.1, gamma=torch.rand(Co, generator=g) + 0.5, beta=t(Co) * 0.2,
             x0=t(N, H, W, C0).to(dtype), m0=t(N, H, W, C0).to(dtype), gz=t(N, H, W, Co).to(dtype), gr0=t(N, H, W, C0).to(dtype))
    if C1:
        d.update(x1=t(N, H, W, C1).to(dtype), c1=t(N, H, W, C1).to(dtype), gr1=t(N, H, W, C1).to(dtype))
    return d


def _pt_fp64(d, groups):
    """the same graph in fp64 PyTorch: z = relu(BN(conv(cat(x0, x1)))), r0 = x0 * m0, r1 = relu(x1 + c1)"""
    nchw = lambda k: d[k].double().permute(0, 3, 1, 2)
    x0 = nchw("x0").clone().requires_grad_(True)
    xs, outs, gs = [x0], [x0 * nchw("m0")], [nchw("gr0")]
    if "x1" in d:
        x1 = nchw("x1").clone().requires_grad_(True)
        xs.append(x1)
        outs.append(torch.relu(x1 + nchw("c1")))
        gs.append(nchw("gr1"))
    y = F.conv2d(torch.cat(xs, 1), d["w"].double(), padding=1, groups=groups)
    z = torch.relu(F.batch_norm(y, None, None, d["gamma"].double(), d["beta"].double(), True, 0.1, 1e-5))
    torch.autograd.backward([z] + outs, [nchw("gz")] + gs)
    return [x.grad.permute(0, 2, 3, 1) for x in xs]


def _pt_hip(d, groups, passthrough):
    """the layer on the GPU; passthrough = 0: the second consumers read the sources themselves and autograd sums the gradients"""
    from xview2_amd import nn as xnn, ops
    cin = d["w"].shape[1] * groups
    conv = torch.nn.Conv2d(cin, d["w"].shape[0], 3, 1, 1, groups=groups, bias=False)
    bn = torch.nn.BatchNorm2d(d["w"].shape[0])
    with torch.no_grad():
        conv.weight.copy_(d["w"])
        bn.weight.copy_(d["gamma"])
        bn.bias.copy_(d["beta"])
    conv.to(DEV)
    bn.to(DEV).train()
    dev = {k: v.to(DEV) for k, v in d.items()}
    x0 = dev["x0"].clone().requires_grad_(True)
    x1 = dev["x1"].clone().requires_grad_(True) if "x1" in d else None
    out = xnn.conv_bn_act(conv, bn, x0, x1, act=ops.ACT_RELU, passthrough=passthrough)
    if passthrough == 3:
        z, a0, a1 = out
    elif passthrough == 1:
        (z, a0), a1 = out, x1
    else:
        z, a0, a1 = out, x0, x1
    outs, gs = [z, a0 * dev["m0"]], [dev["gz"], dev["gr0"]]
    if x1 is not None:
        outs.append(ops.AddReluFn.apply(a1, dev["c1"]))
        gs.append(dev["gr1"])
    torch.autograd.backward(outs, gs)
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    return [x.grad.double().cpu() for x in (x0, x1) if x is not None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(PT_CASES))
def test_pass_through_gradients_against_fp64(case, dtype):
    """every input gradient of a layer whose sources' aliases feed a second consumer (a multiply for x0, AddReluFn for x1), against
    the same graph in fp64.  Gate: max |error| of the aliased run <= 2 x that of the same layer without passthrough (autograd sums
    the two gradients) + one unit in the last place of the storage type at the gradient's maximum (2^-23 / 2^-7 of it) - the
    factor covers the one rounding the epilogue sum saves or spends.
    Measured max |error| aliased / plain (max |gradient|); the layer-level call takes all three shapes:
      one source, epilogue   fp32 dx0 6.791e-07 / 6.791e-07 (6.78)   bf16 dx0 1.032e-01 / 1.012e-01 (6.82)
      groups = 2, afterwards fp32 dx0 1.146e-06 / 1.146e-06 (7.59)   bf16 dx0 2.776e-01 / 2.776e-01 (7.60)
      two sources            fp32 dx0 9.766e-07 / 9.766e-07 (7.94)   bf16 dx0 1.165e-01 / 1.165e-01 (7.92)
                             fp32 dx1 1.080e-06 / 1.080e-06 (3.99)   bf16 dx1 1.111e-01 / 1.111e-01 (3.99)
    (the bf16 figures are single elements whose ReLU mask differs from fp64's after y was rounded to bf16 - in both runs alike)"""
    two, groups, passthrough = PT_CASES[case]
    d = _pt_layer(two, groups, dtype)
    ref = _pt_fp64(d, groups)
    plain = _pt_hip(d, groups, 0)
    alias = _pt_hip(d, groups, passthrough)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -23
    for i, (r, p, a) in enumerate(zip(ref, plain, alias)):
        e_plain, e_alias, top = float((p - r).abs().max()), float((a - r).abs().max()), float(r.abs().max())
        print("%s %s dx%d: aliased %.3e plain %.3e max |grad| %.3e" % (case, dtype, i, e_alias, e_plain, top))
        assert e_alias <= 2 * e_plain + ulp * top, (case, i, e_alias, e_plain, top)


def test_conv_fn_tells_its_kernels_no_maxima(monkeypatch):
    """ConvFn records no maxima in forward; its backward must not hand the kernels any either, even when the gradient it is
    given carries a live token"""
    from xview2_amd import ops
    monkeypatch.setattr(ops, "F16X2", True)
    monkeypatch.setattr(ops, "MATH_MODE", ops.MATH_F32X3)
    torch.manual_seed(2)
    x = torch.randn(2, 7, 9, 64, device=DEV).requires_grad_(True)
    w = (torch.randn(64, 64, 3, 3, device=DEV) * 0.1).requires_grad_(True)
    assert ops._amax_active(x)
    tok = ops._amax_new(x)
    arrived = []

    class Tag(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y):
            return y.view_as(y)

        @staticmethod
        def backward(ctx, dy):
            dy = dy.clone()
            dy._xv2_amax = tok
            return dy

    real_data, calls = ops._conv_backward_data, []

    def backward_data(dy, *args, **kw):
        arrived.append(ops._amax_ptr(dy))
        return real_data(dy, *args, **kw)

    y = Tag.apply(ops.ConvFn.apply(x, None, w, None, ops.conv_cfg(3, 3, 1, 1)))
    gy = torch.randn_like(y)
    monkeypatch.setattr(ops, "_conv_backward_data", backward_data)
    monkeypatch.setattr(ops, "set_amax", lambda *a: calls.append(a))      # (only Tag's and ConvFn's backward run under it)
    y.backward(gy)
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    assert arrived == [tok[0]]          # the gradient reached the node with its token alive
    assert calls == []
    assert x.grad is not None and w.grad is not None
