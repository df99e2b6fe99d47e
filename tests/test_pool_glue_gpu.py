"""The pooling, resampling and glue kernels (csrc/pool.hip; the elementwise, gate and layout kernels of csrc/pointwise.hip)
against the float64 restatement and the derived per-element bounds of tests/pool_ref.py: every case table of that module in
fp32 and, where the kernel is templated on the storage type, with bf16 storage; the accumulate-in-place backward of the
pooling nodes with its fallbacks; the strided operands of the C ABI; NaN in a max-pool window; one case per kernel family that
runs the grid-stride loop into a second sweep.  Outputs the test owns are filled with NaN before the call; results of the
autograd nodes are computed twice, the second time after the allocator's free lists were filled with a NaN pattern, and must
agree bit for bit.  Every comparison prints its error / bound ratio ("pool_ref ratio <operation> <ratio>")."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import pool_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
N, C = R.N_C
NAN_BITS = 0x7fc07fc0      # NaN as fp32 and as a pair of bf16
GRID_CAP = 8192 * 256      # grid_for(): blocks x threads, one four-channel item (or one element) per thread and sweep
RATIOS = {}


def _ops():
    from xview2_amd import ops
    return ops


def _call(*a):
    from xview2_amd._capi import call
    return call(*a)


def _ptr(t, off):
    from xview2_amd._capi import Ptr
    return Ptr(t, off)


def _gen(*key):
    return torch.Generator().manual_seed(7000003 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _ln(shape, g, dt=torch.float32):
    """log-normal values rounded to the storage type (the reference sees the rounded values)"""
    return R.lognormal(tuple(shape), g).to(dt)


def _nan(shape, dt=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dt, device=DEV)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _poison_free_lists(nbytes=0):
    """fill the caching allocator's free lists with NaN: the next torch.empty of a node starts
    out as the pattern, so an element its kernel does not write shows"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    sizes = [1 << 14] * 128 + [1 << 20] * 4 + [(nbytes + 3) // 4] * (2 if nbytes else 0)
    blocks = [torch.empty(n, dtype=torch.int32, device=DEV).fill_(NAN_BITS) for n in sizes]
    torch.cuda.synchronize()
    del blocks


@pytest.fixture(scope="module", autouse=True)
def _release_poisoned_blocks():
    """hand the NaN-filled cached blocks back to the driver when the module is done"""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _twice(run, nbytes=0):
    """run() -> tensors; once, then once more over poisoned free lists: the same bits"""
    first = [t.detach().clone() for t in run()]
    _poison_free_lists(nbytes)
    second = [t.detach() for t in run()]
    for i, (a, b) in enumerate(zip(first, second)):
        assert _same_bits(a, b), "result %d changes with the contents of unwritten memory" % i
    return second


def _ok(op, y, y64, bound, what=""):
    r, where = R.check(y, y64, bound)
    RATIOS[op] = max(RATIOS.get(op, 0.0), r)
    print("pool_ref ratio %s %.4f %s" % (op, r, what))
    assert r <= 1.0, "%s %s: error / bound %.3f at flat index %d" % (op, what, r, where)


def _exact(y, want, what):
    """bit-exact against values computed from the inputs: same dtype, same numbers (NaN nowhere)"""
    y = y.detach().cpu()
    assert y.dtype == want.dtype and y.shape == want.shape, (what, y.dtype, want.dtype, y.shape, want.shape)
    assert torch.equal(y, want), "%s: not bit-exact (%d elements differ)" % (what, int((y != want).sum()))


def _sfx(dt):
    return "_bf16" if dt == torch.bfloat16 else ""


# ---- the accumulate-in-place backward of the pooling nodes ---------------------------------------------------------------

def _passthrough(apply, x, dy, dp, mode):
    """loss = (y * dy).sum() + (alias * dp).sum() through a node with passthrough=True -> x.grad, was dp contiguous"""
    a = x.to(DEV).requires_grad_(True)
    y, alias = apply(a)
    seen = []
    alias.register_hook(lambda g: seen.append(g.is_contiguous()))
    if mode == "inplace":
        loss = (y * dy.to(DEV)).sum() + (alias * dp.to(DEV)).sum()
    elif mode == "fallback":      # the alias's gradient arrives as a permuted view of an NCHW tensor
        loss = (y * dy.to(DEV)).sum() + (alias.permute(0, 3, 1, 2) * dp.permute(0, 3, 1, 2).contiguous().to(DEV)).sum()
    else:                         # only the alias is used: dy is None
        loss = (alias * dp.to(DEV)).sum()
    loss.backward()
    return a.grad, seen


def _check_passthrough(op, apply, x, dy, dp, g64, base, a, T, dt):
    """g64 = f^T(dy) with its bound `base`, scale `a` and window count T"""
    bf16 = dt == torch.bfloat16
    shape = tuple(x.shape)
    nchw_view_contig = torch.empty(shape[0], shape[3], shape[1], shape[2]).permute(0, 2, 3, 1).is_contiguous()
    for mode in ("inplace", "fallback", "alias"):
        seen = None

        def run():
            nonlocal seen
            dx, seen = _passthrough(apply, x, dy, dp, mode)
            return (dx,)
        (dx,) = _twice(run)
        assert dx.dtype == dt
        if mode == "alias":
            _exact(dx, dp, "%s passthrough, alias only" % op)
            continue
        in_place = mode == "inplace" or nchw_view_contig
        assert seen == [in_place], (op, mode, seen)
        ref = dp.double() + g64
        bound = R.accumulated(base, a, dp, T if in_place else 1, ref, bf16=bf16, fallback=not in_place)
        _ok("%s_acc%s" % (op, _sfx(dt)), dx, ref, bound, "%s %s" % (shape, mode))


# ---- max-pool -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ties", [False, True], ids=["lognormal", "ties"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool(shape, dt, ties):
    ops = _ops()
    g = _gen(*shape, ties)
    x = R.tie_heavy(shape, g, dt) if ties else _ln(shape, g, dt)
    y64 = R.maxpool3x3s2_fwd(x)
    dy = _ln(y64.shape, g, dt)

    def run():
        a = x.to(DEV).requires_grad_(True)
        y = ops.MaxPool3x3s2Fn.apply(a)
        y.backward(dy.to(DEV))
        return y, a.grad
    y, dx = _twice(run)
    _exact(y, y64.to(dt), "max-pool forward %s" % (shape,))
    assert torch.equal(y.cpu().double(), y64)
    bound, a, T = R.maxpool_bwd_bound(x, dy)
    dx64 = R.maxpool3x3s2_bwd(x, dy)
    _ok("maxpool_bwd" + _sfx(dt), dx, dx64, R.stored(bound, dx64, dt == torch.bfloat16), "%s ties=%s" % (shape, ties))
    dp = _ln(shape, g, dt)
    _check_passthrough("maxpool", lambda t: ops.MaxPool3x3s2Fn.apply(t, True), x, dy, dp, dx64, bound, a, T, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_maxpool_nan_wins_and_takes_the_gradient(dt):
    """torch: (val > maxval) || isnan(val).  Channel 0: 5.0 at (0, 0) and NaN at (1, 1), the LAST valid tap of output (0, 0);
    channel 1: NaN at (0, 0), the first tap.  Forward and gradient routing as torch's."""
    ops = _ops()
    g = _gen(4, 4)
    x = _ln((1, 4, 4, 4), g, dt)
    x[0, 0, 0, 0], x[0, 1, 1, 0] = 5.0, float("nan")
    x[0, 0, 0, 1] = float("nan")
    y64 = R.maxpool3x3s2_fwd(x)
    assert bool(y64[0, :, :, 0].isnan().all()) and bool(y64[0, 0, 0, 1].isnan()) and int(y64.isnan().sum()) == 5
    dy = _ln(y64.shape, g, dt)
    a = x.to(DEV).requires_grad_(True)
    y = ops.MaxPool3x3s2Fn.apply(a)
    y.backward(dy.to(DEV))
    y = y.detach().cpu().double()
    assert torch.equal(y.isnan(), y64.isnan()), "NaN outputs: kernel %s, torch %s" % (y.isnan().nonzero().tolist(), y64.isnan().nonzero().tolist())
    assert torch.equal(y.nan_to_num(0.0), y64.nan_to_num(0.0))
    bound, _, _ = R.maxpool_bwd_bound(x, dy)
    dx64 = R.maxpool3x3s2_bwd(x, dy)
    assert abs(float(dx64[0, 1, 1, 0]) - float(dy[0, :, :, 0].double().sum())) < 1e-12 and float(dx64[0, 0, 0, 1]) == float(dy[0, 0, 0, 1])
    _ok("maxpool_bwd" + _sfx(dt), a.grad, dx64, R.stored(bound, dx64, dt == torch.bfloat16), "NaN routing")


# ---- avg-pool -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.avg_cases(), ids=lambda c: "k%ds%dp%d%s%s_%dx%d" % (c[0], c[1], c[2], "c" if c[3] else "f", "i" if c[4] else "x", c[5], c[6]))
def test_avgpool(case, dt):
    ops = _ops()
    k, s, pad, ceil, incl, H, W = case
    bf16 = dt == torch.bfloat16
    g = _gen(*case)
    x = _ln((N, H, W, C), g, dt)
    y64 = R.avgpool_fwd(x, k, s, pad, ceil, incl)
    dy = _ln(y64.shape, g, dt)

    def run():
        a = x.to(DEV).requires_grad_(True)
        y = ops.AvgPoolFn.apply(a, k, s, pad, ceil, incl)
        y.backward(dy.to(DEV))
        return y, a.grad
    y, dx = _twice(run)
    assert y.dtype == dt and dx.dtype == dt
    _ok("avgpool_fwd" + _sfx(dt), y, y64, R.stored(R.avgpool_fwd_bound(x, k, s, pad, ceil, incl), y64, bf16), str(case))
    bound, a, T = R.avgpool_bwd_bound(dy, (H, W), k, s, pad, ceil, incl)
    dx64 = R.avgpool_bwd(dy, (H, W), k, s, pad, ceil, incl)
    _ok("avgpool_bwd" + _sfx(dt), dx, dx64, R.stored(bound, dx64, bf16), str(case))
    dp = _ln((N, H, W, C), g, dt)
    _check_passthrough("avgpool", lambda t: ops.AvgPoolFn.apply(t, k, s, pad, ceil, incl, True), x, dy, dp, dx64, bound, a, T, dt)


# ---- adaptive avg-pool --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", R.ADAPTIVE_BINS)
@pytest.mark.parametrize("hw", R.ADAPTIVE_HW, ids=lambda s: "%dx%d" % s)
def test_adaptive_avgpool(hw, bins):
    ops = _ops()
    H, W = hw
    g = _gen(H, W, bins)
    x = _ln((N, H, W, C), g)
    y64 = R.adaptive_fwd(x, bins)
    dy = _ln(y64.shape, g)
    fb = R.adaptive_fwd_bound(x, bins)
    bb, a = R.adaptive_bwd_bound(dy, hw, bins)
    dx64 = R.adaptive_bwd(dy, hw, bins)

    def run():
        t = x.to(DEV).requires_grad_(True)
        y = ops.AdaptiveAvgPoolFn.apply(t, bins)
        y.backward(dy.to(DEV))
        return y, t.grad
    y, dx = _twice(run)
    _ok("adaptive_fwd", y, y64, fb, "%s bins %d" % (hw, bins))
    _ok("adaptive_bwd", dx, dx64, bb, "%s bins %d" % (hw, bins))
    # the input as the upper channel half of a wider tensor whose lower half is NaN: ldx = 2C, pointer offset C
    wide = _nan((N, H, W, 2 * C))
    wide[..., C:] = x.to(DEV)
    y = _nan((N, bins, bins, C))
    _call("xv2_adaptive_avgpool_forward", _ptr(wide, C), 2 * C, N, H, W, C, bins, y)
    _ok("adaptive_fwd", y, y64, fb, "%s bins %d ldx" % (hw, bins))
    # backward into the upper half of a wider gradient: overwrite (NaN before), then accumulate; the lower half keeps its bits
    old = _ln((N, H, W, 2 * C), g)
    dyd = dy.to(DEV)
    wide = _nan((N, H, W, 2 * C))
    _call("xv2_adaptive_avgpool_backward", dyd, N, H, W, C, bins, _ptr(wide, C), 2 * C, 0)
    assert bool(wide[..., :C].isnan().all()), "adaptive backward wrote outside its channel slice"
    _ok("adaptive_bwd", wide[..., C:], dx64, bb, "%s bins %d lddx" % (hw, bins))
    wide = old.to(DEV)
    _call("xv2_adaptive_avgpool_backward", dyd, N, H, W, C, bins, _ptr(wide, C), 2 * C, 1)
    _exact(wide[..., :C], old[..., :C].contiguous(), "adaptive backward, channels outside the slice")
    ref = old[..., C:].double() + dx64
    _ok("adaptive_bwd_acc", wide[..., C:], ref, R.accumulated(bb, a, old[..., C:], 1, ref), "%s bins %d" % (hw, bins))


# ---- bilinear -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.BILINEAR_CASES, ids=lambda c: "%dx%d_to_%dx%d" % c)
def test_bilinear(case):
    ops = _ops()
    IH, IW, OH, OW = case
    g = _gen(*case)
    x = _ln((N, IH, IW, C), g)
    dy = _ln((N, OH, OW, C), g)
    y64 = R.bilinear_fwd(x, OH, OW)
    fb = R.bilinear_fwd_bound(x, OH, OW)
    bb, _ = R.bilinear_bwd_bound(dy, IH, IW)
    dx64 = R.bilinear_bwd(dy, IH, IW)

    def run():
        t = x.to(DEV).requires_grad_(True)
        y = ops.BilinearFn.apply(t, OH, OW)
        y.backward(dy.to(DEV))
        return y, t.grad
    y, dx = _twice(run)
    if (IH, IW) == (OH, OW):
        _exact(y, x, "bilinear identity")
        _exact(dx, dy, "bilinear identity backward")
    _ok("bilinear_fwd", y, y64, fb, str(case))
    _ok("bilinear_bwd", dx, dx64, bb, str(case))
    # forward into, backward out of, the upper channel half of a wider tensor (ldy = lddy = 2C, offset C)
    wide = _nan((N, OH, OW, 2 * C))
    _call("xv2_bilinear_forward", x.to(DEV), N, IH, IW, C, OH, OW, _ptr(wide, C), 2 * C)
    assert bool(wide[..., :C].isnan().all()), "bilinear forward wrote outside its channel slice"
    _ok("bilinear_fwd", wide[..., C:], y64, fb, "%s ldy" % (case,))
    wide[..., C:] = dy.to(DEV)
    dx = _nan((N, IH, IW, C))
    _call("xv2_bilinear_backward", _ptr(wide, C), 2 * C, N, IH, IW, C, OH, OW, dx)
    _ok("bilinear_bwd", dx, dx64, bb, "%s lddy" % (case,))


# ---- gate-mul -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cg", R.GATE_C)
def test_gate_mul(Cg, dt):
    ops = _ops()
    bf16 = dt == torch.bfloat16
    g = _gen(Cg)
    shape = R.GATE_PIX + (Cg,)
    npix = shape[0] * shape[1] * shape[2]
    skip, dout = _ln(shape, g, dt), _ln(shape, g, dt)
    gate = torch.rand(R.GATE_PIX + (1,), generator=g)
    out64, dskip64, dgate64, scale = R.gate_mul(skip, gate, dout)
    ob, sb, gb = R.stored(R.U * out64.abs(), out64, bf16), R.stored(R.U * dskip64.abs(), dskip64, bf16), R.gate_dgate_bound(Cg, scale)

    def run():
        s, t = skip.to(DEV).requires_grad_(True), gate.to(DEV).requires_grad_(True)
        out = ops.GateMulFn.apply(s, t)
        out.backward(dout.to(DEV))
        return out, s.grad, t.grad
    out, dskip, dgate = _twice(run)
    assert out.dtype == dt and dskip.dtype == dt and dgate.dtype == torch.float32
    _ok("gate_out" + _sfx(dt), out, out64, ob, "C=%d" % Cg)
    _ok("gate_dskip" + _sfx(dt), dskip, dskip64, sb, "C=%d" % Cg)
    _ok("gate_dgate" + _sfx(dt), dgate, dgate64, gb, "C=%d" % Cg)
    # skip as the upper channel half of a wider tensor whose lower half is NaN: lds = 2C
    wide = _nan(R.GATE_PIX + (2 * Cg,), dt)
    wide[..., Cg:] = skip.to(DEV)
    gd, dd = gate.to(DEV), dout.to(DEV)
    out, dskip, dgate = _nan(shape, dt), _nan(shape, dt), _nan(R.GATE_PIX + (1,))
    _call("xv2_gate_mul_forward", _ptr(wide, Cg), 2 * Cg, gd, out, npix, Cg, ops._dt(wide))
    _call("xv2_gate_mul_backward", _ptr(wide, Cg), 2 * Cg, gd, dd, dskip, dgate, npix, Cg, ops._dt(wide))
    _ok("gate_out" + _sfx(dt), out, out64, ob, "C=%d lds" % Cg)
    _ok("gate_dskip" + _sfx(dt), dskip, dskip64, sb, "C=%d lds" % Cg)
    _ok("gate_dgate" + _sfx(dt), dgate, dgate64, gb, "C=%d lds" % Cg)


# ---- add-relu, axpby ----------------------------------------------------------------------------------------------------

def _add_relu_inputs(n, g, dt):
    a, b = _ln((1, 1, n // 4, 4), g, dt).reshape(n), _ln((1, 1, n // 4, 4), g, dt).reshape(n)
    b[::5] = -a[::5]          # exact cancellation
    a[1::7] = 0.0
    b[1::7] = 0.0
    a[2::11] = 0.0            # one operand zero
    return a, b


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [4, 1020, 4096])
def test_add_relu(n, dt):
    ops = _ops()
    g = _gen(n)
    a, b = _add_relu_inputs(n, g, dt)
    dr = _ln((1, 1, n // 4, 4), g, dt).reshape(n)
    r64 = R.add_relu(a, b)
    assert int((r64 == 0).sum()) >= n // 5

    def run():
        s, t = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        r = ops.AddReluFn.apply(s, t)
        r.backward(dr.to(DEV))
        return r, s.grad, t.grad
    r, da, db = _twice(run)
    _exact(r, r64.to(dt), "add-relu n=%d" % n)
    want = R.add_relu_bwd(r64, dr).to(dt)      # mask on r > 0
    _exact(da, want, "add-relu da")
    _exact(db, want, "add-relu db")


@pytest.mark.parametrize("coef", [(1.0, 1.0), (0.5, -2.0)])
def test_axpby(coef):
    alpha, beta = coef
    g = _gen(11)
    n = 1020
    a, b = _ln((1, 1, n // 4, 4), g).reshape(n), _ln((1, 1, n // 4, 4), g).reshape(n)
    ad, bd = a.to(DEV), b.to(DEV)
    for (bb, alias) in ((bd, False), (None, False), (bd, True)):
        out = ad.clone() if alias else _nan((n,))
        _call("xv2_axpby", alpha, out if alias else ad, beta, bb, out, n)
        ref, bound = R.axpby(alpha, a, beta, b if bb is not None else None)
        _ok("axpby", out, ref, bound, "alpha %g beta %g b %s alias %s" % (alpha, beta, bb is not None, alias))
        if bb is None and alpha == 1.0:
            _exact(out, a, "axpby copy")
    assert _same_bits(ad, a.to(DEV)) and _same_bits(bd, b.to(DEV))


# ---- layout and channel copies ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c_pad", [None, 4, 8])
def test_nchw_to_nhwc_of_a_channel_slice(c_pad):
    ops = _ops()
    g = _gen(3, c_pad or 0)
    wide = torch.randn(2, 6, 7, 5, generator=g)
    xd = wide.to(DEV)[:, 1:4]      # channels 1..3 of six: batch stride 6 H W
    assert not xd.is_contiguous()
    (y,) = _twice(lambda: (ops.nchw_to_nhwc(xd, c_pad),))
    Cp = 3 if c_pad is None else c_pad
    want = torch.zeros(2, 7, 5, Cp)
    want[..., :3] = wide[:, 1:4].permute(0, 2, 3, 1)
    _exact(y, want, "nchw_to_nhwc c_pad=%s" % c_pad)


def test_nchw_pair_and_nhwc_to_nchw():
    ops = _ops()
    g = _gen(5)
    x = torch.randn(3, 6, 5, 9, generator=g)
    (y,) = _twice(lambda: (ops.nchw_pair_to_nhwc(x.to(DEV)),))
    want = torch.zeros(6, 5, 9, 4)
    want[:3, ..., :3] = x[:, :3].permute(0, 2, 3, 1)
    want[3:, ..., :3] = x[:, 3:].permute(0, 2, 3, 1)
    _exact(y, want, "nchw_pair_to_nhwc")
    t = _ln((2, 5, 9, 12), g)
    (z,) = _twice(lambda: (ops.nhwc_to_nchw(t.to(DEV)),))
    _exact(z, t.permute(0, 3, 1, 2).contiguous(), "nhwc_to_nchw")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cs", [[4], [32, 32], [8, 4, 64]], ids=lambda c: "+".join(map(str, c)))
def test_cat_channels_and_pair_cat(cs, dt):
    ops = _ops()
    g = _gen(*cs)
    xs = [_ln((2, 5, 7, c), g, dt) for c in cs]
    d = _ln((2, 5, 7, sum(cs)), g, dt)

    def run():
        ts = [t.to(DEV).requires_grad_(True) for t in xs]
        out = ops.CatChannelsFn.apply(*ts)
        out.backward(d.to(DEV))
        return [out] + [t.grad for t in ts]
    res = _twice(run)
    _exact(res[0], R.cat_channels(xs).to(dt), "CatChannelsFn %s" % cs)      # (bf16 -> float64 -> bf16 is the identity)
    for got, want in zip(res[1:], R.split_channels(d, cs)):
        _exact(got, want.to(dt), "CatChannelsFn backward %s" % cs)
    # PairCatFn: [2B, H, W, C] -> [B, H, W, 2C], every width of the list
    for c in cs:
        t = _ln((4, 5, 7, c), g, dt)
        dd = _ln((2, 5, 7, 2 * c), g, dt)

        def run2():
            td = t.to(DEV).requires_grad_(True)
            out = ops.PairCatFn.apply(td)
            out.backward(dd.to(DEV))
            return out, td.grad
        out, dtg = _twice(run2)
        _exact(out, R.pair_cat(t).to(dt), "PairCatFn C=%d" % c)
        _exact(dtg, R.pair_split(dd).to(dt), "PairCatFn backward C=%d" % c)


def test_copy_channels_bf16_with_offsets_keeps_the_neighbours():
    """8 channels from offset 4 of a 16-wide bf16 source into offset 8 of a 24-wide destination"""
    ops = _ops()
    g = _gen(16, 24)
    src = _ln((2, 5, 7, 16), g, torch.bfloat16)
    dst = _nan((2, 5, 7, 24), torch.bfloat16)
    _call("xv2_copy_channels", _ptr(src.to(DEV), 4), 16, _ptr(dst, 8), 24, 70, 8, ops.XV2_BF16)
    _exact(dst[..., 8:16], src[..., 4:12].contiguous(), "copy_channels bf16")
    assert bool(dst[..., :8].isnan().all()) and bool(dst[..., 16:].isnan().all()), "copy_channels wrote outside its slice"


def test_channel_counts_off_a_multiple_of_four_are_argument_errors():
    """the ABI's argument error, no launch: the NaN-filled outputs keep their bits"""
    ops = _ops()
    x = torch.ones(1, 4, 4, 6, device=DEV)
    y, idx = _nan((1, 4, 4, 6)), torch.full((1, 4, 4, 6), 0x55, dtype=torch.uint8, device=DEV)
    gate = torch.ones(16, device=DEV)
    calls = [
        ("xv2_maxpool3x3s2_forward", x, 1, 4, 4, 6, y, idx, 0),
        ("xv2_maxpool3x3s2_backward", x, idx, 1, 4, 4, 6, y, 0, 0),
        ("xv2_avgpool_forward", x, 1, 4, 4, 6, 1, 1, 0, 0, 4, 4, y, 0),
        ("xv2_avgpool_backward", x, 1, 4, 4, 6, 1, 1, 0, 0, 4, 4, y, 0, 0),
        ("xv2_adaptive_avgpool_forward", x, 6, 1, 4, 4, 6, 2, y),
        ("xv2_adaptive_avgpool_backward", x, 1, 4, 4, 6, 2, y, 6, 0),
        ("xv2_bilinear_forward", x, 1, 4, 4, 6, 4, 4, y, 6),
        ("xv2_bilinear_backward", x, 6, 1, 4, 4, 6, 4, 4, y),
        ("xv2_gate_mul_forward", x, 6, gate, y, 16, 6, 0),
        ("xv2_gate_mul_backward", x, 6, gate, x, y, y, 16, 6, 0),
        ("xv2_copy_channels", x, 6, y, 6, 16, 6, 0),
        ("xv2_add_relu_forward", x, x, y, 6, 0),
        ("xv2_add_relu_backward", x, x, y, 6, 0),
        ("xv2_axpby", 1.0, x, 1.0, x, y, 6),
    ]
    for c in calls:
        with pytest.raises(RuntimeError, match="multiple"):
            _call(*c)
    torch.cuda.synchronize()
    assert bool(y.isnan().all()) and bool((idx == 0x55).all())


# ---- grid-stride: item count = the grid cap plus a partial second sweep -------------------------------------------------

BIG = (1, 520, 520, 32)
BIG_BYTES = 520 * 520 * 32 * 4


@functools.lru_cache(maxsize=None)
def _big():
    """x, dy of the grid-stride cases (made once; never modified)"""
    g = _gen(520)
    return _ln(BIG, g), _ln(BIG, g)


def _sweeps(items):
    assert items > GRID_CAP and items % GRID_CAP != 0, "no partial second sweep any more: %d items, %d per sweep" % (items, GRID_CAP)


def test_grid_stride_avgpool_1x1():
    ops = _ops()
    x, dy = _big()
    _sweeps(x.numel() // 4)

    def run():
        a = x.to(DEV).requires_grad_(True)
        y = ops.AvgPoolFn.apply(a, 1, 1, 0, True, False)
        y.backward(dy.to(DEV))
        return y, a.grad
    y, dx = _twice(run, BIG_BYTES)
    _ok("avgpool_fwd", y, x.double(), R.U * 2 * x.double().abs(), "520x520x32")
    _ok("avgpool_bwd", dx, dy.double(), R.U * 3 * dy.double().abs(), "520x520x32")
    _exact(y, x, "avg-pool 1x1 is the identity")


def test_grid_stride_maxpool_backward():
    ops = _ops()
    x, _ = _big()
    _sweeps(x.numel() // 4)
    y64 = R.maxpool3x3s2_fwd(x)
    dy = _big()[1][:, :260, :260].contiguous()

    def run():
        a = x.to(DEV).requires_grad_(True)
        y = ops.MaxPool3x3s2Fn.apply(a)
        y.backward(dy.to(DEV))
        return y, a.grad
    y, dx = _twice(run, BIG_BYTES)
    assert torch.equal(y.cpu().double(), y64)
    bound, _, _ = R.maxpool_bwd_bound(x, dy)
    _ok("maxpool_bwd", dx, R.maxpool3x3s2_bwd(x, dy), bound, "520x520x32")


def test_grid_stride_maxpool_forward():
    ops = _ops()
    shape = (1, 1040, 1040, 32)
    _sweeps(520 * 520 * 32 // 4)
    x = _ln(shape, _gen(1040))
    (y,) = _twice(lambda: (ops.MaxPool3x3s2Fn.apply(x.to(DEV)),), BIG_BYTES)
    _exact(y, R.nhwc(F.max_pool2d(R.nchw(x), 3, 2, 1)).contiguous(), "max-pool forward 1040x1040x32")      # exact in any precision


def test_grid_stride_add_relu():
    ops = _ops()
    x, dy = _big()
    _sweeps(x.numel() // 4)
    b = dy.clone()
    b[:, ::3] = -x[:, ::3]
    dr = x.flip(1)

    def run():
        s, t = x.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        r = ops.AddReluFn.apply(s, t)
        r.backward(dr.to(DEV))
        return r, s.grad
    r, da = _twice(run, BIG_BYTES)
    r64 = R.add_relu(x, b)
    _exact(r, r64.float(), "add-relu 520x520x32")
    _exact(da, R.add_relu_bwd(r64, dr).float(), "add-relu backward 520x520x32")


def test_grid_stride_gate_mul():
    """two images: 540,800 pixels, more than gate_mul_bwd_kernel's 16384 blocks of 256 / L = 32 pixels"""
    ops = _ops()
    x, dy = _big()
    skip, dout = torch.cat([x, dy.flip(2)]), torch.cat([dy, x.flip(1)])
    npix = skip.numel() // 32
    assert npix > 16384 * (256 // R.head_lanes(32)) and npix % (16384 * (256 // R.head_lanes(32))) != 0
    _sweeps(skip.numel() // 4)
    gate = torch.rand((2, 520, 520, 1), generator=_gen(521))
    out64, dskip64, dgate64, scale = R.gate_mul(skip, gate, dout)

    def run():
        s, t = skip.to(DEV).requires_grad_(True), gate.to(DEV).requires_grad_(True)
        out = ops.GateMulFn.apply(s, t)
        out.backward(dout.to(DEV))
        return out, s.grad, t.grad
    out, dskip, dgate = _twice(run, 2 * BIG_BYTES)
    _ok("gate_out", out, out64, R.U * out64.abs(), "2x520x520x32")
    _ok("gate_dskip", dskip, dskip64, R.U * dskip64.abs(), "2x520x520x32")
    _ok("gate_dgate", dgate, dgate64, R.gate_dgate_bound(32, scale), "2x520x520x32")


def test_grid_stride_copy_channels_and_nhwc_to_nchw():
    ops = _ops()
    x, dy = _big()
    _sweeps(x.numel() // 4)

    def run():
        a, b = x.to(DEV).requires_grad_(True), dy.to(DEV).requires_grad_(True)
        out = ops.CatChannelsFn.apply(a, b)
        out.backward(out.detach())
        return out, a.grad, b.grad
    out, da, db = _twice(run, 2 * BIG_BYTES)
    _exact(out, torch.cat([x, dy], dim=-1), "CatChannelsFn 520x520x(32+32)")
    _exact(da, x, "CatChannelsFn backward, first source")
    _exact(db, dy, "CatChannelsFn backward, second source")
    _sweeps(x.numel())
    (z,) = _twice(lambda: (ops.nhwc_to_nchw(x.to(DEV)),), BIG_BYTES)
    _exact(z, x.permute(0, 3, 1, 2).contiguous(), "nhwc_to_nchw 520x520x32")


def test_grid_stride_nchw_to_nhwc():
    ops = _ops()
    shape = (2, 3, 1032, 1024)
    _sweeps(2 * 1032 * 1024)
    x = torch.randn(shape, generator=_gen(1032))
    (y,) = _twice(lambda: (ops.nchw_to_nhwc(x.to(DEV), 4),), 2 * 1032 * 1024 * 16)
    want = torch.zeros(2, 1032, 1024, 4)
    want[..., :3] = x.permute(0, 2, 3, 1)
    _exact(y, want, "nchw_to_nhwc 2x3x1032x1024")


def test_grid_stride_bilinear():
    """forward 260 -> 520 (output items beyond the cap); backward of 520 -> 260 (input items beyond the cap)"""
    ops = _ops()
    big, _ = _big()
    small = big[:, :260, :260].contiguous()
    _sweeps(big.numel() // 4)
    (y,) = _twice(lambda: (ops.BilinearFn.apply(small.to(DEV), 520, 520),), BIG_BYTES)
    _ok("bilinear_fwd", y, R.bilinear_fwd(small, 520, 520), R.bilinear_fwd_bound(small, 520, 520), "260 -> 520")
    dy = _big()[1][:, 130:390, 130:390].contiguous()

    def run():
        t = big.to(DEV).requires_grad_(True)
        ops.BilinearFn.apply(t, 260, 260).backward(dy.to(DEV))
        return (t.grad,)
    (dx,) = _twice(run, BIG_BYTES)
    _ok("bilinear_bwd", dx, R.bilinear_bwd(dy, 520, 520), R.bilinear_bwd_bound(dy, 520, 520)[0], "520 -> 260 backward")
