"""The BatchNorm kernels (csrc/norm_act.hip) through the C ABI, one entry point at a time, against tests/bn_ref.py: exact
integer cases over the shape / path tables (bit for bit, no tolerance), real-valued cases against float64 under the derived
bounds ("bn_ref ratio <operation> <error / bound>" is printed for each), the bit-identity claims of include/xv2.h, the F16X2
maximum of the apply passes, operands that are channel slices of wider tensors (NaN in the input gaps, a sentinel in the output
gaps), and outputs and workspaces filled with NaN and then with 2^100: the results must not change.  The inputs of every entry
point are built here or taken from the reference, never from the kernel that precedes it in a layer."""
import itertools

import pytest
import torch

from tests import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
FILLS = (float("nan"), 2.0 ** 100)
EPS, MOM = 1e-5, 0.1
RATIOS = {}


def _capi():
    from xview2_amd import _capi
    return _capi


def _call(*a):
    return _capi().call(*a)


def _gen(*key):
    return torch.Generator().manual_seed(9000011 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _code(dt):
    return R.BF16 if dt == torch.bfloat16 else R.F32


def _sfx(dt):
    return "_bf16" if dt == torch.bfloat16 else ""


def _full(shape, fill, dt=torch.float32):
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), fill, dtype=dt, device=DEV)


def _bits(t):
    t = t.detach().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _both_fills(run):
    """run(fill) -> tensors, with every output and workspace it owns filled with `fill` first: NaN, then 2^100, same bits"""
    first = [t.detach().clone() for t in run(FILLS[0])]
    second = [t.detach().clone() for t in run(FILLS[1])]
    for i, (a, b) in enumerate(zip(first, second)):
        assert _same_bits(a, b), "result %d depends on the contents of unwritten memory" % i
    return second


def _ok(op, y, y64, bound, what=""):
    r, where = R.check(y, y64, bound)
    RATIOS[op] = max(RATIOS.get(op, 0.0), r)
    print("bn_ref ratio %s %.4f %s" % (op, r, what))
    assert r <= 1.0, "%s %s: error / bound %.3f at flat index %d" % (op, what, r, where)


def _exact(y, want, what):
    y = y.detach().cpu()
    assert y.dtype == want.dtype and y.shape == want.shape, (what, y.dtype, want.dtype, y.shape, want.shape)
    assert torch.equal(y, want), "%s: not bit-exact (%d elements differ)" % (what, int((y != want).sum()))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("bn_ref worst " + ", ".join('"%s": %.3f' % kv for kv in sorted(RATIOS.items())))


class In:
    """an input operand on the device: dense, or a channel slice of a wider tensor whose other columns hold NaN"""

    def __init__(self, t, wide=False):
        npix, C = t.shape
        if wide:
            self.ld, off = R.wide_ld(C)
            self.t = _full((npix, self.ld), float("nan"), t.dtype)
            self.t[:, off:off + C] = t.to(DEV)
            self.p = _capi().Ptr(self.t, off)
        else:
            self.ld, self.t = C, t.to(DEV).contiguous()
            self.p = self.t


class Out:
    """an output operand filled with `fill`; as a slice of a wider tensor the other columns must keep the fill's bits"""

    def __init__(self, npix, C, dt, fill, wide=False):
        self.C, self.off = C, 0
        self.ld = C
        if wide:
            self.ld, self.off = R.wide_ld(C)
        self.t = _full((npix, self.ld), fill, dt)
        self.ref = self.t.clone()
        self.p = _capi().Ptr(self.t, self.off) if wide else self.t

    def get(self):
        keep = torch.ones(self.ld, dtype=torch.bool, device=DEV)
        keep[self.off:self.off + self.C] = False
        assert torch.equal(_bits(self.t[:, keep]), _bits(self.ref[:, keep])), "a gap of the output's wider tensor was written"
        return self.t[:, self.off:self.off + self.C].contiguous()


def _ws(nbytes, fill):
    return _full((nbytes + 3) // 4 + 4, fill)


def _bn_ws(npix, C, fill):
    return _ws(_capi().query("xv2_bn_backward_workspace", npix, C), fill)


def _vecs(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


# ---- statistics ----------------------------------------------------------------------------------------------------------

def _tensor_stats(x, fill, wide=False):
    npix, C = x.shape
    xi = In(x, wide)
    sums = _full((C, 2), fill, torch.float64)
    ws = _ws(_capi().query("xv2_bn_tensor_stats_workspace", npix, C), fill)
    _call("xv2_bn_tensor_stats", xi.p, xi.ld, npix, C, sums, ws)
    return sums.cpu()


def _int_sums(x):
    x = x.double()
    return torch.stack([x.sum(0), (x * x).sum(0)], 1)


@pytest.mark.parametrize("C", R.C_ALL)
def test_tensor_stats_exact(C):
    """integers in [-3, 3]: (sum x, sum x^2) bit for bit at every geometry (R.column_form(C)), also with a zero first row"""
    for j, npix in enumerate(R.npix_list(C)):
        x = R.ints((npix, C), -3, 3, _gen(C, npix, 1))
        for k, v in enumerate((x, x - x[0])):
            (sums,) = _both_fills(lambda fill: (_tensor_stats(v, fill, wide=(j + k) % 2 == 1),))
            _exact(sums, _int_sums(v), "tensor_stats C=%d npix=%d (%s)" % (C, npix, R.column_form(C)))


@pytest.mark.parametrize("C,npix", [(8, 2053), (512, 101), (130, 101), (12, 101), (3, 997)])
def test_tensor_stats_real(C, npix):
    for off in (0.0, 30.0):
        x = R.real(npix, C, _gen(C, npix, 2), offset=off)
        want, bound = R.tensor_stats(x)
        (sums,) = _both_fills(lambda fill: (_tensor_stats(x, fill),))
        _ok("tensor_stats", sums, want, bound, "C=%d npix=%d offset=%g" % (C, npix, off))


def _reduce(partial, fill, finalize=None):
    tiles, C, _ = partial.shape
    p = partial.to(DEV).contiguous()
    sums = _full((C, 2), fill, torch.float64)
    scratch = _full((R.SCRATCH_ROWS * C * 2,), fill, torch.float64)
    if finalize is None:
        _call("xv2_bn_reduce_stats", p, tiles, C, sums, scratch)
        return (sums.cpu(),)
    count, gamma, beta, rm, rv = finalize
    outs = [_full((C,), fill) for _ in range(4)]
    gamma, beta, rm, rv = _vecs(gamma, beta, rm, rv)
    _call("xv2_bn_reduce_finalize", p, tiles, C, sums, scratch, count, gamma, beta, EPS, MOM, rm, rv, *outs)
    return (sums.cpu(),) + tuple(o.cpu() for o in outs) + ((rm.cpu(), rv.cpu()) if rm is not None else ())


def _finalize(sums, count, gamma, beta, rm, rv, fill, C):
    outs = [_full((C,), fill) for _ in range(4)]
    gamma, beta, rm, rv = _vecs(gamma, beta, rm, rv)
    _call("xv2_bn_finalize", sums.to(DEV), float(count), gamma, beta, EPS, MOM, rm, rv, *outs, C)
    return tuple(o.cpu() for o in outs) + ((rm.cpu(), rv.cpu()) if rm is not None else ())


@pytest.mark.parametrize("C", R.C_REDUCE)
def test_reduce_stats_partials_exact(C):
    """integer partials: the one-phase fold up to 1024 tiles and the two-phase ticket fold above, bit for bit; and
    xv2_bn_reduce_finalize == xv2_bn_reduce_stats + xv2_bn_finalize, bit for bit"""
    g = _gen(C, 3)
    _, _, gamma, beta = R.coeffs(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    for tiles in R.TILES_1PHASE + R.TILES_2PHASE:
        part = R.ints((tiles, C, 2), -8, 8, g)
        want = part.double().sum(0)
        (sums,) = _both_fills(lambda fill: _reduce(part, fill))
        _exact(sums, want, "reduce_stats C=%d tiles=%d" % (C, tiles))
        count = float(tiles * 64)
        fused = _both_fills(lambda fill: _reduce(part, fill, (count, gamma, beta, rm, rv)))
        pair = _both_fills(lambda fill: _finalize(sums, count, gamma, beta, rm, rv, fill, C))
        _exact(fused[0], want, "reduce_finalize sums C=%d tiles=%d" % (C, tiles))
        for name, a, b in zip(("mean", "invstd", "scale", "shift", "running_mean", "running_var"), fused[1:], pair):
            assert _same_bits(a, b), "reduce_finalize != reduce_stats + finalize: %s, C=%d tiles=%d" % (name, C, tiles)


def _check_finalize(op, got, ref, what):
    for name, t in zip(("mean", "invstd", "scale", "shift", "running_mean", "running_var"), got):
        _ok(op + "_" + name, t, ref[name][0], ref[name][1], what)


def test_finalize_forms():
    """gamma / beta NULL, running statistics NULL, count 1, a variance below 0 by one fp64 rounding"""
    C = 37
    g = _gen(C, 4)
    _, _, gamma, beta = R.coeffs(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    x = R.real(50, C, g, offset=3.0)
    sums, _ = R.tensor_stats(x)
    s1, s2, n = R.negative_var_sums()
    neg = torch.tensor([[s1, s2]] * C, dtype=torch.float64)
    one = torch.stack([x[0].double(), x[0].double() ** 2], 1)
    for what, s, count, ga, be, m, v in (("all", sums, 50.0, gamma, beta, rm, rv), ("no affine", sums, 50.0, None, None, rm, rv),
                                         ("no running", sums, 50.0, gamma, beta, None, None), ("count 1", one, 1.0, gamma, beta, rm, rv),
                                         ("negative variance", neg, n, gamma, beta, rm, rv)):
        ref = R.finalize(s, count, ga, be, EPS, MOM, m, v)
        if what == "negative variance":
            assert float(ref["invstd"][0][0]) == 1.0 / (0.0 + float(torch.tensor(EPS, dtype=torch.float32))) ** 0.5      # clamped
        got = _both_fills(lambda fill: _finalize(s, count, ga, be, m, v, fill, C))
        _check_finalize("finalize", got, ref, what)
        part = torch.stack([s.float(), torch.zeros(C, 2)])      # two tiles of float partials that carry the same sums to fp32
        ref2 = R.finalize(part.double().sum(0), count, ga, be, EPS, MOM, m, v)
        got2 = _both_fills(lambda fill: _reduce(part, fill, (count, ga, be, m, v)))
        _check_finalize("reduce_finalize", got2[1:], ref2, what)


@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("kind", ["constant", "mean_1e4"])
def test_stats_then_finalize_cancellation(C, kind):
    """a constant column (variance 0) and |mean| / std = 1e4 through xv2_bn_tensor_stats + xv2_bn_finalize: what the shifted
    sums exist for.  The sums' bounds enter as dm = b1 / n, dvar = b2 / n + 2 |mean(x - x0)| b1 / n (the variance is
    shift-invariant: the bounds of the shifted sums count, not those of the un-shifted ones)."""
    npix = 37
    g = _gen(C, npix, 5)
    if kind == "constant":
        x = torch.full((npix, C), 1000.1, dtype=torch.float32)
    else:
        x = (1e4 + torch.randn(npix, C, generator=g, dtype=torch.float64)).float()
    want, _ = R.tensor_stats(x)
    t = x.double() - x[0].double()
    b1, b2 = R.sum_bound(t, 1), R.sum_bound(t * t, 2)
    ref = R.finalize(want, npix, None, None, EPS, MOM)
    var = (x.double().var(0, unbiased=False))
    dvar = b2 / npix + 2.0 * t.mean(0).abs() * b1 / npix
    sums = _tensor_stats(x, FILLS[0])
    mean, invstd, _, _ = _finalize(sums, npix, None, None, None, None, FILLS[0], C)
    _ok("stats_finalize_mean", mean, ref["mean"][0], ref["mean"][1] + b1 / npix, kind)
    _ok("stats_finalize_invstd", invstd, ref["invstd"][0], ref["invstd"][1] + ref["invstd"][0] * dvar / (2.0 * (var + EPS)), kind)
    if kind == "mean_1e4":      # the gate has the resolution the case is about: 1e-3 of the value would not pass
        assert float((ref["invstd"][1] / ref["invstd"][0]).max()) < 1e-5


def test_eval_coeffs():
    for C, affine in ((1, True), (37, True), (300, False)):
        g = _gen(C, 6)
        _, _, gamma, beta = R.coeffs(C, g)
        if not affine:
            gamma = beta = None
        rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.01
        ref = R.eval_coeffs(gamma, beta, rm, rv, EPS)

        def run(fill):
            sc, sh = _full((C,), fill), _full((C,), fill)
            _call("xv2_bn_eval_coeffs", *_vecs(gamma, beta, rm, rv), EPS, sc, sh, C)
            return sc.cpu(), sh.cpu()
        sc, sh = _both_fills(run)
        _ok("eval_scale", sc, *ref["scale"], "C=%d" % C)
        _ok("eval_shift", sh, *ref["shift"], "C=%d" % C)


# ---- forward apply -------------------------------------------------------------------------------------------------------

def _forward(y, sc, sh, res, act, dt, fill, wide=False, mask=False):
    npix, C = y.shape
    yi, ri = In(y, wide), (In(res, wide) if res is not None else None)
    z = Out(npix, C, dt, fill, wide)
    scd, shd = _vecs(sc, sh)
    if mask:
        zm = torch.full((npix * (C // 4),), 0xA5, dtype=torch.uint8, device=DEV)
        _call("xv2_bn_act_forward_mask", yi.p, yi.ld, scd, shd, ri.p if ri else None, ri.ld if ri else C, act, z.p, z.ld, npix, C, zm,
              _code(dt))
        return z.get().cpu(), zm.cpu()
    _call("xv2_bn_act_forward", yi.p, yi.ld, scd, shd, ri.p if ri else None, ri.ld if ri else C, act, z.p, z.ld, npix, C, _code(dt))
    return (z.get().cpu(),)


def _forward_case(C, npix, act, dt, with_res, wide, key):
    g = _gen(C, npix, act, key)
    y = R.real(npix, C, g, dt)
    mean, invstd, gamma, beta = R.coeffs(C, g)
    sc, sh = R.fold(mean, invstd, gamma, beta)
    res = R.real(npix, C, g, dt) if with_res else None
    z64, bound, pre = R.forward(y, sc, sh, act, res, dt == torch.bfloat16)
    assert bool((pre != 0).all())
    what = "C=%d npix=%d act=%d res=%d wide=%d" % (C, npix, act, with_res, wide)
    (z,) = _both_fills(lambda fill: _forward(y, sc, sh, res, act, dt, fill, wide))
    _ok("forward" + ("_sigmoid" if act == R.SIGMOID else "") + _sfx(dt), z, z64, bound, what)
    if C % 4 == 0 and act in (R.RELU, R.LEAKY):
        zm, m = _both_fills(lambda fill: _forward(y, sc, sh, res, act, dt, fill, wide, mask=True))
        assert _same_bits(zm, z), "forward_mask: z differs from the z form, " + what
        assert torch.equal(m.reshape(npix, C // 4), R.mask_bytes(zm.float())), "forward_mask: mask byte, " + what
    return z


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", R.C_ALL + (6,))
def test_forward_apply(C, dt):
    """every shape of the tables (C = 6 with ld = 6: the scalar kernel on rows that are not 16-byte aligned), the four
    activations, with and without residual, dense and as slices of wider tensors, z form and mask form"""
    for j, npix in enumerate(R.npix_list(C)):
        for act in R.ACTS:
            _forward_case(C, npix, act, dt, with_res=(j + act) % 2 == 1, wide=(j + act // 2) % 2 == 1 and C != 6, key=7)


def test_forward_apply_second_sweep():
    """1.2 M float4 items: the grid-stride loop runs a second sweep, walking the tensor last-to-first"""
    npix, C = R.EW_SWEEP
    z = _forward_case(C, npix, R.LEAKY, torch.float32, with_res=False, wide=False, key=8)
    assert z.shape == (npix, C)


# ---- backward: column sums -----------------------------------------------------------------------------------------------

def _has_mask_sums(C):
    return R.column_form(C) != "generic"


def _bwd_reduce(form, dz, zin, y, mean, invstd, sc, sh, act, dt, fill, wide=False):
    """form "z": zin = z; "pre": z NULL, the mask recomputed from (sc, sh); "mask": zin = the mask bytes"""
    npix, C = y.shape
    di, yi = In(dz, wide), In(y, wide)
    sums2 = _full((C, 2), fill, torch.float64)
    dga, dbe = _full((C,), fill), _full((C,), fill)
    ws = _bn_ws(npix, C, fill)
    me, inv, scd, shd = _vecs(mean, invstd, sc, sh)
    if form == "mask":
        _call("xv2_bn_act_backward_reduce_mask", di.p, di.ld, zin.to(DEV), yi.p, yi.ld, me, inv, act, npix, C, sums2, dga, dbe, ws,
              _code(dt))
    else:
        zi = In(zin, wide) if form == "z" else None
        _call("xv2_bn_act_backward_reduce", di.p, di.ld, zi.p if zi else None, zi.ld if zi else C, yi.p, yi.ld, me, inv, scd, shd, act,
              npix, C, sums2, dga, dbe, ws, _code(dt))
    return sums2.cpu(), dga.cpu(), dbe.cpu()


def _exact_bwd_inputs(C, npix, dt, key):
    g = _gen(C, npix, key)
    dz, y, z = R.ints((npix, C), -3, 3, g).to(dt), R.ints((npix, C), -4, 4, g).to(dt), R.ints((npix, C), -4, 4, g).to(dt)
    mean = R.ints((C,), -2, 2, g)
    invstd = torch.full((C,), 0.5)
    shift = R.ints((C,), -2, 2, g)
    return dz, y, z, mean, invstd, torch.ones(C), shift


def _exact_bwd_check(form, ins, act, dt, wide, what):
    dz, y, z, mean, invstd, sc, sh = ins
    pre = y.double() + sh.double()
    want, _, _ = R.backward_sums(dz, y, mean, invstd, act, z=None if form == "pre" else z, pre=pre)
    zin = R.mask_bytes(z.float()).reshape(-1) if form == "mask" else z
    sums2, dga, dbe = _both_fills(lambda fill: _bwd_reduce(form, dz, zin, y, mean, invstd, sc, sh, act, dt, fill, wide))
    _exact(sums2, want, "backward_reduce sums2 " + what)
    _exact(dbe, want[:, 0].float(), "backward_reduce dbeta " + what)
    _exact(dga, want[:, 1].float(), "backward_reduce dgamma " + what)
    return sums2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", R.C_ALL)
def test_backward_sums_exact(C, dt):
    """integer dz, y, z, mean and invstd = 0.5: (sum g, sum g xhat), dgamma and dbeta bit for bit at every geometry, from z, from
    the recomputed pre-activation (scale 1, integer shift) and from the mask"""
    forms = ("z", "pre") + (("mask",) if _has_mask_sums(C) else ())
    for j, npix in enumerate(R.npix_list(C)):
        ins = _exact_bwd_inputs(C, npix, dt, 9)
        for k, (form, act) in enumerate(itertools.product(forms, (R.NONE, R.RELU))):
            what = "C=%d npix=%d %s act=%d %s" % (C, npix, form, act, R.column_form(C))
            _exact_bwd_check(form, ins, act, dt, wide=form != "mask" and (j + k) % 2 == 1, what=what)


def test_two_phase_fold_of_double_partials():
    """C = 3, npix = 32 * 1030 + 3: more than 1024 chunks, folded by the ticket kernel; three runs in a row give the same bits
    (the tickets return to zero), for the statistics and for the backward sums"""
    C, npix = R.TWO_PHASE
    x = R.ints((npix, C), -3, 3, _gen(C, npix, 10))
    ins = _exact_bwd_inputs(C, npix, torch.float32, 11)
    for i in range(3):
        _exact(_tensor_stats(x, FILLS[i % 2]), _int_sums(x), "two-phase tensor_stats, run %d" % i)
        _exact_bwd_check("z", ins, R.RELU, torch.float32, False, "two-phase, run %d" % i)


def _real_bwd_inputs(C, npix, act, dt, key, res=False):
    """dz, y, z (the activation's output as the forward stores it, from the float64 reference), coefficients"""
    g = _gen(C, npix, act, key)
    mean, invstd, gamma, beta = R.coeffs(C, g)
    y = (R.real(npix, C, g).double() / invstd.double() * 0.5 + mean.double()).to(dt)      # xhat of order 1
    sc, sh = R.fold(mean, invstd, gamma, beta)
    r = R.real(npix, C, g, dt) if res else None
    z64, _, pre = R.forward(y, sc, sh, act, r)
    assert bool((pre != 0).all()), "an exact zero in the pre-activation"
    dz = R.real(npix, C, g, dt)
    return dz, y, z64.to(dt), mean, invstd, gamma, sc, sh, pre


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", R.REAL_C)
def test_backward_sums_real(C, dt):
    npix = R.npix_list(C)[-1]
    forms = ("z", "pre") + (("mask",) if _has_mask_sums(C) else ())
    for form, act in itertools.product(forms, R.ACTS):
        if form == "mask" and act in (R.NONE, R.SIGMOID):
            continue
        dz, y, z, mean, invstd, gamma, sc, sh, pre = _real_bwd_inputs(C, npix, act, dt, 12, res=form != "pre")
        want, bound, _ = R.backward_sums(dz, y, mean, invstd, act, z=None if form == "pre" else z, pre=pre)
        zin = R.mask_bytes(z.float()).reshape(-1) if form == "mask" else z
        wide = form == "z" and act % 2 == 1
        sums2, dga, dbe = _both_fills(lambda fill: _bwd_reduce(form, dz, zin, y, mean, invstd, sc, sh, act, dt, fill, wide))
        what = "C=%d npix=%d %s act=%d" % (C, npix, form, act)
        _ok("backward_sums" + _sfx(dt), sums2, want, bound, what)
        _ok("dbeta" + _sfx(dt), dbe, want[:, 0], R.f32_of(want[:, 0], bound[:, 0]), what)
        _ok("dgamma" + _sfx(dt), dga, want[:, 1], R.f32_of(want[:, 1], bound[:, 1]), what)
        if form == "mask":
            zs = _bwd_reduce("z", dz, z, y, mean, invstd, sc, sh, act, dt, FILLS[0])
            assert all(_same_bits(a, b) for a, b in zip(zs, (sums2, dga, dbe))), "mask form != z form: " + what


# ---- backward: apply -----------------------------------------------------------------------------------------------------

def _bwd_apply(form, dz, zin, y, mean, invstd, gamma, sc, sh, sums2, count, act, train, want_res, dt, fill, wide=False, slots=None):
    npix, C = y.shape
    di, yi = In(dz, wide), In(y, wide)
    dy = Out(npix, C, dt, fill, wide)
    dres = Out(npix, C, dt, fill, wide) if want_res else None
    me, inv, ga, scd, shd = _vecs(mean, invstd, gamma, sc, sh)
    s2 = sums2.to(DEV)
    if slots is not None:
        _capi().set_amax(None, None, None, slots)
    if form == "mask":
        _call("xv2_bn_act_backward_apply_mask", di.p, di.ld, zin.to(DEV), yi.p, yi.ld, me, inv, ga, s2, float(count), act, train, dy.p,
              dy.ld, dres.p if dres else None, dres.ld if dres else C, npix, C, _code(dt))
    else:
        zi = In(zin, wide) if form == "z" else None
        _call("xv2_bn_act_backward_apply", di.p, di.ld, zi.p if zi else None, zi.ld if zi else C, yi.p, yi.ld, me, inv, ga, scd, shd, s2,
              float(count), act, train, dy.p, dy.ld, dres.p if dres else None, dres.ld if dres else C, npix, C, _code(dt))
    return (dy.get().cpu(),) + ((dres.get().cpu(),) if dres else ())


APPLY_CONFIGS = [(f, a) for f, a in itertools.product(("z", "pre", "mask"), R.ACTS) if not (f == "mask" and a in (R.NONE, R.SIGMOID))]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", R.C_ALL)
def test_backward_apply(C, dt):
    """dy and dres at every shape of the tables (R.apply_form(C): rows, float4 or scalar kernel), sums2 from the float64
    reference; z form, recomputed form and mask form, with and without dres and gamma, training and eval mode, dense and as
    slices of wider tensors"""
    bf = dt == torch.bfloat16
    for j, npix in enumerate(R.npix_list(C)):
        for k, (form, act) in enumerate(APPLY_CONFIGS):
            if form == "mask" and C % 4:
                continue
            h = ((C * 131 + j * 17 + k) * 2654435761 >> 7) & 0xffff      # the other axes: scrambled, so that none follows another
            want_res, no_gamma, train, wide = h & 1 == 1, (h >> 1) % 4 == 0, 0 if (h >> 3) % 3 == 0 else 1, form != "mask" and (h >> 5) & 1 == 1
            dz, y, z, mean, invstd, gamma, sc, sh, pre = _real_bwd_inputs(C, npix, act, dt, 13, res=form != "pre")
            gamma = None if no_gamma else gamma
            sums2, _, parts = R.backward_sums(dz, y, mean, invstd, act, z=None if form == "pre" else z, pre=pre)
            dy64, bdy, dr64, bdr = R.backward_apply(parts, sums2, float(npix), invstd, gamma, train, bf)
            zin = R.mask_bytes(z.float()).reshape(-1) if form == "mask" else z
            what = "C=%d npix=%d %s act=%d train=%d dres=%d gamma=%d wide=%d %s" % (C, npix, form, act, train, want_res, not no_gamma,
                                                                                     wide, R.apply_form(C))
            got = _both_fills(lambda fill: _bwd_apply(form, dz, zin, y, mean, invstd, gamma, sc, sh, sums2, npix, act, train, want_res,
                                                      dt, fill, wide))
            op = ("backward_apply" if train else "backward_apply_eval") + ("_sigmoid" if act == R.SIGMOID else "") + _sfx(dt)
            _ok(op, got[0], dy64, bdy, what)
            if want_res:
                _ok("dres" + ("_sigmoid" if act == R.SIGMOID else "") + _sfx(dt), got[1], dr64, bdr, what)
            if form == "mask":
                zs = _bwd_apply("z", dz, z, y, mean, invstd, gamma, sc, sh, sums2, npix, act, train, want_res, dt, FILLS[0])
                assert all(_same_bits(a, b) for a, b in zip(zs, got)), "mask form != z form: " + what


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,form", [(8, "z"), (8, "pre"), (8, "mask"), (512, "mask"), (512, "pre"), (12, "z"), (130, "pre")])
def test_backward_one_call_is_reduce_plus_apply(C, form, dt):
    """xv2_bn_act_backward == xv2_bn_act_backward_reduce[_mask] + xv2_bn_act_backward_apply[_mask], bit for bit (the apply of
    the pair is handed the pair's own sums2)"""
    npix, act = R.npix_list(C)[-1], R.LEAKY
    dz, y, z, mean, invstd, gamma, sc, sh, _ = _real_bwd_inputs(C, npix, act, dt, 14, res=form != "pre")
    zin = R.mask_bytes(z.float()).reshape(-1) if form == "mask" else z

    def fused(fill):
        di, yi = In(dz), In(y)
        zi = In(z) if form == "z" else None
        dy, dres = Out(npix, C, dt, fill), Out(npix, C, dt, fill)
        sums2, dga, dbe = _full((C, 2), fill, torch.float64), _full((C,), fill), _full((C,), fill)
        ws = _bn_ws(npix, C, fill)
        me, inv, ga, scd, shd = _vecs(mean, invstd, gamma, sc, sh)
        _call("xv2_bn_act_backward", di.p, C, zi.p if zi else None, C, zin.to(DEV) if form == "mask" else None, yi.p, C, me, inv, ga,
              None if form == "mask" else scd, None if form == "mask" else shd, act, float(npix), dy.p, C, dres.p, C, npix, C, sums2, dga,
              dbe, ws, _code(dt))
        return sums2.cpu(), dga.cpu(), dbe.cpu(), dy.get().cpu(), dres.get().cpu()
    one = _both_fills(fused)
    red = _bwd_reduce(form, dz, zin, y, mean, invstd, sc, sh, act, dt, FILLS[0])
    app = _bwd_apply(form, dz, zin, y, mean, invstd, gamma, sc, sh, red[0], npix, act, 1, True, dt, FILLS[0])
    for name, a, b in zip(("sums2", "dgamma", "dbeta", "dy", "dres"), one, red + app):
        assert _same_bits(a, b), "%s of the one-call form differs, C=%d %s" % (name, C, form)


# ---- the F16X2 maximum of the apply passes -------------------------------------------------------------------------------

def _slots():
    return torch.zeros(64 * 32, dtype=torch.int32, device=DEV)


def _recorded(slots):
    return int(slots.view(64, 32)[:, 0].max().item())


@pytest.mark.parametrize("C", [8, 6])
def test_forward_records_maximum(C):
    """vector and scalar kernel: the maximum of the 64 slots is max |z| bit for bit; the context serves one call"""
    npix = 999
    g = _gen(C, 15)
    y = R.real(npix, C, g)
    mean, invstd, gamma, beta = R.coeffs(C, g)
    sc, sh = R.fold(mean, invstd, gamma, beta)
    slots = _slots()
    _capi().set_amax(None, None, None, slots)
    (z,) = _forward(y, sc, sh, None, R.LEAKY, torch.float32, FILLS[0])
    assert _recorded(slots) == R.amax_bits(z)
    slots.zero_()
    _forward(y, sc, sh, None, R.LEAKY, torch.float32, FILLS[0])
    torch.cuda.synchronize()
    assert _recorded(slots) == 0, "the F16X2 context outlived the call it was set for"


@pytest.mark.parametrize("C", [8, 12])
def test_backward_apply_records_maximum(C):
    """rows kernel (recorded by the blocks) and generic kernel (a pass over dy behind it)"""
    npix, act = 999, R.RELU
    dz, y, z, mean, invstd, gamma, sc, sh, _ = _real_bwd_inputs(C, npix, act, torch.float32, 16)
    sums2, _, _ = R.backward_sums(dz, y, mean, invstd, act, z=z)
    slots = _slots()
    (dy,) = _bwd_apply("z", dz, z, y, mean, invstd, gamma, sc, sh, sums2, npix, act, 1, False, torch.float32, FILLS[1], slots=slots)
    assert _recorded(slots) == R.amax_bits(dy)
    slots.zero_()
    _bwd_apply("z", dz, z, y, mean, invstd, gamma, sc, sh, sums2, npix, act, 1, False, torch.float32, FILLS[1])
    torch.cuda.synchronize()
    assert _recorded(slots) == 0, "the F16X2 context outlived the call it was set for"


# ---- BatchNorm over a handful of rows ------------------------------------------------------------------------------------

def _rows_forward(y, rows, parts, gamma, beta, rm, rv, train, act, fill):
    C = y.shape[1]
    outs = [_full((parts, C), fill) for _ in range(4)]
    z = _full(tuple(y.shape), fill)
    ga, be, m, v = _vecs(gamma, beta, rm, rv)
    _call("xv2_bn_rows_forward", y.to(DEV), rows, C, parts, ga, be, EPS, MOM, m, v, train, act, *outs, z)
    return tuple(o.cpu() for o in outs) + (z.cpu(),) + ((m.cpu(), v.cpu()) if m is not None else ())


@pytest.mark.parametrize("C", R.ROWS_C)
def test_rows_forward(C):
    for rows, parts, train, act in itertools.product(R.ROWS_ROWS + (1,), (1, 2), (1, 0), R.ACTS):
        if (rows == 1 and train) or (rows + parts + train + act) % 2:      # (half of the product: every value of each axis stays)
            continue
        g = _gen(C, rows, parts, train, act, 17)
        far = rows == 64 and parts == 1      # |mean| >> std
        y = R.real(rows * parts, C, g, offset=3000.0 if far else 0.0)
        _, _, gamma, beta = R.coeffs(C, g)
        rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        if act == R.NONE:
            gamma = beta = None
        with_running = not (train and act == R.RELU)
        ref = R.rows_forward(y, rows, parts, gamma, beta, EPS, MOM, rm if with_running else None, rv if with_running else None, train, act)
        got = _both_fills(lambda fill: _rows_forward(y, rows, parts, gamma, beta, rm if with_running else None,
                                                     rv if with_running else None, train, act, fill))
        what = "C=%d rows=%d parts=%d train=%d act=%d" % (C, rows, parts, train, act)
        for name, t in zip(("mean", "invstd", "scale", "shift", "z"), got):
            _ok("rows_" + name + ("_sigmoid" if act == R.SIGMOID and name == "z" else ""), t, ref[name][0], ref[name][1], what)
        if with_running and train:      # updated part after part
            _ok("rows_running_mean", got[5], *ref["running_mean"], what)
            _ok("rows_running_var", got[6], *ref["running_var"], what)
        elif with_running:
            assert torch.equal(got[5], rm) and torch.equal(got[6], rv), "eval mode wrote the running statistics"


@pytest.mark.parametrize("C", R.ROWS_C)
def test_rows_backward(C):
    for rows, parts, train, act in itertools.product(R.ROWS_ROWS + (1,), (1, 2), (1, 0), R.ACTS):
        if (rows == 1 and train) or (rows + parts + train + act) % 2 == 0:
            continue
        g = _gen(C, rows, parts, train, act, 18)
        n = rows * parts
        y, dz = R.real(n, C, g), R.real(n, C, g)
        mean = torch.randn(parts, C, generator=g)
        invstd = torch.rand(parts, C, generator=g) * 2.0 + 0.25
        _, _, gamma, beta = R.coeffs(C, g)
        gamma = None if act == R.NONE else gamma
        z = torch.cat([R.forward(y[s * rows:(s + 1) * rows], *R.fold(mean[s], invstd[s], gamma, beta), act)[0] for s in range(parts)]).float()
        ref = R.rows_backward(dz, z, y, mean, invstd, gamma, rows, parts, act, train)

        def run(fill):
            dy, dga, dbe = _full((n, C), fill), _full((C,), fill), _full((C,), fill)
            _call("xv2_bn_rows_backward", dz.to(DEV), z.to(DEV), y.to(DEV), mean.to(DEV), invstd.to(DEV), _vecs(gamma)[0], rows, C, parts,
                  act, train, dy, dga, dbe)
            return dy.cpu(), dga.cpu(), dbe.cpu()
        got = _both_fills(run)
        what = "C=%d rows=%d parts=%d train=%d act=%d" % (C, rows, parts, train, act)
        for name, t in zip(("dy", "dgamma", "dbeta"), got):
            _ok("rows_" + name + ("_sigmoid" if act == R.SIGMOID else ""), t, ref[name][0], ref[name][1], what)


# ---- operands the vector forms cannot take are rejected, not re-routed ---------------------------------------------------

def test_misaligned_column_operands_are_rejected():
    """C % 4 == 0 with a stride or a base address that breaks the 4-element accesses: the call returns the error and launches
    nothing (the outputs keep their fill)"""
    C, npix = 8, 40
    Ptr = _capi().Ptr
    x = torch.zeros(npix * 12 + 8, device=DEV)
    sums = _full((C, 2), 7.0, torch.float64)
    ws = _bn_ws(npix, C, 7.0)
    for p, ld in ((Ptr(x, 1), C), (x, C + 1), (x, C + 2)):
        with pytest.raises(RuntimeError, match="bn_tensor_stats"):
            _call("xv2_bn_tensor_stats", p, ld, npix, C, sums, ws)
    vec = torch.ones(C + 4, device=DEV)
    dga, dbe = _full((C,), 7.0), _full((C,), 7.0)
    for dt in DTYPES:
        t = torch.zeros(npix * 12 + 8, dtype=dt, device=DEV)
        for dzp, zp, yp, mp in ((Ptr(t, 1), t, t, vec), (t, Ptr(t, 2), t, vec), (t, t, Ptr(t, 3), vec), (t, t, t, Ptr(vec, 1))):
            with pytest.raises(RuntimeError, match="bn backward"):
                _call("xv2_bn_act_backward_reduce", dzp, C, zp, C, yp, C, mp, vec, vec, vec, R.RELU, npix, C, sums, dga, dbe, ws, _code(dt))
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((dga == 7.0).all()) and bool((dbe == 7.0).all()) and bool((ws == 7.0).all())
