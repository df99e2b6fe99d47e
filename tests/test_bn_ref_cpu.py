"""The restatement and the gates of tests/bn_ref.py, tested without a GPU: the float64 reference is F.batch_norm + activation with
torch.autograd.grad in float64 (z, dy, dres, dgamma, dbeta and the running statistics, training and eval mode); an fp32 CPU
emulation of the kernels' arithmetic passes every gate on the tables, with sequential summation and with the order reversed (this
pins the bounds); deliberately wrong variants fail their gate (the gates have teeth)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

EPS, MOM = 1e-5, 0.1
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOM))


def _gen(*key):
    return torch.Generator().manual_seed(3000017 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _ratio(y, y64, bound):
    return R.check(y, y64, bound)[0]


def _ok(y, y64, bound, what):
    r, where = R.check(y, y64, bound)
    assert r <= 1.0, "%s: error / bound %.3f at flat index %d" % (what, r, where)


# ---- (a) the reference is torch's ----------------------------------------------------------------------------------------

def _torch_act(v, a):
    if a == R.RELU:
        return F.relu(v)
    if a == R.LEAKY:
        return F.leaky_relu(v, R.SLOPE)
    if a == R.SIGMOID:
        return torch.sigmoid(v)
    return v


def _close(a, b, what, tol=1e-11):
    a, b = a.detach().double(), b.detach().double()
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), what


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("with_res", [False, True])
def test_reference_is_torch_batch_norm(act, train, with_res):
    npix, C = 23, 7
    g = _gen(act, train, with_res)
    y = R.real(npix, C, g, offset=0.5).double().requires_grad_(True)
    res = R.real(npix, C, g).double().requires_grad_(True) if with_res else None
    dz = R.real(npix, C, g).double()
    _, _, gamma, beta = R.coeffs(C, g)
    gamma, beta = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g).double(), (torch.rand(C, generator=g) + 0.5).double()
    rm, rv = rm0.clone(), rv0.clone()
    bn = F.batch_norm(y, rm, rv, gamma, beta, bool(train), MOM32, EPS32)
    z = _torch_act(bn if res is None else bn + res, act)
    grads = torch.autograd.grad(z, [y, gamma, beta] + ([res] if with_res else []), dz)
    # the same through the op-level restatement
    yd = y.detach()
    if train:
        sums, _ = R.tensor_stats(yd)
        fin = R.finalize(sums, npix, gamma.detach().float(), beta.detach().float(), EPS, MOM, rm0.float(), rv0.float())
        mean, invstd = fin["mean"][0], fin["invstd"][0]
        sc, sh = fin["scale"][0], fin["shift"][0]
        _close(fin["running_mean"][0], rm, "running_mean")
        _close(fin["running_var"][0], rv, "running_var")
    else:
        mean, invstd = rm0, 1.0 / torch.sqrt(rv0 + EPS32)
        co = R.eval_coeffs(gamma.detach().float(), beta.detach().float(), rm0.float(), rv0.float(), EPS)
        sc, sh = co["scale"][0], co["shift"][0]
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    z64, _, pre = R.forward(yd, sc, sh, act, None if res is None else res.detach())
    _close(z64, z, "z")
    for form in ("z", "pre"):
        sums2, _, parts = R.backward_sums(dz, yd, mean, invstd, act, z=z64 if form == "z" else None, pre=pre)
        dy, _, dres, _ = R.backward_apply(parts, sums2, float(npix), invstd, gamma.detach(), train)
        _close(dy, grads[0], "dy " + form)
        _close(sums2[:, 1], grads[1], "dgamma " + form)
        _close(sums2[:, 0], grads[2], "dbeta " + form)
        if with_res:
            _close(dres, grads[3], "dres " + form)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("train", [1, 0])
def test_rows_reference_is_torch_batch_norm(act, train):
    rows, parts, C = 5, 2, 6
    g = _gen(act, train, 2)
    y = R.real(rows * parts, C, g, offset=2.0)
    dz = R.real(rows * parts, C, g)
    _, _, gamma, beta = R.coeffs(C, g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.double(), rv0.double()
    ref = R.rows_forward(y, rows, parts, gamma, beta, EPS, MOM, rm0, rv0, train, act)
    zs, dys = [], []
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    for s in range(parts):
        ys = y[s * rows:(s + 1) * rows].double().requires_grad_(True)
        z = _torch_act(F.batch_norm(ys, rm, rv, ga, be, bool(train), MOM32, EPS32), act)
        zs.append(z)
        dys.append((ys, z))
    _close(ref["z"][0], torch.cat(zs), "rows z")
    if train:
        _close(ref["running_mean"][0], rm, "rows running_mean")
        _close(ref["running_var"][0], rv, "rows running_var")
    zc = torch.cat(zs)
    grads = torch.autograd.grad(zc, [t[0] for t in dys] + [ga, be], dz.double())
    back = R.rows_backward(dz, zc.detach(), y, ref["mean"][0], ref["invstd"][0], gamma, rows, parts, act, train)
    _close(back["dy"][0], torch.cat(grads[:parts]), "rows dy")
    _close(back["dgamma"][0], grads[parts], "rows dgamma")
    _close(back["dbeta"][0], grads[parts + 1], "rows dbeta")


# ---- (b) an fp32 emulation of the kernels' arithmetic passes -------------------------------------------------------------

def seq_sum(t, reverse=False, dtype=torch.float32, skip=()):
    """rows added one after the other in `dtype`"""
    acc = torch.zeros(t.shape[1:], dtype=dtype)
    order = range(t.shape[0] - 1, -1, -1) if reverse else range(t.shape[0])
    for r in order:
        if r not in skip:
            acc = acc + t[r].to(dtype)
    return acc


def emu_tensor_stats(x, reverse=False, **kw):
    x = x.float()
    t = x - x[0]
    s1, s2 = seq_sum(t, reverse, **kw).double(), seq_sum(t * t, reverse, **kw).double()
    n, x0 = float(x.shape[0]), x[0].double()
    return torch.stack([s1 + n * x0, s2 + 2.0 * x0 * s1 + n * x0 * x0], 1)


def emu_act_grad(z, a):
    one = torch.ones_like(z)
    if a == R.RELU:
        return (z > 0).float()
    if a == R.LEAKY:
        return torch.where(z > 0, one, torch.full_like(z, 0.01))
    if a == R.SIGMOID:
        return z * (1.0 - z)
    return one


def emu_fma(y, sc, sh):
    """one rounding (the product of two fp32 values is exact in float64)"""
    return (y.double() * sc.double() + sh.double()).float()


def emu_g(dz, a, z=None, y=None, sc=None, sh=None):
    if z is not None:
        return dz.float() * emu_act_grad(z.float(), a)
    u = emu_fma(y.float(), sc, sh)
    if a == R.SIGMOID:
        return dz.float() * emu_act_grad(1.0 / (1.0 + torch.exp(-u)), a)
    return dz.float() * emu_act_grad(u, a)


def emu_backward_sums(g, y, mean, invstd, reverse=False, **kw):
    xh = (y.float() - mean) * invstd
    return torch.stack([seq_sum(g, reverse, **kw).double(), seq_sum(g * xh, reverse, **kw).double()], 1)


def emu_forward(y, sc, sh, a, res=None, dt=torch.float32):
    o = emu_fma(y.float(), sc, sh)
    if res is not None:
        o = o + res.float()
    if a == R.RELU:
        o = o.clamp_min(0.0)
    elif a == R.LEAKY:
        o = torch.where(o > 0, o, 0.01 * o)
    elif a == R.SIGMOID:
        o = 1.0 / (1.0 + torch.exp(-o))
    return o.to(dt)


def emu_backward_apply(g, y, mean, invstd, gamma, sums2, count, train, dt=torch.float32, divide=True):
    gi = invstd if gamma is None else gamma * invstd
    if not train:
        return (gi * g).to(dt)
    inv_count = torch.tensor(1.0 / count if divide else 1.0, dtype=torch.float64).float()
    sg, sgx = sums2[:, 0].float() * inv_count, sums2[:, 1].float() * inv_count
    xh = (y.float() - mean) * invstd
    return (gi * (g - sg - xh * sgx)).to(dt)


def emu_finalize(sums, count, gamma, beta, rm, rv, normalise_unbiased=False, running_biased=False):
    """bn_fold.h with its fp32 roundings, numpy"""
    f = np.float32
    s = sums.numpy()
    m = s[:, 0] / count
    var = np.maximum(s[:, 1] / count - m * m, 0.0)
    unb = var * count / (count - 1.0) if count > 1.0 else var
    inv = 1.0 / np.sqrt((unb if normalise_unbiased else var) + np.float64(f(EPS)))
    g = np.ones_like(m, dtype=f) if gamma is None else gamma.numpy()
    b = np.zeros_like(m, dtype=f) if beta is None else beta.numpy()
    sc = g * inv.astype(f)
    sf = b - m.astype(f) * sc
    out = {"mean": m.astype(f), "invstd": inv.astype(f), "scale": sc, "shift": sf}
    if rm is not None:
        keep = f(1.0) - f(MOM)
        out["running_mean"] = keep * rm.numpy() + f(MOM) * m.astype(f)
        out["running_var"] = keep * rv.numpy() + f(MOM) * (var if running_biased else unb).astype(f)
    return {k: torch.from_numpy(np.asarray(v, dtype=f)) for k, v in out.items()}


CPU_C = (4, 64, 512, 3, 12, 130)


@pytest.mark.parametrize("C", CPU_C)
@pytest.mark.parametrize("reverse", [False, True])
def test_fp32_emulation_passes_the_sum_gates(C, reverse):
    for npix in R.npix_list(C)[:4] + (101,):
        g = _gen(C, npix, 3)
        for off in (0.0, 30.0):
            x = R.real(npix, C, g, offset=off)
            want, bound = R.tensor_stats(x)
            _ok(emu_tensor_stats(x, reverse), want, bound, "tensor_stats C=%d npix=%d" % (C, npix))
        xi = R.ints((npix, C), -3, 3, g)
        assert torch.equal(emu_tensor_stats(xi, reverse), R.tensor_stats(xi)[0])      # the exact cases are exact
        for act, form in ((R.NONE, "z"), (R.RELU, "pre"), (R.LEAKY, "z"), (R.SIGMOID, "z"), (R.SIGMOID, "pre"), (R.LEAKY, "pre")):
            mean, invstd, gamma, beta = R.coeffs(C, g)
            y = (R.real(npix, C, g).double() / invstd.double() * 0.5 + mean.double()).float()
            dz = R.real(npix, C, g)
            sc, sh = R.fold(mean, invstd, gamma, beta)
            z64, _, pre = R.forward(y, sc, sh, act)
            z = z64.float()
            want, bound, _ = R.backward_sums(dz, y, mean, invstd, act, z=z if form == "z" else None, pre=pre)
            gg = emu_g(dz, act, z if form == "z" else None, y, sc, sh)
            got = emu_backward_sums(gg, y, mean, invstd, reverse)
            what = "backward_sums C=%d npix=%d act=%d %s" % (C, npix, act, form)
            _ok(got, want, bound, what)
            _ok(got[:, 1].float(), want[:, 1], R.f32_of(want[:, 1], bound[:, 1]), what + " dgamma")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", CPU_C)
def test_fp32_emulation_passes_the_apply_gates(C, dt):
    bf = dt == torch.bfloat16
    for npix in (1, 9, 101):
        for act in R.ACTS:
            g = _gen(C, npix, act, 4)
            mean, invstd, gamma, beta = R.coeffs(C, g)
            y = (R.real(npix, C, g).double() / invstd.double() * 0.5 + mean.double()).to(dt)
            dz, res = R.real(npix, C, g, dt), R.real(npix, C, g, dt)
            sc, sh = R.fold(mean, invstd, gamma, beta)
            for r in (None, res):
                z64, bound, pre = R.forward(y, sc, sh, act, r, bf)
                _ok(emu_forward(y, sc, sh, act, r, dt), z64, bound, "forward C=%d npix=%d act=%d" % (C, npix, act))
            z64, _, pre = R.forward(y, sc, sh, act)
            z = z64.to(dt)
            for form, train in (("z", 1), ("pre", 1), ("z", 0), ("pre", 0)):
                sums2, _, parts = R.backward_sums(dz, y, mean, invstd, act, z=z if form == "z" else None, pre=pre)
                dy64, bdy, dr64, bdr = R.backward_apply(parts, sums2, float(npix), invstd, gamma, train, bf)
                gg = emu_g(dz, act, z if form == "z" else None, y, sc, sh)
                what = "C=%d npix=%d act=%d %s train=%d" % (C, npix, act, form, train)
                _ok(emu_backward_apply(gg, y, mean, invstd, gamma, sums2, float(npix), train, dt), dy64, bdy, "dy " + what)
                _ok(gg.to(dt), dr64, bdr, "dres " + what)


def _finalize_inputs(C, key):
    g = _gen(C, key)
    _, _, gamma, beta = R.coeffs(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    x = R.real(50, C, g, offset=3.0)
    return R.tensor_stats(x)[0], gamma, beta, rm, rv


def test_fp32_emulation_passes_the_finalize_gates():
    C = 37
    sums, gamma, beta, rm, rv = _finalize_inputs(C, 5)
    s1, s2, n = R.negative_var_sums()
    assert s2 / n - (s1 / n) ** 2 < 0.0
    neg = torch.tensor([[s1, s2]] * C, dtype=torch.float64)
    for s, count, ga, be, m, v in ((sums, 50.0, gamma, beta, rm, rv), (sums, 50.0, None, None, None, None), (neg, n, gamma, beta, rm, rv),
                                   (sums / 50.0, 1.0, gamma, beta, rm, rv)):
        ref = R.finalize(s, count, ga, be, EPS, MOM, m, v)
        got = emu_finalize(s, count, ga, be, m, v)
        for k in got:
            _ok(got[k], ref[k][0], ref[k][1], "finalize %s count=%g" % (k, count))
    co = R.eval_coeffs(gamma, beta, rm, rv, EPS)
    inv = 1.0 / torch.sqrt(rv + torch.tensor(EPS))
    _ok(gamma * inv, *co["scale"], "eval scale")
    _ok(beta - rm * (gamma * inv), *co["shift"], "eval shift")


def test_mask_bytes_and_amax_bits():
    z = torch.tensor([[0.5, -1.0, 0.0, 2.0, -3.0, -0.0, 1e-30, float("-inf")]])
    assert R.mask_bytes(z).tolist() == [[0b1001, 0b0100]]
    assert R.amax_bits(torch.tensor([1.0, -2.0, 0.5])) == 0x40000000


# ---- (c) wrong variants fail ---------------------------------------------------------------------------------------------

def test_wrong_last_row_of_a_chunk_dropped():
    C = 8
    npix = R.npix_list(C)[3]                  # one full chunk and a second chunk of one row
    last = 8 * R.rows_per_pass(C) - 1
    g = _gen(1, 6)
    xi = R.ints((npix, C), -3, 3, g) + 4.0    # (no zero row: the dropped one always shows)
    assert not torch.equal(emu_tensor_stats(xi, skip=(last,)), R.tensor_stats(xi)[0])
    x = R.real(npix, C, g)
    want, bound = R.tensor_stats(x)
    assert _ratio(emu_tensor_stats(x, skip=(last,)), want, bound) > 1.0
    mean, invstd, _, _ = R.coeffs(C, g)
    dz, y = R.real(npix, C, g), R.real(npix, C, g)
    want, bound, (g64, _, _) = R.backward_sums(dz, y, mean, invstd, R.NONE, z=y)
    assert _ratio(emu_backward_sums(g64.float(), y, mean, invstd, skip=(last,)), want, bound) > 1.0


def test_wrong_channel_group_summed_twice():
    C, npix = 512, 37
    g = _gen(2, 6)
    x = R.real(npix, C, g)
    want, bound = R.tensor_stats(x)
    t = x.float() - x[0]
    twice = torch.stack([seq_sum(t).double(), seq_sum(t * t).double()], 1)
    twice[256:] *= 2.0
    x0 = x[0].double()
    twice = torch.stack([twice[:, 0] + npix * x0, twice[:, 1] + 2.0 * x0 * twice[:, 0] + npix * x0 * x0], 1)
    r, where = R.check(twice, want, bound)
    assert r > 1.0 and where >= 2 * 256
    assert _ratio(emu_tensor_stats(x), want, bound) <= 1.0


def test_wrong_variance_conventions():
    C = 37
    sums, gamma, beta, rm, rv = _finalize_inputs(C, 7)
    ref = R.finalize(sums, 50.0, gamma, beta, EPS, MOM, rm, rv)
    bad = emu_finalize(sums, 50.0, gamma, beta, rm, rv, normalise_unbiased=True)
    assert _ratio(bad["invstd"], *ref["invstd"]) > 1.0 and _ratio(bad["scale"], *ref["scale"]) > 1.0
    assert _ratio(bad["running_var"], *ref["running_var"]) <= 1.0
    bad = emu_finalize(sums, 50.0, gamma, beta, rm, rv, running_biased=True)
    assert _ratio(bad["running_var"], *ref["running_var"]) > 1.0
    assert _ratio(bad["invstd"], *ref["invstd"]) <= 1.0


def test_wrong_mask_bit_order():
    g = _gen(3, 6)
    z = R.real(9, 8, g)
    m = R.mask_bytes(z)
    rev = torch.zeros_like(m)
    for k in range(4):
        rev |= ((m >> k) & 1) << (3 - k)
    assert not torch.equal(rev, m)
    # ... and read back in the wrong order, the backward sums leave their bound
    bits_bad = torch.stack([(rev >> k) & 1 for k in range(4)], -1).reshape(9, 8).float() * 2.0 - 1.0
    mean, invstd, _, _ = R.coeffs(8, g)
    dz, y = R.real(9, 8, g), R.real(9, 8, g)
    want, bound, _ = R.backward_sums(dz, y, mean, invstd, R.RELU, z=z)
    assert _ratio(emu_backward_sums(emu_g(dz, R.RELU, bits_bad), y, mean, invstd), want, bound) > 1.0


def test_wrong_sg_not_divided_by_count():
    C, npix = 12, 9
    g = _gen(4, 6)
    mean, invstd, gamma, _ = R.coeffs(C, g)
    dz, y = R.real(npix, C, g), R.real(npix, C, g)
    sums2, _, parts = R.backward_sums(dz, y, mean, invstd, R.NONE, z=y)
    dy64, bdy, _, _ = R.backward_apply(parts, sums2, float(npix), invstd, gamma)
    assert _ratio(emu_backward_apply(dz, y, mean, invstd, gamma, sums2, float(npix), 1), dy64, bdy) <= 1.0
    assert _ratio(emu_backward_apply(dz, y, mean, invstd, gamma, sums2, float(npix), 1, divide=False), dy64, bdy) > 1.0


def test_wrong_fp16_accumulation():
    C, npix = 8, 257
    g = _gen(5, 6)
    x = R.real(npix, C, g)
    want, bound = R.tensor_stats(x)
    assert _ratio(emu_tensor_stats(x, dtype=torch.float16), want, bound) > 1.0
    mean, invstd, _, _ = R.coeffs(C, g)
    dz, y = R.real(npix, C, g), R.real(npix, C, g)
    want, bound, _ = R.backward_sums(dz, y, mean, invstd, R.LEAKY, z=y)
    gg = emu_g(dz, R.LEAKY, y)
    assert _ratio(emu_backward_sums(gg, y, mean, invstd), want, bound) <= 1.0
    assert _ratio(emu_backward_sums(gg, y, mean, invstd, dtype=torch.float16), want, bound) > 1.0


def test_wrong_stale_maximum():
    g = _gen(6, 6)
    z = R.real(64, 8, g)
    z[40, 3] = 2.0 * float(z.abs().max())      # the maximum lies in the second half
    assert R.amax_bits(z[:32]) != R.amax_bits(z) and R.amax_bits(z[:32]) < R.amax_bits(z)


def test_path_tables():
    """the tables reach every form norm_act.hip chooses by shape, and the exact cases stay exact in fp32"""
    assert {R.column_form(C) for C in R.C_ALL} == {"vector", "grouped", "generic"}
    assert {C for C in R.C_ALL if R.apply_form(C) == "float4"} == {12, 24, 96, 192, 320}
    assert {C for C in R.C_ALL if R.apply_form(C) == "scalar"} == {1, 3, 65, 130}
    assert max(R.TILES_1PHASE) == R.RS1_MAX_TILES < min(R.TILES_2PHASE)
    C, npix = R.TWO_PHASE
    assert -(-npix // 32) > R.RS1_MAX_TILES      # 32 rows: the minimal chunk of the generic form
    for C in R.C_ALL:
        assert max(R.npix_list(C)) * 36 < 2 ** 23 and R.TWO_PHASE[1] * 36 < 2 ** 23      # exact cases stay exact in fp32
    assert R.EW_SWEEP[0] * R.EW_SWEEP[1] // 4 > 4096 * 256
