"""The gates of tests/pool_ref.py, tested without a GPU: torch's own fp32 CPU operations pass them on every case of the tables
(this pins the bounds), deliberately wrong float64 variants fail them on at least one case (the gates have teeth), and the
output extent AvgPoolFn computes agrees with torch's."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import pool_ref as R

N, C = R.N_C


def _gen(*key):
    return torch.Generator().manual_seed(1000003 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _f32_bwd(f, x, dy):
    x = x.clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(f(x), x, dy)
    return dx


def _ok(y, y64, bound, what):
    r, where = R.check(y, y64, bound)
    assert r <= 1.0, "%s: error / bound %.3f at flat index %d" % (what, r, where)
    return r


# ---- (a) fp32 CPU operations pass ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
@pytest.mark.parametrize("ties", [False, True])
def test_maxpool_fp32_cpu_passes(shape, ties):
    g = _gen(*shape, ties)
    x = R.tie_heavy(shape, g) if ties else R.lognormal(shape, g)
    f = lambda t: R.nhwc(F.max_pool2d(R.nchw(t), 3, 2, 1))      # noqa: E731
    y = f(x)
    assert torch.equal(y.double(), R.maxpool3x3s2_fwd(x))
    dy = R.lognormal(tuple(y.shape), g)
    dx64 = R.maxpool3x3s2_bwd(x, dy)
    assert torch.equal(R.maxpool3x3s2_bwd_rule(x, dy, "first"), dx64), "the spelled-out backward is not torch's"
    bound, _, T = R.maxpool_bwd_bound(x, dy)
    assert float(T.max()) <= 4
    _ok(_f32_bwd(f, x, dy), dx64, bound, "max-pool backward %s" % (shape,))


@pytest.mark.parametrize("case", R.avg_cases())
def test_avgpool_fp32_cpu_passes(case):
    k, s, pad, ceil, incl, H, W = case
    g = _gen(*case)
    x = R.lognormal((N, H, W, C), g)
    f = lambda t: R.nhwc(F.avg_pool2d(R.nchw(t), k, s, pad, ceil, incl))      # noqa: E731
    y64 = R.avgpool_fwd(x, k, s, pad, ceil, incl)
    _ok(f(x), y64, R.avgpool_fwd_bound(x, k, s, pad, ceil, incl), "avg-pool forward %s" % (case,))
    dy = R.lognormal(tuple(y64.shape), g)
    bound, _, T = R.avgpool_bwd_bound(dy, (H, W), k, s, pad, ceil, incl)
    assert float(T.max()) <= math.ceil(k / s) ** 2
    dx64 = R.avgpool_bwd(dy, (H, W), k, s, pad, ceil, incl)
    _ok(_f32_bwd(f, x, dy), dx64, bound, "avg-pool backward %s" % (case,))
    # the spelled-out form the wrong variants below are made from is the same map
    Mh, Mw = R.avg_matrix(H, k, s, pad, ceil, incl), R.avg_matrix(W, k, s, pad, ceil, incl)
    _ok(R.sep_fwd(x, Mh, Mw), y64, 1e-15 * R.avgpool_fwd(x.double().abs(), k, s, pad, ceil, incl), "avg_matrix %s" % (case,))


@pytest.mark.parametrize("hw", R.ADAPTIVE_HW)
@pytest.mark.parametrize("bins", R.ADAPTIVE_BINS)
def test_adaptive_fp32_cpu_passes(hw, bins):
    H, W = hw
    g = _gen(H, W, bins)
    x = R.lognormal((N, H, W, C), g)
    f = lambda t: R.nhwc(F.adaptive_avg_pool2d(R.nchw(t), bins))      # noqa: E731
    y64 = R.adaptive_fwd(x, bins)
    _ok(f(x), y64, R.adaptive_fwd_bound(x, bins), "adaptive forward %s bins %d" % (hw, bins))
    dy = R.lognormal(tuple(y64.shape), g)
    bound, _ = R.adaptive_bwd_bound(dy, hw, bins)
    _ok(_f32_bwd(f, x, dy), R.adaptive_bwd(dy, hw, bins), bound, "adaptive backward %s bins %d" % (hw, bins))
    _ok(R.sep_fwd(x, R.ada_matrix(H, bins), R.ada_matrix(W, bins)), y64, 1e-15 * R.adaptive_fwd(x.double().abs(), bins), "ada_matrix")


@pytest.mark.parametrize("case", R.BILINEAR_CASES)
def test_bilinear_fp32_cpu_passes(case):
    IH, IW, OH, OW = case
    g = _gen(*case)
    x = R.lognormal((N, IH, IW, C), g)
    f = lambda t: R.nhwc(F.interpolate(R.nchw(t), (OH, OW), mode="bilinear", align_corners=True))      # noqa: E731
    y64 = R.bilinear_fwd(x, OH, OW)
    if (IH, IW) == (OH, OW):
        assert torch.equal(f(x).double(), x.double()) and torch.equal(y64, x.double())
    _ok(f(x), y64, R.bilinear_fwd_bound(x, OH, OW), "bilinear forward %s" % (case,))
    dy = R.lognormal((N, OH, OW, C), g)
    bound, a = R.bilinear_bwd_bound(dy, IH, IW)
    dx64 = R.bilinear_bwd(dy, IH, IW)
    _ok(_f32_bwd(f, x, dy), dx64, bound, "bilinear backward %s" % (case,))
    Mh, Mw = R.bil_matrix(IH, OH), R.bil_matrix(IW, OW)
    _ok(R.sep_bwd(dy, Mh, Mw), dx64, 1e-13 * a, "bil_matrix %s" % (case,))


@pytest.mark.parametrize("Cg", R.GATE_C)
def test_gate_mul_fp32_cpu_passes(Cg):
    g = _gen(Cg)
    skip, dout = R.lognormal(R.GATE_PIX + (Cg,), g), R.lognormal(R.GATE_PIX + (Cg,), g)
    gate = torch.rand(R.GATE_PIX + (1,), generator=g)
    out, dskip, dgate, scale = R.gate_mul(skip, gate, dout)
    _ok(skip * gate, out, R.U * out.abs(), "gate out")
    _ok(dout * gate, dskip, R.U * dskip.abs(), "gate dskip")
    _ok((dout * skip).sum(-1, keepdim=True), dgate, R.gate_dgate_bound(Cg, scale), "gate dgate C=%d" % Cg)


def test_add_relu_and_concat_reference():
    g = _gen(7)
    a, b = R.lognormal((2, 3, 5, 8), g), R.lognormal((2, 3, 5, 8), g)
    b[0] = -a[0]
    a[1, 0] = 0.0
    r = R.add_relu(a, b)
    assert torch.equal(r, F.relu(a + b).double()) and float(r[0].abs().max()) == 0.0
    dr = R.lognormal((2, 3, 5, 8), g)
    assert torch.equal(R.add_relu_bwd(r, dr), _f32_bwd(lambda t: F.relu(t + b), a, dr).double())
    ab, bb = a.bfloat16(), b.bfloat16()
    assert torch.equal(R.add_relu(ab, bb), F.relu(ab.float() + bb.float()).bfloat16().double())
    xs = [R.lognormal((2, 3, 5, c), g) for c in (8, 4, 64)]
    cat = R.cat_channels(xs)
    assert all(torch.equal(p, q.double()) for p, q in zip(R.split_channels(cat, (8, 4, 64)), xs))
    t = R.lognormal((4, 3, 5, 8), g)
    assert torch.equal(R.pair_split(R.pair_cat(t)), t.double())
    assert torch.equal(R.pair_cat(t)[1, :, :, 8:], t[3].double())


def test_accumulate_bound_counts_every_addition():
    """avg-pool backward, k = 3, s = 1, pad = 1, onto a gradient `old` much larger than its own terms, in the kernel's order
    (old first, then one fp32 addition per window): within the bound that counts T_i additions onto old, beyond one that
    counts a single addition"""
    g = _gen(31)
    H, W = 17, 19
    dy = R.lognormal((N, H, W, C), g)
    old = R.lognormal((N, H, W, C), g) * 64.0
    inv = torch.tensor(1.0, dtype=torch.float32) / 9.0
    acc = old.clone()
    dyp = F.pad(dy, (0, 0, 1, 1, 1, 1))
    for kh in (2, 1, 0):          # windows in ascending (oh, ow): oh = ih + 1 - kh
        for kw in (2, 1, 0):
            inside = F.pad(torch.ones(N, H, W, 1), (0, 0, 1, 1, 1, 1))[:, kh:kh + H, kw:kw + W] > 0
            acc = torch.where(inside, acc + dyp[:, kh:kh + H, kw:kw + W] * inv, acc)
    bound, a, T = R.avgpool_bwd_bound(dy, (H, W), 3, 1, 1, False, True)
    ref = old.double() + R.avgpool_bwd(dy, (H, W), 3, 1, 1, False, True)
    r_all, _ = R.check(acc, ref, R.accumulated(bound, a, old, T, ref))
    r_one, _ = R.check(acc, ref, R.accumulated(bound, a, old, 1, ref))
    assert r_all <= 1.0 < r_one, (r_all, r_one)


# ---- (b) wrong variants fail --------------------------------------------------------------------------------------------

def _killed(cases, run):
    """run(case) -> error / bound ratio of the wrong variant; at least one case must reject it"""
    worst = [run(c) for c in cases]
    assert any(r > 1.0 for r in worst), "the wrong variant passes every case: %s" % (worst,)


def _avg_io(case):
    k, s, pad, ceil, incl, H, W = case
    g = _gen(*case)
    x = R.lognormal((N, H, W, C), g)
    return x, R.avgpool_fwd(x, k, s, pad, ceil, incl), R.avgpool_fwd_bound(x, k, s, pad, ceil, incl)


def test_avgpool_count_include_pad_flipped_fails():
    def run(case):
        k, s, pad, ceil, incl, H, W = case
        x, y64, b = _avg_io(case)
        return R.check(R.avgpool_fwd(x, k, s, pad, ceil, not incl), y64, b)[0]
    _killed(R.avg_cases(), run)


def test_avgpool_unclipped_divisor_fails():
    def run(case):
        k, s, pad, ceil, incl, H, W = case
        x, y64, b = _avg_io(case)
        wrong = R.sep_fwd(x, R.avg_matrix(H, k, s, pad, ceil, incl, full_divisor=True), R.avg_matrix(W, k, s, pad, ceil, incl, full_divisor=True))
        return R.check(wrong, y64, b)[0]
    _killed(R.avg_cases(), run)


def test_avgpool_ceil_without_last_window_rule_fails():
    def run(case):
        k, s, pad, ceil, incl, H, W = case
        x, y64, b = _avg_io(case)
        wrong = R.sep_fwd(x, R.avg_matrix(H, k, s, pad, ceil, incl, last_rule=False), R.avg_matrix(W, k, s, pad, ceil, incl, last_rule=False))
        return R.check(wrong, y64, b)[0]
    _killed(R.avg_cases(), run)


def test_adaptive_end_floor_fails():
    def run(c):
        (H, W), bins = c
        x = R.lognormal((N, H, W, C), _gen(H, W, bins))
        wrong = R.sep_fwd(x, R.ada_matrix(H, bins, end_floor=True), R.ada_matrix(W, bins, end_floor=True))
        return R.check(wrong, R.adaptive_fwd(x, bins), R.adaptive_fwd_bound(x, bins))[0]
    _killed([(hw, b) for hw in R.ADAPTIVE_HW for b in R.ADAPTIVE_BINS], run)


def test_bilinear_align_corners_false_fails():
    def run(case):
        IH, IW, OH, OW = case
        x = R.lognormal((N, IH, IW, C), _gen(*case))
        return R.check(R.bilinear_fwd(x, OH, OW, align_corners=False), R.bilinear_fwd(x, OH, OW), R.bilinear_fwd_bound(x, OH, OW))[0]
    _killed(R.BILINEAR_CASES, run)


def test_bilinear_backward_narrow_candidate_range_fails():
    def run(case):
        IH, IW, OH, OW = case
        dy = R.lognormal((N, OH, OW, C), _gen(*case))
        wrong = R.sep_bwd(dy, R.bil_matrix_dropped(IH, OH), R.bil_matrix_dropped(IW, OW))
        return R.check(wrong, R.bilinear_bwd(dy, IH, IW), R.bilinear_bwd_bound(dy, IH, IW)[0])[0]
    _killed(R.BILINEAR_CASES, run)


def test_bilinear_candidate_range_holds_every_contribution():
    """bil_range as the kernel computes it loses nothing: every output with a non-zero weight lies inside [lo, hi]"""
    for (IH, IW, OH, OW) in R.BILINEAR_CASES + [(260, 260, 520, 520), (520, 520, 260, 260)]:
        for (I, O) in ((IH, OH), (IW, OW)):
            M = R.bil_matrix(I, O)
            for i, (lo, hi) in enumerate(R.bil_candidates(I, O)):
                nz = torch.nonzero(M[:, i]).flatten()
                assert nz.numel() == 0 or (int(nz.min()) >= lo and int(nz.max()) <= hi), (I, O, i, lo, hi)


@pytest.mark.parametrize("rule", ["last", "all"])
def test_maxpool_wrong_tie_rule_fails(rule):
    def run(shape):
        g = _gen(*shape, True)
        x = R.tie_heavy(shape, g)
        dy = R.lognormal(tuple(R.maxpool3x3s2_fwd(x).shape), g)
        return R.check(R.maxpool3x3s2_bwd_rule(x, dy, rule), R.maxpool3x3s2_bwd(x, dy), R.maxpool_bwd_bound(x, dy)[0])[0]
    _killed(R.MAXPOOL_SHAPES, run)


def test_gate_dgate_first_chunk_only_fails():
    def run(Cg):
        g = _gen(Cg)
        skip, dout = R.lognormal(R.GATE_PIX + (Cg,), g), R.lognormal(R.GATE_PIX + (Cg,), g)
        _, _, dgate, scale = R.gate_mul(skip, torch.rand(R.GATE_PIX + (1,), generator=g), dout)
        return R.check(R.gate_dgate_first_chunk(skip, dout), dgate, R.gate_dgate_bound(Cg, scale))[0]
    _killed(R.GATE_C, run)


def test_check_rejects_what_it_must():
    y64 = torch.tensor([1.0, 0.0, -2.0], dtype=torch.float64)
    b = torch.tensor([1e-6, 0.0, 1e-6], dtype=torch.float64)
    assert R.check(y64.float(), y64, b) == (0.0, 0)
    assert R.check(torch.tensor([1.0, 1e-30, -2.0]), y64, b) == (math.inf, 1)          # bound 0: exact or nothing
    assert R.check(torch.tensor([1.0, 0.0, float("nan")]), y64, b) == (math.inf, 2)
    assert R.check(torch.zeros(4), y64, b)[0] == math.inf                                # another shape
    r, where = R.check(torch.tensor([1.0, 0.0, -2.0 - 5e-7], dtype=torch.float64), y64, b)
    assert where == 2 and abs(r - 0.5) < 1e-6


# ---- (c) the output extent of AvgPoolFn ---------------------------------------------------------------------------------

def test_avgpool_out_size_is_torchs():
    from xview2_amd.ops import avgpool_out_size
    n = 0
    for k in (1, 2, 3):
        for s in (1, 2, 3):
            for pad in range(k // 2 + 1):
                for ceil in (False, True):
                    for L in range(1, 41):
                        if L + 2 * pad < k:
                            continue      # torch rejects it
                        want = F.avg_pool2d(torch.zeros(1, 1, L, L), k, s, pad, ceil).shape[-1]
                        assert avgpool_out_size(L, k, s, pad, ceil) == want == R.avgpool_out_size(L, k, s, pad, ceil), (L, k, s, pad, ceil)
                        n += 1
    assert n > 1000
