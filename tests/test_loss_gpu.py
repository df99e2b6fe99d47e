"""The loss, argmax and F1-count kernels (csrc/loss.hip, csrc/loss_px.h) against the fp64 restatement and the derived
per-element bounds of tests/loss_ref.py, on the case tables that tests/test_loss_ref_cpu.py checks without a GPU.

The kernels are called through the C ABI.  Every output (dlogits, the 32 doubles of acc, the loss, the workspace of exactly
xv2_loss_workspace bytes) is a view inside a larger allocation; each case runs twice, with the outputs and everything around
them preset to NaN and to 2^100: the two runs must agree bit for bit and leave every guard element, acc[15:] included, as it
was.  Each comparison prints `loss_ref ratio <op> <ratio>` (error / bound, worst element); profiles/loss_ref_ratios.md holds
the worst per operation.

Pinned: the empty building mask (0.0 for dice alone, NaN otherwise, all-zero gradient); a NaN or +Inf logit on a counted pixel
gives a non-finite loss, in every channel and for every label (mse: the ReLU keeps a NaN; coral: +Inf on a level the label has
reached is NaN as in the oracle, whose 0 * Inf it is, not logsigmoid(+Inf) = 0); a NaN on a masked-out pixel changes nothing."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests.golden.cases import ARGS

pytestmark = pytest.mark.gpu

PAD = 64
FILLS = (float("nan"), 2.0 ** 100)


def dev():
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """n elements inside an allocation of n + 2 PAD, all preset to `fill`"""

    def __init__(self, n, dtype, fill):
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev())
        self.before = bits(self.buf)
        self.n = n
        self.view = self.buf[PAD:PAD + n]

    def intact(self, written=None):
        """the guards, and the elements of the view from `written` on, are what they were"""
        now = bits(self.buf)
        lo = PAD + (self.n if written is None else written)
        return torch.equal(now[:PAD], self.before[:PAD]) and torch.equal(now[lo:], self.before[lo:])


def run(x, y, terms, post, ls, scales, fill):
    """forward and one backward per (gscale, weight) through the C ABI -> acc [15] f64, loss f32 0-d, [dlogits]"""
    from xview2_amd import _capi
    N, C, H, W = x.shape
    xg, yg = x.to(dev()).contiguous(), y.to(dev()).contiguous()
    ws_bytes = _capi.query("xv2_loss_workspace", N, C, H, W)
    assert ws_bytes % 8 == 0
    ws = Guarded(ws_bytes // 4, torch.float32, fill)
    acc = Guarded(32, torch.float64, fill)
    loss = Guarded(1, torch.float32, fill)
    assert acc.view.data_ptr() % 8 == 0 and ws.view.data_ptr() % 8 == 0
    _capi.call("xv2_loss_forward", xg, yg, N, C, H, W, ls, post, terms, acc.view, loss.view, ws.view)
    grads = []
    for gscale, weight in scales:
        d = Guarded(x.numel(), torch.float32, fill)
        gs = torch.full((1,), gscale, dtype=torch.float32, device=dev())
        _capi.call("xv2_loss_backward", xg, yg, N, C, H, W, ls, post, terms, acc.view, gs, float(weight), d.view)
        torch.cuda.synchronize()
        assert d.intact(), "dlogits guard"
        grads.append(d.view.cpu().reshape(x.shape))
    torch.cuda.synchronize()
    assert ws.intact() and loss.intact(), "workspace / loss guard"
    assert acc.intact(written=15), "acc guard or acc[15:]"
    return acc.view[:15].cpu(), loss.view.cpu().reshape(()), grads


def run_twice(x, y, terms, post, ls=1, scales=((1.0, 1.0),)):
    a = run(x, y, terms, post, ls, scales, FILLS[0])
    b = run(x, y, terms, post, ls, scales, FILLS[1])
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), "acc / loss depend on what was there"
    for ga, gb in zip(a[2], b[2]):
        assert torch.equal(bits(ga), bits(gb)), "dlogits depend on what was there"
    return a


def close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item() / scale
    assert err <= tol, "%s: rel-to-max error %.3e > %.1e" % (what, err, tol)


def family(case):
    return case["tpl"] if R.aux(case["terms"]) else "c%d" % case["C"]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_loss_kernels_within_their_bounds(case):
    x, y = R.make(case)
    args = (x, y, case["terms"], case["post"], case["ls"])
    acc, loss, grads = run_twice(*args, scales=case["scales"])
    B = R.bounds(*args)
    fam = family(case)
    worst = {"acc": R.check(acc, B["acc64"], B["acc"]), "loss": R.check(loss, B["loss64"], B["loss"])}
    g1 = None
    for (gscale, weight), g in zip(case["scales"], grads):
        g64 = R.backward(*args, gscale, weight)
        g1 = g64 if (gscale, weight) == (1.0, 1.0) else g1
        r = R.check(g, g64, B["grad"] * R.scale(gscale, weight))
        if gscale == 0.0:
            assert float(g.abs().max()) == 0.0, "gscale = 0 must give exact zeros"
        worst["grad"] = max(worst.get("grad", r), r)
    for what, (ratio, where) in worst.items():
        print("loss_ref ratio %s_%s %.4f" % (fam, what, ratio))
    for what, (ratio, where) in worst.items():
        assert ratio <= 1.0, "%s %s: error / bound %.3f at %d" % (case["name"], what, ratio, where)
    if case["regime"] == "randn2":      # the two scalar tolerances of tests/test_ops_gpu.py, meaningful in this regime
        L = float(B["loss64"])
        assert abs(float(loss) - L) <= 2e-6 * max(1.0, abs(L))
        close(grads[0], g1, 2e-5, "dlogits " + case["name"])


# ---- pinned behaviours ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("terms,C", R.EMPTY_MASK)
def test_empty_building_mask(terms, C):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, C, 5, 9, generator=g) * 2
    y = torch.zeros(2, 5, 9, dtype=torch.uint8)
    acc, loss, (d,) = run_twice(x, y, terms, 1)
    _, L = R.forward(x, y, terms, 1)
    assert float(acc[14]) == 0.0
    if terms == R.DICE:
        assert float(L) == 0.0 and float(loss) == 0.0 and not math.copysign(1.0, float(loss)) < 0
    else:
        assert math.isnan(float(L)) and math.isnan(float(loss))
    assert float(d.abs().max()) == 0.0


NONFINITE = [("c2", 1), ("c2", 2), ("c2", 4), ("c2", 7), ("c4post", 1), ("c4post", 6), ("c4post", 7), ("mse", R.MSE),
             ("coral", R.CORAL)]


@pytest.mark.parametrize("tpl,terms", NONFINITE)
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_nonfinite_logit_on_a_counted_pixel_gives_a_nonfinite_loss(tpl, terms, value):
    case = R._case(tpl, (2, 7, 13, 1), terms)
    x, y = R.make(case)
    _, mask = R.targets(y, x.shape, case["post"], 1)
    for c in range(x.shape[1]):
        n, h, w = (int(v) for v in torch.nonzero(mask)[3 + c])
        xc = x.clone()
        xc[n, c, h, w] = value
        _, loss, _ = run_twice(xc, y, terms, case["post"])
        assert not math.isfinite(float(loss)), (c, float(loss))


@pytest.mark.parametrize("tpl", ["c4post", "c2post", "mse", "coral"])
def test_nan_on_a_masked_out_pixel_changes_nothing(tpl):
    case = R._case(tpl, (2, 7, 13, 1))
    x, y = R.make(case)
    _, mask = R.targets(y, x.shape, 1, 1)
    n, h, w = (int(v) for v in torch.nonzero(~mask)[2])
    x0, x1 = x.clone(), x.clone()
    x0[n, :, h, w] = 0.0
    x1[n, :, h, w] = 0.0
    x1[n, x.shape[1] - 1, h, w] = float("nan")
    a = run_twice(x0, y, case["terms"], 1)
    b = run_twice(x1, y, case["terms"], 1)
    assert math.isfinite(float(a[1]))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert torch.equal(bits(a[2][0]), bits(b[2][0])) and float(b[2][0][n, :, h, w].abs().max()) == 0.0


# ---- composition through criterion.Loss and compute_loss -------------------------------------------------------------------

BIT = {"dice": R.DICE, "focal": R.FOCAL, "ce": R.CE, "ohem": R.CE, "ohem_hard": R.CE}


def groups(names):
    """criterion.Loss: the distinct terms share one launch, a name given again goes into a further launch"""
    left = {}
    for n in names:
        left[BIT[n]] = left.get(BIT[n], 0) + 1
    out = []
    while left:
        out.append(sum(left))
        left = {b: k - 1 for b, k in left.items() if k > 1}
    return out


COMPOSED = ([("pre", "dice+dice"), ("pre", "ce+ohem"), ("post", "focal+ce+focal"), ("post", "ohem_hard"), ("post", "ohem_hard+dice")] +
            [(task, "+".join(p)) for task in ("pre", "post") for p in itertools.permutations(("dice", "focal", "ce"))])


@pytest.mark.parametrize("task,loss_str", COMPOSED)
def test_composed_loss_strings(task, loss_str):
    from xview2_amd import criterion
    post = int(task == "post")
    case = R._case("c4post" if post else "c2", (2, 7, 13, 1))
    x, y = R.make(case)
    names = loss_str.split("+")
    xg = x.to(dev()).requires_grad_(True)
    lh = criterion.Loss(ARGS(type=task, loss_str=loss_str))(xg, y.to(dev()))
    lh.backward()
    xr = x.double().requires_grad_(True)
    lr = sum(R.forward(xr, y, BIT[n], post)[1] for n in names)
    lr.backward()
    gl = groups(names)
    assert sorted(b for g in gl for b in (1, 2, 4) if g & b) == sorted(BIT[n] for n in names)
    parts = [(R.bounds(x, y, g, post), R.backward(x, y, g, post)) for g in gl]
    extra = (len(gl) - 1) * R.U      # the launches' results are added in fp32, the loss and every gradient element
    bl = sum(B["loss"] for B, _ in parts) + extra * sum(abs(B["loss64"]) for B, _ in parts)
    bg = sum(B["grad"] for B, _ in parts) + extra * sum(g.abs() for _, g in parts)
    rl, rg = R.check(lh.detach().reshape(()), lr.detach(), bl), R.check(xg.grad, xr.grad, bg)
    print("loss_ref ratio composed_loss %.4f\nloss_ref ratio composed_grad %.4f" % (rl[0], rg[0]))
    assert rl[0] <= 1.0 and rg[0] <= 1.0, (rl, rg)


def test_deep_supervision_three_heads_non_square():
    from xview2_amd import criterion
    a = ARGS(type="post", loss_str="focal+dice", deep_supervision=True)
    g = torch.Generator().manual_seed(31)
    preds = [torch.randn(2, 4, 24 // s, 40 // s, generator=g) * 2 for s in (1, 2, 4)]
    y = torch.randint(0, 5, (2, 24, 40), generator=g, dtype=torch.uint8)
    pg = [p.to(dev()).requires_grad_(True) for p in preds]
    lh = criterion.compute_loss(criterion.Loss(a), pg, y.to(dev()), True)
    lh.backward()
    terms, c_norm = R.FOCAL | R.DICE, 1 / (2 - 2 ** -3)
    Bs = [R.bounds(p, y, terms, 1, 2 ** j) for j, p in enumerate(preds)]
    L = c_norm * sum(0.5 ** j * B["loss64"] for j, B in enumerate(Bs))
    # two additions, c_norm as fp32 and the product with it: 4 u of the terms' magnitudes
    bL = c_norm * sum(0.5 ** j * (B["loss"] + 4 * R.U * abs(B["loss64"])) for j, B in enumerate(Bs))
    r = R.check(lh.detach().reshape(()), L, bL)
    print("loss_ref ratio ds_loss %.4f" % r[0])
    assert r[0] <= 1.0, r
    for j, (p, B) in enumerate(zip(preds, Bs)):
        w = c_norm * 0.5 ** j
        g64 = w * R.backward(p, y, terms, 1, 2 ** j)
        r = R.check(pg[j].grad, g64, w * B["grad"] + 2 * R.U * g64.abs())      # (the incoming gradient is w as fp32)
        print("loss_ref ratio ds_grad %.4f" % r[0])
        assert r[0] <= 1.0, (j, r)


@pytest.mark.parametrize("loss_str,C", [("mse+dice", 4), ("coral+ce", 4), ("dice+mse", 1), ("ce+coral", 3)])
def test_mse_and_coral_do_not_compose(loss_str, C):
    from xview2_amd import criterion
    fn = criterion.Loss(ARGS(type="post", loss_str=loss_str))
    x = torch.randn(2, C, 5, 9).to(dev())
    y = torch.randint(0, 5, (2, 5, 9), dtype=torch.uint8).to(dev())
    with pytest.raises(RuntimeError):
        fn(x, y)


# ---- argument errors: refused before any launch -----------------------------------------------------------------------------

def test_argument_errors_come_before_any_launch():
    from xview2_amd import _capi
    x = torch.randn(1, 5, 4, 6).to(dev())
    y = torch.ones(1, 4, 6, dtype=torch.uint8, device=dev())
    ws = Guarded(_capi.query("xv2_loss_workspace", 1, 4, 4, 6) // 4, torch.float32, FILLS[1])
    acc, loss = Guarded(32, torch.float64, FILLS[1]), Guarded(1, torch.float32, FILLS[1])
    for terms, C in ((0, 2), (9, 4), (R.DICE, 3), (R.MSE, 2), (R.CORAL, 4), (7, 1)):
        with pytest.raises(RuntimeError):
            _capi.call("xv2_loss_forward", x, y, 1, C, 4, 6, 1, 0, terms, acc.view, loss.view, ws.view)
    # lstride = 0, H = 0, N = 0 and a null labels pointer, forward and backward
    d = Guarded(x.numel(), torch.float32, FILLS[1])
    gs = torch.ones(1, dtype=torch.float32, device=dev())
    for N, H, ls, labels in ((1, 4, 0, y), (1, 0, 1, y), (0, 4, 1, y), (1, 4, 1, None)):
        with pytest.raises(RuntimeError):
            _capi.call("xv2_loss_forward", x, labels, N, 4, H, 6, ls, 0, R.CE, acc.view, loss.view, ws.view)
        with pytest.raises(RuntimeError):
            _capi.call("xv2_loss_backward", x, labels, N, 4, H, 6, ls, 0, R.CE, acc.view, gs, 1.0, d.view)
    out = Guarded(24, torch.uint8, 7)
    with pytest.raises(RuntimeError):
        _capi.call("xv2_argmax_nchw", x, 1, 5, 24, 0, out.view)
    with pytest.raises(RuntimeError):
        _capi.call("xv2_argmax_nchw", x, 1, 1, 24, 0, out.view)
    counts = Guarded(12, torch.int64, 3)
    for n_class, total in ((6, 24), (1, 24), (5, 0)):
        with pytest.raises(RuntimeError):
            _capi.call("xv2_f1_counts", y, y, total, n_class, 0, counts.view)
    torch.cuda.synchronize()
    for gd in (ws, acc, loss, d, out, counts):
        assert gd.intact(written=0)


# ---- xv2_argmax_nchw -----------------------------------------------------------------------------------------------------------

def argmax_gpu(x, add):
    from xview2_amd import _capi
    N, C, hw = x.shape
    out = Guarded(N * hw, torch.uint8, 99)
    _capi.call("xv2_argmax_nchw", x.to(dev()).contiguous(), N, C, hw, add, out.view)
    torch.cuda.synchronize()
    assert out.intact()
    return out.view.cpu().reshape(N, hw).long()


SPECIAL = [float("nan"), -math.inf, math.inf, 0.0, -0.0, 1.0]


def argmax_input(N, C, hw, seed, nonfinite=0.1):
    """values from a small set (ties in most pixels, +0.0 against -0.0), +-Inf and NaN sprinkled over every channel"""
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor([-1.0, -0.0, 0.0, 1.0, 2.0])[torch.randint(0, 5, (N, C, hw), generator=g)]
    pick = torch.rand((N, C, hw), generator=g)
    x = torch.where(pick < nonfinite, torch.tensor(float("nan")), x)
    x = torch.where((pick >= nonfinite) & (pick < 1.5 * nonfinite), torch.tensor(math.inf), x)
    return torch.where((pick >= 1.5 * nonfinite) & (pick < 2 * nonfinite), torch.tensor(-math.inf), x)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("add", [0, 1])
def test_argmax_equals_torch_argmax(C, add):
    for hw in (1, 255, 257, 7 * 13):
        for nonfinite in (0.0, 0.1):
            x = argmax_input(2, C, hw, 100 * C + hw, nonfinite)
            assert torch.equal(argmax_gpu(x, add), torch.argmax(x, 1) + add), (hw, nonfinite)
    g = torch.Generator().manual_seed(C)
    x = torch.randn(3, C, 257, generator=g)
    assert torch.equal(argmax_gpu(x, add), torch.argmax(x, 1) + add)
    # every combination of NaN, -Inf, +Inf, +0.0, -0.0 and 1 over the channels, one pixel each
    rows = torch.tensor(list(itertools.product(SPECIAL, repeat=C)), dtype=torch.float32)
    x = rows.t().contiguous().view(1, C, -1)
    want = torch.argmax(x, 1) + add
    assert torch.equal(argmax_gpu(x, add), want)
    if C == 3:      # what "a NaN is the maximum, the first one wins" means, spelled out
        nan = float("nan")
        x = torch.tensor([[nan, 1, 2], [1, nan, 3], [1, nan, nan], [math.inf, 1, nan], [0.0, -0.0, -1]]).t().contiguous()
        assert argmax_gpu(x.view(1, 3, 5), add)[0].tolist() == [v + add for v in (0, 1, 1, 2, 0)]


def test_argmax_second_sweep():
    x = argmax_input(1, 4, 1025 * 1024, 7, 0.02)
    assert torch.equal(argmax_gpu(x, 1), torch.argmax(x, 1) + 1)


# ---- xv2_f1_counts -------------------------------------------------------------------------------------------------------------

def f1_numpy(pred, tgt, n_class, masked):
    p, t = pred.numpy().astype(np.int64), tgt.numpy().astype(np.int64)
    if masked:
        p, t = p[t > 0], t[t > 0]
    out = np.zeros(12, dtype=np.int64)
    for c in range(1, n_class):
        out[(c - 1) * 3:(c - 1) * 3 + 3] = [np.sum((p == c) & (t == c)), np.sum((p != c) & (t == c)), np.sum((p == c) & (t != c))]
    return out


def f1_gpu(pred, tgt, n_class, masked, counts):
    from xview2_amd import _capi
    _capi.call("xv2_f1_counts", pred.to(dev()), tgt.to(dev()), pred.numel(), n_class, masked, counts.view)
    torch.cuda.synchronize()
    return counts.view.cpu().numpy().copy()


@pytest.mark.parametrize("n_class", [2, 3, 4, 5])
@pytest.mark.parametrize("masked", [0, 1])
def test_f1_counts_equal_a_numpy_count(n_class, masked):
    for total in (1, 255, 256, 257, 2 ** 22 + 3):
        g = torch.Generator().manual_seed(total % 1000 + n_class)
        pred = torch.randint(0, 6, (total,), generator=g, dtype=torch.uint8)      # 0 .. 5: values outside the counted classes occur
        tgt = torch.randint(0, 6, (total,), generator=g, dtype=torch.uint8)
        counts = Guarded(12, torch.int64, 0)
        start = np.arange(12, dtype=np.int64) * 1000 + 5      # non-zero initial counts are kept, every call adds
        counts.view.copy_(torch.from_numpy(start))
        one = f1_numpy(pred, tgt, n_class, masked)
        assert np.array_equal(f1_gpu(pred, tgt, n_class, masked, counts), start + one), total
        assert np.array_equal(f1_gpu(pred, tgt, n_class, masked, counts), start + 2 * one), total
        now = bits(counts.buf)
        assert torch.equal(now[:PAD], counts.before[:PAD]) and torch.equal(now[PAD + 12:], counts.before[PAD + 12:])
        assert one[(n_class - 1) * 3:].sum() == 0
    # all pixels in one class: a hit for that class, nothing for any other; and all of them missed
    for c in range(0, 6):
        pred = torch.full((257,), c, dtype=torch.uint8)
        for tgt in (pred, torch.full((257,), (c + 1) % 6, dtype=torch.uint8)):
            counts = Guarded(12, torch.int64, 0)
            assert np.array_equal(f1_gpu(pred, tgt, n_class, masked, counts), f1_numpy(pred, tgt, n_class, masked))
