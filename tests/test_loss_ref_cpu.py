"""The gates of tests/loss_ref.py, checked without a GPU: (a) the bounds admit a correct fp32 evaluation in the kernels' order of
operations, (b) every deliberately wrong variant exceeds a bound on some case of the tables, (c) the closed-form gradient
equals autograd and the restatement equals the oracle's Loss, (d) the empty building mask is pinned to the oracle's
behaviour."""
import math

import pytest
import torch

from tests import loss_ref as R
from tests.golden.cases import ARGS, LOSS_CASES, loss_inputs

BITS = {"dice": R.DICE, "focal": R.FOCAL, "ce": R.CE, "ohem": R.CE, "mse": R.MSE, "coral": R.CORAL}


def ratios(case, fwd, bwd):
    """worst ratio over the acc sums, the loss and every gradient of one case; fwd / bwd produce what is compared"""
    x, y = R.make(case)
    args = (x, y, case["terms"], case["post"], case["ls"])
    B = R.bounds(*args)
    acc, loss = fwd(*args)
    out = {"acc": R.check(acc, B["acc64"], B["acc"])[0], "loss": R.check(loss.reshape(()), B["loss64"].reshape(()), B["loss"])[0]}
    worst = 0.0
    for gscale, weight in case["scales"]:
        g = bwd(*args, acc, gscale, weight)
        g64 = R.backward(*args, gscale, weight)
        r = R.check(g, g64, B["grad"] * R.scale(gscale, weight))[0]
        if gscale == 0.0:
            assert float(g64.abs().max()) == 0.0
        worst = max(worst, r)
    out["grad"] = worst
    return out


@pytest.mark.parametrize("case", R.SMALL, ids=[c["name"] for c in R.SMALL])
def test_bounds_admit_the_fp32_transcription(case):
    r = ratios(case, R.f32_forward, R.f32_backward)
    assert max(r.values()) <= 1.0, r


def test_the_tables_hold_what_they_should():
    names = {c["name"] for c in R.CASES}
    assert len(names) == len(R.CASES) and sum(c["big"] for c in R.CASES) == 4
    for tpl in ("c2", "c4post"):
        assert {c["terms"] for c in R.CASES if c["tpl"] == tpl} == set(range(1, 8))
        assert {c["regime"] for c in R.CASES if c["tpl"] == tpl} == set(R.REGIMES)
    assert {(c["N"], c["H"], c["W"], c["ls"]) for c in R.SMALL if c["tpl"] == "coral"} >= set(R.SHAPES)
    assert all(c["H"] != c["W"] for c in R.CASES if c["H"] > 1)
    assert R.sweeps(1025 * 1024, R.FWD_BLOCKS) == 5 and R.sweeps(1025 * 1024, R.BWD_BLOCKS) == 2
    assert R.sweeps(17 * 256, R.FWD_BLOCKS) == 1
    for c in R.SMALL:      # every case has a counted pixel, the label patterns are what their names say
        x, y = R.make(c)
        t, mask = R.targets(y, x.shape, c["post"], c["ls"])
        assert mask.any() and x.dtype == torch.float32 and y.dtype == torch.uint8
        assert tuple(y.shape) == (c["N"], c["H"] * c["ls"], c["W"] * c["ls"])
        if c["labels"] == "one_pixel":
            assert int(mask.sum()) == 1
        if c["labels"] == "image0_background":
            assert not mask[0].any() and mask[1].all()
        if c["labels"] == "only":
            assert len(set(t[mask].tolist())) == 1
        if c["labels"] == "absent" and not R.aux(c["terms"]):
            assert int(t[mask].max()) < c["C"] - 1
        if c["regime"] == "pm80":
            assert set(x.unique().tolist()) == {-80.0, 80.0}
        if c["regime"] == "offset1e4":
            assert float(x.min()) > 9.9e3


def wrong_fwd(wrong):
    return lambda *a: R.forward(*a, wrong=wrong)


def wrong_bwd(wrong):
    return lambda x, y, terms, post, ls, acc, gscale, weight: R.backward(x, y, terms, post, ls, gscale, weight, wrong=wrong)


# variant -> the cases that are searched for a ratio > 1 (a filter on the tables, to keep the search short)
VARIANTS = {
    "dice_bg_c2": lambda c: c["tpl"] == "c2" and c["terms"] & R.DICE,
    "dice_div_C": lambda c: c["tpl"] == "c2" and c["terms"] & R.DICE,
    "dP_no_eps": lambda c: c["terms"] & R.DICE and not R.aux(c["terms"]),
    "focal_bwd_term": lambda c: c["terms"] & R.FOCAL and not R.aux(c["terms"]),
    "n_all_post": lambda c: c["post"],
    "post_no_shift": lambda c: c["post"],
    "label_hw_swapped": lambda c: True,
    "label_no_row_stride": lambda c: c["ls"] > 1,
    "drop_partial_block": lambda c: (c["N"] * c["H"] * c["W"]) % 256,
    "drop_second_sweep": lambda c: c["big"] and c["tpl"] == "c2",
    "coral_levels": lambda c: c["terms"] == R.CORAL,
    "mse_grad_at_nonpositive": lambda c: c["terms"] == R.MSE,
    "weight_ignored": lambda c: len(c["scales"]) > 1,
}


@pytest.mark.parametrize("wrong", sorted(VARIANTS))
def test_a_wrong_variant_exceeds_a_bound(wrong):
    tried = 0
    for case in R.CASES:
        if (case["big"] and wrong != "drop_second_sweep") or not VARIANTS[wrong](case):
            continue
        tried += 1
        r = ratios(case, wrong_fwd(wrong), wrong_bwd(wrong))
        if max(r.values()) > 1.0:
            return
    raise AssertionError("%s passes every bound on %d cases" % (wrong, tried))


def test_the_correct_fp64_evaluation_passes_its_own_gates():
    for case in R.SMALL[::7]:
        r = ratios(case, wrong_fwd(None), wrong_bwd(None))
        assert max(r.values()) <= 1e-6, (case["name"], r)


def _terms(loss_str):
    bits = 0
    for n in loss_str.split("+"):
        bits |= BITS[n]
    return bits


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_restatement_equals_the_oracle_and_its_autograd(name):
    from oracle import torch_ref
    a = ARGS(**LOSS_CASES[name])
    yp, yt = loss_inputs(a, batch=2, size=24)
    post, terms = a.type == "post", _terms(a.loss_str)
    xo = yp.double().requires_grad_(True)
    lo = torch_ref.Loss(a)(xo, yt)
    tol = 1e-12
    if a.loss_str == "mse":      # the oracle's float targets stop its fp64 backward: its gradient is taken in fp32
        x32 = yp.clone().requires_grad_(True)
        torch_ref.Loss(a)(x32, yt).backward()
        xo.grad, tol = x32.grad.double(), 4 * R.U
    else:
        lo.backward()
    xr = yp.double().requires_grad_(True)
    _, lr = R.forward(xr, yt, terms, post, 1)
    lr.backward()
    assert abs(float(lr.detach()) - float(lo.detach())) <= 1e-12 * abs(float(lo.detach()))
    scale = float(xo.grad.abs().max())
    assert float((xr.grad - xo.grad).abs().max()) <= tol * scale
    g = R.backward(yp, yt, terms, post, 1)
    assert float((g - xr.grad).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("case", R.SMALL[::3], ids=[c["name"] for c in R.SMALL[::3]])
def test_closed_form_gradient_equals_autograd_on_the_tables(case):
    x, y = R.make(case)
    xr = x.double().requires_grad_(True)
    _, L = R.forward(xr, y, case["terms"], case["post"], case["ls"])
    L.backward()
    g = R.backward(x, y, case["terms"], case["post"], case["ls"])
    assert float((g - xr.grad).abs().max()) <= 1e-12 * max(float(xr.grad.abs().max()), 1e-300)


def test_deep_supervision_on_a_non_square_input_equals_the_oracle():
    from oracle import torch_ref
    a = ARGS(type="post", loss_str="focal+dice", deep_supervision=True)
    g = torch.Generator().manual_seed(31)
    preds = [torch.randn(2, 4, 24 // s, 40 // s, generator=g, dtype=torch.float64) * 2 for s in (1, 2, 4)]
    y = torch.randint(0, 5, (2, 24, 40), generator=g, dtype=torch.uint8)
    po = [p.clone().requires_grad_(True) for p in preds]
    lo = torch_ref.compute_loss(torch_ref.Loss(a), po, y, True)
    lo.backward()
    pr = [p.clone().requires_grad_(True) for p in preds]
    lr = sum(0.5 ** j * R.forward(p, y, R.FOCAL | R.DICE, 1, 2 ** j)[1] for j, p in enumerate(pr)) / (2 - 2 ** -3)
    lr.backward()
    assert abs(float(lr.detach()) - float(lo.detach())) <= 1e-12 * abs(float(lo.detach()))
    for j, (o, r, p) in enumerate(zip(po, pr, preds)):
        scale = float(o.grad.abs().max())
        assert float((r.grad - o.grad).abs().max()) <= 1e-12 * scale
        w = float(torch.tensor(0.5 ** j / (2 - 2 ** -3), dtype=torch.float32))
        closed = R.backward(p, y, R.FOCAL | R.DICE, 1, 2 ** j, 1.0, w)
        assert float((closed - o.grad).abs().max()) <= 1e-7 * scale      # (w is an fp32 value here)


@pytest.mark.parametrize("terms,C", R.EMPTY_MASK)
def test_empty_building_mask_is_pinned_to_the_oracle(terms, C):
    from oracle import torch_ref
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, C, 5, 9, generator=g) * 2
    y = torch.zeros(2, 5, 9, dtype=torch.uint8)
    _, L = R.forward(x, y, terms, 1)
    want_zero = terms == R.DICE
    assert float(L) == 0.0 if want_zero else math.isnan(float(L))
    assert float(R.backward(x, y, terms, 1).abs().max()) == 0.0
    acc, lf = R.f32_forward(x, y, terms, 1)
    assert float(lf) == 0.0 if want_zero else math.isnan(float(lf))
    assert float(R.f32_backward(x, y, terms, 1, 1, acc).abs().max()) == 0.0
    # the oracle: the same value wherever it returns one (it raises for focal: a mean over an empty dimension)
    names = [n for n, b in (("dice", R.DICE), ("focal", R.FOCAL), ("ce", R.CE), ("mse", R.MSE), ("coral", R.CORAL)) if terms & b]
    if "focal" in names or C == 2:      # (C = 2 under post is not a configuration of the oracle's models)
        return
    a = ARGS(type="post", loss_str="+".join(names))
    xo = (x.clone() if terms == R.MSE else x.double()).requires_grad_(True)
    lo = torch_ref.Loss(a)(xo, y)
    assert float(lo.detach()) == 0.0 if want_zero else math.isnan(float(lo.detach()))
    lo.backward()
    assert float(xo.grad.abs().max()) == 0.0
