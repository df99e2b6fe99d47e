"""The ``lovasz`` kernels (csrc/lovasz.hip, csrc/sort.hip) against the fp64 restatement in tests/lovasz_ref.py.

On every shape: (a) the errors decoded from the kernel's keys against fp64, 2e-6 absolute, flag bits and sentinels exact;
(b) ``sorted`` bit-equal to numpy's sort of the kernel's OWN keys and the records equal to the counts (integers: no margin);
(c) the gradient against the weights that the numpy model reads out of the kernel's own keys and sorted rows, times the fp64
softmax Jacobian; (d) the loss against the fp64 reference.  Tolerances are the loss tests' own (tests/test_ops_gpu.py): loss
2e-6 * max(1, |L|) against fp64, gradient 2e-5 relative to the largest element.

The gradient is compared END TO END with fp64 autograd only where the fp32 and the fp64 evaluation order the errors alike:
on random inputs a flip between two near-equal errors moves single weights by about 1 / G (while the loss moves by ~1e-9),
so those inputs do not qualify.  Qualifying inputs: the lattice of tests/lovasz_ref.py (C = 2, all probabilities distinct
and no foreground error within 1e-5 of a background error, asserted first; a flip inside one set swaps two weights between
neighbours of equal rank counts, i.e. changes nothing), and inputs whose ties are exact in both precisions."""
import os

import numpy as np
import pytest
import torch

from tests import lovasz_ref as R
from tests.golden.cases import ARGS

pytestmark = pytest.mark.gpu

GAP = 1e-5


def dev():
    return torch.device("cuda:0")


def close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item() / scale
    print("%s: rel-to-max error %.3e" % (what, err))
    assert err <= tol, "%s: rel-to-max error %.3e > %.1e" % (what, err, tol)


def run(logits, labels, ls=1, post=False, mask=None, gscale=1.0, grad=True):
    """forward + backward through the C ABI: loss, keys [C, M] uint32, sorted [C, M] uint32, records [C, 4], sums [5], dlogits"""
    from xview2_amd import _capi, ops
    loss, keys, srt, rec, sums, lg = ops.lovasz_forward(logits.to(dev()), labels.to(dev()), ls, post, mask)
    N, C, H, W = lg.shape
    d = torch.empty_like(lg)
    if grad:
        gs = torch.full((1,), gscale, dtype=torch.float32, device=dev())
        _capi.call("xv2_lovasz_backward", lg, N, C, H, W, keys, srt, rec, sums, gs, d)
    torch.cuda.synchronize()
    return (loss.cpu(), keys.cpu().numpy().view(np.uint32), srt.cpu().numpy().view(np.uint32), rec.cpu().numpy(),
            sums.cpu().numpy(), d.cpu() if grad else None)


def span(mask):
    cs = [c for c in range(4) if (mask >> c) & 1]
    return range(cs[0], cs[-1] + 1)


def check(logits, labels, ls=1, post=False, mask=None, grad=True, end_to_end=False):
    """(a) - (d) on one input; returns what run() returns"""
    N, C = logits.shape[:2]
    mask = R.class_mask(C, post) if mask is None else mask
    out = run(logits, labels, ls, post, mask, grad=grad)
    loss, keys, srt, rec, sums, d = out
    e64, fg, valid, p64 = R.errors(logits, labels, post, ls)
    # (a)
    for c in range(C):
        got, f, v = R.decode_keys(keys[c])
        assert np.array_equal(v, valid.numpy()) and np.array_equal(f, fg[c].numpy()), "flags of class %d" % c
        assert (keys[c][~v] == R.SKIP).all()
        if v.any():
            err = np.abs(got.astype(np.float64)[v] - e64[c].numpy()[v]).max()
            assert err <= 2e-6, "errors of class %d: %.3e" % (c, err)
    # (b)
    for c in span(mask):
        assert np.array_equal(srt[c], np.sort(keys[c])), "sorted row %d" % c
    want = R.records(keys, mask)
    assert np.array_equal(rec, want), (rec, want)
    present = [c for c in range(C) if want[c, 3]]
    assert sums[4] == len(present)
    for c in range(C):
        lc = R.sorted_loss(srt[c]) if c in present else 0.0
        assert abs(sums[c] - lc) <= 1e-12 * max(1.0, lc), (c, sums[c], lc)
    # (c)
    if grad:
        g = torch.zeros_like(p64)
        for c in present:
            g[c] = torch.from_numpy(R.key_weights(keys[c], srt[c])) / len(present)
        formula = p64 * (g - (g * p64).sum(0, keepdim=True))
        formula = formula.reshape(C, N, -1).permute(1, 0, 2).reshape(logits.shape)
        if present:
            close(d, formula, 2e-5, "dlogits vs formula")
        else:
            assert not d.any()
    # (d)
    x = logits.double().requires_grad_(True)
    ref = R.lovasz_sorted(x, labels, post, ls, mask)
    print("loss %.9g reference %.12g" % (float(loss), float(ref.detach())))
    assert abs(float(loss) - float(ref.detach())) <= 2e-6 * max(1.0, abs(float(ref.detach())))
    if end_to_end:
        x2 = logits.double().requires_grad_(True)
        R.lovasz_ranked(x2, labels, post, ls, mask).backward()
        close(d, x2.grad, 2e-5, "dlogits vs reference")
    return out


def randn_case(shape, seed, post=False, absent=None, pos=0.3):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = torch.randn(shape, generator=g) * 2
    if post:
        y = torch.randint(0, C + 1, (N, H, W), generator=g, dtype=torch.uint8)
        if absent is not None:
            y[y == absent + 1] = 0
    else:
        y = (torch.rand(N, H, W, generator=g) < pos).to(torch.uint8)
    return x, y


def test_odd_shape_pre():
    x, y = randn_case((3, 2, 37, 53), 41)
    _, _, _, rec, _, _ = check(x, y)
    assert rec[0, 3] == 0 and rec[1, 3] == 1 and rec[1, 2] == 0


def test_post_with_skipped_pixels_and_an_absent_class():
    x, y = randn_case((2, 4, 64, 64), 42, post=True, absent=2)
    _, keys, _, rec, _, d = check(x, y, post=True)
    assert rec[:, 3].tolist() == [1, 1, 0, 1] and rec[2, 0] == 0 and (rec[:, 2] == int((y == 0).sum())).all()
    skipped = (y == 0).unsqueeze(1).expand_as(d)
    assert (d[skipped] == 0).all() and (d[~skipped] != 0).any()


def test_every_class_of_four_without_the_building_mask():
    """C = 4, post off: label = class, every class in the mean, nothing skipped"""
    g = torch.Generator().manual_seed(43)
    x = torch.randn(1, 4, 19, 23, generator=g) * 2
    y = torch.randint(0, 4, (1, 19, 23), generator=g, dtype=torch.uint8)
    _, _, _, rec, _, _ = check(x, y, mask=0b1111)
    assert rec[:, 3].tolist() == [1, 1, 1, 1] and (rec[:, 2] == 0).all()
    # a mask with a gap: the rows in between are sorted along, the mean is over the two named classes
    check(x, y, mask=0b1001)


@pytest.mark.parametrize("post", [False, True])
def test_no_building_pixel_gives_exact_zeros(post):
    C = 4 if post else 2
    x = torch.randn(2, C, 17, 9, generator=torch.Generator().manual_seed(44)) * 2
    loss, keys, srt, rec, sums, d = check(x, torch.zeros(2, 17, 9, dtype=torch.uint8), post=post)
    assert float(loss) == 0.0 and not d.any() and not sums.any() and not rec[:, 3].any()
    if post:
        assert (keys == R.SKIP).all()


def test_every_pixel_foreground():
    x = torch.randn(2, 2, 11, 13, generator=torch.Generator().manual_seed(45)) * 2
    y = torch.ones(2, 11, 13, dtype=torch.uint8)
    loss, _, _, rec, _, _ = check(x, y, end_to_end=True)
    assert rec[1].tolist() == [2 * 11 * 13, 0, 0, 1]
    # no background: every weight is 1 / G, the loss is the mean error
    want = float((1 - torch.softmax(x.double(), 1)[:, 1]).mean())
    assert abs(float(loss) - want) <= 2e-6


def test_constant_logits_all_tied():
    """every background error equals p > every foreground error 1 - p: the background is one tied group in front, each of
    its weights G / (G (G + Nb)) = 1 / M, and so is each foreground weight (B_> = Nb)"""
    x = torch.zeros(1, 2, 16, 16)
    x[:, 1] = 0.75
    y = torch.zeros(1, 16, 16, dtype=torch.uint8)
    y[0, :5] = 1
    loss, keys, srt, rec, sums, d = check(x, y, end_to_end=True)
    assert rec[1].tolist() == [80, 176, 0, 1]
    g = d.reshape(2, -1)
    bg = (y.reshape(-1) == 0)
    assert (g[:, bg] == g[:, bg][:, :1]).all() and float(g[1, bg][0]) != 0.0
    p1 = float(torch.softmax(torch.tensor([0.0, 0.75], dtype=torch.float64), 0)[1])
    want = p1 * (1 - p1) / 256
    assert abs(float(g[1, bg][0]) - want) <= 2e-5 * want
    assert abs(float(g[1, ~bg][0]) + want) <= 2e-5 * want
    assert abs(float(loss) - (176 * p1 + 80 * (1 - p1)) / 256) <= 2e-6
    # the other way round (p < 1 - p) the foreground comes first, the Jaccard loss is 1 before the first background entry
    # and the background weighs nothing
    x[:, 1] = -0.75
    loss, _, _, _, _, d = check(x, y, end_to_end=True)
    assert not d.reshape(2, -1)[:, bg].any() and abs(float(loss) - p1) <= 2e-6


def test_two_values_with_a_tied_group_across_foreground_and_background():
    """logits (0, 0) give p = 1 - p = 0.5 exactly, in fp32 and fp64: one tied group that holds foreground AND background
    entries (the foreground goes first, the background shares), next to well separated errors from the logit 2"""
    g = torch.Generator().manual_seed(46)
    x = torch.zeros(2, 2, 12, 12)
    x[:, 1] = 2.0 * (torch.rand(2, 12, 12, generator=g) < 0.4).float()
    y = (torch.rand(2, 12, 12, generator=g) < 0.4).to(torch.uint8)
    _, keys, _, _, _, _ = check(x, y, end_to_end=True)
    half = (keys[1] & R.LOW) == 0x3F000000
    assert (half & (keys[1] >= R.SIGN)).sum() > 5 and (half & (keys[1] < R.SIGN)).sum() > 5


@pytest.mark.parametrize("shape,seed", [((1, 2, 22, 24), 47), ((2, 2, 64, 64), 48)])
def test_lattice_gradient_end_to_end(shape, seed):
    x, y = R.lattice_inputs(shape, seed)
    gap = R.min_fg_bg_gap(x, y)
    print("fg/bg gap %.3e" % gap)
    assert gap >= GAP
    check(x, y, end_to_end=True)


def test_many_chunks():
    x, y = randn_case((2, 2, 256, 256), 49)
    check(x, y)


def test_megapixel_keys_sort_and_loss():
    x, y = randn_case((1, 2, 1024, 1024), 50, pos=0.05)
    check(x, y, grad=False)


def test_saturated_logits_many_zero_errors():
    """randn * 60 logits saturate the fp32 softmax: p is exactly 1 or exactly 0 for many pixels, a large tied group at error 0
    with foreground and background entries (the fp64 errors are tiny, not 0: the loss does not see the difference)"""
    g = torch.Generator().manual_seed(51)
    x = torch.randn(2, 2, 40, 40, generator=g) * 60
    y = (torch.rand(2, 40, 40, generator=g) < 0.4).to(torch.uint8)
    _, keys, _, _, _, _ = check(x, y)
    zero = (keys[1] & R.LOW) == 0
    assert zero.mean() > 0.05 and (zero & (keys[1] >= R.SIGN)).sum() > 20 and (zero & (keys[1] < R.SIGN)).sum() > 20


def test_nan_logit_gives_a_nan_loss_and_returns():
    x, y = randn_case((2, 2, 16, 16), 52)
    x[1, 1, 3, 4] = float("nan")
    loss, keys, srt, rec, sums, d = run(x, y)          # returns: nothing waits on a value
    assert np.isnan(float(loss)) and np.isnan(sums[1]) and sums[4] == 1
    q = 256 + 3 * 16 + 4
    assert (keys[1, q] & R.LOW) == R.NAN and (keys[0, q] & R.LOW) == R.NAN
    assert np.array_equal(srt[1], np.sort(keys[1])) and np.array_equal(rec, R.records(keys, 0b10))


def test_two_calls_are_bit_equal():
    x, y = randn_case((2, 4, 48, 48), 53, post=True)
    a, b = run(x, y, post=True), run(x, y, post=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[5], b[5])
    for i in range(1, 5):
        assert np.array_equal(a[i], b[i])


def test_gscale_scales_the_gradient():
    x, y = randn_case((1, 2, 20, 20), 54)
    a, b = run(x, y), run(x, y, gscale=0.25)
    assert torch.equal(a[5] * 0.25, b[5])


def _ds_inputs():
    preds = [R.lattice_logits((2, 2, s, s), 55 + s) for s in (32, 16, 8)]
    y = (torch.rand(2, 32, 32, generator=torch.Generator().manual_seed(56)) < 0.3).to(torch.uint8)
    return preds, y


def test_deep_supervision_keeps_each_heads_buffers():
    """criterion.compute_loss runs the three heads' forward passes before any backward: each node owns its keys, sorted
    rows and records, so a head's gradient is bit-equal to that head's run alone"""
    from oracle import torch_ref
    from xview2_amd import criterion
    a = ARGS(type="pre", loss_str="lovasz+dice", deep_supervision=True)
    preds, y = _ds_inputs()
    for j, p in enumerate(preds):
        assert R.min_fg_bg_gap(p, y, label_stride=2 ** j) >= GAP
    dice = torch_ref.Loss(ARGS(type="pre", loss_str="dice"))
    pr = [p.clone().double().requires_grad_(True) for p in preds]
    lo = 0
    for j, p in enumerate(pr):
        s = 2 ** j
        lo = lo + 0.5 ** j * (dice(p, y[:, ::s, ::s]) + R.lovasz_ranked(p, y, label_stride=s))
    lo = lo / (2 - 2 ** -3)
    lo.backward()
    loss_fn = criterion.Loss(a)
    pg = [p.to(dev()).requires_grad_(True) for p in preds]
    lh = criterion.compute_loss(loss_fn, pg, y.to(dev()), True)
    lh.backward()
    lh, lo = float(lh.detach()), float(lo.detach())
    assert abs(lh - lo) <= 2e-6 * max(1.0, abs(lo))
    c_norm = 1 / (2 - 2 ** -3)
    for j, (g, r, p) in enumerate(zip(pg, pr, preds)):
        close(g.grad, r.grad, 2e-5, "ds dlogits head %d" % j)
        alone = p.to(dev()).requires_grad_(True)
        la = loss_fn(alone, y.to(dev()), label_stride=2 ** j)
        (c_norm * (la if j == 0 else 0.5 ** j * la)).backward()
        assert torch.equal(alone.grad, g.grad), "head %d" % j


def test_criterion_composes_the_term():
    from xview2_amd import criterion
    x0, y = randn_case((2, 2, 24, 24), 57)

    def value(loss_str, type_="pre", xx=x0, yy=y):
        x = xx.to(dev()).requires_grad_(True)
        l = criterion.Loss(ARGS(type=type_, loss_str=loss_str))(x, yy.to(dev()))
        l.backward()
        return l.detach().cpu(), x.grad.cpu()
    l1, g1 = value("lovasz")
    ref = float(R.lovasz_sorted(x0, y))
    assert abs(float(l1) - ref) <= 2e-6 * max(1.0, ref)
    # a term named twice counts twice, exactly
    l2, g2 = value("lovasz+lovasz")
    assert float(l2) == 2 * float(l1) and torch.equal(g2, 2 * g1)
    # joined: the sum of the parts, whatever the order of the names
    lce, gce = value("ce")
    la, ga = value("lovasz+ce")
    lb, gb = value("ce+lovasz")
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert float(la) == float(lce + l1) and torch.equal(ga, gce + g1)
    lf, _ = value("focal+lovasz")
    assert abs(float(lf) - float(value("focal")[0]) - float(l1)) <= 2e-6
    # post is real: the four damage classes over building pixels, not CE
    xp, yp = randn_case((2, 4, 24, 24), 58, post=True)
    lp, gp = value("lovasz", "post", xp, yp)
    refp = float(R.lovasz_sorted(xp, yp, True))
    assert abs(float(lp) - refp) <= 2e-6 * max(1.0, refp)
    assert abs(float(lp) - float(value("ce", "post", xp, yp)[0])) > 1e-3
    assert not gp[(yp == 0).unsqueeze(1).expand_as(gp)].any()


def test_cli_trains_with_lovasz(tmp_path, monkeypatch):
    import main as cli
    from xview2_amd.lightning import Model
    seen = []
    step = Model.training_step

    def recording(self, batch, i):
        loss = step(self, batch, i)
        seen.append(loss.detach())
        return loss
    monkeypatch.setattr(Model, "training_step", recording)
    res = str(tmp_path / "run")
    m = cli.main(["--exec_mode", "train", "--type", "pre", "--loss_str", "lovasz+ce", "--epochs", "1", "--results", res,
                  "--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
                  "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3"])
    assert len(seen) == 3 and all(np.isfinite(float(l)) for l in seen)
    assert os.path.exists(os.path.join(res, "checkpoints", "last.ckpt"))
    assert all(torch.isfinite(p).all() for p in m.parameters())
