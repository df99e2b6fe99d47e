"""The ``wce`` kernels (csrc/wce.hip, csrc/wce_px.h) against the fp64 restatement in tests/wce_ref.py.

Distances are integers and are compared with ==.  The border map, the loss and the gradient are held to the per-element
bounds derived in tests/wce_ref.py (worst error / bound ratio printed, <= 1 asserted; where a bound is 0 the result must be
equal).  The fp64 loss takes the fp64 map of the REFERENCE distances, so a wrong distance shows in the loss as well."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import wce_ref as R
from tests.golden.cases import ARGS

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def u16(t):
    return t.cpu().numpy().astype(np.int64)


def gpu_distances(masks, rad):
    """masks: list of uint8 [H, W] of one shape -> (D1, D2) int64 [B, H, W] from the kernel"""
    from xview2_amd import ops
    d1, d2 = ops.border_distances(torch.from_numpy(np.stack(masks)).to(dev()), rad)
    torch.cuda.synchronize()
    assert d1.dtype == torch.uint16 and d2.dtype == torch.uint16
    return u16(d1), u16(d2)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(mask, R, D1, D2) of a named fixture, the reference computed once"""
    make, rad = R.BIG if name == "big" else {**R.RANDOM, **R.SPECIAL}[name]
    m = make()
    return (m, rad) + R.distances(m, rad)


def same(got, want, what):
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, first at %s: %s instead of %s" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# ---- distances -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.RANDOM) + list(R.SPECIAL))
def test_distances_equal_the_definition(name):
    m, rad, D1, D2 = fixture(name)
    g1, g2 = gpu_distances([m], rad)
    same(g1[0], D1, name + " D1")
    same(g2[0], D2, name + " D2")
    if name == "equidistant":
        assert g1[0, 4, 7] == 16 and g2[0, 4, 7] == 16
    if name == "smaller_than_the_window":
        assert (g2 == R.NONE).all() and (g1 != R.NONE).any()
    if name in ("empty", "full"):
        assert (g1 == R.NONE).all() and (g2 == R.NONE).all()


def test_images_of_a_batch_are_independent():
    masks = [R.rectangles(37, 45, s, n) for s, n in ((1, 30), (2, 12), (5, 20))]
    g1, g2 = gpu_distances(masks, 5)
    for b, m in enumerate(masks):
        D1, D2 = R.distances(m, 5)
        same(g1[b], D1, "image %d D1" % b)
        same(g2[b], D2, "image %d D2" % b)
    # an image alone gives what it gives inside the batch
    a1, a2 = gpu_distances(masks[1:2], 5)
    assert np.array_equal(a1[0], g1[1]) and np.array_equal(a2[0], g2[1])


def test_megapixel_map():
    m, rad, D1, D2 = fixture("big")
    g1, g2 = gpu_distances([m], rad)
    same(g1[0], D1, "D1")
    same(g2[0], D2, "D2")


# ---- the map -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,w0,sigma", [("70x67_r32", 10.0, 5.0), ("37x45_r8", 10.0, 2.0), ("70x67_r32", 3.0, 1.5),
                                           ("equidistant", 1.0, 0.7)])
def test_border_weights_within_the_bound(name, w0, sigma):
    from xview2_amd import ops
    m, rad, D1, D2 = fixture(name)
    d1, d2 = ops.border_distances(torch.from_numpy(m[None]).to(dev()), rad)
    got = ops.border_weights(d1, d2, w0, sigma).cpu()
    want, bound = R.border_map(D1[None], D2[None], w0, sigma)
    ratio, where = R.check(got, torch.from_numpy(want), torch.from_numpy(bound))
    print("%s w0 %g sigma %g: worst error / bound %.3f at %d" % (name, w0, sigma, ratio, where))
    assert ratio <= 1.0
    none = torch.from_numpy(D2[None] == R.NONE)
    assert (got[none] == 0).all() and (got[~none] > 0).any()
    assert got.dtype == torch.float32 and got.shape == (1,) + m.shape


# ---- loss and gradient ---------------------------------------------------------------------------------------------------

def run(x, y, cw, ls=1, post=False, border=None, gscale=1.0):
    """forward + backward through the C ABI -> loss [1], sums [2], dlogits (CPU tensors)"""
    from xview2_amd import _capi, ops
    cwt = torch.tensor(cw, dtype=torch.float32, device=dev())
    loss, sums, lg, lb = ops.wce_forward(x.to(dev()), y.to(dev()), cwt, ls, post, border)
    N, C, H, W = lg.shape
    d = torch.full_like(lg, float("nan"))
    gs = torch.full((1,), gscale, dtype=torch.float32, device=dev())
    d1, d2, w0, sigma = (None, None, 0.0, 1.0) if border is None else border
    _capi.call("xv2_wce_backward", lg, lb, N, C, H, W, ls, 1 if post else 0, cwt, d1, d2, float(w0), float(sigma), sums, gs, d)
    torch.cuda.synchronize()
    return loss.cpu(), sums.cpu(), d.cpu()


def border_inputs(masks, rad, w0, sigma):
    """labels uint8 [B, H, W], the kernel's border tuple for them, and the fp64 map and its bound from the REFERENCE distances"""
    from xview2_amd import ops
    y = torch.from_numpy(np.stack(masks))
    d1, d2 = ops.border_distances(y.to(dev()), rad)
    ref = [R.border_map(*R.distances(m, rad), w0, sigma) for m in masks]
    return y, (d1, d2, w0, sigma), np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])


def check(x, y, cw, ls=1, post=False, border=None, bmap=None, bbound=None, gscale=1.0, what=""):
    loss, sums, d = run(x, y, cw, ls, post, border, gscale)
    b = R.bounds(x, y, cw, post, ls, bmap, bbound)
    err = abs(float(loss) - b["loss64"])
    print("%s loss %.9g reference %.12g error / bound %.3f" % (what, float(loss), b["loss64"], err / max(b["loss"], 1e-300)))
    assert err <= b["loss"]
    assert abs(float(sums[1]) - b["S1"]) <= 1e-6 * max(1.0, b["S1"])
    want = R.backward(x, y, cw, post, ls, bmap, gscale)
    ratio, where = R.check(d, want, b["grad"] * abs(R.f32(gscale)))
    print("%s dlogits worst error / bound %.3f at %d" % (what, ratio, where))
    assert ratio <= 1.0
    return loss, sums, d


def test_class_weights_pre():
    x, y = R.case((1, 2, 22, 24), 61)
    check(x, y, (1.0, 3.0), what="pre 22x24")


def test_class_weights_post_with_a_zero_weight_and_an_absent_class():
    x, y = R.case((2, 4, 33, 31), 62, post=True, absent=2)
    _, _, d = check(x, y, (0.5, 0.0, 2.0, 4.0), post=True, what="post 33x31")
    dropped = (y == 0).unsqueeze(1).expand_as(d)
    zero_w = (y == 2).unsqueeze(1).expand_as(d)
    assert (d[dropped] == 0).all() and (d[zero_w] == 0).all() and (d[~dropped & ~zero_w] != 0).any()
    assert not (y == 3).any()


def test_border_term_pre():
    masks = [R.rectangles(37, 45, 1, 30), R.rectangles(37, 45, 2, 12)]
    y, border, bmap, bbound = border_inputs(masks, R.default_radius(2.0), 10.0, 2.0)
    assert (bmap > 1.0).sum() > 50          # the border part carries real weight here
    x, _ = R.case((2, 2, 37, 45), 63)
    check(x, y, (1.0, 3.0), border=border, bmap=bmap, bbound=bbound, what="border 37x45")


def test_deep_supervision_heads_share_one_distance_pair():
    masks = [R.rectangles(64, 64, 8, 40), R.rectangles(64, 64, 9, 25)]
    y, border, bmap, bbound = border_inputs(masks, 8, 10.0, 2.5)
    for ls, seed in ((1, 64), (2, 65), (4, 66)):
        x, _ = R.case((2, 2, 64 // ls, 64 // ls), seed)
        assert (bmap[:, ::ls, ::ls] > 0.5).sum() > 10
        check(x, y, (1.0, 2.0), ls=ls, border=border, bmap=bmap, bbound=bbound, what="stride %d" % ls)


def test_many_blocks():
    masks = [R.rectangles(256, 256, 10 + i, 150, 3, 12) for i in range(2)]
    y, border, bmap, bbound = border_inputs(masks, 8, 10.0, 2.5)
    x, _ = R.case((2, 2, 256, 256), 67)
    check(x, y, (0.25, 4.0), border=border, bmap=bmap, bbound=bbound, what="256x256")


@pytest.mark.parametrize("shape,post,seed", [((1, 2, 22, 24), False, 68), ((2, 4, 33, 31), True, 69)])
def test_unit_weights_equal_the_ce_term(shape, post, seed):
    """all weights 1 and no border: the existing ``ce`` term of LossFn on the same inputs, within the wce bound"""
    from xview2_amd import ops
    x, y = R.case(shape, seed, post)
    cw = (1.0,) * shape[1]
    loss, _, d = check(x, y, cw, post=post, what="unit weights")
    xg = x.to(dev()).requires_grad_(True)
    lce = ops.LossFn.apply(xg, y.to(dev()), ops.LOSS_CE, post, 1)
    lce.backward()
    b = R.bounds(x, y, cw, post)
    assert abs(float(loss) - float(lce.detach())) <= b["loss"]
    ratio, _ = R.check(d, xg.grad.cpu().double(), b["grad"])
    print("wce against ce: worst difference / bound %.3f" % ratio)
    assert ratio <= 1.0


def test_no_weight_gives_exact_zeros():
    xp, _ = R.case((2, 4, 17, 9), 70, post=True)
    loss, sums, d = run(xp, torch.zeros(2, 17, 9, dtype=torch.uint8), (1.0,) * 4, post=True)
    assert float(loss) == 0.0 and not np.signbit(float(loss)) and not d.any() and not sums.any()
    # every present class weighted 0
    x, _ = R.case((2, 2, 17, 9), 71)
    loss, sums, d = run(x, torch.ones(2, 17, 9, dtype=torch.uint8), (1.0, 0.0))
    assert float(loss) == 0.0 and not np.signbit(float(loss)) and not d.any() and float(sums[1]) == 0.0


def test_nan_logit_gives_a_nan_loss_and_returns():
    x, y = R.case((2, 2, 16, 16), 72)
    x[1, 1, 3, 4] = float("nan")
    loss, sums, d = run(x, y, (1.0, 3.0))          # returns: nothing waits on a value
    assert np.isnan(float(loss)) and np.isnan(float(sums[0])) and float(sums[1]) > 0
    assert torch.isnan(d[1, :, 3, 4]).all() and torch.isfinite(d[0]).all()


def test_two_calls_are_bit_equal_and_gscale_scales_the_gradient():
    masks = [R.rectangles(48, 48, 12, 30), R.rectangles(48, 48, 13, 30)]
    y, border, _, _ = border_inputs(masks, 6, 10.0, 2.0)
    x, _ = R.case((2, 2, 48, 48), 73)
    a, b = run(x, y, (1.0, 3.0), border=border), run(x, y, (1.0, 3.0), border=border)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    c = run(x, y, (1.0, 3.0), border=border, gscale=0.25)
    assert torch.equal(a[2] * 0.25, c[2]) and torch.equal(a[0], c[0])
    # the distances themselves
    from xview2_amd import ops
    again = ops.border_distances(y.to(dev()), 6)
    assert np.array_equal(u16(again[0]), u16(border[0])) and np.array_equal(u16(again[1]), u16(border[1]))


def test_forward_and_map_entry_hold_the_same_weight_bits():
    """class weights 0 and distance maps that are NONE but for one pixel: sum w IS that pixel's border weight, added to 0 once; it
    must equal the map entry's fp32 value bit for bit (the one device function of wce_px.h)"""
    from xview2_amd import ops
    m, rad, D1, D2 = fixture("37x45_r8")
    d1, d2 = ops.border_distances(torch.from_numpy(m[None]).to(dev()), rad)
    bm = ops.border_weights(d1, d2, 7.0, 3.0).cpu()
    x, _ = R.case((1, 2, 37, 45), 74)
    y = torch.zeros(1, 37, 45, dtype=torch.uint8)
    ys, xs = np.nonzero(D2 != R.NONE)
    for i in range(0, len(ys), max(1, len(ys) // 8)):
        one1, one2 = np.full((1, 37, 45), R.NONE, np.uint16), np.full((1, 37, 45), R.NONE, np.uint16)
        one1[0, ys[i], xs[i]], one2[0, ys[i], xs[i]] = D1[ys[i], xs[i]], D2[ys[i], xs[i]]
        border = (torch.from_numpy(one1).to(dev()), torch.from_numpy(one2).to(dev()), 7.0, 3.0)
        _, sums, _ = run(x, y, (0.0, 0.0), border=border)
        assert float(sums[1]) == float(bm[0, ys[i], xs[i]]) and float(sums[1]) > 0


# ---- composition and the command line ------------------------------------------------------------------------------------

def test_criterion_composes_the_term():
    from xview2_amd import criterion
    masks = [R.rectangles(24, 24, 14, 12, 2, 4), R.rectangles(24, 24, 15, 12, 2, 4)]
    y = torch.from_numpy(np.stack(masks))
    x0, _ = R.case((2, 2, 24, 24), 75)
    kw = dict(type="pre", class_weights="1,3", border_weight=10.0, border_sigma=2.0)

    def value(loss_str, **over):
        x = x0.to(dev()).requires_grad_(True)
        l = criterion.Loss(ARGS(loss_str=loss_str, **{**kw, **over}))(x, y.to(dev()))
        l.backward()
        return l.detach().cpu(), x.grad.cpu()
    lw, gw = value("wce")
    bmap, bbound = zip(*[R.border_map(*R.distances(m, 6), 10.0, 2.0) for m in masks])
    b = R.bounds(x0, y, (1.0, 3.0), bmap=np.stack(bmap), bmap_bound=np.stack(bbound))
    assert abs(float(lw) - b["loss64"]) <= b["loss"]
    ld, gd = value("dice")
    la, ga = value("wce+dice")
    lb, gb = value("dice+wce")
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert float(la) == float(lw + ld) and torch.equal(ga, gw + gd)
    l2, g2 = value("wce+wce")          # a term named twice counts twice, exactly
    assert float(l2) == 2 * float(lw) and torch.equal(g2, 2 * gw)
    lv, _ = value("lovasz+wce")
    assert abs(float(lv) - float(value("lovasz")[0]) - float(lw)) <= 2e-6
    # the flags are read: without the border, and with unit weights, the value moves
    assert abs(float(value("wce", border_weight=0.0)[0]) - float(lw)) > 1e-4
    assert abs(float(value("wce", class_weights=None)[0]) - float(lw)) > 1e-4


def test_compute_loss_launches_the_distances_once_per_batch(monkeypatch):
    from xview2_amd import criterion, ops
    calls = []
    real = ops.border_distances

    def counting(labels, rad):
        calls.append((tuple(labels.shape), rad))
        return real(labels, rad)
    monkeypatch.setattr(ops, "border_distances", counting)
    y = torch.from_numpy(np.stack([R.rectangles(64, 64, 8, 40), R.rectangles(64, 64, 9, 25)])).to(dev())
    preds = [R.case((2, 2, s, s), 76 + s)[0] for s in (64, 32, 16)]
    a = ARGS(type="pre", loss_str="wce+dice", deep_supervision=True, class_weights="1,3", border_weight=10.0, border_sigma=2.0)
    loss_fn = criterion.Loss(a)
    pg = [p.to(dev()).requires_grad_(True) for p in preds]
    total = criterion.compute_loss(loss_fn, pg, y, True)
    total.backward()
    assert calls == [((2, 64, 64), 6)]
    # the heads one by one, each computing its own maps: the same bits
    c_norm = 1 / (2 - 2 ** -3)
    for j, (p, g) in enumerate(zip(preds, pg)):
        alone = p.to(dev()).requires_grad_(True)
        la = loss_fn(alone, y, label_stride=2 ** j)
        (c_norm * (la if j == 0 else 0.5 ** j * la)).backward()
        assert torch.equal(alone.grad, g.grad), "head %d" % j
    assert len(calls) == 4
    # without a border weight nothing is launched
    del calls[:]
    off = criterion.Loss(ARGS(type="pre", loss_str="wce+dice", deep_supervision=True, class_weights="1,3"))
    criterion.compute_loss(off, [p.to(dev()) for p in preds], y, True)
    off(preds[0].to(dev()), y)
    assert calls == []


def _train(monkeypatch, tmp_path, name, extra):
    import main as cli
    from xview2_amd.lightning import Model
    seen = []
    step = Model.training_step

    def recording(self, batch, i):
        loss = step(self, batch, i)
        seen.append(loss.detach().clone())
        return loss
    monkeypatch.setattr(Model, "training_step", recording)
    res = str(tmp_path / name)
    m = cli.main(["--exec_mode", "train", "--type", "pre", "--epochs", "1", "--results", res, "--data", "synthetic",
                  "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
                  "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "2"] + extra)
    monkeypatch.setattr(Model, "training_step", step)
    return m, [l.cpu() for l in seen], res


def test_cli_trains_with_wce(tmp_path, monkeypatch):
    m, seen, res = _train(monkeypatch, tmp_path, "run", ["--loss_str", "wce+dice", "--class_weights", "1,3",
                                                         "--border_weight", "10"])
    assert len(seen) == 2 and all(np.isfinite(float(l)) for l in seen)
    assert m.loss.wants_border and m.loss.class_weights == [1.0, 3.0] and m.loss.border_radius == 15
    assert os.path.exists(os.path.join(res, "checkpoints", "last.ckpt"))
    assert all(torch.isfinite(p).all() for p in m.parameters())


def test_cli_without_the_flags_reaches_none_of_the_new_code(tmp_path, monkeypatch):
    """--loss_str dice without the new flags: no launch of a new entry point, and the same loss bits whether or not the new
    code is there to be reached (every new op replaced by one that raises).  The losses of an earlier commit are not stored
    here: they would pin every kernel of the network to its present bits."""
    from xview2_amd import ops
    names = []
    real = ops.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(ops, "call", recording)
    _, plain, _ = _train(monkeypatch, tmp_path, "plain", ["--loss_str", "dice"])
    assert names and not [n for n in names if n.startswith(("xv2_wce", "xv2_border"))]
    assert "xv2_loss_forward" in names and "xv2_loss_backward" in names

    def refuse(*a, **k):
        raise AssertionError("the wce code was reached without its flags")
    for f in ("border_distances", "border_weights", "wce_forward"):
        monkeypatch.setattr(ops, f, refuse)
    monkeypatch.setattr(ops.WceFn, "forward", staticmethod(refuse))
    _, again, _ = _train(monkeypatch, tmp_path, "again", ["--loss_str", "dice"])
    assert len(plain) == 2 and len(again) == 2
    for a, b in zip(plain, again):
        assert torch.equal(a, b) and np.isfinite(float(a))
