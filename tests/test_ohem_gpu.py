"""The ``ohem_hard`` kernels (csrc/ohem.hip) against the fp64 restatement in tests/ohem_ref.py.

On every shape: (a) the per-pixel losses against fp64 cross-entropy, 2e-6 absolute; (b) the per-image record bit-exact
against numpy's sort of the kernel's OWN downloaded per-pixel losses (no margin needed: integers); (c) the gradient against
the formula evaluated on the host from the kernel's record and the fp64 softmax; (d) loss and gradient end to end against
the reference.  (d)'s gradient needs the fp32 and the fp64 evaluation to select the same pixels: the fp64 gap between the
k-th and the (k+1)-th largest negative loss must be >= 1e-5, ten times the largest per-pixel fp32 error seen (1e-6); the seeds
of the random shapes are chosen so that it is, and the tests assert it first.  Tolerances are the loss tests' own
(tests/test_ops_gpu.py): loss 2e-6 * max(1, |L|) against fp64, gradient 2e-5 relative to the largest element."""
import os

import numpy as np
import pytest
import torch

from tests import ohem_ref as R
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
    assert err <= tol, "%s: rel-to-max error %.3e > %.1e" % (what, err, tol)


def run(logits, labels, ls=1, gscale=1.0):
    """forward + backward through the C ABI: loss, px_loss bits [N, M] uint32, records [N, 8], sums [3], dlogits"""
    from xview2_amd import _capi, ops
    loss, px, rec, sums, lg, lb = ops.ohem_forward(logits.to(dev()), labels.to(dev()), ls)
    N, C, H, W = lg.shape
    d = torch.empty_like(lg)
    gs = torch.full((1,), gscale, dtype=torch.float32, device=dev())
    _capi.call("xv2_ohem_backward", lg, lb, N, C, H, W, ls, px, rec, sums, gs, d)
    torch.cuda.synchronize()
    return (loss.cpu(), px.cpu().numpy().view(np.uint32), rec.cpu().numpy(), sums.cpu().numpy(), d.cpu())


def host_weights(px_bits, rec):
    """the weights the backward pass must apply, from the kernel's own per-pixel losses and record"""
    w = np.zeros(px_bits.shape, dtype=np.float64)
    for i in range(px_bits.shape[0]):
        cp, cn, k, tb, c_gt, c_eq, r, _ = (int(v) for v in rec[i])
        key = px_bits[i]
        w[i][key >= R.SIGN] = 1.0
        if k:
            t = np.uint32(tb & 0xffffffff)
            w[i][(key < R.SIGN) & (key > t)] = 1.0
            w[i][key == t] = np.float64(np.float32(r) / np.float32(c_eq))
    return w


def check(logits, labels, ls=1, need_gap=False, ties=False, grad=True):
    """(a) - (d) on one input; returns the kernel's records"""
    loss, px, rec, sums, d = run(logits, labels, ls)
    l64, y = R.pixel_ce(logits, labels, ls)
    N, C = logits.shape[:2]
    neg = (y == 0).numpy()
    # (a)
    got = px.view(np.float32).astype(np.float64)
    assert np.array_equal(px[~neg], np.full(int((~neg).sum()), 0xbf800000, dtype=np.uint32))
    assert (px[neg] < R.SIGN).all()
    if neg.any():
        err = np.abs(got[neg] - l64.numpy()[neg]).max()
        assert err <= 2e-6, "per-pixel loss: %.3e" % err
    # (b)
    want = np.array([R.forward_record(px[i]) for i in range(N)], dtype=np.int32)
    assert np.array_equal(rec, want), (rec, want)
    count = int(sum(want[:, 0]) + sum(want[:, 2]))
    assert sums[2] == count
    if grad:
        # (c)
        w = torch.from_numpy(host_weights(px, rec))
        p = torch.softmax(logits.double().reshape(N, C, -1), 1)
        onehot = torch.zeros_like(p).scatter_(1, y.clamp(max=C - 1).unsqueeze(1), 1.0)
        formula = (w.unsqueeze(1) * (p - onehot) / count).reshape(logits.shape)
        close(d, formula, 2e-5, "dlogits vs formula")
    # (d)
    x = logits.double().requires_grad_(True)
    ref = R.ohem_hard(x, labels, ls)
    gap = R.boundary_gap(logits, labels, ls)
    print("loss %.9g reference %.12g boundary gap %.3e" % (float(loss), float(ref.detach()), gap))
    assert abs(float(loss) - float(ref.detach())) <= 2e-6 * max(1.0, abs(float(ref.detach())))
    if need_gap:
        assert gap >= GAP, "choose another seed: gap %.3e" % gap
    if grad and (gap >= GAP or (ties and gap == 0.0)):
        ref.backward()
        close(d, x.grad, 2e-5, "dlogits vs reference")
    return rec


def randn_case(shape, pos, seed):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = torch.randn(shape, generator=g) * 2
    y = torch.zeros(N, H, W, dtype=torch.uint8)
    if pos > 0:
        y = (torch.rand(N, H, W, generator=g) < pos).to(torch.uint8)
        if C == 4:
            y = y * torch.randint(1, 4, (N, H, W), generator=g, dtype=torch.uint8)
    return x, y


# (shape, share of positives, seed): odd sizes with a different k per image; no positives (k = max(Cn // 4, 5)); 2 Cp > Cn
# (every negative kept); C = 4
RANDOM = {"odd_3x2x37x53": ((3, 2, 37, 53), 0.10, 11), "nopos_2x2x9x11": ((2, 2, 9, 11), 0.0, 12),
          "manypos_2x2x48x48": ((2, 2, 48, 48), 0.60, 13), "c4_2x4x64x64": ((2, 4, 64, 64), 0.10, 18)}


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_shapes(name):
    shape, pos, seed = RANDOM[name]
    x, y = randn_case(shape, pos, seed)
    rec = check(x, y, need_gap=True)
    if name.startswith("odd"):
        assert len({int(k) for k in rec[:, 2]}) == 3
    if name.startswith("nopos"):
        assert (rec[:, 0] == 0).all() and (rec[:, 2] == 99 // 4).all()
    if name.startswith("manypos"):
        assert (2 * rec[:, 0] > rec[:, 1]).all() and (rec[:, 2] == rec[:, 1]).all()


def test_fewer_negatives_than_the_floor_and_none_at_all():
    g = torch.Generator().manual_seed(14)
    x = torch.randn(1, 2, 2, 2, generator=g) * 2
    y = torch.tensor([[[0, 1], [0, 0]]], dtype=torch.uint8)
    assert check(x, y)[0].tolist()[:3] == [1, 3, 3]
    x = torch.randn(1, 2, 1, 3, generator=g) * 2
    rec = check(x, torch.ones(1, 1, 3, dtype=torch.uint8))
    assert rec[0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("cn,k", [(20, 5), (23, 5), (24, 6)])
def test_k_at_the_quarter_boundary(cn, k):
    g = torch.Generator().manual_seed(15 + cn)
    x = torch.randn(1, 2, 1, cn, generator=g) * 2
    rec = check(x, torch.zeros(1, 1, cn, dtype=torch.uint8))
    assert rec[0].tolist()[:3] == [0, cn, k]


def test_all_tied_and_threshold_inside_a_tied_class():
    """constant logits: one class of 256 equal losses, k = 64 of them kept, every weight exactly 1 / 4"""
    x = torch.zeros(1, 2, 16, 16)
    x[:, 1] = 0.75
    y = torch.zeros(1, 16, 16, dtype=torch.uint8)
    loss, px, rec, sums, d = run(x, y)
    assert rec[0].tolist()[:3] == [0, 256, 64] and rec[0].tolist()[4:] == [0, 256, 64, 0]
    assert np.float32(64) / np.float32(256) == 0.25
    g = d.reshape(2, -1)
    assert (g == g[:, :1]).all() and float(g[0, 0]) != 0.0
    p1 = torch.softmax(torch.tensor([0.0, 0.75], dtype=torch.float64), 0)[1]
    assert abs(float(g[1, 0]) - 0.25 * float(p1) / 64) <= 2e-5 * 0.25 * float(p1) / 64
    check(x, y, ties=True)
    # two values: 40 hard pixels, 216 easy ones -> the threshold is the easy class and 24 of its 216 places are taken;
    # 100 hard pixels -> the threshold is the hard class, 64 of 100
    for hard, want in ((40, [40, 216, 24]), (100, [0, 100, 64])):
        x = torch.zeros(1, 2, 16, 16)
        idx = torch.randperm(256, generator=torch.Generator().manual_seed(hard))[:hard]
        x[0, 1].view(-1)[idx] = 3.0
        x[0, 1] -= 1.0
        rec = check(x, y, ties=True)
        assert rec[0].tolist()[4:7] == want


def test_many_blocks_per_image():
    """256 x 256: 16 histogram blocks per image, the partial tables and the fixed-order sums across blocks"""
    x, y = randn_case((2, 2, 256, 256), 0.10, 17)
    check(x, y)


def test_megapixel_record_and_loss():
    x, y = randn_case((1, 2, 1024, 1024), 0.05, 19)
    check(x, y, grad=False)


def _select(rows, ks):
    from xview2_amd import ops
    bits = np.stack(rows).astype(np.uint32)
    vals = torch.from_numpy(bits.view(np.float32).copy()).to(dev())
    rec = ops.topk_select(vals, torch.tensor(ks, dtype=torch.int32, device=dev())).cpu().numpy()
    want = np.array([R.select_record(bits[i], ks[i]) for i in range(len(ks))], dtype=np.int32)
    assert np.array_equal(rec, want), (rec, want)
    return rec


def test_select_stage_on_crafted_buffers():
    rng = np.random.default_rng(21)
    # 4096 consecutive bit patterns (the top digit is shared, the low digits decide), shuffled, one row per k
    base = (0x3f800000 + np.arange(4096, dtype=np.uint32))
    ks = [1, 2, 1000, 1024, 1025, 2049, 4095, 4096, 5000, 0]
    _select([rng.permutation(base) for _ in ks], ks)
    # values on both sides of each digit boundary (bit 21 and bit 10), repeated so that ties straddle it too
    edge = np.array([0x3fdfffff, 0x3fe00000, 0x3fe00001, 0x3f8003ff, 0x3f800400, 0x3f800401, 0x001fffff, 0x00200000,
                     0x000003ff, 0x00000400, 0x7f7fffff, 0x7f800000], dtype=np.uint32)
    row = np.repeat(edge, 3)
    _select([rng.permutation(row) for _ in range(1, 37, 5)], list(range(1, 37, 5)))
    # denormals only; zeros of both signs among small values (-0.0 is a zero, not a skipped entry)
    den = rng.integers(1, 1 << 23, 777, dtype=np.uint32)
    _select([den, den, den], [1, 300, 777])
    zeros = np.concatenate([np.zeros(10, np.uint32), np.full(7, 0x80000000, np.uint32), np.arange(1, 6, dtype=np.uint32)])
    rec = _select([rng.permutation(zeros) for _ in range(3)], [5, 6, 22])
    assert rec[1].tolist() == [0, 22, 6, 0, 5, 17, 1, 0]
    # +Inf, and NaN above it
    top = np.concatenate([np.full(4, 0x7f800000, np.uint32), np.full(2, 0x7fc00000, np.uint32),
                          rng.integers(0, 0x7f800000, 50, dtype=np.uint32)])
    rec = _select([top, top, top], [2, 3, 7])
    assert rec[0].tolist()[3:7] == [0x7fc00000, 0, 2, 2] and rec[1].tolist()[3:7] == [0x7f800000, 2, 4, 1]
    # all equal
    _select([np.full(300, 0x40490fdb, np.uint32)] * 3, [1, 150, 300])
    # skipped entries (sign bit set: negative numbers, negative NaN) interleaved with candidates; several blocks per row
    cand = rng.integers(0, 0x7f800000, 10000, dtype=np.uint32)
    skip = rng.integers(0x80000001, 0xffffffff, 10000, dtype=np.uint32, endpoint=True)
    mixed = np.where(rng.random(10000) < 0.5, cand, skip)
    rec = _select([mixed, mixed, cand, skip], [1, 2500, 9999, 3])
    assert rec[3].tolist() == [0] * 8


def test_nan_wins_and_stays_in_its_image():
    x, y = randn_case((2, 2, 16, 16), 0.10, 22)
    _, _, rec0, _, _ = run(x, y)
    q = int(torch.nonzero(y[0].reshape(-1) == 0)[5])
    x.view(2, 2, -1)[0, 1, q] = float("nan")
    loss, px, rec, sums, d = run(x, y)          # returns: nothing waits on a value
    assert np.isnan(float(loss))
    assert np.array_equal(rec[1], rec0[1])
    # the NaN is ONE bit pattern above +Inf: the largest of image 0's negatives, so among the k selected (above t)
    assert px[0, q] == 0x7fc00000 and rec[0].tolist()[:3] == rec0[0].tolist()[:3]
    assert px[0, q] > np.uint32(rec[0, 3]) and rec[0, 4] == rec[0, 2] - 1
    assert np.array_equal(rec, np.array([R.forward_record(px[i]) for i in range(2)], dtype=np.int32))
    assert np.isnan(sums[1]) and np.isfinite(sums[0])


def test_two_calls_are_bit_equal():
    x, y = randn_case((2, 2, 96, 96), 0.10, 23)
    a, b = run(x, y), run(x, y)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_backward_argument_errors_come_before_any_launch():
    """lstride = 0, H = 0, N = 0 and a null labels pointer are refused on the host: dlogits and its guards keep their fill"""
    from xview2_amd import _capi, ops
    x, y = randn_case((1, 2, 4, 6), 0.3, 29)
    loss, px, rec, sums, lg, lb = ops.ohem_forward(x.to(dev()), y.to(dev()))
    gs = torch.ones(1, dtype=torch.float32, device=dev())
    pad = 64
    buf = torch.full((lg.numel() + 2 * pad,), 2.0 ** 100, dtype=torch.float32, device=dev())
    before = buf.clone()
    d = buf[pad:pad + lg.numel()]
    for N, H, ls, labels in ((1, 4, 0, lb), (1, 0, 1, lb), (0, 4, 1, lb), (1, 4, 1, None)):
        with pytest.raises(RuntimeError):
            _capi.call("xv2_ohem_backward", lg, labels, N, 2, H, 6, ls, px, rec, sums, gs, d)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


def _ds_inputs():
    g = torch.Generator().manual_seed(24)
    preds = [torch.randn(2, 2, s, s, generator=g) * 2 for s in (32, 16, 8)]
    y = (torch.rand(2, 32, 32, generator=g) < 0.15).to(torch.uint8)
    return preds, y


def test_deep_supervision_keeps_each_heads_buffers():
    """criterion.compute_loss runs the three heads' forward passes before any backward: each node owns its per-pixel
    losses and record, so a head's gradient is bit-equal to that head's run alone"""
    from oracle import torch_ref
    from xview2_amd import criterion
    a = ARGS(type="pre", loss_str="ohem_hard+dice", deep_supervision=True)
    preds, y = _ds_inputs()
    for j, p in enumerate(preds):
        assert R.boundary_gap(p, y, 2 ** j) >= GAP
    dice = torch_ref.Loss(ARGS(type="pre", loss_str="dice"))
    pr = [p.clone().double().requires_grad_(True) for p in preds]
    lo = 0
    for j, p in enumerate(pr):
        s = 2 ** j
        lo = lo + 0.5 ** j * (dice(p, y[:, ::s, ::s]) + R.ohem_hard(p, y, s))
    lo = lo / (2 - 2 ** -3)
    lo.backward()
    loss_fn = criterion.Loss(a)
    pg = [p.to(dev()).requires_grad_(True) for p in preds]
    lh = criterion.compute_loss(loss_fn, pg, y.to(dev()), True)
    lh.backward()
    assert abs(float(lh) - float(lo)) <= 2e-6 * max(1.0, abs(float(lo)))
    c_norm = 1 / (2 - 2 ** -3)
    for j, (g, r, p) in enumerate(zip(pg, pr, preds)):
        close(g.grad, r.grad, 2e-5, "ds dlogits head %d" % j)
        alone = p.to(dev()).requires_grad_(True)
        la = loss_fn(alone, y.to(dev()), label_stride=2 ** j)
        (c_norm * (la if j == 0 else 0.5 ** j * la)).backward()
        assert torch.equal(alone.grad, g.grad), "head %d" % j


def test_post_is_ce_and_ohem_is_still_ce():
    from tests.golden.cases import loss_inputs
    from xview2_amd import criterion

    def both(a, b):
        yp, yt = loss_inputs(a, batch=2, size=24)
        out = []
        for args in (a, b):
            x = yp.to(dev()).requires_grad_(True)
            l = criterion.Loss(args)(x, yt.to(dev()))
            l.backward()
            out.append((l.detach().cpu(), x.grad.cpu()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        return yp, yt, out[0]
    both(ARGS(type="post", loss_str="ohem_hard"), ARGS(type="post", loss_str="ce"))
    both(ARGS(type="post", loss_str="ohem_hard+dice"), ARGS(type="post", loss_str="ce+dice"))
    yp, yt, (l_ce, _) = both(ARGS(type="pre", loss_str="ohem"), ARGS(type="pre", loss_str="ce"))
    # ... and under pre the new term is a different number, through the public module
    x = yp.to(dev()).requires_grad_(True)
    l_hard = criterion.Loss(ARGS(type="pre", loss_str="ohem_hard"))(x, yt.to(dev()))
    ref = R.ohem_hard(yp, yt)
    assert abs(float(l_hard) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref))) and abs(float(l_hard) - float(l_ce)) > 1e-3
    # a term named twice counts twice
    l2 = criterion.Loss(ARGS(type="pre", loss_str="ohem_hard+ohem_hard"))(x, yt.to(dev()))
    assert float(l2) == 2 * float(l_hard)


def test_cli_trains_with_ohem_hard(tmp_path, monkeypatch):
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
    m = cli.main(["--exec_mode", "train", "--type", "pre", "--loss_str", "ohem_hard+dice", "--epochs", "1", "--results", res,
                  "--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
                  "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3"])
    assert len(seen) == 3 and all(np.isfinite(float(l)) for l in seen)
    assert os.path.exists(os.path.join(res, "checkpoints", "last.ckpt"))
    assert all(torch.isfinite(p).all() for p in m.parameters())
