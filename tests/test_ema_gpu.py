"""The weight average on the GPU (csrc/optim.hip xv2_ema_update_dev, optim.FlatEMA, Trainer(ema_decay), --ema_decay /
--eval_ema) against the float64 restatement (tests/ema_ref.py), teacher-forced per call: the restatement is fed the
device's previous average and the parameters of the call, and every element must lie within the derived bound."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import ema_ref

pytestmark = pytest.mark.gpu

# the entry point's grid is min(ceil(ceil(n / 4) / 256), 4096) blocks of 256 threads, one float4 per thread and trip: 4096 * 256 * 4
# = 2^22 elements per trip, so 2^22 + 5 elements give thread 0 a second trip of the 16-byte loop and leave one tail element
TWO_TRIPS = 2 ** 22 + 5
SIZES = [1, 3, 4, 5, 255, 1024, 1025, 1000003, TWO_TRIPS]
# (decay, warm-up, counter before the call): t = 3 under warm-up gives d = 4 / 13 for both 0.9 and 0.9999, and 0 for decay 0
MODES = [(0.0, False, 0), (0.0, True, 3), (0.9, False, 7), (0.9, True, 3), (0.9, True, 500), (0.9999, False, 0), (0.9999, True, 3),
         (0.9999, True, 10 ** 6)]
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan")]

_BUF = {}


def _buffers():
    """one pair of random host buffers for every entry-point test, never written after this"""
    if not _BUF:
        gen = torch.Generator().manual_seed(31)
        _BUF["e"] = 0.1 * torch.randn(TWO_TRIPS + 8, generator=gen, dtype=torch.float32)
        _BUF["p"] = 0.1 * torch.randn(TWO_TRIPS + 8, generator=gen, dtype=torch.float32)
    return _BUF["e"], _BUF["p"]


def _update(ema, param, decay, warmup, count, guard=None):
    from xview2_amd._capi import call
    call("xv2_ema_update_dev", ema, param, ema.numel(), float(decay), int(warmup), count, guard)
    torch.cuda.synchronize()


def _planted(n, e, p):
    """0, -0, +-Inf and NaN in `param`, each at another lane of a 16-byte group of its own (elements 0, 5, 10, 15, 16: the three
    group neighbours of each stay ordinary values and are checked against the bound like every element), two more in the tail
    behind the last whole group, and an Inf in `ema` where the parameter is finite.  A buffer too short for that takes the
    specials in its first elements."""
    e, p = e[:n].clone(), p[:n].clone()
    if n > 24:
        for g, v in enumerate(SPECIALS):
            p[4 * g + g % 4] = v
        e[22] = float("inf")
        e[21] = float("-inf")
        tail = n - n % 4
        if n % 4:
            p[n - 1] = float("nan")
        if n % 4 > 1:
            p[tail] = float("inf")
    else:
        for i in range(min(n, len(SPECIALS))):
            p[i] = SPECIALS[(i + n) % len(SPECIALS)]
    return e, p


def _run_modes(e0, p0, misalign_e=False, misalign_p=False):
    n = e0.numel()
    hold_e = torch.empty(n + 8, dtype=torch.float32, device="cuda")
    hold_p = torch.empty(n + 8, dtype=torch.float32, device="cuda")
    ema = hold_e[1:1 + n] if misalign_e else hold_e[4:4 + n]
    param = hold_p[1:1 + n] if misalign_p else hold_p[4:4 + n]
    assert (ema.data_ptr() % 16 != 0) == misalign_e and (param.data_ptr() % 16 != 0) == misalign_p
    param.copy_(p0)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for decay, warm, t in MODES:
        ema.copy_(e0)
        count.fill_(t)
        _update(ema, param, decay, warm, count)
        worst = ema_ref.check(ema, e0, p0, ema_ref.om32(decay, t, warm))
        print("n=%d decay=%g warmup=%d t=%d: largest error / bound %.3f" % (n, decay, warm, t, worst))
        assert int(count.item()) == t + 1
        assert torch.equal(param.cpu().view(torch.int32), p0.view(torch.int32))          # the parameters are only read


@pytest.mark.parametrize("n", SIZES)
def test_the_kernel_matches_the_restatement(n):
    e, p = _buffers()
    e0, p0 = _planted(n, e, p)
    if n > 24:
        assert bool(torch.isfinite(p0[[1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19]]).all())
    _run_modes(e0, p0)


@pytest.mark.parametrize("which", ["ema", "param", "both"])
def test_a_pointer_off_16_byte_alignment_takes_the_scalar_loop(which):
    e, p = _buffers()
    e0, p0 = _planted(1027, e, p)
    _run_modes(e0, p0, misalign_e=which in ("ema", "both"), misalign_p=which in ("param", "both"))


@pytest.mark.parametrize("off", [0, 1])
def test_equal_average_and_parameter_stay_bit_for_bit(off):
    e, _ = _buffers()
    n = 262147
    e0 = e[:n].clone()
    e0[8] = 0.0
    hold_e = torch.empty(n + 8, dtype=torch.float32, device="cuda")
    ema, param = hold_e[4 - off:4 - off + n], e0.cuda()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for decay, warm, t in MODES:
        ema.copy_(e0)
        count.fill_(t)
        _update(ema, param, decay, warm, count)
        assert torch.equal(ema.cpu().view(torch.int32), e0.view(torch.int32)), (decay, warm, t)
    # the one value the arithmetic cannot hold: an average of -0 comes back as +0 ((-0) - (-0) = +0, then +0 + -0 = +0), the
    # same number; the restatement says the same
    e0[9] = -0.0
    ema.copy_(e0)
    param.copy_(e0)
    _update(ema, param, 0.9, True, count)
    got = ema.cpu()
    assert torch.equal(got, e0) and got.view(torch.int32)[9] == 0
    assert torch.equal(got.view(torch.int32)[:9], e0.view(torch.int32)[:9])
    assert torch.equal(got.view(torch.int32)[10:], e0.view(torch.int32)[10:])


def test_the_warmup_schedule_over_a_hundred_calls():
    e, p = _buffers()
    n = 37
    ema, param = e[:n].cuda(), p[:n].cuda()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in range(101):
        prev = ema.clone()
        _update(ema, param, 0.9, True, count)
        ema_ref.check(ema, prev, param, ema_ref.om32(0.9, t))
        assert int(count.item()) == t + 1
    # the whole chain against the restatement run on its own: 101 updates, each within its bound of a contraction
    ref = e[:n].double()
    for t in range(101):
        ref = ema_ref.update(ref, p[:n], ema_ref.om32(0.9, t))
    # (a step's bound is at most 2^-22 (|p - e| + |e|), and every value here is below 0.6 in magnitude)
    assert float(torch.maximum(e[:n].abs().max(), p[:n].abs().max())) < 0.6
    assert float((ema.cpu().double() - ref).abs().max()) <= 101 * 2.0 ** -22 * 1.8


# ---------------------------------------------------------------------------------------------------------------
# the guard record
def _record(skip, coef):
    rec = torch.zeros(16, dtype=torch.int32)
    rec.view(torch.float32)[1] = coef
    rec[2] = skip
    return rec.cuda()


def _banded(values, band=64):
    hold = torch.full((values.numel() + 2 * band,), 7.25, dtype=values.dtype)
    hold[band:band + values.numel()] = values
    hold = hold.cuda()
    return hold, hold[band:band + values.numel()]


@pytest.mark.parametrize("n", [5, 1027, 262147])
def test_a_record_that_says_skip_leaves_the_average_and_the_counter_bit_for_bit(n):
    from xview2_amd._capi import Ptr
    e, p = _buffers()
    hold_e, ema = _banded(e[:n])
    hold_p, param = _banded(p[:n])
    counts = torch.tensor([77, 5, 99], dtype=torch.int32, device="cuda")
    before = (hold_e.clone(), hold_p.clone(), counts.clone())
    _update(ema, param, 0.9, True, Ptr(counts, 1), _record(1, 0.25))
    assert torch.equal(hold_e, before[0]) and torch.equal(hold_p, before[1]) and torch.equal(counts, before[2])
    # skip = 0: the coefficient is ignored, the result is the unguarded call's bit for bit, and the bands stay intact
    _update(ema, param, 0.9, True, Ptr(counts, 1), _record(0, 0.25))
    hold_t, twin = _banded(e[:n])
    count_t = torch.tensor([5], dtype=torch.int32, device="cuda")
    _update(twin, param, 0.9, True, count_t)
    assert torch.equal(hold_e, hold_t) and not torch.equal(hold_e, before[0])
    assert torch.equal(hold_p, before[1]) and counts.tolist() == [77, 6, 99] and int(count_t.item()) == 6
    ema_ref.check(ema, e[:n], p[:n], ema_ref.om32(0.9, 5))


# ---------------------------------------------------------------------------------------------------------------
# FlatEMA behind two optimizers on a ragged shape set (the shapes of tests/test_optimizers_gpu.py)
SHAPES = [(64, 32, 3, 3), (256, 64, 1, 1), (64, 3, 7, 7), (5, 64), (64,), (7,), (16, 16), (2, 70000)]


def _views(opt, flat):
    return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(opt.params, opt.offsets)]


def _feed(opt, gen, scale=1e-2):
    opt.zero_grad()
    for v in _views(opt, opt.flat_g):
        v.copy_(scale * torch.randn(v.shape, generator=gen))


@pytest.mark.parametrize("name", ["adamw", "novograd"])
def test_flat_ema_follows_the_optimizer_on_the_ragged_shapes(name):
    from xview2_amd.optim import FlatEMA, make_flat_optimizer
    gen = torch.Generator().manual_seed(13)
    params = [torch.nn.Parameter((0.1 * torch.randn(s, generator=gen)).cuda()) for s in SHAPES]
    opt = make_flat_optimizer(name, params, lr=1e-2, weight_decay=1e-2)
    ema = FlatEMA(opt, 0.9)
    assert ema.ema.shape == opt.flat_p.shape and torch.equal(ema.ema, opt.flat_p) and ema.ema.data_ptr() != opt.flat_p.data_ptr()
    pad = torch.ones(opt.total, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) == opt.total - sum(p.numel() for p in opt.params) > 0
    for t in range(5):
        _feed(opt, gen)
        prev = ema.ema.clone()
        opt.step()
        ema.update()
        torch.cuda.synchronize()
        worst = ema_ref.check(ema.ema, prev, opt.flat_p, ema_ref.om32(0.9, t))
        print(name, "step", t + 1, "largest error / bound %.3f" % worst)
        assert not torch.equal(ema.ema, prev) and not torch.equal(ema.ema, opt.flat_p)
        assert bool((ema.ema.cpu()[pad] == 0).all()) and bool((opt.flat_p.cpu()[pad] == 0).all())
        assert ema.state_dict() == {"decay": 0.9, "warmup": True, "updates": t + 1}
    # a non-finite gradient under skip_nonfinite: the step and the average are both skipped
    opt.set_guard(skip_nonfinite=True)
    _feed(opt, gen)
    opt.step()
    ema.update()
    assert ema.state_dict()["updates"] == 6 and int(opt.step_dev.item()) == 6
    before = (opt.flat_p.clone(), ema.ema.clone())
    _feed(opt, gen)
    opt.flat_g[opt.offsets[-1] + 12345] = float("inf")
    opt.step()
    ema.update()
    torch.cuda.synchronize()
    assert opt.guard_stats()["skip"] == 1
    assert torch.equal(opt.flat_p, before[0]) and torch.equal(ema.ema, before[1])
    assert ema.state_dict()["updates"] == 6 and opt.step_count == 7 and int(opt.step_dev.item()) == 6
    _feed(opt, gen)
    opt.step()
    ema.update()
    worst = ema_ref.check(ema.ema, before[1], opt.flat_p, ema_ref.om32(0.9, 6))
    assert ema.state_dict()["updates"] == 7 == opt.step_count - 1


def test_flat_ema_state_dict_round_trip_restores_counter_and_buffer_by_name():
    from xview2_amd.optim import FlatEMA, make_flat_optimizer
    gen = torch.Generator().manual_seed(17)

    def build():
        m = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Conv2d(5, 7, 1)).cuda()
        return m, make_flat_optimizer("adamw", m.parameters(), lr=1e-2)
    m, opt = build()
    ema = FlatEMA(opt, 0.9)
    for _ in range(3):
        _feed(opt, gen)
        opt.step()
        ema.update()
    sd, esd = ema.state_dict(), {k: v.clone().cpu() for k, v in ema.model_state_dict(m).items()}
    assert sd["updates"] == 3 and set(esd) == set(m.state_dict())
    m2, opt2 = build()
    other = FlatEMA(opt2, 0.9)
    other.load_state_dict(sd, esd, m2)
    assert torch.equal(other.ema, ema.ema) and int(other.count_dev.item()) == 3


# ---------------------------------------------------------------------------------------------------------------
# the swap
def _model(seed=1):
    from tests.golden.cases import ARGS
    from xview2_amd import networks
    from xview2_amd.weights import deterministic_init_
    a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
    torch.manual_seed(0)
    m = networks.UNetLoc(a)
    deterministic_init_(m, seed)
    return a, m.cuda().train()


def _train_step(a, m, opt, ema, x, y):
    from xview2_amd import criterion
    m.train()
    opt.zero_grad()
    criterion.Loss(a)(m(x), y).backward()
    opt.step()
    ema.update()


def _three_steps():
    from tests.golden.cases import labels, model_input
    from xview2_amd.optim import FlatEMA, make_flat_optimizer
    a, m = _model()
    x, y = model_input(a, batch=2).cuda(), labels(a, batch=2).cuda()
    opt = make_flat_optimizer("adamw", m.parameters(), lr=1e-3, weight_decay=1e-2)
    ema = FlatEMA(opt, decay=0.5, warmup=False)
    for _ in range(3):
        _train_step(a, m, opt, ema, x, y)
    return a, m, opt, ema, x, y


@torch.no_grad()
def _eval_logits(m, x):
    m.eval()
    out = m(x).clone()
    torch.cuda.synchronize()
    return out


def test_the_swap_computes_with_the_average_and_leaves_training_untouched():
    from xview2_amd import networks
    a, m, opt, ema, x, y = _three_steps()
    before = _eval_logits(m, x)
    live = opt.flat_p.clone()
    avg = {k: v.clone() for k, v in ema.model_state_dict(m).items()}
    ptrs = [p.data_ptr() for p in m.parameters()]
    with ema.applied():
        inside = _eval_logits(m, x)
        assert [p.data_ptr() for p in m.parameters()] == ptrs           # the same views
        for k, v in ema.model_state_dict(m).items():                    # inside, the average is what the model holds
            assert torch.equal(v, avg[k]), k
        with pytest.raises(RuntimeError):
            ema.update()
    after = _eval_logits(m, x)
    fresh = networks.UNetLoc(a)
    fresh.load_state_dict(avg)
    fresh_logits = _eval_logits(fresh.cuda(), x)
    assert torch.equal(inside, fresh_logits)            # stale layouts of the live weights would show here ...
    assert torch.equal(after, before)                   # ... and stale layouts of the average here
    assert not torch.equal(inside, before) and torch.equal(opt.flat_p, live)
    # an exception inside the context still restores the weights
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            assert not torch.equal(opt.flat_p, live)
            raise ZeroDivisionError
    assert torch.equal(opt.flat_p, live) and torch.equal(_eval_logits(m, x), before)
    # a fourth step against a twin that never entered the context
    _train_step(a, m, opt, ema, x, y)
    a2, m2, opt2, ema2, _, _ = _three_steps()
    _train_step(a2, m2, opt2, ema2, x, y)
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_p, opt2.flat_p) and torch.equal(ema.ema, ema2.ema)
    for (k, u), (_, v) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(u, v), k
    assert ema.state_dict()["updates"] == ema2.state_dict()["updates"] == 4


# ---------------------------------------------------------------------------------------------------------------
# the CLI: the arguments of tests/test_trainer_gpu.py::test_resume_continues_the_uninterrupted_run_bit_for_bit
COMMON = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
          "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3",
          "--exec_mode", "train", "--type", "pre", "--loss_str", "dice", "--use_scheduler", "--warmup", "1",
          "--final_lr", "1e-5"]
EVAL = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
        "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3", "--exec_mode", "eval", "--type", "pre"]


def _last(root, name):
    return os.path.join(root, name, "checkpoints", "last.ckpt")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """one epoch with the average, one without, and the uninterrupted two-epoch run: trained once for the tests below"""
    import main as cli
    root = str(tmp_path_factory.mktemp("ema_cli"))
    with_ema = COMMON + ["--ema_decay", "0.9"]
    model = cli.main(with_ema + ["--epochs", "1", "--results", os.path.join(root, "half")])
    cli.main(with_ema + ["--epochs", "2", "--results", os.path.join(root, "full")])
    cli.main(COMMON + ["--epochs", "1", "--results", os.path.join(root, "plain")])
    # (every registered name of a buffer: FusedUNet registers its stages twice, and state_dict() carries both names)
    return {"root": root, "with_ema": with_ema, "buffers": {k for k, _ in model.named_buffers(remove_duplicate=False)}}


def test_the_checkpoint_carries_the_average_next_to_the_live_weights(runs):
    blob = torch.load(_last(runs["root"], "half"), map_location="cpu", weights_only=False)
    sd, esd = blob["state_dict"], blob["ema_state_dict"]
    assert list(esd) == list(sd) and all(esd[k].shape == sd[k].shape and esd[k].dtype == sd[k].dtype for k in sd)
    assert blob["ema"] == {"decay": 0.9, "warmup": True, "updates": 3} and blob["global_step"] == 3
    buffers = runs["buffers"]
    assert buffers and buffers < set(sd)
    assert all(torch.equal(esd[k], sd[k]) for k in buffers)
    moved = [k for k in sd if k not in buffers and not torch.equal(esd[k], sd[k])]
    assert "model.unet.enc_l1.0.weight" in moved and len(moved) > (len(sd) - len(buffers)) // 2
    assert all(bool(torch.isfinite(v).all()) for v in esd.values() if v.is_floating_point())
    # the epoch's record says which weights were validated
    lines = [ln for ln in open(os.path.join(runs["root"], "half", "logs.json")) if ln.startswith("DLLL ")]
    data = json.loads(lines[-1][5:])["data"]
    assert data["ema"] is True and {"f1", "val_loss", "top_f1"} <= set(data)
    # the same command without --ema_decay: no ema* key, no "ema" in the record
    plain = torch.load(_last(runs["root"], "plain"), map_location="cpu", weights_only=False)
    assert not [k for k in plain if k.startswith("ema")] and set(plain) == set(blob) - {"ema", "ema_state_dict"}
    lines = [ln for ln in open(os.path.join(runs["root"], "plain", "logs.json")) if ln.startswith("DLLL ")]
    assert "ema" not in json.loads(lines[-1][5:])["data"]
    # and the average changed nothing about training: the live weights are those of the run without it
    assert all(torch.equal(plain["state_dict"][k], sd[k]) for k in sd)


def test_resume_continues_the_average_of_the_uninterrupted_run_bit_for_bit(runs):
    import main as cli
    root = runs["root"]
    ck = os.path.join(root, "half.ckpt")
    shutil.copy(_last(root, "half"), ck)
    cli.main(runs["with_ema"] + ["--epochs", "2", "--results", os.path.join(root, "res"), "--ckpt", ck])
    full = torch.load(_last(root, "full"), map_location="cpu", weights_only=False)
    res = torch.load(_last(root, "res"), map_location="cpu", weights_only=False)
    assert full["ema"] == res["ema"] == {"decay": 0.9, "warmup": True, "updates": 6}
    for key in ("state_dict", "ema_state_dict"):
        assert set(full[key]) == set(res[key])
        for k in full[key]:
            assert torch.equal(full[key][k], res[key][k]), (key, k)
    # --ema_decay on a checkpoint without an average: it starts from the loaded weights with counter 0
    ck2 = os.path.join(root, "plain.ckpt")
    shutil.copy(_last(root, "plain"), ck2)
    cli.main(runs["with_ema"] + ["--epochs", "2", "--results", os.path.join(root, "late"), "--ckpt", ck2])
    late = torch.load(_last(root, "late"), map_location="cpu", weights_only=False)
    assert late["ema"]["updates"] == 3 and late["global_step"] == 6
    assert all(torch.equal(late["state_dict"][k], full["state_dict"][k]) for k in full["state_dict"])


def test_eval_ema_evaluates_the_averaged_weights(runs):
    import main as cli
    root = runs["root"]
    ck = _last(root, "half")
    probs = {}
    for name, extra in (("live", []), ("avg", ["--eval_ema"])):
        out = os.path.join(root, "eval_" + name)
        cli.main(EVAL + ["--ckpt", ck, "--results", out] + extra)
        files = sorted(os.listdir(os.path.join(out, "probs")))
        assert len(files) == 4
        probs[name] = [np.load(os.path.join(out, "probs", f)) for f in files]
    assert all(np.isfinite(p).all() for p in probs["avg"])
    assert any(not np.array_equal(u, v) for u, v in zip(probs["live"], probs["avg"]))
    with pytest.raises(KeyError, match="last.ckpt"):
        cli.main(EVAL + ["--ckpt", _last(root, "plain"), "--results", os.path.join(root, "eval_none"), "--eval_ema"])
