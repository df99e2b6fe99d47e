"""Gradient accumulation on the GPU (csrc/optim.hip xv2_grad_accumulate, FlatOptimizer.accumulate / step,
GradReducer.prepare(sync=False), Trainer(accumulate_grad_batches), --accumulate_grad_batches) against the host restatement
(tests/accum_ref.py) and against twins that are fed the group's sum.  A correctly rounded fp32 addition has one answer: every
comparison is on bits."""
import gc
import os
import socket

import pytest
import torch

from tests import accum_ref
from tests import test_grad_guard_gpu as gg
from tests import test_optimizers_gpu as og
from tests.golden.cases import ARGS, labels, model_input

pytestmark = pytest.mark.gpu

# the entry point's grid is min(ceil(ceil(n / 4) / 256), 4096) blocks of 256 threads, one float4 per thread and trip: 2^22 elements
# per trip, so 2^22 + 5 elements give thread 0 a second trip of the 16-byte loop and leave one tail element
TWO_TRIPS = 2 ** 22 + 5
SIZES = [1, 3, 4, 5, 255, 1024, 1025, 1000003, TWO_TRIPS]
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan")]
BAND, CANARY = 64, 7.25

_BUF = {}


def _buffers():
    """one pair of random host buffers for every entry-point test, never written after this"""
    if not _BUF:
        gen = torch.Generator().manual_seed(41)
        _BUF["a"] = 0.1 * torch.randn(TWO_TRIPS, generator=gen, dtype=torch.float32)
        _BUF["g"] = 0.1 * torch.randn(TWO_TRIPS, generator=gen, dtype=torch.float32)
    return _BUF["a"], _BUF["g"]


def _planted(n, a, g):
    """0, -0, +-Inf and NaN in `grad` at elements 0, 5, 10, 15, 16 (each at another lane of a 16-byte group of its own) and
    in `acc` at 25, 30, 35, 36, 41 opposite ordinary values; three meetings (-0 + -0, +0 + -0, Inf + -Inf) in the groups
    behind; two more in the tail behind the last whole group.  A buffer too short for that takes the specials in its first
    elements of both arrays, in different rotations."""
    a, g = a[:n].clone(), g[:n].clone()
    if n > 64:
        for k, v in enumerate(SPECIALS):
            g[4 * k + k % 4] = v
            a[24 + 4 * k + (k + 1) % 4] = v
        a[48], g[48] = -0.0, -0.0
        a[53], g[53] = 0.0, -0.0
        a[58], g[58] = float("inf"), float("-inf")
        tail = n - n % 4
        if n % 4:
            g[n - 1] = float("nan")
        if n % 4 > 1:
            a[tail] = float("inf")
    else:
        for i in range(min(n, len(SPECIALS))):
            g[i] = SPECIALS[(i + n) % len(SPECIALS)]
            a[i] = SPECIALS[(2 * i + n + 1) % len(SPECIALS)]
    return a, g


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run_modes(a0, g0, misalign_a=False, misalign_g=False):
    """each mode on a slice in the middle of a larger buffer with canary stretches on both sides"""
    from xview2_amd._capi import call
    n = a0.numel()
    oa, og_ = BAND + int(misalign_a), BAND + int(misalign_g)
    hold_a = torch.empty(n + 2 * BAND + 4, dtype=torch.float32, device="cuda")
    hold_g = torch.empty(n + 2 * BAND + 4, dtype=torch.float32, device="cuda")
    acc, grad = hold_a[oa:oa + n], hold_g[og_:og_ + n]
    assert (acc.data_ptr() % 16 != 0) == misalign_a and (grad.data_ptr() % 16 != 0) == misalign_g
    for mode in (accum_ref.OPEN, accum_ref.ADD, accum_ref.CLOSE):
        hold_a.fill_(CANARY)
        hold_g.fill_(CANARY)
        acc.copy_(a0)
        grad.copy_(g0)
        call("xv2_grad_accumulate", acc, grad, n, mode)
        torch.cuda.synchronize()
        want_a, want_g = accum_ref.apply(mode, a0, g0)
        assert accum_ref.same_bits(acc, want_a), (n, mode, "acc")
        assert accum_ref.same_bits(grad, want_g), (n, mode, "grad")
        # the array a mode only reads keeps its bits, NaN payloads included
        if mode != accum_ref.CLOSE:
            assert torch.equal(_bits(grad), _bits(g0)), (n, mode)
        else:
            assert torch.equal(_bits(acc), _bits(a0)), (n, mode)
        for hold, off in ((hold_a, oa), (hold_g, og_)):
            h = hold.cpu()
            assert bool((h[:off] == CANARY).all()) and bool((h[off + n:] == CANARY).all()), (n, mode)


@pytest.mark.parametrize("n", SIZES)
def test_the_kernel_matches_the_restatement(n):
    a, g = _buffers()
    a0, g0 = _planted(n, a, g)
    if n > 64:
        # the group neighbours of the planted values stay ordinary, and the planted sums are what IEEE says
        assert bool(torch.isfinite(g0[[1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19]]).all())
        s = a0 + g0
        assert int(s.view(torch.int32)[48]) == -2 ** 31 and int(s.view(torch.int32)[53]) == 0 and bool(torch.isnan(s[58]))
    _run_modes(a0, g0)


@pytest.mark.parametrize("which", ["acc", "grad", "both"])
def test_a_pointer_off_16_byte_alignment_takes_the_scalar_loop(which):
    a, g = _buffers()
    a0, g0 = _planted(1027, a, g)
    _run_modes(a0, g0, misalign_a=which in ("acc", "both"), misalign_g=which in ("grad", "both"))


# ---------------------------------------------------------------------------------------------------------------
# 2. FlatOptimizer.accumulate / step on the ragged shape set, every rule
def _grads(params, gen):
    cur = [p.detach().double().cpu() for p in params]
    return [og._grad(p, k, gen).float() for p, k in zip(cur, og.KINDS)]


def _group(opt, micro, scale=0.5):
    """zero_grad / feed / accumulate ... zero_grad / feed / step(scale)"""
    for k, gs in enumerate(micro):
        gg._feed(opt, gs)
        if k < len(micro) - 1:
            opt.accumulate()
            assert opt.pending == k + 1
    opt.step(scale)
    assert opt.pending == 0 and opt.buckets_closed is False


def _twin_group(twin, micro, scale=0.5):
    """the twin is fed the left-to-right sum and stepped with scale / m, divided in double"""
    gg._feed(twin, [accum_ref.group_sum([gs[i] for gs in micro]) for i in range(len(micro[0]))])
    twin.step(float(scale / len(micro)))


@pytest.mark.parametrize("name,momentum", og.CASES)
def test_groups_of_micro_gradients_equal_the_twin_fed_their_sum(name, momentum):
    init, gen = gg._init()
    opt, params = gg._make(name, momentum, init)
    twin, _ = gg._make(name, momentum, init)
    assert opt.flat_acc is None and opt.pending == 0
    # three groups in a row: a stale flat_acc (3 after 2), a count that is not reset (1 after 2) or a double close would show
    for m in (2, 1, 3):
        micro = [_grads(params, gen) for _ in range(m)]
        _group(opt, micro)
        _twin_group(twin, micro)
        torch.cuda.synchronize()
        assert gg._same(gg._everything(opt), gg._everything(twin)), (name, m)
        want = torch.cat([torch.nn.functional.pad(s.flatten(), (0, -s.numel() % 4))
                          for s in (accum_ref.group_sum([gs[i] for gs in micro]) for i in range(len(micro[0])))])
        assert accum_ref.same_bits(opt.flat_g, want), (name, m)              # the closed gradient is the group's sum
    assert int(opt.step_dev.item()) == int(twin.step_dev.item()) == 3 and opt.step_count == 3
    assert opt.flat_acc is not None and opt.flat_acc.shape == opt.flat_g.shape
    assert twin.flat_acc is None                                             # pending == 0 throughout: never allocated


# ---------------------------------------------------------------------------------------------------------------
# 3. with the guard
@pytest.mark.parametrize("name,momentum", [("adamw", 0.0), ("novograd", 0.0)])
def test_a_group_whose_sum_clips_equals_the_twins_clipped_step(name, momentum):
    init, gen = gg._init()
    opt, params = gg._make(name, momentum, init)
    twin, _ = gg._make(name, momentum, init)
    for o in (opt, twin):
        o.set_guard(max_norm=0.25)
    for m in (3, 2):
        micro = [_grads(params, gen) for _ in range(m)]
        _group(opt, micro)
        _twin_group(twin, micro)
        a, b = opt.guard_stats(), twin.guard_stats()
        assert a == b and a["coef"] < 1.0 and a["skip"] == 0, (a, b)      # the norm of the mean gradient, seen once
        assert gg._same(gg._everything(opt), gg._everything(twin))
    assert opt.guard_stats()["steps"] == opt.guard_stats()["clipped"] == 2


@pytest.mark.parametrize("name,momentum", [("adamw", 0.0), ("sgd", 0.9), ("adamp", 0.0)])
def test_an_inf_in_the_first_micro_gradient_skips_the_one_step_of_its_group(name, momentum):
    init, gen = gg._init()
    opt, params = gg._make(name, momentum, init)
    twin, _ = gg._make(name, momentum, init)                 # never sees the bad group, carries no guard
    opt.set_guard(skip_nonfinite=True)
    micro = [_grads(params, gen) for _ in range(2)]
    _group(opt, micro)
    _twin_group(twin, micro)
    assert gg._same(gg._everything(opt), gg._everything(twin))
    before = gg._everything(opt)
    bad = [_grads(params, gen) for _ in range(3)]
    bad[0][gg.LARGE].view(-1)[12345] = float("inf")
    _group(opt, bad)
    st = opt.guard_stats()
    assert (st["skip"], st["skipped"], st["steps"], st["skipped_in_a_row"]) == (1, 1, 2, 1)     # one skipped step, not m
    assert gg._same(gg._everything(opt), before)
    # the next group's open overwrites flat_acc: nothing outlives the group
    micro = [_grads(params, gen) for _ in range(2)]
    _group(opt, micro)
    _twin_group(twin, micro)
    assert gg._same(gg._everything(opt), gg._everything(twin))
    st = opt.guard_stats()
    assert (st["skip"], st["skipped"], st["steps"]) == (0, 1, 3) and int(opt.step_dev.item()) == 2
    assert bool(torch.isfinite(opt.flat_acc).all())


# ---------------------------------------------------------------------------------------------------------------
# 4. a model
def _build(kind):
    from xview2_amd import networks
    from xview2_amd.optim import make_flat_optimizer
    from xview2_amd.weights import deterministic_init_
    if kind == "loc":
        a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
        torch.manual_seed(0)
        m = networks.UNetLoc(a)
    else:                                                    # shared weights: the U-Net runs twice per forward pass
        a = ARGS(type="post", dmg_model="siamese", loss_str="focal+dice")
        torch.manual_seed(0)
        m = networks.get_dmg_unet(a)
    deterministic_init_(m, 1)
    m.cuda().train()
    return a, m, make_flat_optimizer("adamw", m.parameters(), lr=1e-3, weight_decay=1e-2)


def _batch(a, k, batch=2):
    return model_input(a, batch=batch, seed=1234 + 10 * k).cuda(), labels(a, batch=batch, seed=99 + 10 * k).cuda()


def _micro(a, m, opt, xy, red=None, sync=True):
    from xview2_amd import criterion
    opt.zero_grad()
    if red is not None:
        red.prepare(sync=sync)
    loss = criterion.compute_loss(criterion.Loss(a), m(xy[0]), xy[1], a.deep_supervision)
    loss.backward()
    return loss


def test_two_micro_batches_of_the_same_batch_equal_one_plain_step():
    a, m, opt = _build("loc")
    _, m2, twin = _build("loc")
    assert torch.equal(opt.flat_p, twin.flat_p)
    xy = _batch(a, 0)
    _micro(a, m, opt, xy)
    opt.accumulate()
    _micro(a, m, opt, xy)
    opt.step()                                               # 2 g * 0.5 = g exactly
    _micro(a, m2, twin, xy)
    twin.step()
    torch.cuda.synchronize()
    assert accum_ref.same_bits(opt.flat_g, (2.0 * twin.flat_g).cpu())
    assert torch.equal(opt.flat_p, twin.flat_p)
    for s in opt.STATE:
        assert torch.equal(getattr(opt, s), getattr(twin, s)), s
    assert twin.flat_acc is None


@pytest.mark.parametrize("kind", ["loc", "siamese"])
def test_the_closed_gradient_of_two_micro_batches_is_their_left_to_right_sum(kind):
    from xview2_amd import ops
    a, m, opt = _build(kind)
    _, m2, twin = _build(kind)
    b0, b1 = _batch(a, 0), _batch(a, 1)
    _micro(a, m, opt, b0)
    opt.accumulate()
    _micro(a, m, opt, b1)
    opt.step()                                               # (the rule only reads flat_g: it holds the closed sum afterwards)
    gs = []
    for xy in (b0, b1):                                      # the twin never steps: both gradients at the same weights
        _micro(a, m2, twin, xy)
        ops.join_wgrad_stream()
        twin._gather_foreign_grads()
        gs.append(twin.flat_g.cpu().clone())
    assert not torch.equal(gs[0], gs[1]) and float(gs[0].abs().max()) > 0.0
    assert accum_ref.same_bits(opt.flat_g, accum_ref.group_sum(gs))


# ---------------------------------------------------------------------------------------------------------------
# 5. the reducer on a single-rank NCCL group: the collectives are identities, so the bits are those of the run without them
def test_single_rank_nccl_groups_equal_the_run_without_collectives():
    import torch.distributed as dist
    from xview2_amd import dist as xdist
    from xview2_amd import networks, nn as xnn, ops
    from xview2_amd.optim import FlatAdamW
    from xview2_amd.weights import deterministic_init_
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    K = 3
    try:
        a = ARGS(encoder="resnet50", deep_supervision=True)
        batches = [_batch(a, k) for k in range(2 * K)]
        out = {}
        for mode, overlap in (("plain", True), ("dist", True), ("dist_no_overlap", False)):
            ops.FORCE_COLLECTIVES = mode != "plain"
            xnn.SYNC_BN = False
            torch.manual_seed(0)
            m = networks.UNetLoc(a)
            deterministic_init_(m, 1)
            m.cuda().train()
            opt = FlatAdamW(m.parameters(), lr=1e-3)
            red = xdist.GradReducer(opt, bucket_bytes=8 << 20, overlap=overlap)      # small buckets: several fire inside backward
            assert red.enabled == (mode != "plain") and xnn.SYNC_BN == (mode != "plain")
            assert not red.enabled or len(red.buckets) >= 4
            for k, xy in enumerate(batches):
                closes = k % K == K - 1
                _micro(a, m, opt, xy, red, sync=closes)
                if red.enabled:
                    fired = len(red.handles)
                    assert (fired >= 2) if (closes and overlap) else (fired == 0), (mode, k, fired)
                if closes:
                    assert opt.pending == K - 1
                    opt.step(red.finish())
                    assert opt.pending == 0 and opt.buckets_closed is False
                else:
                    opt.accumulate()
            torch.cuda.synchronize()
            var = [k for k in m.state_dict() if k.endswith("running_var")][3]
            out[mode] = (opt.flat_p.clone(), m.state_dict()[var].clone(), int(opt.step_dev.item()))
        for mode in ("dist", "dist_no_overlap"):
            assert torch.equal(out["plain"][0], out[mode][0]), mode
            assert torch.equal(out["plain"][1], out[mode][1]), mode
            assert out[mode][2] == out["plain"][2] == 2
    finally:
        ops.FORCE_COLLECTIVES = False
        xnn.SYNC_BN = False
        xdist.reset_peer_exchange()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------
# 6. two ranks sharing the GPU
def _two_rank_worker(rank, world, port, outdir):
    """one of two ranks sharing cuda:0 (gloo carries the buckets and the SyncBatchNorm statistics, as in
    tests/test_optimizers_gpu.py::_fit_worker): two groups of K = 2, once with the overlapped reducer and once without"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    os.environ.setdefault("XV2_SYNCBN", "rccl")
    import torch.distributed as dist
    from xview2_amd import dist as xdist
    from xview2_amd import networks, nn as xnn
    from xview2_amd.optim import FlatAdamW
    from xview2_amd.weights import deterministic_init_
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
        batches = [_batch(a, 100 * rank + k) for k in range(4)]
        res = {}
        for overlap in (True, False):
            torch.manual_seed(0)
            m = networks.UNetLoc(a)
            deterministic_init_(m, 1)
            m.cuda().train()
            opt = FlatAdamW(m.parameters(), lr=1e-3)
            red = xdist.GradReducer(opt, bucket_bytes=8 << 20, overlap=overlap)
            assert red.enabled and red.world == 2 and xnn.SYNC_BN
            for k, xy in enumerate(batches):
                closes = k % 2 == 1
                _micro(a, m, opt, xy, red, sync=closes)
                if closes:
                    opt.step(red.finish())
                else:
                    opt.accumulate()
            torch.cuda.synchronize()
            res[overlap] = opt.flat_p.cpu()
        torch.save(res, os.path.join(outdir, "acc_%d.pt" % rank))
    finally:
        xnn.SYNC_BN = False
        dist.destroy_process_group()


def test_two_ranks_end_identical_and_overlap_changes_no_bit(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0, "rank process exit code %s" % p.exitcode
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "acc_%d.pt" % r), weights_only=False) for r in range(2))
    for overlap in (True, False):
        assert torch.equal(r0[overlap], r1[overlap]) and bool(torch.isfinite(r0[overlap]).all()), overlap
    assert torch.equal(r0[True], r0[False])                  # a sum of two addends has one order


def test_a_loader_that_ends_before_its_len_cannot_leave_a_group_open(tmp_path):
    import main as cli
    from xview2_amd.lightning import Model
    from xview2_amd.trainer import Trainer
    args = cli.build_parser().parse_args(["--encoder", "resnet50", "--type", "pre", "--loss_str", "ce", "--precision", "32",
                                          "--epochs", "1", "--results", str(tmp_path)])
    a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
    x, y = _batch(a, 0)

    class Short(list):
        def __len__(self):
            return 4                                         # ... and three batches come: the third opens a group nobody closes

        def train_dataloader(self):
            return self

    trainer = Trainer(gpus=1, precision=32, max_epochs=1, checkpoint_callback=False, default_root_dir=str(tmp_path),
                      accumulate_grad_batches=2)
    trainer.validate = lambda model, dm: None
    try:
        with pytest.raises(RuntimeError, match="1 micro-batches of an open accumulation group"):
            trainer.fit(Model(args), Short([{"image": x, "mask": y}] * 3))
    finally:
        gc.unfreeze()                                        # (fit froze the collector after its first step and did not return)
    assert trainer.global_step == 1


# ---------------------------------------------------------------------------------------------------------------
# 7. one synthetic CLI epoch
def test_one_synthetic_cli_epoch_takes_three_optimizer_steps_for_five_batches(tmp_path):
    import main as cli
    from xview2_amd.utils.scheduler import NoamLR
    argv = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2", "--val_batch_size", "2",
            "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "5", "--exec_mode", "train", "--type", "pre",
            "--loss_str", "dice", "--epochs", "1", "--use_scheduler", "--warmup", "1", "--final_lr", "1e-5"]
    args = cli.build_parser().parse_args(argv)

    class Opt:
        def __init__(self):
            self.param_groups = [{"lr": 1.0}]

    def schedule_after(steps_per_epoch, steps):
        o = Opt()
        s = NoamLR(o, warmup_epochs=args.warmup, total_epochs=args.epochs, steps_per_epoch=steps_per_epoch, init_lr=args.init_lr,
                   max_lr=args.lr, final_lr=args.final_lr)
        for _ in range(steps):
            s.step()
        return o.param_groups[0]["lr"]

    assert schedule_after(3, 3) != schedule_after(5, 3)
    for extra, steps in ((["--accumulate_grad_batches", "2"], 3), ([], 5)):
        root = os.path.join(str(tmp_path), "k%d" % steps)
        cli.main(argv + extra + ["--results", root])
        blob = torch.load(os.path.join(root, "checkpoints", "last.ckpt"), map_location="cpu", weights_only=False)
        assert blob["global_step"] == steps
        assert blob["optimizer_states"][0]["step"] == steps
        # the schedule stands where `steps` steps of a `steps`-step epoch put it
        assert blob["optimizer_states"][0]["lr"] == schedule_after(steps, steps)
        assert all(bool(torch.isfinite(v).all()) for v in blob["state_dict"].values() if v.is_floating_point())
