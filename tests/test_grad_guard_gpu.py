"""The gradient guard on the GPU (csrc/optim.hip xv2_grad_guard, the guarded instantiations of every optimizer kernel,
FlatOptimizer.set_guard, Trainer(gradient_clip_val, skip_nonfinite)) against the float64 restatements
(tests/guard_ref.py, tests/optim_ref.py) and against unguarded twins."""
import json
import math
import os
import socket

import pytest
import torch

from tests import guard_ref
from tests import test_optimizers_gpu as og

pytestmark = pytest.mark.gpu

CASES, SHAPES, KINDS = og.CASES, og.SHAPES, og.KINDS
SMALL, LARGE = SHAPES.index((7,)), SHAPES.index((2, 70000))


# ---------------------------------------------------------------------------------------------------------------
# 1. the entry point
def _record(rec):
    rec = rec.cpu()
    f, i = rec.view(torch.float32), rec.view(torch.int32)
    return {"norm": float(f[0]), "coef": float(f[1]), "skip": int(i[2]), "row": int(i[3]), "steps": int(rec[2]),
            "clipped": int(rec[3]), "skipped": int(rec[4]), "norm_max": float(f[10])}


def _guard_call(g, grad_scale, max_norm, skip, rec=None):
    from xview2_amd._capi import call, query
    ws = torch.zeros(query("xv2_grad_guard_workspace", g.numel()) // 8, dtype=torch.float64, device="cuda")
    rec = torch.zeros(8, dtype=torch.int64, device="cuda") if rec is None else rec
    call("xv2_grad_guard", g, g.numel(), grad_scale, max_norm, int(skip), ws, rec)
    torch.cuda.synchronize()
    return rec


_BUF = {}


def _buffer():
    """one random buffer (and its CPU copy) for every entry-point test"""
    if not _BUF:
        gen = torch.Generator().manual_seed(21)
        host = torch.randn(262147 + 5, generator=gen, dtype=torch.float32) * 3e-2
        _BUF.update(host=host, dev=host.cuda())
    return _BUF["host"], _BUF["dev"]


@pytest.mark.parametrize("n,off", [(1, 0), (3, 0), (5, 0), (1027, 0), (262147, 0), (262147, 1)])
def test_norm_and_coef_match_the_restatement(n, off):
    host, dev = _buffer()
    g = dev[off:off + n]
    assert (g.data_ptr() % 16 != 0) == (off == 1)           # the offset slice takes the scalar path
    norm, _, _ = guard_ref.guard([host[off:off + n]], 0.5)
    for max_norm in (0.5 * norm, 2.0 * norm, 0.0):
        want = guard_ref.guard([host[off:off + n]], 0.5, max_norm)
        got = _record(_guard_call(g, 0.5, max_norm, False))
        print("n=%d off=%d max_norm=%.6g: norm %.9g (ref %.9g) coef %.9g (ref %.9g)" % (n, off, max_norm, got["norm"], want[0],
                                                                                       got["coef"], want[1]))
        assert abs(got["norm"] - want[0]) <= 1e-6 * want[0]
        assert abs(got["coef"] - want[1]) <= 1e-6 * want[1]
        assert (got["coef"] < 1.0) == (max_norm == 0.5 * norm) and (max_norm == 0.5 * norm or got["coef"] == 1.0)
        assert (got["skip"], got["steps"], got["clipped"], got["skipped"]) == (0, 1, int(got["coef"] < 1.0), 0)
        assert got["norm_max"] == got["norm"]


def test_two_runs_give_bit_identical_records_and_the_counters_accumulate():
    _, dev = _buffer()
    a, b = _guard_call(dev[:262147], 1.0, 0.3, True), _guard_call(dev[:262147], 1.0, 0.3, True)
    assert torch.equal(a, b)
    # a non-finite element: skip only when asked to, torch's coefficient otherwise; the record keeps the finite maximum
    bad = dev[:1027].clone()
    first = _record(_guard_call(bad, 1.0, 0.3, True))
    for value, coef_is in ((float("inf"), lambda c: c == 0.0), (float("nan"), math.isnan)):
        bad[1000] = value
        rec = _guard_call(bad, 1.0, 0.3, True)
        r = _record(rec)
        assert (r["skip"], r["skipped"], r["row"], r["clipped"]) == (1, 1, 1, 0) and not math.isfinite(r["norm"])
        r = _record(_guard_call(bad, 1.0, 0.3, True, rec))
        assert (r["skip"], r["skipped"], r["row"], r["steps"]) == (1, 2, 2, 2)
        r = _record(_guard_call(dev[:1027], 1.0, 0.3, True, rec))
        assert (r["skip"], r["skipped"], r["row"], r["steps"], r["clipped"]) == (0, 2, 0, 3, 1)
        assert r["norm_max"] == r["norm"] == first["norm"]
        r = _record(_guard_call(bad, 1.0, 0.3, False))
        assert r["skip"] == 0 and r["skipped"] == 0 and coef_is(r["coef"]) and r["norm_max"] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# 2. every rule honours the guard, on the ragged shape set
def _init():
    gen = torch.Generator().manual_seed(11)
    init = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    init[1] = init[1] / init[1].reshape(256, -1).norm(dim=1).reshape(256, 1, 1, 1)    # layer-view rows of equal norm
    return init, gen


def _make(name, momentum, init, lr=1e-3, wd=1e-2):
    from xview2_amd.optim import make_flat_optimizer
    params = [torch.nn.Parameter(x.float().cuda()) for x in init]
    return make_flat_optimizer(name, params, lr=lr, weight_decay=wd, momentum=momentum), params


def _feed(opt, gs):
    opt.zero_grad()
    for g, v in zip(gs, og._views(opt, opt.flat_g)):
        v.copy_(g.float())


def _everything(opt):
    """every array a step may write"""
    out = {"p": opt.flat_p.clone(), "step": opt.step_dev.clone()}
    out.update((s, getattr(opt, s).clone()) for s in opt.STATE)
    for extra in ("decision", "exp_avg_norm", "aux"):
        if hasattr(opt, extra):
            out[extra] = getattr(opt, extra).clone()
    return out


def _same(a, b):
    # (bit for bit; NaN-free by construction wherever this is called)
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _fresh_grads(params, gen):
    cur = [p.detach().double().cpu() for p in params]
    gs = [og._grad(p, k, gen) for p, k in zip(cur, KINDS)]
    assert og._margins_ok(cur, gs)
    return gs


@pytest.mark.parametrize("name,momentum", CASES)
def test_a_guard_that_does_not_clip_costs_nothing_numerically(name, momentum):
    init, gen = _init()
    opt, params = _make(name, momentum, init)
    twin, _ = _make(name, momentum, init)
    opt.set_guard(max_norm=1e9)
    for _ in range(3):
        gs = _fresh_grads(params, gen)
        for o in (opt, twin):
            _feed(o, gs)
            o.step(0.5)
        st = opt.guard_stats()
        assert st["coef"] == 1.0 and st["skip"] == 0
        assert _same(_everything(opt), _everything(twin))
    assert opt.guard_stats()["clipped"] == 0 and opt.guard_stats()["steps"] == 3 and int(opt.step_dev.item()) == 3


@pytest.mark.parametrize("name,momentum", CASES)
def test_clipped_steps_match_the_restatement_on_clipped_gradients(name, momentum):
    init, gen = _init()
    lr0, wd, gscale, max_norm = 1e-3, 1e-2, 0.5, 0.25
    opt, params = _make(name, momentum, init, lr0, wd)
    opt.set_guard(max_norm=max_norm)
    ref_p, st = [x.float().double() for x in init], {}
    for t in range(1, 4):
        gs = _fresh_grads(params, gen)
        _feed(opt, gs)
        opt.step(gscale)
        torch.cuda.synchronize()
        g32 = [g.float() for g in gs]
        norm, coef, _ = guard_ref.guard(g32, gscale, max_norm)
        assert norm > 4 * max_norm                           # (well below the actual norm)
        got = opt.guard_stats()
        assert abs(got["norm"] - norm) <= 1e-6 * norm and abs(got["coef"] - coef) <= 1e-6 * coef
        dec = og._ref_step(name, ref_p, [gscale * g for g in guard_ref.clipped(g32, coef)], st, lr0, t, wd, momentum, lr0)
        flat = torch.cat([v.detach().double().cpu().flatten() for v in og._views(opt, opt.flat_p)])
        rel = og._rel(flat, torch.cat([x.flatten() for x in ref_p]))
        print(name, momentum, "step", t, "parameters rel", rel)
        assert rel <= 2e-6, (name, t, rel)
        og._compare_state(opt, name, st, 2e-6, (name, t))
        if name == "adamp":
            assert opt.decision.cpu().tolist() == dec
    st = opt.guard_stats()
    assert st["clipped"] == st["steps"] == 3 and st["skipped"] == 0 and int(opt.step_dev.item()) == 3


@pytest.mark.parametrize("name,momentum", CASES)
def test_a_non_finite_gradient_skips_the_step_bit_for_bit(name, momentum):
    init, gen = _init()
    opt, params = _make(name, momentum, init)
    twin, _ = _make(name, momentum, init)                    # never sees a bad step, carries no guard
    opt.set_guard(skip_nonfinite=True)
    skipped = 0

    def both(gs):
        for o in (opt, twin):
            _feed(o, gs)
            o.step(0.5)
        assert _same(_everything(opt), _everything(twin))

    both(_fresh_grads(params, gen))
    for bad in (float("nan"), float("inf")):
        for tensor in (SMALL, LARGE):
            before = _everything(opt)
            gs = _fresh_grads(params, gen)
            gs[tensor].view(-1)[gs[tensor].numel() // 2] = bad
            _feed(opt, gs)
            opt.step(0.5)
            skipped += 1
            st = opt.guard_stats()
            assert (st["skip"], st["skipped"], st["skipped_in_a_row"]) == (1, skipped, 1) and not math.isfinite(st["norm"])
            assert _same(_everything(opt), before), (name, bad, tensor)
            both(_fresh_grads(params, gen))                  # the next finite step: as if the bad one never came
            assert opt.guard_stats()["skipped_in_a_row"] == 0
    assert int(opt.step_dev.item()) == int(twin.step_dev.item()) == 5 and opt.step_count == 9
    # without skip_nonfinite: torch's behaviour - the update goes through and the parameters are no longer finite
    for bad, tensor in ((float("nan"), SMALL), (float("inf"), LARGE)):
        loud, lp = _make(name, momentum, init)
        loud.set_guard(max_norm=1e9, skip_nonfinite=False)
        gs = _fresh_grads(lp, gen)
        gs[tensor].view(-1)[0] = bad
        _feed(loud, gs)
        loud.step(0.5)
        assert not bool(torch.isfinite(loud.flat_p).all()) and int(loud.step_dev.item()) == 1
        assert loud.guard_stats()["skipped"] == 0


# ---------------------------------------------------------------------------------------------------------------
# 3. state_dict() after a skipped step
@pytest.mark.parametrize("name", ["adamw", "novograd"])
def test_state_dict_after_a_skipped_step_resumes_the_finite_run_bit_for_bit(name):
    init, gen = _init()
    opt, params = _make(name, 0.0, init)
    whole, _ = _make(name, 0.0, init)                        # the uninterrupted finite run
    opt.set_guard(skip_nonfinite=True)
    g1 = _fresh_grads(params, gen)
    for o in (opt, whole):
        _feed(o, g1)
        o.step()
    bad = _fresh_grads(params, gen)
    bad[SMALL][0] = float("nan")
    _feed(opt, bad)
    opt.step()
    sd = opt.state_dict()
    assert opt.step_count == 2 and sd["step"] == int(opt.step_dev.item()) == 1
    assert whole.state_dict()["step"] == 1                   # (without a guard: the host's count, as before)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    resumed, _ = _make(name, 0.0, [v.detach().double().cpu() for v in og._views(opt, opt.flat_p)])
    resumed.load_state_dict(sd)
    g2 = _fresh_grads(params, gen)
    for o in (resumed, whole):
        _feed(o, g2)
        o.step()
    assert _same(_everything(resumed), _everything(whole))
    assert int(resumed.step_dev.item()) == 2


# ---------------------------------------------------------------------------------------------------------------
# 4. model level
def test_a_guarded_model_step_equals_the_twin_stepped_with_the_coefficient():
    from xview2_amd import ops
    from xview2_amd.optim import make_flat_optimizer
    a, m = og._model("resnet50")
    _, m2 = og._model("resnet50")
    opt = make_flat_optimizer("adamw", m.parameters(), lr=1e-3, weight_decay=1e-2)
    twin = make_flat_optimizer("adamw", m2.parameters(), lr=1e-3, weight_decay=1e-2)
    assert torch.equal(opt.flat_p, twin.flat_p)
    loss = og._backward(a, m, opt, batch=2)
    assert torch.isfinite(loss)
    ops.join_wgrad_stream()
    opt._gather_foreign_grads()
    norm, _, _ = guard_ref.guard([opt.flat_g.cpu()])
    opt.set_guard(max_norm=0.5 * norm)
    opt.step()
    st = opt.guard_stats()
    want = guard_ref.guard([opt.flat_g.cpu()], 1.0, 0.5 * norm)
    print("model norm %.9g (ref %.9g) coef %.9g (ref %.9g)" % (st["norm"], want[0], st["coef"], want[1]))
    assert abs(st["norm"] - norm) <= 1e-6 * norm and abs(st["coef"] - want[1]) <= 1e-6 * want[1] and st["clipped"] == 1
    twin.zero_grad()
    twin.flat_g.copy_(opt.flat_g)
    twin.step(grad_scale=st["coef"])
    torch.cuda.synchronize()
    for got, ref in [(opt.flat_p, twin.flat_p)] + [(getattr(opt, s), getattr(twin, s)) for s in opt.STATE]:
        assert og._rel(got.cpu(), ref.cpu()) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------
# 5. hipGraph replay, one replayed step with a NaN in the gradient
def test_hipgraph_replay_of_a_guarded_step_matches_eager_steps():
    from tests.golden.cases import ARGS, labels, model_input
    from xview2_amd import criterion, networks, ops
    from xview2_amd.graph import GraphedStep
    from xview2_amd.optim import make_flat_optimizer
    from xview2_amd.weights import deterministic_init_
    a = ARGS(encoder="resnet50", deep_supervision=True)
    x, y = model_input(a).cuda(), labels(a).cuda()
    lrs = [1e-3, 1e-3, 7e-4, 1.3e-3, 4e-4]           # (the two warm-up steps of the graphed run share one rate)
    poisons = [0.0, 0.0, 0.0, float("nan"), 0.0]     # added to one gradient element: step 4, a replayed one, is bad
    res = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        m = networks.UNetLoc(a)
        deterministic_init_(m, 1)
        m.cuda().train()
        opt = make_flat_optimizer("adamw", m.parameters(), lr=lrs[0], weight_decay=1e-2)
        opt.set_guard(max_norm=0.05, skip_nonfinite=True)
        lf = criterion.Loss(a)
        poison = torch.zeros(1, device="cuda")
        k = opt.offsets[0] + 5

        def step():
            opt.zero_grad()
            loss = criterion.compute_loss(lf, m(x), y, True)
            loss.backward()
            ops.join_wgrad_stream()                  # (the weight gradients are complete before one is poisoned)
            opt.flat_g[k:k + 1].add_(poison)
            opt.step()
            return loss
        snaps = []
        if mode == "eager":
            for lr, bad in zip(lrs, poisons):
                opt.param_groups[0]["lr"] = lr
                poison.fill_(bad)
                step()
                snaps.append(opt.flat_p.clone())
        else:
            g = GraphedStep(step, opt, [], warmup=2)
            snaps = [None, None]
            for lr, bad in zip(lrs[2:], poisons[2:]):
                opt.param_groups[0]["lr"] = lr
                poison.fill_(bad)
                g()
                snaps.append(opt.flat_p.clone())
        torch.cuda.synchronize()
        res[mode] = (snaps, [getattr(opt, s).clone() for s in opt.STATE], int(opt.step_dev.item()), opt.guard_stats())
    e, g = res["eager"], res["graph"]
    assert all(torch.equal(u, v) for u, v in zip(e[0][2:], g[0][2:]))
    assert torch.equal(e[0][3], e[0][2]) and not torch.equal(e[0][4], e[0][3])      # the bad step moved nothing
    assert all(torch.equal(u, v) for u, v in zip(e[1], g[1]))
    assert e[2] == g[2] == 4
    assert e[3]["skipped"] == g[3]["skipped"] == 1 and e[3]["steps"] == g[3]["steps"] == 5
    assert {k: v for k, v in e[3].items()} == {k: v for k, v in g[3].items()}
    assert bool(torch.isfinite(e[0][4]).all())


# ---------------------------------------------------------------------------------------------------------------
# 6. the trainer: a dead epoch says so; two ranks; the CLI
def test_an_epoch_of_skipped_steps_raises(tmp_path):
    from types import SimpleNamespace
    from xview2_amd.trainer import Trainer
    t = Trainer(gpus=1, precision=32, default_root_dir=str(tmp_path), skip_nonfinite=True)
    stats = {"norm": float("nan"), "coef": 1.0, "skip": 1, "skipped_in_a_row": 3, "steps": 3, "clipped": 0, "skipped": 3,
             "norm_max": 0.0}
    model, seen = SimpleNamespace(), {"steps": 0, "clipped": 0, "skipped": 0}
    with pytest.raises(RuntimeError, match="3 of 3"):
        t._report_guard(model, SimpleNamespace(guard_stats=lambda: dict(stats)), 0, seen)
    stats.update(steps=6, skipped=5, clipped=1, norm_max=2.5)
    t._report_guard(model, SimpleNamespace(guard_stats=lambda: dict(stats)), 1, seen)         # one step of three trained
    assert model.epoch_extras == {"grad_norm_max": 2.5, "clipped_steps": 1, "skipped_steps": 2}


def _guarded_fit_worker(rank, world, port, outdir):
    """one of two ranks sharing cuda:0, as tests/test_optimizers_gpu.py::_fit_worker: one guarded trainer step"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    os.environ.setdefault("XV2_SYNCBN", "rccl")
    import torch.distributed as dist
    import main as cli
    from tests.golden.cases import ARGS, labels, model_input
    from xview2_amd import nn as xnn
    from xview2_amd.lightning import Model
    from xview2_amd.trainer import Trainer
    from xview2_amd.weights import deterministic_init_
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        args = cli.build_parser().parse_args(["--optimizer", "adamw", "--encoder", "resnet50", "--type", "pre",
                                              "--loss_str", "ce", "--precision", "32", "--epochs", "1", "--lr", "1e-3",
                                              "--gradient_clip_val", "1e-3", "--skip_nonfinite",
                                              "--results", os.path.join(outdir, "r%d" % rank)])
        a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
        x, y = model_input(a, batch=4), labels(a, batch=4)
        per = 4 // world
        batch = {"image": x[per * rank:per * (rank + 1)].cuda(), "mask": y[per * rank:per * (rank + 1)].cuda()}

        class OneBatch:
            def train_dataloader(self):
                return [batch]

        trainer = Trainer(gpus=1, precision=32, max_epochs=1, checkpoint_callback=False, default_root_dir=args.results,
                          gradient_clip_val=args.gradient_clip_val, skip_nonfinite=args.skip_nonfinite)
        assert trainer.world == world
        trainer.validate = lambda model, dm: None          # (this test is about the training step)
        model = Model(args)
        deterministic_init_(model.model, 1)
        trainer.fit(model, OneBatch())
        after = torch.cat([p.detach().cpu().flatten() for p in model.parameters()])
        torch.save((after, trainer.guard_log), os.path.join(outdir, "fit_%d.pt" % rank))
    finally:
        xnn.SYNC_BN = False
        dist.destroy_process_group()


def test_two_ranks_take_the_same_decision_and_end_identical(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_guarded_fit_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0, "rank process exit code %s" % p.exitcode
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "fit_%d.pt" % r), weights_only=False) for r in range(2))
    assert torch.equal(r0[0], r1[0]) and bool(torch.isfinite(r0[0]).all())
    assert r0[1] == r1[1] and len(r0[1]) == 1
    log = r0[1][0]
    assert (log["steps"], log["clipped_steps"], log["skipped_steps"]) == (1, 1, 0) and log["grad_norm_max"] > 1e-3
    assert log["total"]["coef"] < 1.0


def test_one_synthetic_cli_epoch_with_both_flags_writes_the_guard_keys(tmp_path):
    import main as cli
    argv = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
            "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "2",
            "--exec_mode", "train", "--type", "pre", "--loss_str", "dice", "--epochs", "1", "--optimizer", "adamw",
            "--gradient_clip_val", "0.5", "--skip_nonfinite", "--results", str(tmp_path)]
    trained = cli.main(argv)
    assert math.isfinite(float(trained.logged["val_loss"]))
    lines = [ln for ln in open(os.path.join(str(tmp_path), "logs.json")) if ln.startswith("DLLL ")]
    data = json.loads(lines[-1][5:])["data"]
    assert {"grad_norm_max", "clipped_steps", "skipped_steps"} <= set(data) and {"f1", "val_loss", "top_f1"} <= set(data)
    assert data["skipped_steps"] == 0 and 0 <= data["clipped_steps"] <= 2 and data["grad_norm_max"] > 0.0
