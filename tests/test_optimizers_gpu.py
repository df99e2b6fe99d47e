"""The flat fused HIP optimizers of every --optimizer choice (xview2_amd.optim, csrc/optim.hip) against the float64
restatement (tests/optim_ref.py), and through the training surfaces: hipGraph replay, checkpoint resume, data parallel
ranks and the CLI."""
import math
import os
import shutil
import socket

import pytest
import torch

from tests import optim_ref

pytestmark = pytest.mark.gpu

# flat state arrays of each flat optimizer, by the restatement's state names
FLAT_STATE = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"),
              "radam": ("exp_avg", "exp_avg_sq"), "adabelief": ("exp_avg", "exp_avg_var"),
              "adabound": ("exp_avg", "exp_avg_sq"), "adamp": ("exp_avg", "exp_avg_sq"), "novograd": ("exp_avg",)}
CASES = [("sgd", 0.9), ("sgd", 0.0)] + [(n, 0.0) for n in optim_ref.RULES if n != "sgd"]
# the AdamW kernel (the default path, unchanged) takes its betas as fp32 and forms 1 - beta in fp32; its restatement
# gets the betas as that kernel sees them (1 - 0.999f is 1.3e-5 away from 0.001)
F32_BETAS = (float(torch.tensor(0.9, dtype=torch.float32)), float(torch.tensor(0.999, dtype=torch.float32)))


def _ref_step(name, ps, gs, st, lr, t, wd, momentum, base_lr):
    if name in ("adam", "adamw"):
        return optim_ref.adamw(ps, gs, st, lr, t, wd, betas=F32_BETAS)
    return optim_ref.step(name, ps, gs, st, lr, t, wd=wd, momentum=momentum, base_lr=base_lr)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def _views(opt, flat):
    return [flat[o:o + p.numel()].view(p.shape) for p, o in zip(opt.params, opt.offsets)]


def _ref_state(opt, name):
    """the flat optimizer's state as the restatement's per-tensor lists (float64, CPU)"""
    st = {k: [v.detach().double().cpu().clone() for v in _views(opt, getattr(opt, k))]
          for k in FLAT_STATE[name] if k in opt.STATE}
    if name == "novograd":
        st["exp_avg_norm"] = [x.clone() for x in opt.exp_avg_norm.detach().double().cpu().unbind(0)]
    return st


def _compare_state(opt, name, st, tol, what):
    for k in FLAT_STATE[name]:
        if k not in opt.STATE:
            continue
        got = torch.cat([v.detach().double().cpu().flatten() for v in _views(opt, getattr(opt, k))])
        ref = torch.cat([v.flatten() for v in st[k]])
        assert _rel(got, ref) <= tol, (what, k, _rel(got, ref))
    if name == "novograd":
        assert _rel(opt.exp_avg_norm.cpu(), torch.stack(st["exp_avg_norm"])) <= tol, (what, "exp_avg_norm")


# ---------------------------------------------------------------------------------------------------------------
# 1. kernels vs the restatement on a synthetic flat set
SHAPES = [(64, 32, 3, 3), (256, 64, 1, 1), (64, 3, 7, 7), (5, 64), (64,), (7,), (16, 16), (2, 70000)]
# how each tensor's gradient is built (AdamP's decision it should produce): rows orthogonal to p -> channel view,
# rows at |cos| ~ 0.7 cancelling over the tensor -> layer view, a large radial part -> no projection
KINDS = ["channel", "layer", "none", "none", "free", "free", "zero", "layer"]
EXPECT = {"channel": 1, "layer": 2, "none": 0, "free": 0, "zero": 1}   # (a zero gradient has cosine 0)


def _grad(p, kind, gen):
    """float64 gradient for parameter p (float64) of the given kind"""
    if kind == "zero":
        return torch.zeros_like(p)
    r = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    if kind == "free":
        return r
    rows = p.shape[0]
    pv, rv = p.reshape(rows, -1), r.reshape(rows, -1)
    o = rv - (rv * pv).sum(1, keepdim=True) / (pv * pv).sum(1, keepdim=True) * pv
    if kind == "channel":
        return o.reshape(p.shape)
    pn = pv.norm(dim=1, keepdim=True)
    if kind == "layer":
        # g_r = A o_r/|o_r| + s_r K/|p_r|^2 p_r: dot(g_r, p_r) = s_r K with alternating signs sums to zero
        A = float(pn.mean())
        K = A * float(pn.mean())
        sign = torch.tensor([1.0, -1.0] * (rows // 2), dtype=torch.float64)[:, None]
        return (A * o / o.norm(dim=1, keepdim=True) + sign * K / pn ** 2 * pv).reshape(p.shape)
    return (rv + 0.5 * rv.norm() / pv.norm() * pv).reshape(p.shape)


def _margins_ok(ps, gs):
    """no AdamP test of this data lies within 1e-3 (relative) of its threshold"""
    for p, g in zip(ps, gs):
        if p.dim() < 2:
            continue
        for rows in (p.shape[0], 1):
            pv, gv = p.reshape(rows, -1), g.reshape(rows, -1)
            thr = 0.1 / math.sqrt(pv.shape[1])
            c = float(torch.nn.functional.cosine_similarity(gv, pv, dim=1, eps=1e-8).abs().max())
            if abs(c - thr) <= 1e-3 * thr:
                return False
    return True


@pytest.mark.parametrize("name,momentum", CASES)
def test_flat_kernels_match_the_restatement(name, momentum):
    from xview2_amd.optim import make_flat_optimizer
    gen = torch.Generator().manual_seed(11)
    init = [0.1 * torch.randn(s, generator=gen, dtype=torch.float64) for s in SHAPES]
    init[1] = init[1] / init[1].reshape(256, -1).norm(dim=1).reshape(256, 1, 1, 1)    # layer-view rows of equal norm
    params = [torch.nn.Parameter(x.float().cuda()) for x in init]
    lr0, wd, gscale = 1e-3, 1e-2, 0.5
    opt = make_flat_optimizer(name, params, lr=lr0, weight_decay=wd, momentum=momentum)
    ref_p, st = [x.float().double() for x in init], {}
    seen = set()
    for t in range(1, 11):
        lr = lr0 * (1.0 + 0.25 * ((3 * t) % 4))                    # a different rate every step
        opt.param_groups[0]["lr"] = lr
        cur = [p.detach().double().cpu() for p in params]
        gs = [_grad(p, k, gen) for p, k in zip(cur, KINDS)]
        assert _margins_ok(cur, gs)
        opt.zero_grad()
        for g, v in zip(gs, _views(opt, opt.flat_g)):
            v.copy_(g.float())
        opt.step(gscale)
        torch.cuda.synchronize()
        scaled = [gscale * g.float().double() for g in gs]
        dec = _ref_step(name, ref_p, scaled, st, lr, t, wd, momentum, lr0)
        got = torch.cat([v.detach().double().cpu().flatten() for v in _views(opt, opt.flat_p)])
        assert _rel(got, torch.cat([x.flatten() for x in ref_p])) <= 2e-6, (name, t)
        _compare_state(opt, name, st, 2e-6, (name, t))
        if name == "adamp":
            assert opt.decision.cpu().tolist() == dec, (t, dec)
            assert dec == [EXPECT[k] for k in KINDS], (t, dec)
            seen.update(dec)
    assert opt.step_dev.item() == 10
    if name == "adamp":
        assert seen == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------
# 2. model level: the HIP step against the restatement on the same snapshots
def _model(encoder, seed=1):
    from tests.golden.cases import ARGS
    from xview2_amd import networks
    from xview2_amd.weights import deterministic_init_
    a = ARGS(encoder=encoder, loss_str="ce", type="pre")
    torch.manual_seed(0)
    m = networks.UNetLoc(a)
    deterministic_init_(m, seed)
    return a, m.cuda().train()


def _backward(a, m, opt, batch=2):
    from tests.golden.cases import labels, model_input
    from xview2_amd import criterion
    x, y = model_input(a, batch=batch).cuda(), labels(a, batch=batch).cuda()
    opt.zero_grad()
    loss = criterion.Loss(a)(m(x), y)
    loss.backward()
    return loss


@pytest.mark.parametrize("encoder", ["resnet50", "resnest50"])
@pytest.mark.parametrize("name,momentum", CASES)
def test_model_steps_match_the_restatement_on_snapshots(encoder, name, momentum):
    from xview2_amd import ops
    from xview2_amd.optim import make_flat_optimizer
    a, m = _model(encoder)
    lr0 = 1e-3
    opt = make_flat_optimizer(name, m.parameters(), lr=lr0, weight_decay=1e-2, momentum=momentum)
    for t in range(1, 4):
        lr = lr0 * (1.0 - 0.2 * (t - 1))
        opt.param_groups[0]["lr"] = lr
        loss = _backward(a, m, opt)
        assert torch.isfinite(loss)
        ops.join_wgrad_stream()
        opt._gather_foreign_grads()
        ps = [v.detach().double().cpu() for v in _views(opt, opt.flat_p)]
        gs = [v.detach().double().cpu() for v in _views(opt, opt.flat_g)]
        st = _ref_state(opt, name)
        opt.step()
        torch.cuda.synchronize()
        _ref_step(name, ps, gs, st, lr, t, 1e-2, momentum, lr0)
        got = torch.cat([v.detach().double().cpu().flatten() for v in _views(opt, opt.flat_p)])
        assert _rel(got, torch.cat([x.flatten() for x in ps])) <= 2e-6, (name, t)
        _compare_state(opt, name, st, 2e-6, (name, t))


# ---------------------------------------------------------------------------------------------------------------
# 3. / 4. adam is adamw; the reductions are reproducible
def _run(encoder, name, steps, wd=0.0):
    from xview2_amd.optim import make_flat_optimizer
    a, m = _model(encoder)
    opt = make_flat_optimizer(name, m.parameters(), lr=1e-3, weight_decay=wd)
    for _ in range(steps):
        _backward(a, m, opt)
        opt.step()
    torch.cuda.synchronize()
    return opt.flat_p.clone()


def test_adam_and_adamw_give_bit_identical_parameters():
    assert torch.equal(_run("resnet50", "adam", 2, wd=1e-2), _run("resnet50", "adamw", 2, wd=1e-2))


@pytest.mark.parametrize("name", ["adamp", "novograd"])
def test_segmented_rules_are_bitwise_reproducible(name):
    assert torch.equal(_run("resnest50", name, 3), _run("resnest50", name, 3))


# ---------------------------------------------------------------------------------------------------------------
# 5. hipGraph replay under a changing learning rate
@pytest.mark.parametrize("name", ["novograd", "adamp", "adabound"])
def test_hipgraph_replay_matches_eager_steps_under_a_changing_lr(name):
    from tests.golden.cases import ARGS, labels, model_input
    from xview2_amd import criterion, networks
    from xview2_amd.graph import GraphedStep
    from xview2_amd.optim import make_flat_optimizer
    from xview2_amd.weights import deterministic_init_
    a = ARGS(encoder="resnet50", deep_supervision=True)
    x, y = model_input(a).cuda(), labels(a).cuda()
    lrs = [1e-3, 1e-3, 7e-4, 1.3e-3, 4e-4]           # (the two warm-up steps of the graphed run share one rate)
    res = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        m = networks.UNetLoc(a)
        deterministic_init_(m, 1)
        m.cuda().train()
        opt = make_flat_optimizer(name, m.parameters(), lr=lrs[0], weight_decay=1e-2)
        lf = criterion.Loss(a)

        def step():
            opt.zero_grad()
            loss = criterion.compute_loss(lf, m(x), y, True)
            loss.backward()
            opt.step()
            return loss
        if mode == "eager":
            losses = []
            for lr in lrs:
                opt.param_groups[0]["lr"] = lr
                losses.append(float(step()))
        else:
            g = GraphedStep(step, opt, [], warmup=2)
            losses = [None, None]
            for lr in lrs[2:]:
                opt.param_groups[0]["lr"] = lr
                losses.append(float(g()))
        torch.cuda.synchronize()
        res[mode] = (losses, opt.flat_p.clone(), [getattr(opt, s).clone() for s in opt.STATE], int(opt.step_dev.item()))
    assert res["eager"][0][2:] == res["graph"][0][2:]
    assert torch.equal(res["eager"][1], res["graph"][1])
    assert all(torch.equal(u, v) for u, v in zip(res["eager"][2], res["graph"][2]))
    assert res["eager"][3] == res["graph"][3] == 5


# ---------------------------------------------------------------------------------------------------------------
# 6. CLI resume bit for bit
@pytest.mark.parametrize("name", ["novograd", "adabound"])
def test_resume_continues_the_uninterrupted_run_bit_for_bit(tmp_path, name):
    import main as cli
    common = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
              "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "3",
              "--exec_mode", "train", "--type", "pre", "--loss_str", "dice", "--use_scheduler", "--warmup", "1",
              "--final_lr", "1e-5", "--optimizer", name, "--weight_decay", "1e-2"]
    full = cli.main(common + ["--epochs", "2", "--results", str(tmp_path / "full")])
    cli.main(common + ["--epochs", "1", "--results", str(tmp_path / "half")])
    ck = str(tmp_path / "half.ckpt")
    shutil.copy(os.path.join(str(tmp_path / "half"), "checkpoints", "last.ckpt"), ck)
    blob = torch.load(ck, map_location="cpu", weights_only=False)
    st = blob["optimizer_states"][0]
    assert blob["global_step"] == 3 and st["step"] == 3
    assert ("exp_avg_norm" if name == "novograd" else "base_lr") in st
    resumed = cli.main(common + ["--epochs", "2", "--results", str(tmp_path / "res"), "--ckpt", ck])
    a, b = full.state_dict(), resumed.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------
# 7. two ranks through the trainer == one process with the global batch
def _fit_worker(rank, world, port, outdir, name):
    """one rank of `world` sharing cuda:0: Model.configure_optimizers + Trainer.fit for one step on this rank's share of
    a global batch of 4 (gloo carries the buckets and the SyncBatchNorm statistics)"""
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
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        args = cli.build_parser().parse_args(["--optimizer", name, "--encoder", "resnet50", "--type", "pre",
                                              "--loss_str", "ce", "--precision", "32", "--epochs", "1", "--lr", "1e-3",
                                              "--results", os.path.join(outdir, "r%d_%d" % (world, rank))])
        a = ARGS(encoder="resnet50", loss_str="ce", type="pre")
        x, y = model_input(a, batch=4), labels(a, batch=4)
        per = 4 // world
        batch = {"image": x[per * rank:per * (rank + 1)].cuda(), "mask": y[per * rank:per * (rank + 1)].cuda()}

        class OneBatch:
            def train_dataloader(self):
                return [batch]

        trainer = Trainer(gpus=1, precision=32, max_epochs=1, checkpoint_callback=False,
                          default_root_dir=args.results)
        assert trainer.world == world
        trainer.validate = lambda model, dm: None          # (this test is about the training step)
        model = Model(args)
        deterministic_init_(model.model, 1)
        before = torch.cat([p.detach().flatten() for p in model.parameters()]).clone()
        trainer.fit(model, OneBatch())
        after = torch.cat([p.detach().cpu().flatten() for p in model.parameters()])
        torch.save((before, after, bool(xnn.SYNC_BN)), os.path.join(outdir, "fit%d_%d.pt" % (world, rank)))
    finally:
        xnn.SYNC_BN = False
        if world > 1:
            dist.destroy_process_group()


def _spawn(world, outdir, name):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_fit_worker, args=(r, world, port, outdir, name)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0, "rank process exit code %s" % p.exitcode


@pytest.mark.parametrize("name", ["sgd", "adamp"])
def test_two_ranks_through_the_trainer_equal_one_process_with_the_global_batch(tmp_path, name):
    out = str(tmp_path)
    _spawn(2, out, name)
    _spawn(1, out, name)
    r0, r1 = (torch.load(os.path.join(out, "fit2_%d.pt" % r), weights_only=False) for r in range(2))
    one = torch.load(os.path.join(out, "fit1_0.pt"), weights_only=False)
    assert r0[2] and r1[2] and not one[2]                   # SyncBatchNorm on at world 2 only
    assert torch.equal(r0[0], one[0]) and torch.equal(r0[1], r1[1])     # same start, ranks end identical
    d2, d1 = (r0[1] - r0[0]).double(), (one[1] - one[0]).double()
    if name == "sgd":
        # the update is -lr * g: the all-reduced gradient of the two halves must be the global batch's
        cos = float((d2 * d1).sum() / (d2.norm() * d1.norm()))
        assert cos > 0.9999 and _rel(d2, d1) <= 1e-2, (cos, _rel(d2, d1))
    else:
        # a first Adam-type step moves each weight by ~lr * sign(g): compare the parameters (as the AdamW twin does)
        assert _rel(r0[1], one[1]) <= 2.5e-3


# ---------------------------------------------------------------------------------------------------------------
# 8. every choice trains through main.py
@pytest.mark.parametrize("name", optim_ref.RULES)
def test_every_optimizer_trains_one_synthetic_epoch_through_the_cli(tmp_path, name):
    import main as cli
    from xview2_amd.lightning import Model
    argv = ["--data", "synthetic", "--encoder", "resnet50", "--precision", "32", "--batch_size", "2",
            "--val_batch_size", "2", "--train_size", "64", "--eval_size", "64", "--steps_per_epoch", "2",
            "--exec_mode", "train", "--type", "pre", "--loss_str", "dice", "--epochs", "1", "--optimizer", name,
            "--weight_decay", "1e-2", "--results", str(tmp_path)]
    trained = cli.main(argv)
    torch.manual_seed(1)                                   # main.py seeds with --seed (1) before building the model
    start = Model(cli.build_parser().parse_args(argv))
    assert math.isfinite(float(trained.logged["val_loss"]))
    a, b = start.state_dict(), trained.state_dict()
    moved = [k for k in a if a[k].is_floating_point() and "running" not in k and not torch.equal(a[k], b[k].cpu())]
    assert all(torch.isfinite(v).all() for v in b.values() if v.is_floating_point())
    assert "model.unet.enc_l1.0.weight" in moved and len(moved) > len([k for k in a if k.endswith("weight")]) // 2
