"""Every --optimizer choice is a flat fused optimizer (xview2_amd.optim), and the float64 restatement of the eight rules
(tests/optim_ref.py) agrees with torch's own implementations where torch has one.  No GPU needed."""
import ctypes

import pytest
import torch

from tests import optim_ref

CLASSES = {"sgd": "FlatSGD", "adam": "FlatAdamW", "adamw": "FlatAdamW", "radam": "FlatRAdam",
           "adabelief": "FlatAdaBelief", "adabound": "FlatAdaBound", "adamp": "FlatAdamP", "novograd": "FlatNovoGrad"}


@pytest.mark.parametrize("name", optim_ref.RULES)
def test_every_optimizer_choice_configures_a_flat_optimizer(tmp_path, name):
    import main as cli
    from xview2_amd.lightning import OPTIMIZERS, Model
    from xview2_amd.optim import FlatOptimizer
    assert name in OPTIMIZERS
    args = cli.build_parser().parse_args(["--optimizer", name, "--encoder", "resnet50", "--type", "pre",
                                          "--results", str(tmp_path), "--weight_decay", "1e-2"])
    model = Model(args)
    opt = model.configure_optimizers()
    assert isinstance(opt, FlatOptimizer), type(opt)
    assert type(opt).__name__ == CLASSES[name]
    n = sum(p.numel() for p in model.parameters() if p.requires_grad)
    assert sum(p.numel() for p in opt.params) == n and opt.total >= n
    assert all(getattr(opt, s).shape == opt.flat_p.shape for s in opt.STATE)
    sd = opt.state_dict()
    assert sd["step"] == 0 and sd["lr"] == args.lr and all(s in sd for s in opt.STATE)


def test_make_flat_optimizer_maps_every_name_to_its_rule():
    from xview2_amd import optim
    lin = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Linear(8, 4))
    for name, cls in CLASSES.items():
        opt = optim.make_flat_optimizer(name, lin.parameters(), lr=1e-3, weight_decay=1e-2, momentum=0.9)
        assert type(opt) is getattr(optim, cls), name
        assert isinstance(opt, optim.FlatOptimizer)
    # adam is the AdamW rule (apex FusedAdam's default adam_w_mode): same class, same hyperparameters
    a = optim.make_flat_optimizer("adam", lin.parameters(), lr=1e-3, weight_decay=1e-2)
    w = optim.make_flat_optimizer("adamw", lin.parameters(), lr=1e-3, weight_decay=1e-2)
    assert (a.betas, a.eps, a.weight_decay) == (w.betas, w.eps, w.weight_decay) == ((0.9, 0.999), 1e-8, 1e-2)
    # sgd ignores --weight_decay (the reference passes none to FusedSGD); momentum 0 keeps no buffer
    s = optim.make_flat_optimizer("sgd", lin.parameters(), lr=1e-3, weight_decay=1e-2, momentum=0.9)
    assert s.weight_decay == 0.0 and s.STATE == ("momentum_buffer",)
    assert optim.make_flat_optimizer("sgd", lin.parameters(), lr=1e-3, momentum=0.0).STATE == ()
    b = optim.make_flat_optimizer("adabound", lin.parameters(), lr=2e-3)
    assert b.state_dict()["base_lr"] == 2e-3
    ng = optim.make_flat_optimizer("novograd", lin.parameters(), lr=1e-3)
    assert ng.state_dict()["exp_avg_norm"].shape == (len(ng.params),)
    with pytest.raises(ValueError):
        optim.make_flat_optimizer("lamb", lin.parameters(), lr=1e-3)


def test_segment_table_rows_cover_every_tensor_once():
    from xview2_amd import optim
    shapes = [(64, 32, 3, 3), (256, 64, 1, 1), (5, 64), (64,), (7,), (2, 70000)]
    ps = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    opt = optim.FlatAdamP(ps, lr=1e-3)
    rows, tens = opt.rows.tolist(), opt.tensors.tolist()
    assert len(tens) == len(shapes) and len(rows) == 64 + 256 + 5 + 1 + 1 + 2
    for i, (s, (r0, nr, numel, multi)) in enumerate(zip(shapes, tens)):
        assert nr == (s[0] if len(s) >= 2 else 1) and numel == torch.Size(s).numel() and multi == int(len(s) >= 2)
        mine = rows[r0:r0 + nr]
        assert all(t == i for _, _, t in mine)
        assert mine[0][0] == opt.offsets[i] and sum(ln for _, ln, _ in mine) == numel
        assert all(b[0] == a[0] + a[1] for a, b in zip(mine, mine[1:]))
    assert opt.partials.shape == (len(rows), 4) and opt.decision.shape == (len(shapes),)


def _torch_twin(name, params, lr):
    if name == "sgd0":
        return torch.optim.SGD(params, lr=lr, momentum=0.0)
    if name == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9)
    if name in ("adam", "adamw"):
        return torch.optim.AdamW(params, lr=lr, weight_decay=1e-2)
    return torch.optim.RAdam(params, lr=lr, weight_decay=1e-2, decoupled_weight_decay=True)


@pytest.mark.parametrize("name", ["sgd", "sgd0", "adam", "adamw", "radam"])
def test_restatement_matches_torch_twin_in_float64(name):
    gen = torch.Generator().manual_seed(3)
    shapes = [(16, 8, 3, 3), (16,), (5, 7)]
    init = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    grads = [[torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes] for _ in range(20)]
    lrs = [1e-2 * (1 + 0.3 * ((i * 7) % 5)) for i in range(20)]
    tp = [torch.nn.Parameter(x.clone()) for x in init]
    topt = _torch_twin(name, tp, lrs[0])
    mine, st = [x.clone() for x in init], {}
    rule, mom = ("sgd", 0.9 if name == "sgd" else 0.0) if name.startswith("sgd") else (name, 0.0)
    for t in range(1, 21):
        for g in topt.param_groups:
            g["lr"] = lrs[t - 1]
        for p, g in zip(tp, grads[t - 1]):
            p.grad = g.clone()
        topt.step()
        optim_ref.step(rule, mine, grads[t - 1], st, lrs[t - 1], t, wd=0.0 if rule == "sgd" else 1e-2, momentum=mom)
    for a, b in zip(mine, tp):
        rel = float((a - b.detach()).abs().max()) / float(b.detach().abs().max())
        assert rel <= 1e-12, (name, rel)


def test_adamp_restatement_picks_the_channel_then_the_layer_view():
    gen = torch.Generator().manual_seed(5)
    p = torch.randn(8, 32, dtype=torch.float64, generator=gen)
    # g orthogonal to every row of p: the channel view fires
    g = torch.randn(8, 32, dtype=torch.float64, generator=gen)
    g_orth = g - (g * p).sum(1, keepdim=True) / (p * p).sum(1, keepdim=True) * p
    assert optim_ref.adamp_view(p, g_orth) == 1
    # rows of equal norm, g at cos +-0.5 alternating: every row fails the channel test, the rows cancel in the layer view
    pe = p / p.norm(dim=1, keepdim=True)
    o = g_orth / g_orth.norm(dim=1, keepdim=True)
    sign = torch.tensor([1.0, -1.0] * 4, dtype=torch.float64)[:, None]
    g_layer = o + sign * pe / 3 ** 0.5
    cos = torch.nn.functional.cosine_similarity(g_layer, pe, dim=1)
    assert float(cos.abs().min()) > 0.49 and abs(float((g_layer * pe).sum())) < 1e-12
    assert optim_ref.adamp_view(pe, g_layer) == 2
    # g proportional to p: neither view fires; 1-d tensors never project
    assert optim_ref.adamp_view(p, 0.3 * p) == 0
    assert optim_ref.adamp_view(p[0], g_orth[0]) == 0
    # the projection removes the radial part of the step and decays by wd_ratio
    ps, st = [p.clone()], {}
    dec = optim_ref.adamp(ps, [g_orth], st, 1e-2, 1, 0.0)
    assert dec == [1]
    step = (ps[0] - p)
    assert float((step * p).sum(1).abs().max()) < 1e-3 * float(step.norm()) * float(p.norm())


def test_optimizer_prototypes_parse_and_are_declared():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    declared = _lib.declared_symbols()
    P, I, I64, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    want = {       # (betas by value as double, the other hyperparameters as float, lr and step by device pointer)
        "xv2_flat_step_dev": [I, P, P, P, P, I64, P, P, D, D] + [F] * 7 + [P],
        "xv2_adamp_step_dev": [P, I64, P, I] + [P] * 9 + [D, D] + [F] * 5 + [P],
        "xv2_novograd_step_dev": [P, I64, P, I] + [P] * 7 + [D, D] + [F] * 3 + [P],
    }
    for name, argt in want.items():
        assert name in declared
        rt, got = protos[name]
        assert rt is ctypes.c_int and got == argt, name
    # the AdamW entry point the default path uses is untouched
    assert protos["xv2_adamw_step_dev"][1] == [P, P, P, P, I64, P, F, F, F, F, P, F, P]
