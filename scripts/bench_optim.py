"""Time one step of every --optimizer rule (xview2_amd.optim) on the real parameter shapes of cfg2 (UNetLoc, resnet50) and
cfg5 (fused damage U-Net, resnest200 --attention --ppm --deep_supervision): device events around the rule's launches
(the step-counter increment included, the packed-weight refresh every rule shares excluded), after warm-up.  Prints ms,
the ratio to AdamW and the effective GB/s of the bytes each implementation moves (fp32 arrays: AdamW / radam /
adabelief / adabound read p, g and two moments and write three arrays back; adamp re-reads p, m and v in its apply pass;
novograd reads g once for the norms, then p, g, m).
--guard times every rule twice in the same run, without and with the gradient guard (FlatOptimizer.set_guard: the norm pass
over g, its one-block fold and the guarded kernels), and prints the difference.
usage: python scripts/bench_optim.py [--configs cfg2,cfg5] [--steps 100] [--warmup 10] [--guard]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RULES = [("adamw", 0.0), ("sgd", 0.9), ("sgd", 0.0), ("radam", 0.0), ("adabelief", 0.0), ("adabound", 0.0),
         ("adamp", 0.0), ("novograd", 0.0)]
ARRAYS_MOVED = {"adamw": 7, "sgd0.9": 5, "sgd0.0": 3, "radam": 7, "adabelief": 7, "adabound": 7, "adamp": 10, "novograd": 6}


def shapes(cfg):
    from bench import make_args
    from xview2_amd import networks
    if cfg == "cfg2":
        m = networks.UNetLoc(make_args("resnet50", "pre", "dice"))
    else:
        m = networks.get_dmg_unet(make_args("resnest200", "post", "focal+dice", "fused", attention=True, ppm=True,
                                            deep_supervision=True))
    seen, out = set(), []
    for p in m.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            out.append(tuple(p.shape))
    return out


def time_rule(name, momentum, shp, steps, warmup, guard=False):
    from xview2_amd import optim
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter(0.05 * torch.randn(s, device="cuda", generator=gen)) for s in shp]
    opt = optim.make_flat_optimizer(name, params, lr=3e-4, weight_decay=1e-2, momentum=momentum)
    opt.flat_g.copy_(1e-3 * torch.randn(opt.total, device="cuda", generator=gen))
    if guard:
        opt.set_guard(max_norm=1.0, skip_nonfinite=True)       # (the norm of this gradient is >= 5: every step clips)
    if name == "adamw":
        from xview2_amd._capi import call

        def launch():
            opt._guard_pass(1.0)
            call("xv2_adamw_step_dev", opt.flat_p, opt.flat_g, opt.exp_avg, opt.exp_avg_sq, opt.flat_p.numel(),
                 opt.lr_dev, 0.9, 0.999, 1e-8, 1e-2, opt.step_dev, 1.0)
    else:
        def launch():
            opt._guard_pass(1.0)
            opt._launch(1.0)
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(opt.flat_p).all()
    if guard:
        st = opt.guard_stats()
        assert st["steps"] == st["clipped"] == steps + warmup and st["skipped"] == 0, st
    return e0.elapsed_time(e1) / steps, opt.total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg2,cfg5"], help="comma or space separated")
    ap.add_argument("--guard", action="store_true", help="time each rule with and without the gradient guard")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert a.steps >= 50
    for cfg in ",".join(a.configs).split(","):
        shp = shapes(cfg)
        res, guarded = {}, {}
        for name, mu in RULES:
            key = name + ("%.1f" % mu if name == "sgd" else "")
            res[key] = time_rule(name, mu, shp, a.steps, a.warmup)
            if a.guard:
                guarded[key] = time_rule(name, mu, shp, a.steps, a.warmup, guard=True)
        base = res["adamw"][0]
        n = res["adamw"][1]
        print("%s: %d tensors, %.1f M parameters" % (cfg, len(shp), n / 1e6))
        for key, (ms, total) in res.items():
            gbs = ARRAYS_MOVED[key] * 4 * total / (ms * 1e-3) / 1e9
            line = "  %-10s %8.3f ms  %5.2fx adamw  %7.0f GB/s" % (key, ms, ms / base, gbs)
            if a.guard:
                gms = guarded[key][0]
                line += "   guarded %8.3f ms  (+%.1f us, %.2fx)" % (gms, (gms - ms) * 1e3, gms / ms)
            print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
