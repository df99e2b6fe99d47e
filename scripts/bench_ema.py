"""Cost of the weight average (csrc/optim.hip xv2_ema_update_dev, optim.FlatEMA).

    python scripts/bench_ema.py [--iters 200] [--rounds 3] [--steps 10] [--no-step]

1. The launch alone on the flat parameter buffer of the benchmark's single-GPU model (--type pre --encoder resnet50), next to
   the flat AdamW launch on the same buffers: event-timed after warm-up, the two alternating `--rounds` times.  The average
   moves 12 bytes per element (read ema and param, write ema), AdamW 28 (read param, grad and two moments, write param and
   the moments); both calls include their one-thread counter increment.
2. One training step of that configuration, 2 x 1024 x 1024, fp32, without and with the average (decay 0.999) updated after
   the optimizer step: same process, same model, alternating.

Prints one JSON line at the end."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from xview2_amd import _capi, criterion, networks  # noqa: E402
from xview2_amd.optim import FlatAdamW, FlatEMA  # noqa: E402
from xview2_amd.weights import deterministic_init_  # noqa: E402

EMA_BYTES, ADAMW_BYTES = 12, 28      # per element


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def build(dev):
    a = bench.make_args()
    bench.set_precision(32)
    torch.manual_seed(0)
    model = networks.UNetLoc(a)
    deterministic_init_(model, 1)
    model.to(dev).train()
    optim = FlatAdamW(model.parameters(), lr=3e-4, weight_decay=0.0)
    return a, model, optim, FlatEMA(optim, 0.999)


def launch_cost(optim, ema, iters, rounds):
    n = optim.total
    optim.flat_g.copy_(1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(2)).to(optim.flat_g.device))
    keep = optim.flat_p.clone()

    def adamw():
        _capi.call("xv2_adamw_step_dev", optim.flat_p, optim.flat_g, optim.exp_avg, optim.exp_avg_sq, n, optim.lr_dev,
                   0.9, 0.999, 1e-8, 0.0, optim.step_dev, 1.0)

    rows = {"adamw": [], "ema": []}
    for _ in range(rounds):
        rows["adamw"].append(round(1e3 * timed(adamw, iters), 1))
        rows["ema"].append(round(1e3 * timed(ema.update, iters), 1))
    # the timed launches moved the weights, the moments and both counters: put the start back for the step legs
    optim.flat_p.copy_(keep)
    ema.ema.copy_(keep)
    ema.count_dev.zero_()
    optim.step_dev.zero_()
    optim.exp_avg.zero_()
    optim.exp_avg_sq.zero_()
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    expect = EMA_BYTES / ADAMW_BYTES * 1.25
    out = {"elements": n, "iters": iters, "us": rows, "median_us": med,
           "tbytes_per_s": {"adamw": round(ADAMW_BYTES * n / med["adamw"] / 1e6, 2),
                            "ema": round(EMA_BYTES * n / med["ema"] / 1e6, 2)},
           "ema_over_adamw": round(med["ema"] / med["adamw"], 3), "expected_at_most": round(expect, 3),
           "meets_expectation": med["ema"] <= expect * med["adamw"]}
    print("launch, us per call over %d elements: adamw %s  ema %s  (ratio %.3f, expected <= %.3f)"
          % (n, rows["adamw"], rows["ema"], out["ema_over_adamw"], expect), flush=True)
    return out


def step_cost(a, model, optim, ema, dev, steps, rounds):
    loss_fn = criterion.Loss(a)
    x, y = bench.synthetic_batch(a, 2, 1024, 1, dev)

    def step(averaged):
        optim.zero_grad()
        loss = criterion.compute_loss(loss_fn, model(x), y, a.deep_supervision)
        loss.backward()
        optim.step()
        if averaged:
            ema.update()
        return loss

    rows = {"off": [], "ema_decay 0.999": []}
    for _ in range(rounds):
        for name, averaged in (("off", False), ("ema_decay 0.999", True)):
            for _ in range(3):
                loss = step(averaged)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(steps):
                loss = step(averaged)
            t1.record()
            torch.cuda.synchronize()
            rows[name].append(round(t0.elapsed_time(t1) / steps, 3))
            print("step %-16s %.3f ms (loss %.5f)" % (name, rows[name][-1], float(loss.detach())), flush=True)
    return {"config": "--type pre --encoder resnet50, 2 x 1024 x 1024, fp32", "steps": steps, "ms_per_step": rows,
            "updates": ema.state_dict()["updates"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--no-step", action="store_true", help="the launch alone, no training steps")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ema: no GPU (timings are only meaningful on the MI355X)")
    dev = torch.device("cuda", 0)
    a, model, optim, ema = build(dev)
    out = {"launch": launch_cost(optim, ema, args.iters, args.rounds)}
    if not args.no_step:
        out["step"] = step_cost(a, model, optim, ema, dev, args.steps, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
