"""Cost of gradient accumulation (csrc/optim.hip xv2_grad_accumulate, optim.FlatOptimizer.accumulate).

    python scripts/bench_accumulate.py [--iters 200] [--rounds 3] [--micro 12] [--no-step]

1. The launch alone in its three modes (open 8, add and close 12 bytes per element) next to the weight average's launch
   (xv2_ema_update_dev, 12 bytes per element) on the same two buffers in the same run: event-timed after warm-up, the four
   alternating `--rounds` times.  Two buffer sizes: the flat buffer of the benchmark's single-GPU model (--type pre --encoder
   resnet50) and that of cfg5 (--type post --dmg_model fused --encoder resnest200 --attention --ppm --deep_supervision), whose
   layout is taken from the model built on the host.
2. The time per micro-batch of the benchmark's resnet50 step, 2 x 1024 x 1024, fp32, at K = 1 (every micro-batch steps) and at
   K = 4 (three accumulate() calls, then one step()): same process, same model, alternating, `--micro` micro-batches per timing.

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
from xview2_amd.optim import FlatAdamW  # noqa: E402
from xview2_amd.weights import deterministic_init_  # noqa: E402

BYTES = {"open": 8, "add": 12, "close": 12, "ema": 12}      # per element
MODES = {"open": 0, "add": 1, "close": 2}


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


def flat_total(model):
    """the length of a FlatOptimizer's buffers for this model: every trainable tensor once, padded to 16 bytes"""
    seen, total = set(), 0
    for p in model.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            total += (p.numel() + 3) // 4 * 4
    return total


def launch_cost(name, n, dev, iters, rounds):
    gen = torch.Generator().manual_seed(2)
    grad = (1e-3 * torch.randn(n, generator=gen)).to(dev)
    acc = torch.zeros(n, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def mode(m):
        return lambda: _capi.call("xv2_grad_accumulate", acc, grad, n, m)

    def ema():
        # (acc as the average, grad as the parameters: the same two arrays)
        _capi.call("xv2_ema_update_dev", acc, grad, n, 0.999, 1, count, None)

    legs = [(k, mode(m)) for k, m in MODES.items()] + [("ema", ema)]
    rows = {k: [] for k, _ in legs}
    for _ in range(rounds):
        for k, fn in legs:
            acc.zero_()          # (close adds acc into grad: with acc at zero the values stay where they are)
            if k == "add":
                acc.copy_(grad)
            rows[k].append(round(1e3 * timed(fn, iters), 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    out = {"buffer": name, "elements": n, "iters": iters, "us": rows, "median_us": med,
           "tbytes_per_s": {k: round(BYTES[k] * n / med[k] / 1e6, 2) for k in rows},
           "add_over_ema": round(med["add"] / med["ema"], 3)}
    print("%s, %d elements, us per call: %s" % (name, n, rows), flush=True)
    return out


def step_cost(dev, micro, rounds):
    a = bench.make_args()
    bench.set_precision(32)
    torch.manual_seed(0)
    model = networks.UNetLoc(a)
    deterministic_init_(model, 1)
    model.to(dev).train()
    optim = FlatAdamW(model.parameters(), lr=3e-4, weight_decay=0.0)
    loss_fn = criterion.Loss(a)
    x, y = bench.synthetic_batch(a, 2, 1024, 1, dev)

    def run(k, n):
        for i in range(n):
            optim.zero_grad()
            loss = criterion.compute_loss(loss_fn, model(x), y, a.deep_supervision)
            loss.backward()
            if (i + 1) % k == 0:
                optim.step()
            else:
                optim.accumulate()
        return loss

    rows = {"K=1": [], "K=4": []}
    for _ in range(rounds):
        for name, k in (("K=1", 1), ("K=4", 4)):
            loss = run(k, 4)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            loss = run(k, micro)
            t1.record()
            torch.cuda.synchronize()
            rows[name].append(round(t0.elapsed_time(t1) / micro, 3))
            print("%s %.3f ms per micro-batch (loss %.5f)" % (name, rows[name][-1], float(loss.detach())), flush=True)
    return {"config": "--type pre --encoder resnet50, 2 x 1024 x 1024, fp32", "elements": optim.total,
            "micro_batches_per_timing": micro, "ms_per_micro_batch": rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--micro", type=int, default=12, help="micro-batches per timing (a multiple of 4)")
    p.add_argument("--no-step", action="store_true", help="the launches alone, no training steps")
    args = p.parse_args()
    if args.micro < 4 or args.micro % 4:
        sys.exit("bench_accumulate: --micro must be a positive multiple of 4")
    if not torch.cuda.is_available():
        sys.exit("bench_accumulate: no GPU (timings are only meaningful on the MI355X)")
    dev = torch.device("cuda", 0)
    sizes = [("resnet50 (cfg2)", flat_total(networks.UNetLoc(bench.make_args()))),
             ("cfg5 (fused resnest200)", flat_total(networks.get_dmg_unet(bench.make_args(
                 "resnest200", "post", "focal+dice", "fused", attention=True, ppm=True, deep_supervision=True))))]
    out = {"launch": [launch_cost(name, n, dev, args.iters, args.rounds) for name, n in sizes]}
    if not args.no_step:
        out["step"] = step_cost(dev, args.micro, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
