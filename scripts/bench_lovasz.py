"""Cost of the `lovasz` loss term (csrc/lovasz.hip, csrc/sort.hip) against the mean cross-entropy.

    python scripts/bench_lovasz.py [--iters 100] [--rounds 3] [--steps 10] [--no-step]

1. The term alone, forward + backward through `criterion.Loss` on 2 x 2 x 1024 x 1024 logits (about 5 % building pixels in
   rectangles, the benchmark's masks): `ce` against `lovasz`, event-timed after warm-up, the two alternating `--rounds`
   times; then each launch's time as the library's launch-bracketing profiler sees it (its events add their own overhead)
   next to the bytes it moves.
2. One training step of the benchmark's single-GPU configuration (--type pre --encoder resnet50, 2 x 1024 x 1024, fp32)
   with `--loss_str dice` against `lovasz+dice`, same process, alternating.

Prints one JSON line at the end."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from xview2_amd import _capi, criterion  # noqa: E402


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


def kernel_times(fn):
    _capi.query("xv2_prof_enable", 1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for i in range(_capi.query("xv2_prof_num_records")):
        kid, ms, fl, by = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _capi._func("xv2_prof_record")(i, ctypes.addressof(kid), ctypes.addressof(ms), ctypes.addressof(fl),
                                       ctypes.addressof(by))
        name = _capi.query("xv2_prof_kernel_name", kid.value).decode()
        n, t, b = out.get(name, (0, 0.0, 0.0))
        out[name] = (n + 1, t + ms.value, b + by.value)
    _capi.query("xv2_prof_enable", 0)
    return {k: {"launches": n, "us": round(1e3 * t, 1), "mbytes": round(b / 1e6, 2)} for k, (n, t, b) in sorted(out.items())}


def term_cost(dev, iters, rounds):
    a = bench.make_args(loss_str="ce")
    _, y = bench.synthetic_tiles(a, 2, 1024, 1)
    y = y.to(dev)
    x = (torch.randn(2, 2, 1024, 1024, generator=torch.Generator().manual_seed(2)) * 2).to(dev).requires_grad_(True)

    def make(loss_str):
        fn = criterion.Loss(bench.make_args(loss_str=loss_str))

        def run():
            x.grad = None
            fn(x, y).backward()
        return run
    ce, hard = make("ce"), make("lovasz")
    rows = {"ce": [], "lovasz": []}
    for _ in range(rounds):
        rows["ce"].append(round(1e3 * timed(ce, iters), 1))
        rows["lovasz"].append(round(1e3 * timed(hard, iters), 1))
    out = {"shape": [2, 2, 1024, 1024], "positives": round(float((y > 0).float().mean()), 4), "iters": iters,
           "fwd_bwd_us": rows, "lovasz_launches": kernel_times(hard)}
    print("term fwd+bwd, us per call: ce %s  lovasz %s" % (rows["ce"], rows["lovasz"]), flush=True)
    for k, v in out["lovasz_launches"].items():
        print("  %-22s x%d  %8.1f us  %8.2f MB" % (k, v["launches"], v["us"], v["mbytes"]), flush=True)
    return out


def step_cost(dev, steps, rounds):
    rows = {"dice": [], "lovasz+dice": []}
    for _ in range(rounds):
        for s in rows:
            leg = bench.config_leg(s, bench.make_args(loss_str=s), 32, 1024, 2, dev, steps=steps, warmup=3, parity=False)
            rows[s].append(leg["ms_per_step"])
            print("step %-16s %.3f ms (loss %.5f)" % (s, leg["ms_per_step"], leg["loss"]), flush=True)
    return {"config": "--type pre --encoder resnet50, 2 x 1024 x 1024, fp32", "steps": steps, "ms_per_step": rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--no-step", action="store_true", help="the term alone, no training steps")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lovasz: no GPU (timings are only meaningful on the MI355X)")
    dev = torch.device("cuda", 0)
    out = {"term": term_cost(dev, a.iters, a.rounds)}
    if not a.no_step:
        out["step"] = step_cost(dev, a.steps, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
