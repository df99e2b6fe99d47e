"""Cost of the `wce` loss term (csrc/wce.hip) against the mean cross-entropy.

    python scripts/bench_wce.py [--iters 100] [--rounds 3] [--steps 10] [--no-step]

1. The term alone, forward + backward through `criterion.Loss` on 2 x 2 x 1024 x 1024 logits (the benchmark's rectangle masks):
   `ce` against `wce` with class weights only and `wce` with the border map (its distance launch included, R = 15),
   event-timed after warm-up, alternating `--rounds` times.
2. The distance launch alone (`ops.border_distances`, component labelling included) on the same 2 x 1024 x 1024 labels at
   R = 8, 15 and 32, and on a denser map of 600 small rectangles per image, where far more pixels have a building in reach.
3. One training step of the benchmark's single-GPU configuration (--type pre --encoder resnet50, 2 x 1024 x 1024, fp32)
   with `--loss_str dice` against `wce+dice` with class weights 1,3 alone and with the border weight 10 as well, same
   process, alternating.  `--no-term` runs this part alone.

Prints one JSON line at the end."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from xview2_amd import criterion, ops  # noqa: E402

WCE = dict(class_weights="1,3", border_weight=10.0, border_sigma=5.0, border_radius=0)


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


def dense_labels(dev):
    g = torch.Generator().manual_seed(4)
    m = torch.zeros(2, 1024, 1024, dtype=torch.uint8)
    for b in range(2):
        for _ in range(600):
            h, w = [int(v) for v in torch.randint(4, 25, (2,), generator=g)]
            y0, x0 = int(torch.randint(0, 1024 - h, (1,), generator=g)), int(torch.randint(0, 1024 - w, (1,), generator=g))
            m[b, y0:y0 + h, x0:x0 + w] = 1
    return m.to(dev)


def term_cost(dev, iters, rounds):
    _, y = bench.synthetic_tiles(bench.make_args(loss_str="ce"), 2, 1024, 1)
    y = y.to(dev)
    x = (torch.randn(2, 2, 1024, 1024, generator=torch.Generator().manual_seed(2)) * 2).to(dev).requires_grad_(True)

    def make(loss_str, **kw):
        fn = criterion.Loss(bench.make_args(loss_str=loss_str, **kw))

        def run():
            x.grad = None
            fn(x, y).backward()
        return run
    legs = {"ce": make("ce"), "wce_class_weights": make("wce", class_weights="1,3"), "wce_border": make("wce", **WCE)}
    rows = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            rows[k].append(round(1e3 * timed(fn, iters), 1))
    print("term fwd+bwd, us per call: %s" % rows, flush=True)
    dist = {}
    for name, lab in (("benchmark_masks", y), ("600_rectangles", dense_labels(dev))):
        d2 = ops.border_distances(lab, 15)[1]
        share = float((d2.to(torch.int32) != ops.BORDER_NONE).float().mean())
        dist[name] = {"building_share": round(float((lab > 0).float().mean()), 4), "d2_share_r15": round(share, 4)}
        for rad in (8, 15, 32):
            dist[name]["r%d_us" % rad] = [round(1e3 * timed(lambda: ops.border_distances(lab, rad), iters), 1) for _ in range(rounds)]
        print("distances %-16s %s" % (name, dist[name]), flush=True)
    return {"shape": [2, 2, 1024, 1024], "iters": iters, "fwd_bwd_us": rows, "distances": dist}


def step_cost(dev, steps, rounds):
    legs = {"dice": ("dice", {}), "wce+dice, class weights": ("wce+dice", dict(class_weights="1,3")), "wce+dice, border": ("wce+dice", WCE)}
    rows = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (s, kw) in legs.items():
            leg = bench.config_leg(s, bench.make_args(loss_str=s, **kw), 32, 1024, 2, dev, steps=steps, warmup=3, parity=False)
            rows[k].append(leg["ms_per_step"])
            print("step %-24s %.3f ms (loss %.5f)" % (k, leg["ms_per_step"], leg["loss"]), flush=True)
    return {"config": "--type pre --encoder resnet50, 2 x 1024 x 1024, fp32", "steps": steps, "ms_per_step": rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--no-step", action="store_true", help="the term and the distances alone, no training steps")
    p.add_argument("--no-term", action="store_true", help="the training steps alone")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wce: no GPU (timings are only meaningful on the MI355X)")
    dev = torch.device("cuda", 0)
    out = {} if a.no_term else {"term": term_cost(dev, a.iters, a.rounds)}
    if not a.no_step:
        out["step"] = step_cost(dev, a.steps, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
