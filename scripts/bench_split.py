"""Cost of splitting touching buildings (csrc/split.hip) next to the --buildings launches on the same maps, and next to
the numpy / scipy restatement on the host.

    timeout -k 10 900 python scripts/bench_split.py [--iters 10] [--rounds 3] [--radii 2,4] [--out profiles/split_cost.md]

One process.  The map is the 4096 x 4096 blob scene of scripts/bench_buildings.py (a 17 x 17 box-filtered hashed field
thresholded at 0.525, tests/buildings_ref.blobs) as a uint8 mask.  Per radius R (r2 = R^2), event-timed after warm-up, the
legs alternating within every round:
  split      xv2_split_seed, as many xv2_split_grow calls of 8 sweeps as ops.split_buildings needed on this map, and
             xv2_split_finish, on a resident workspace and without the read-back of `pending` between the calls
  buildings  xv2_label_components and xv2_building_table on the split map: what --buildings launches afterwards
Then once per radius ops.split_buildings by the host clock (with its one read-back per grow call), the launch-bracketing
profiler's time per kernel, and for the first radius the restatement of tests/split_ref.py on the host, which the GPU map is
compared with.  Writes the record as markdown to --out and prints it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import buildings_ref as BR  # noqa: E402
import split_ref as SR  # noqa: E402
from bench_buildings import kernel_times, timed  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import buildings  # noqa: E402

SWEEPS = 8


def bench_radius(mask_np, R, iters, rounds, restate, lines):
    dev = torch.device("cuda", 0)
    mask = torch.from_numpy(mask_np[None]).to(dev)
    B, H, W = mask.shape
    r2 = R * R
    out, calls, L = ops.split_buildings(mask, r2, SWEEPS, return_labels=True)
    ws = torch.empty(int(_capi.query("xv2_split_workspace", B, H, W)), dtype=torch.uint8, device=dev)
    pending = torch.empty((1,), dtype=torch.int32, device=dev)
    got = torch.empty_like(mask)

    def split():
        _capi.call("xv2_split_seed", mask, B, H, W, r2, ws)
        for _ in range(calls):
            _capi.call("xv2_split_grow", mask, B, H, W, SWEEPS, ws, pending)
        _capi.call("xv2_split_finish", mask, B, H, W, ws, got, None)

    labels = ops.label_components(out)
    cap = buildings.first_capacity(H, W)
    cap = max(cap, int(ops.building_table(labels, out, None, cap)[1].max()))
    tws = torch.empty(int(_capi.query("xv2_building_table_workspace", B, H, W)), dtype=torch.uint8, device=dev)
    rows = torch.empty((B, cap, 16), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)

    def table():
        _capi.call("xv2_label_components", out, B, H, W, None, labels)
        _capi.call("xv2_building_table", labels, out, None, B, H, W, cap, tws, rows, count)

    legs = {"split": split, "buildings": table}
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(got, out) and int(pending.item()) == 0
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    ks = kernel_times(split)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.split_buildings(mask, r2, SWEEPS)
    torch.cuda.synchronize()
    t_module = time.perf_counter() - t0
    pieces_before = int(ops.building_table(ops.label_components(mask), mask, None, cap)[1][0])
    px = B * H * W
    lines.append("## R = %d (r2 = %d, cap = %d)" % (R, r2, SR.cap_of(r2)))
    lines.append("")
    lines.append("Seeds: %d; buildings before the split: %d, after: %d; pixels cut: %d; grow calls of %d sweeps until the last "
                 "sweep of a call changed nothing: %d (at most %d sweeps)."
                 % (int(torch.unique(L).numel()) - 1, pieces_before, int(count[0]), int((out != mask).sum()), SWEEPS, calls,
                    SWEEPS * calls))
    lines.append("")
    lines.append("| leg | µs per call, %d rounds of %d calls | median | ns per pixel |" % (rounds, iters))
    lines.append("|---|---|---|---|")
    for k in legs:
        med = statistics.median(times[k])
        lines.append("| %s | %s | %.1f | %.4f |" % (k, ", ".join("%.1f" % t for t in times[k]), med, 1e3 * med / px))
    lines.append("")
    lines.append("Per kernel, one bracketed split (the brackets' events add their own overhead; `sp_grow_kernel` is the sum "
                 "over %d sweeps): " % (SWEEPS * calls) + ", ".join("`%s` %.1f µs" % kv for kv in sorted(ks.items())) + ".")
    lines.append("")
    lines.append("`ops.split_buildings` (allocations, seed, grow calls with one read-back each, finish), host clock, the second "
                 "call: %.2f ms." % (1e3 * t_module))
    equal = True
    if restate:
        t0 = time.perf_counter()
        want, _, n_rounds = SR.split(mask_np, r2)
        t_host = time.perf_counter() - t0
        equal = np.array_equal(out[0].cpu().numpy(), want)
        lines.append("numpy restatement (tests/split_ref.split: brute-force distance, %d synchronous rounds, cut) on the host: "
                     "%.1f s.  GPU map equal to it: %s." % (n_rounds, t_host, equal))
    lines.append("")
    return equal


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--radii", default="2,4")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_split.py measures on the MI355X; there is no CPU fallback")
    H = W = 4096
    mask = BR.blobs(5, H, W, thresh=0.525, box=17).astype(np.uint8)
    lines = ["# Cost of splitting touching buildings (`--split R`)", "",
             "One MI355X (%s), `python scripts/bench_split.py --iters %d --rounds %d --radii %s`, one process.  One %d x %d blob "
             "scene, foreground %.1f %% of the pixels.  Device events around %d calls after warm-up, the legs alternating within "
             "each round.  Recorded, not gated: the feature is off by default and a run that does not ask for it launches "
             "nothing new." % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.radii, H, W, 100.0 * float(mask.mean()),
                               a.iters), ""]
    ok = True
    for i, R in enumerate(int(v) for v in a.radii.split(",")):
        ok = bench_radius(mask, R, a.iters, a.rounds, i == 0, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU map differs from the restatement")


if __name__ == "__main__":
    main()
