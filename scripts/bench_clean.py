"""Cost of filling holes and dropping small buildings (csrc/clean.hip) next to the --buildings launches on the same maps, and
next to the scipy.ndimage restatement on the host.

    timeout -k 10 600 python scripts/bench_clean.py [--iters 10] [--rounds 3] [--out profiles/clean_cost.md]

One process.  The map is the 4096 x 4096 blob scene of scripts/bench_split.py (a 17 x 17 box-filtered hashed field
thresholded at 0.525, tests/buildings_ref.blobs) as a uint8 mask, with a hashed damage map on it.  For (min_area, max_hole) =
(16, 16) and (0, H * W):
  clean      xv2_clean_buildings on a resident workspace: the sum of the launch-bracketing profiler's kernel times of one
             call, and device events around --iters calls (which also see the stats memset and the gaps between launches)
  buildings  xv2_label_components and xv2_building_table on the cleaned maps: what --buildings launches afterwards, measured
             the same two ways in the same run
  host       the same rule through scipy.ndimage.label on the host (localization map only), which the GPU map is compared
             with
Writes the record as markdown to --out and prints it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import buildings_ref as BR  # noqa: E402
from bench_buildings import kernel_times, timed  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import buildings  # noqa: E402

EIGHT = np.ones((3, 3), dtype=int)


def host_clean(pre, A, M):
    """the rule on the localization map alone: (map, seconds)"""
    t0 = time.perf_counter()
    out = pre.copy()
    if M > 0:
        lab, n = ndimage.label(pre == 0, structure=EIGHT)
        fill = np.bincount(lab.ravel(), minlength=n + 1) <= M
        fill[0] = False
        fill[np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))] = False
        out[fill[lab]] = 1
    if A > 1:
        lab, n = ndimage.label(out != 0)
        small = np.bincount(lab.ravel(), minlength=n + 1) < A
        small[0] = False
        out[small[lab]] = 0
    return out, time.perf_counter() - t0


def bench_pair(pre_np, post_np, A, M, iters, rounds, lines):
    dev = torch.device("cuda", 0)
    pre, post = torch.from_numpy(pre_np[None]).to(dev), torch.from_numpy(post_np[None]).to(dev)
    B, H, W = pre.shape
    ws = ops.clean_workspace(B, H, W, dev)
    out, pout = torch.empty_like(pre), torch.empty_like(post)
    stats = torch.empty((B, 4), dtype=torch.int64, device=dev)

    def clean():
        _capi.call("xv2_clean_buildings", pre, post, B, H, W, A, M, ws, out, pout, stats)

    clean()
    labels = ops.label_components(out)
    cap = buildings.first_capacity(H, W)
    cap = max(cap, int(ops.building_table(labels, pout, None, cap)[1].max()))
    tws = torch.empty(int(_capi.query("xv2_building_table_workspace", B, H, W)), dtype=torch.uint8, device=dev)
    rows = torch.empty((B, cap, 16), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)

    def table():
        _capi.call("xv2_label_components", out, B, H, W, None, labels)
        _capi.call("xv2_building_table", labels, pout, None, B, H, W, cap, tws, rows, count)

    legs = {"clean": clean, "buildings": table}
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    kt = {k: kernel_times(fn) for k, fn in legs.items()}
    want, t_host = host_clean(pre_np, A, M)
    equal = np.array_equal(out[0].cpu().numpy(), want)
    before = int(ops.building_table(ops.label_components(pre), post, None, cap)[1][0])
    s = stats[0].cpu().tolist()
    k_clean, k_table = sum(kt["clean"].values()), sum(kt["buildings"].values())
    lines.append("## min_area = %d, max_hole = %d" % (A, M))
    lines.append("")
    lines.append("Holes filled: %d (%d pixels); buildings dropped: %d (%d pixels); buildings before: %d, after: %d."
                 % (s[0], s[1], s[2], s[3], before, int(count[0])))
    lines.append("")
    lines.append("| leg | kernel times of one call, µs | µs per call by device events, %d rounds of %d calls | median |"
                 % (rounds, iters))
    lines.append("|---|---|---|---|")
    for k in legs:
        lines.append("| %s | %.1f | %s | %.1f |" % (k, sum(kt[k].values()), ", ".join("%.1f" % t for t in times[k]),
                                                    statistics.median(times[k])))
    lines.append("| host (scipy.ndimage) | %.0f | | |" % (1e6 * t_host))
    lines.append("")
    lines.append("Ratios by kernel times: clean / buildings %.2f, host / clean %.0f.  GPU map equal to the host's: %s."
                 % (k_clean / k_table, 1e6 * t_host / k_clean, equal))
    lines.append("")
    for k in legs:
        lines.append("Per kernel, %s (the two labellings of a clean call share their kernels' names): " % k
                     + ", ".join("`%s` %.1f µs" % kv for kv in sorted(kt[k].items())) + ".")
    lines.append("")
    return equal


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_clean.py measures on the MI355X; there is no CPU fallback")
    H = W = 4096
    pre = BR.blobs(5, H, W, thresh=0.525, box=17).astype(np.uint8)
    post = (pre * (1 + BR._hash(6, (H, W), 4))).astype(np.uint8)
    lines = ["# Cost of filling holes and dropping small buildings (`--fill_holes M`, `--min_area A`)", "",
             "One MI355X (%s), `python scripts/bench_clean.py --iters %d --rounds %d`, one process.  One %d x %d blob scene, "
             "foreground %.1f %% of the pixels.  Recorded, not gated: the feature is off by default and a run that does not ask "
             "for it launches nothing new." % (torch.cuda.get_device_name(0), a.iters, a.rounds, H, W, 100.0 * float(pre.mean())),
             ""]
    ok = True
    for A, M in ((16, 16), (0, H * W)):
        ok = bench_pair(pre, post, A, M, a.iters, a.rounds, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU map differs from the host's")


if __name__ == "__main__":
    main()
