"""Cost of the threshold / class-scale sweep (csrc/calibrate.hip, xview2_amd/utils/calibrate.py): the histogram launch next to
its byte floor, to its own naive form (one LDS atomic per pixel), and to the brute force it replaces (one fuse launch and one
count launch per grid point); and the host's derivation of every grid point from the histogram.

    timeout -k 10 600 python scripts/bench_calibrate.py [--iters 10] [--rounds 3] [--out profiles/calibrate_cost.md]

One process.  Inputs: 8 tiles of 1024 x 1024 from tests/postproc_ref.py (`buildings`, 4-channel damage scores, targets from
other seeds; their background's localization score is spread evenly over (0, 0.1), i.e. over ten values of k), the same
tiles with the background's score divided by 20 (below 0.005, one value of k: what a trained sigmoid gives), and 8 tiles whose
every pixel falls into one bin.  Thresholds: the default grid of 100.  Scale lists: none
(S = 1) and --scale_grid 0.5,1,2 (S = 27).  Each launch is measured twice: the launch-bracketing profiler's kernel time of one
call, and device events around --iters calls.  The HBM rate the floor is divided by is measured here, by a device-to-device
copy of 1 GiB (read + written bytes over event time), and quoted next to the data-sheet rate.
Writes the record as markdown to --out and prints it."""
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
import postproc_ref as R  # noqa: E402
from bench_buildings import kernel_times, timed  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import calibrate  # noqa: E402

FORMS = (("naive", 0), ("1 round", 1), ("2 rounds", 2), ("8 rounds", 8))     # per-wave combining rounds, 0 = one atomic per pixel
BEST = "1 round"                                                            # the library's default (calibrate.hip DEFAULT_ROUNDS)
SPEC_TBS = 8.0      # HBM3E data-sheet rate of the MI355X


def copy_rate(dev, iters):
    a = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    torch.cuda.synchronize()
    us = statistics.median(timed(lambda: b.copy_(a), iters) for _ in range(3))
    return 2.0 * a.numel() / (us * 1e-6) / 1e12      # TB/s, read + written


def measure(fn, iters, rounds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ev = [timed(fn, iters) for _ in range(rounds)]
    return sum(kernel_times(fn).values()), ev


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_calibrate.py measures on the MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    B, H, W = 8, 1024, 1024
    px = B * H * W
    T = calibrate.threshold_grid(0.01)
    n = len(T)
    scales27 = calibrate.scale_list(scale_grid="0.5,1,2")
    cls = [R.buildings(11 + 10 * k) for k in range(B)]
    loc = torch.from_numpy(np.stack([R.loc_from_mask(12 + 10 * k, c > 0) for k, c in enumerate(cls)])).to(dev)
    dmg = torch.from_numpy(np.stack([R.probs_from_classes(13 + 10 * k, c, 4) for k, c in enumerate(cls)])).to(dev)
    dt = torch.from_numpy(np.stack([R.buildings(500 + 10 * k).astype(np.uint8) for k in range(B)])).to(dev)
    lt = (dt > 0).to(torch.uint8)
    one = (torch.full((B, H, W), 0.5, device=dev), torch.zeros((B, 4, H, W), device=dev), torch.ones_like(lt),
           torch.full_like(dt, 2))
    one[1][:, 1] = 1
    sure = torch.where(loc <= 0.1, loc / 20, loc)
    th = torch.from_numpy(T).to(dev)
    sc = torch.from_numpy(np.array(scales27, dtype=np.float32)).to(dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(inputs, scales, hist):
        l, d, t1, t2 = inputs
        S = 1 if scales is None else scales.shape[0]
        return lambda: _capi.call("xv2_calibrate_hist", l, d, 0, t1, t2, B, H, W, th, n, scales, S, hist, bad)

    rate = copy_rate(dev, a.iters)
    lines = ["# Cost of the threshold / class-scale sweep (`python -m xview2_amd.utils.calibrate`)", "",
             "One MI355X (%s), `python scripts/bench_calibrate.py --iters %d --rounds %d`, one process.  %d tiles of %d x %d, "
             "%d thresholds.  Recorded, not gated: the sweep is a tool of its own and nothing else launches it." %
             (torch.cuda.get_device_name(0), a.iters, a.rounds, B, H, W, n), "",
             "HBM rate measured in this run by a device-to-device copy of 1 GiB: **%.2f TB/s** (read + written); data sheet "
             "%.1f TB/s.  The pass reads 22 B per pixel with 4 damage channels (26 with 5) once per scale vector: the floor of "
             "one scale vector over these %d pixels is %.1f µs at the measured rate and %.1f µs at the data-sheet rate."
             % (rate, SPEC_TBS, px, 22.0 * px / rate / 1e6, 22.0 * px / SPEC_TBS / 1e6), "",
             "## The histogram launch", "",
             "| input | S | form | kernel time of one call, µs | µs per call by device events, %d rounds of %d | floor at the "
             "measured rate, µs | kernel time / floor |" % (a.rounds, a.iters),
             "|---|---|---|---|---|---|---|"]
    hists, ktime = {}, {}
    for iname, inputs in (("buildings", (loc, dmg, lt, dt)), ("buildings, sure background", (sure, dmg, lt, dt)),
                          ("one bin", one)):
        for S, scales in ((1, None), (27, sc)):
            for form, rounds in FORMS:
                _capi.query("xv2_calibrate_hist_rounds", rounds)
                hist = torch.zeros((S, n + 1, 4, 2, 5), dtype=torch.int64, device=dev)
                fn = launch(inputs, scales, hist)
                fn()
                hists[(iname, S, form)] = hist.clone()
                k, ev = measure(fn, a.iters, a.rounds)
                floor = 22.0 * px * S / rate / 1e6
                ktime[(iname, S, form)] = k
                lines.append("| %s | %d | %s | %.1f | %s | %.1f | %.2f |" % (iname, S, form, k, ", ".join("%.1f" % t for t in ev),
                                                                           floor, k / floor))
    _capi.query("xv2_calibrate_hist_rounds", -1)
    names = ("buildings", "buildings, sure background", "one bin")
    same = all(torch.equal(hists[(i, S, "naive")], hists[(i, S, f)]) for i in names for S in (1, 27) for f, _ in FORMS)
    bg = int(hists[("buildings", 1, "naive")][0, :11, :, 0, 0].sum())
    bg1 = int(hists[("buildings, sure background", 1, "naive")][0, 1, :, 0, 0].sum())
    ratio = lambda i, S: ktime[(i, S, "naive")] / ktime[(i, S, BEST)]
    lines += ["", "Every form gives the same histogram: %s.  On the buildings tiles %.1f %% of the pixels are true background scored "
              "below 0.1, spread over 40 bins (k = 1..10, r, t = 0, d = 0); with the sure background %.1f %% fall into the four bins "
              "(k = 1, r, t = 0, d = 0).  Naive over the default (%s), kernel times at S = 1 and S = 27: %s."
              % (same, 100.0 * bg / px, 100.0 * bg1 / px, BEST,
                 "; ".join("%s %.2f and %.2f" % (i, ratio(i, 1), ratio(i, 27)) for i in names)), ""]

    # the brute force: one fuse launch and one count launch per grid point
    pre, post = torch.empty_like(lt), torch.empty_like(lt)
    counts = torch.zeros((B, 16), dtype=torch.int64, device=dev)
    pts = [(30, 10), (50, 0), (99, 99), (10, 5), (70, 30)]
    per_point = []
    for i, j in pts:
        def fn(i=i, j=j):
            _capi.call("xv2_postprocess_ex", loc, dmg, 0, B, H, W, 0, 0, None, pre, post, None, float(T[i]), float(T[j]), None)
            _capi.call("xv2_xview2_counts", pre, post, lt, dt, B, H * W, counts)
        k, ev = measure(fn, a.iters, a.rounds)
        per_point.append((k, statistics.median(ev)))
    kp = statistics.median(x[0] for x in per_point)
    ep = statistics.median(x[1] for x in per_point)
    npts = n * (n + 1) // 2
    lines += ["## Against the brute force", "",
              "One grid point the long way is `pp_fuse_kernel` + `xview2_counts_kernel` on the same tiles: %.1f µs of kernel time, "
              "%.1f µs per point by device events (medians over the points %s).  The grid has n (n + 1) / 2 = %d pairs per scale "
              "vector.  Measured at those %d points and multiplied, not run in full:" % (kp, ep, pts, npts, len(pts)), "",
              "| S | points | brute force, kernel time x points, ms | histogram launch, ms | ratio |", "|---|---|---|---|---|"]
    for S in (1, 27):
        h = ktime[("buildings", S, BEST)]
        lines.append("| %d | %d | %.1f | %.3f | %.0f |" % (S, npts * S, kp * npts * S / 1e3, h / 1e3, kp * npts * S / h))

    # the host's share
    lines += ["", "## The host derivation", "",
              "From the buildings histogram: `derive` (all counts), `score_table` (all scores) and `best` (the maximum, near-ties "
              "scored again one by one), wall time of one run each on the host.", "",
              "| S | derive, ms | score_table, ms | best, ms |", "|---|---|---|---|"]
    for S in (1, 27):
        h = hists[("buildings", S, BEST)].cpu().numpy()
        t0 = time.perf_counter()
        c = calibrate.derive(h)
        t1 = time.perf_counter()
        tab = calibrate.score_table(c)
        t2 = time.perf_counter()
        calibrate.best(c, tab)
        t3 = time.perf_counter()
        lines.append("| %d | %.1f | %.1f | %.1f |" % (S, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
    lines += ["", "Not measured: 5-channel input, label maps, reading the .npy and .png files, and the two verifying passes of "
              "the tool (they are `post_process_tiles` and `xv2_xview2_counts`, unchanged).", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not same:
        raise SystemExit("the naive and the combined histogram differ")


if __name__ == "__main__":
    main()
