"""Per-tile cost of the offline post-processing (csrc/postproc.hip) on xBD-like 1024^2 tiles: ~300 rectangular and
L-shaped buildings, five-channel damage probabilities (background first), batches of 1, 8 and 32.

    python scripts/bench_postprocess.py [--batches 1,8,32] [--iters 20]

Prints, per batch size: GPU time per tile for components + dilate (rate 3) and for the fuse alone (event-timed after
warm-up), effective bandwidth against the 6.3 TB/s HBM roof (input bytes + workspace traffic), each kernel's time per
tile as the library's launch-bracketing profiler sees it (its events add their own overhead, most visible at B = 1),
and once the host time of the numpy restatement and of the reference-style per-building loop on one tile.

Per-kernel times from the trace, one batch size per run, components + dilate launches only:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python scripts/bench_postprocess.py --batches 8 --modes full --no-bracket --no-cpu"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import postproc_ref as R  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402

HBM = 6.3e12


def tiles(n):
    out = []
    for k in range(n):
        cls = R.buildings(900 + 7 * k)
        out.append((R.loc_from_mask(901 + 7 * k, cls > 0), R.probs_from_classes(902 + 7 * k, cls, 5)))
    return out


def timed(fn, iters):
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
        t, b = out.get(name, (0.0, 0.0))
        out[name] = (t + ms.value, b + by.value)
    _capi.query("xv2_prof_enable", 0)
    return out


def reference_style(loc, dmg):
    """the reference's per-building loop (post_process.py:40-43 restated): one full-tile scan per component"""
    pre, post = R.fuse(loc, dmg)
    comp = R.scipy_numbering(R.label_min_index(post > 0))
    for k in range(1, int(comp.max()) + 1):
        sel = comp == k
        vals, counts = np.unique(post[sel], return_counts=True)
        post[sel] = vals[np.argmax(counts)]
    return R.dilate(pre, 3), R.dilate(post, 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="1,8,32")
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--modes", default="full,fuse", help="full (components + dilate) and / or fuse (fuse only)")
    p.add_argument("--no-bracket", action="store_true", help="skip the launch-bracketing profiler pass")
    p.add_argument("--no-cpu", action="store_true", help="skip the host timings")
    a = p.parse_args()
    modes = a.modes.split(",")
    batches = [int(b) for b in a.batches.split(",")]
    base = tiles(4)
    dev = torch.device("cuda", 0)
    rows = []
    for B in batches:
        loc = torch.from_numpy(np.stack([base[i % 4][0] for i in range(B)])).to(dev)
        dmg = torch.from_numpy(np.stack([base[i % 4][1] for i in range(B)])).to(dev)
        ws = ops.postprocess_workspace(B, 1024, 1024, True, dev)
        full = lambda: ops.postprocess(loc, dmg, components=True, rate=3, workspace=ws)   # noqa: E731
        fuse = lambda: ops.postprocess(loc, dmg, components=False, rate=0)                 # noqa: E731
        t_full = timed(full, a.iters) if "full" in modes else float("nan")
        t_fuse = timed(fuse, a.iters) if "fuse" in modes else float("nan")
        ks = {} if a.no_bracket else kernel_times(full)
        in_bytes = B * 1024 * 1024 * (4 + 20)
        moved = sum(b for _, b in ks.values())   # algorithmic bytes of every launch (inputs, workspace, outputs)
        row = {"B": B, "full_us_per_tile": 1e3 * t_full / B, "fuse_us_per_tile": 1e3 * t_fuse / B,
               "full_TBps": moved / (t_full * 1e-3) / 1e12, "fuse_TBps": (in_bytes + 2 * B * 1024 * 1024) / (t_fuse * 1e-3) / 1e12,
               "bracketed_kernels_us_per_tile": {k: round(1e3 * t / B, 1) for k, (t, _) in sorted(ks.items())}}
        row["full_roof_frac"] = row["full_TBps"] * 1e12 / HBM
        rows.append(row)
        print("B=%-3d full %.1f us/tile (%.2f TB/s, %.0f%% of roof)  fuse %.1f us/tile (%.2f TB/s)  %s"
              % (B, row["full_us_per_tile"], row["full_TBps"], 100 * row["full_roof_frac"], row["fuse_us_per_tile"],
                 row["fuse_TBps"], row["bracketed_kernels_us_per_tile"]), flush=True)
    if a.no_cpu:
        print(json.dumps({"gpu": rows}))
        return
    loc, dmg = base[0]
    t0 = time.perf_counter()
    R.post_process(loc, dmg, components=True, rate=3)
    t1 = time.perf_counter()
    reference_style(loc, dmg)
    t2 = time.perf_counter()
    cpu = {"numpy_restatement_ms_per_tile": 1e3 * (t1 - t0), "reference_style_ms_per_tile": 1e3 * (t2 - t1)}
    print("host: numpy restatement %.0f ms/tile, reference-style per-building loop %.0f ms/tile"
          % (cpu["numpy_restatement_ms_per_tile"], cpu["reference_style_ms_per_tile"]))
    print(json.dumps({"gpu": rows, "cpu": cpu}))


if __name__ == "__main__":
    main()
