"""Cost of the per-building table (csrc/buildings.hip) next to xv2_postprocess with components on the same maps, and
next to the scipy.ndimage path on the host.

    timeout -k 10 900 python scripts/bench_buildings.py [--iters 20] [--rounds 3] [--out profiles/buildings_cost.md]

One process.  Two shapes: B = 8 tiles of 1024 x 1024 (xBD-like: ~300 rectangular and L-shaped buildings each, the
generator of tests/postproc_ref.py) and one 4096 x 4096 scene of random blobs (a 17 x 17 box-filtered hashed field
thresholded at 0.525, tests/buildings_ref.blobs).  The row capacity is the module's first capacity, or the count when
that is larger (the module's second run).  Per shape, event-timed after warm-up, the legs alternating within every round:
  table        the five launches of xv2_building_table on preallocated buffers (labels, maps and workspace resident)
  label        xv2_label_components of pre != 0, which utils.buildings.building_table runs in front of the table
  postprocess  xv2_postprocess with components (no dilation) on the same loc / dmg maps
Then once per shape the launch-bracketing profiler's time per kernel, the module call utils.buildings.building_table
(labelling, table, the two copies to the host) by the host clock, and the scipy.ndimage restatement of
tests/buildings_ref.py on the host.  The GPU table is compared with the restatement at the timed sizes.  Writes the record
as markdown to --out and prints it."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import buildings_ref as BR  # noqa: E402
import postproc_ref as PR  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import buildings  # noqa: E402


def tiles_1024(n):
    locs, dmgs = [], []
    for k in range(n):
        cls = PR.buildings(900 + 7 * k)
        locs.append(PR.loc_from_mask(901 + 7 * k, cls > 0))
        dmgs.append(PR.probs_from_classes(902 + 7 * k, cls, 4))
    return np.stack(locs), np.stack(dmgs)


def scene_4096():
    H = W = 4096
    cls = np.where(BR.blobs(5, H, W, thresh=0.525, box=17), 1 + PR.hash_int(6, (H, W), 4), 0)
    return PR.loc_from_mask(7, cls > 0)[None], PR.probs_from_classes(8, cls, 4)[None]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters      # microseconds per call


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
        out[name] = out.get(name, 0.0) + 1e3 * ms.value
    _capi.query("xv2_prof_enable", 0)
    return out


def bench_shape(name, loc_np, dmg_np, iters, rounds, lines):
    dev = torch.device("cuda", 0)
    B, H, W = loc_np.shape
    loc, dmg = torch.from_numpy(loc_np).to(dev), torch.from_numpy(dmg_np).to(dev)
    pws = ops.postprocess_workspace(B, H, W, True, dev)
    pre, post = ops.postprocess(loc, dmg, components=True, rate=0, workspace=pws)
    labels = ops.label_components(pre)
    cap = buildings.first_capacity(H, W)
    cap = max(cap, int(ops.building_table(labels, post, loc, cap)[1].max()))
    need = int(_capi.query("xv2_building_table_workspace", B, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rows = torch.empty((B, cap, 16), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    legs = {
        "table": lambda: _capi.call("xv2_building_table", labels, post, loc, B, H, W, cap, ws, rows, count),
        "label": lambda: _capi.call("xv2_label_components", pre, B, H, W, None, labels),
        "postprocess": lambda: ops.postprocess(loc, dmg, components=True, rate=0, workspace=pws),
    }
    for fn in legs.values():                     # warm-up of every leg at this shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    n = count.cpu().numpy()
    assert int(n.max()) <= cap, "first capacity %d below the count %d" % (cap, int(n.max()))
    ks = kernel_times(legs["table"])
    buildings.building_table(pre, post, loc)     # the first call of a shape pays torch's first slicing copy and allocations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = buildings.building_table(pre, post, loc)
    t_module = time.perf_counter() - t0
    pre_h, post_h = pre.cpu().numpy(), post.cpu().numpy()
    t0 = time.perf_counter()
    want = BR.table(pre_h[0], post_h[0], loc_np[0])
    t_host = time.perf_counter() - t0
    equal = np.array_equal(got[0], want)
    px = B * H * W
    lines.append("## %s: B = %d, %d x %d" % (name, B, H, W))
    lines.append("")
    lines.append("Components per tile: %s (row capacity %d per tile); foreground %.1f %% of the pixels."
                 % (", ".join(str(int(v)) for v in n), cap, 100.0 * float((pre_h != 0).mean())))
    lines.append("")
    lines.append("| leg | µs per call, %d rounds of %d calls | median | ns per pixel |" % (rounds, iters))
    lines.append("|---|---|---|---|")
    for k in legs:
        med = statistics.median(times[k])
        lines.append("| %s | %s | %.1f | %.4f |" % (k, ", ".join("%.1f" % t for t in times[k]), med, 1e3 * med / px))
    ratio = statistics.median(times["table"]) / statistics.median(times["postprocess"])
    lines.append("")
    lines.append("Table launches over `xv2_postprocess` with components: %.2f (%s)."
                 % (ratio, "above it" if ratio > 1 else "below it"))
    lines.append("")
    lines.append("Per kernel, one bracketed call (the brackets' events add their own overhead): "
                 + ", ".join("`%s` %.1f µs" % kv for kv in sorted(ks.items())) + ".")
    lines.append("")
    lines.append("`utils.buildings.building_table` (labelling, table, `count` and the rows copied back), host clock, the second call: "
                 "%.2f ms for the batch.  `scipy.ndimage` restatement (tests/buildings_ref.table) of tile 0 on the host: "
                 "%.1f ms.  GPU table of tile 0 equal to it: %s." % (1e3 * t_module, 1e3 * t_host, equal))
    lines.append("")
    return equal


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "buildings_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_buildings.py measures on the MI355X; there is no CPU fallback")
    lines = ["# Cost of the per-building table (`--buildings`)", "",
             "One MI355X (%s), `python scripts/bench_buildings.py --iters %d --rounds %d`, one process.  Device events around "
             "%d calls after warm-up, the legs alternating within each round.  Recorded, not gated: the feature is off by "
             "default and a run that does not ask for it launches nothing new." % (
                 torch.cuda.get_device_name(0), a.iters, a.rounds, a.iters), ""]
    ok = bench_shape("xBD-like tiles", *tiles_1024(8), a.iters, a.rounds, lines)
    ok = bench_shape("blob scene", *scene_4096(), a.iters, a.rounds, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU table differs from the restatement")


if __name__ == "__main__":
    main()
