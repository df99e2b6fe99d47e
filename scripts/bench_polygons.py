"""Cost of tracing the building outlines (csrc/polygons.hip) next to the per-building table (csrc/buildings.hip) on the same
label maps in the same run.

    timeout -k 10 900 python scripts/bench_polygons.py [--iters 20] [--rounds 3] [--out profiles/polygons_cost.md]

One process.  The two shapes of scripts/bench_buildings.py: B = 8 tiles of 1024 x 1024 (xBD-like: some hundred rectangular and
L-shaped buildings each) and one 4096 x 4096 scene of random blobs.  Per shape, event-timed after warm-up, the legs
alternating within every round, all on preallocated buffers:
  count   the two launches of xv2_polygon_count
  trace   the launches of xv2_polygon_trace with the totals the count gave
  table   the five launches of xv2_building_table (the yardstick: what --buildings costs on the same maps)
  label   xv2_label_components of pre != 0, which both run behind
Then once per shape the launch-bracketing profiler's time per kernel name with its number of launches, the pointer-doubling
rounds that did work (the head of the trace workspace), the edge, vertex and ring counts, and the module call
utils.polygons.building_polygons by the host clock.  There is no host comparator.  The result is checked at the timed
sizes without a sequential tracer: the rings' 2A summed per root against twice the table's areas, the ring count against
the component counts of scipy.ndimage, and an even-odd rasterisation of tile 0's rings against its mask.  Writes the
record as markdown to --out and prints it."""
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
import polygons_ref as R  # noqa: E402
from bench_buildings import scene_4096, tiles_1024, timed  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import buildings, polygons  # noqa: E402


def kernel_times(fn):
    """name -> (microseconds, launches) of one bracketed call"""
    import ctypes
    _capi.query("xv2_prof_enable", 1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for i in range(_capi.query("xv2_prof_num_records")):
        kid, ms, fl, by = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _capi._func("xv2_prof_record")(i, ctypes.addressof(kid), ctypes.addressof(ms), ctypes.addressof(fl),
                                       ctypes.addressof(by))
        name = _capi.query("xv2_prof_kernel_name", kid.value).decode()
        t, n = out.get(name, (0.0, 0))
        out[name] = (t + 1e3 * ms.value, n + 1)
    _capi.query("xv2_prof_enable", 0)
    return out


def even_odd(rings, verts, H, W):
    """tests/polygons_ref.rasterise in array form: vertical ring edges counted to the left of every pixel centre"""
    d = np.zeros((H + 1, W + 1), dtype=np.int32)
    for r in rings:
        p = verts[r[3]:r[3] + r[2]].astype(np.int64)
        q = np.roll(p, -1, axis=0)
        v = (p[:, 0] == q[:, 0]) & (p[:, 1] != q[:, 1])
        np.add.at(d, (np.minimum(p[v, 1], q[v, 1]), p[v, 0]), 1)
        np.add.at(d, (np.maximum(p[v, 1], q[v, 1]), p[v, 0]), -1)
    return (np.cumsum(np.cumsum(d, axis=0), axis=1)[:H, :W] & 1).astype(bool)


def bench_shape(name, loc_np, dmg_np, iters, rounds, lines):
    dev = torch.device("cuda", 0)
    B, H, W = loc_np.shape
    loc, dmg = torch.from_numpy(loc_np).to(dev), torch.from_numpy(dmg_np).to(dev)
    pre, post = ops.postprocess(loc, dmg, components=True, rate=0, workspace=ops.postprocess_workspace(B, H, W, True, dev))
    labels = ops.label_components(pre)
    counts_h = ops.polygon_count(labels).cpu().numpy()
    E, V = int(counts_h[:, 0].sum()), int(counts_h[:, 1].sum())
    cap = buildings.first_capacity(H, W)
    cap = max(cap, int(ops.building_table(labels, post, loc, cap)[1].max()))
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)     # noqa: E731
    ws_c = u8(_capi.query("xv2_polygon_count_workspace", B, H, W))
    ws_t = u8(_capi.query("xv2_polygon_trace_workspace", B, H, W, E))
    ws_b = u8(_capi.query("xv2_building_table_workspace", B, H, W))
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    rings = torch.empty((V // 4, 8), dtype=torch.int64, device=dev)
    verts = torch.empty((V, 2), dtype=torch.int32, device=dev)
    ring_count = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    rows = torch.empty((B, cap, 16), dtype=torch.int64, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    legs = {
        "count": lambda: _capi.call("xv2_polygon_count", labels, B, H, W, ws_c, counts),
        "trace": lambda: _capi.call("xv2_polygon_trace", labels, B, H, W, E, V, ws_t, rings, verts, ring_count, status),
        "table": lambda: _capi.call("xv2_building_table", labels, post, loc, B, H, W, cap, ws_b, rows, count),
        "label": lambda: _capi.call("xv2_label_components", pre, B, H, W, None, labels),
    }
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    ks = kernel_times(legs["trace"])
    kc = kernel_times(legs["count"])
    did = ws_t[16:32].cpu().numpy().view(np.int32)[1:3].tolist()
    assert int(status.item()) == 0 and np.array_equal(counts.cpu().numpy(), counts_h)
    polygons.building_polygons(pre)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    polys = polygons.building_polygons(pre)
    t_module = time.perf_counter() - t0
    # the checks
    n = ring_count.cpu().numpy().astype(np.int64)
    rings_h, verts_h = rings[:int(n.sum())].cpu().numpy(), verts.cpu().numpy()
    table = buildings.building_table(pre, post, loc)
    pre_h = pre.cpu().numpy()
    ok = True
    ends = np.cumsum(n)
    for b in range(B):
        r = rings_h[ends[b] - n[b]:ends[b]]
        roots, inv = np.unique(r[:, 0], return_inverse=True)
        area2 = np.zeros(len(roots), dtype=np.int64)
        np.add.at(area2, inv, r[:, 4])
        ok = ok and np.array_equal(roots, table[b][:, 0]) and np.array_equal(area2, 2 * table[b][:, 1])
        ok = ok and np.all(r[:, 6] == b) and len(polys[b]) == len(table[b])
    ok = ok and int(n[0]) == R.expected_ring_count(pre_h[0])
    ok = ok and np.array_equal(even_odd(rings_h[:n[0]], verts_h, H, W), pre_h[0] != 0)
    px = B * H * W
    lines.append("## %s: B = %d, %d x %d" % (name, B, H, W))
    lines.append("")
    lines.append("Boundary edges %d, vertices %d, rings %d (per tile: %s), buildings %d; the longest ring has %d edges; "
                 "foreground %.1f %% of the pixels.  Pointer-doubling rounds that did work: %d for the leaders, %d for the "
                 "ranks, of %d launched each."
                 % (E, V, int(n.sum()), ", ".join(str(int(v)) for v in n), sum(len(t) for t in table),
                    int(rings_h[:, 5].max()), 100.0 * float((pre_h != 0).mean()), did[0], did[1], ks["pg_min_kernel"][1]))
    lines.append("")
    lines.append("| leg | µs per call, %d rounds of %d calls | median | ns per pixel |" % (rounds, iters))
    lines.append("|---|---|---|---|")
    med = {k: statistics.median(times[k]) for k in legs}
    for k in legs:
        lines.append("| %s | %s | %.1f | %.4f |" % (k, ", ".join("%.1f" % t for t in times[k]), med[k], 1e3 * med[k] / px))
    lines.append("")
    lines.append("Count and trace launches over the five `--buildings` launches on the same maps in the same run: %.2f "
                 "(medians of %d rounds of %d calls each; one process, one run)."
                 % ((med["count"] + med["trace"]) / med["table"], rounds, iters))
    lines.append("")
    lines.append("Per kernel name, one bracketed call (the brackets' events add their own overhead; a name launched several "
                 "times is summed): " + ", ".join("`%s` %.1f µs in %d" % (k, v[0], v[1]) for k, v in sorted({**kc, **ks}.items()))
                 + ".")
    lines.append("")
    lines.append("`utils.polygons.building_polygons` (labelling, count, the one read-back, trace, the arrays copied back and "
                 "grouped into Python lists), host clock, the second call: %.1f ms for the batch.  Checks at this size "
                 "(2A per root against the table's areas, ring count against scipy's component counts, even-odd "
                 "rasterisation of tile 0): %s." % (1e3 * t_module, "passed" if ok else "FAILED"))
    lines.append("")
    return bool(ok)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_polygons.py measures on the MI355X; there is no CPU fallback")
    lines = ["# Cost of the building outlines (`--polygons`)", "",
             "One MI355X (%s), `python scripts/bench_polygons.py --iters %d --rounds %d`, one process.  Device events around "
             "%d calls after warm-up, the legs alternating within each round.  Recorded, not gated: the feature is off by "
             "default and a run that does not ask for it launches nothing new.  No cost was fixed in advance and there is no "
             "host comparator; the yardstick is the `--buildings` launches on the same input in the same run "
             "(`profiles/buildings_cost.md` has the earlier figure)." % (
                 torch.cuda.get_device_name(0), a.iters, a.rounds, a.iters), ""]
    ok = bench_shape("xBD-like tiles", *tiles_1024(8), a.iters, a.rounds, lines)
    ok = bench_shape("blob scene", *scene_4096(), a.iters, a.rounds, lines) and ok
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the traced rings fail a check")


if __name__ == "__main__":
    main()
