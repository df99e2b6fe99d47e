"""Cost of simplifying the building outlines (csrc/simplify.hip) next to counting and tracing them (csrc/polygons.hip) on the
same label map in the same run, and what the tolerance saves behind the device: vertices, file size and host time.

    timeout -k 10 900 python scripts/bench_simplify.py [--iters 100] [--rounds 3] [--out profiles/simplify_cost.md]

One process.  The 4096 x 4096 blob scene of scripts/bench_polygons.py (some 85 000 rings, most of them small).  Event-timed
after warm-up, the legs alternating within every round, all on preallocated buffers:
  count      the two launches of xv2_polygon_count
  trace      the launches of xv2_polygon_trace with the totals the count gave
  T = ...    the three launches of xv2_polygon_simplify on the traced table, at T = 0.5, 1 and 2 pixels
  T = 1, ... the same at T = 1 on the table's rings of at most 64 vertices alone (the kernel's register path) and on the
             longer ones alone (its whole-block path), to see where the time goes
Then once per tolerance the launch-bracketing profiler's time per kernel name, the vertices kept, the rings by flag, and by
the host clock the module call utils.polygons.building_polygons (device work, the read-back, the grouping into Python lists)
and utils.polygons.write_geojson with the size of the file, each next to the same call without a tolerance.  The result is
checked at the timed size without the recursive restatement: the kept vertices are a subsequence of each ring's own that
starts with its first vertex, column 4 is their shoelace sum, and a sample of rings equals tests/simplify_ref.py.  Writes
the record as markdown to --out and prints it."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import simplify_ref as S  # noqa: E402
from bench_buildings import scene_4096, timed  # noqa: E402
from bench_polygons import kernel_times  # noqa: E402
from xview2_amd import _capi, ops  # noqa: E402
from xview2_amd.utils import buildings, polygons  # noqa: E402

TOLERANCES = (0.5, 1.0, 2.0)


def check(rings_h, verts_h, out_r, out_v, q, sample=400):
    """the structural checks on every ring, the restatement on a sample of them"""
    ok = np.array_equal(out_r[:, 3], np.cumsum(out_r[:, 2]) - out_r[:, 2])
    ok = ok and np.array_equal(out_r[:, [0, 1, 5, 6]], rings_h[:, [0, 1, 5, 6]])
    x, y = out_v[:, 0].astype(np.int64), out_v[:, 1].astype(np.int64)
    last = out_r[:, 3] + out_r[:, 2] - 1
    nxt = np.arange(len(out_v)) + 1
    nxt[last] = out_r[:, 3]                                    # (every traced ring keeps at least 3 vertices)
    cross = x * y[nxt] - x[nxt] * y
    ok = ok and np.array_equal(np.add.reduceat(cross, out_r[:, 3]), out_r[:, 4])
    ok = ok and np.array_equal(out_v[out_r[:, 3]], verts_h[rings_h[:, 3]])
    step = max(1, len(rings_h) // sample)
    vl, ol = verts_h.tolist(), out_v.tolist()
    for r, o in zip(rings_h[::step].tolist(), out_r[::step].tolist()):
        kept, flag, _ = S.simplify_ring(vl[r[3]:r[3] + r[2]], q)
        ok = ok and [list(p) for p in kept] == ol[o[3]:o[3] + o[2]] and flag == o[7]
    big = int(np.argmax(rings_h[:, 2]))                        # and the longest ring
    r, o = rings_h[big].tolist(), out_r[big].tolist()
    ok = ok and [list(p) for p in S.simplify_ring(vl[r[3]:r[3] + r[2]], q)[0]] == ol[o[3]:o[3] + o[2]]
    return bool(ok)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_simplify.py measures on the MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    loc_np, dmg_np = scene_4096()
    B, H, W = loc_np.shape
    loc, dmg = torch.from_numpy(loc_np).to(dev), torch.from_numpy(dmg_np).to(dev)
    pre, post = ops.postprocess(loc, dmg, components=True, rate=0, workspace=ops.postprocess_workspace(B, H, W, True, dev))
    labels = ops.label_components(pre)
    counts_h = ops.polygon_count(labels).cpu().numpy()
    E, V = int(counts_h[:, 0].sum()), int(counts_h[:, 1].sum())
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)     # noqa: E731
    ws_c = u8(_capi.query("xv2_polygon_count_workspace", B, H, W))
    ws_t = u8(_capi.query("xv2_polygon_trace_workspace", B, H, W, E))
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    rings = torch.empty((V // 4, 8), dtype=torch.int64, device=dev)
    verts = torch.empty((V, 2), dtype=torch.int32, device=dev)
    ring_count = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _capi.call("xv2_polygon_trace", labels, B, H, W, E, V, ws_t, rings, verts, ring_count, status)
    n = int(ring_count.sum())
    ws_s = u8(_capi.query("xv2_polygon_simplify_workspace", n, V))
    out_rings = torch.empty((n, 8), dtype=torch.int64, device=dev)
    out_verts = torch.empty((V, 2), dtype=torch.int32, device=dev)
    out_total = torch.empty((1,), dtype=torch.int64, device=dev)
    qs = [polygons.quantise_tolerance(T) for T in TOLERANCES]
    legs = {
        "count": lambda: _capi.call("xv2_polygon_count", labels, B, H, W, ws_c, counts),
        "trace": lambda: _capi.call("xv2_polygon_trace", labels, B, H, W, E, V, ws_t, rings, verts, ring_count, status),
    }
    for T, q in zip(TOLERANCES, qs):
        legs["T = %g" % T] = (lambda q=q: _capi.call("xv2_polygon_simplify", rings, verts, n, V, q, ws_s, out_rings, out_verts,
                                                     out_total))
    rings_h, verts_h = rings[:n].cpu().numpy(), verts.cpu().numpy()
    parts = {}
    for name, pick in (("T = 1, rings <= 64", rings_h[:, 2] <= 64), ("T = 1, rings > 64", rings_h[:, 2] > 64)):
        part = rings_h[pick].copy()
        idx = np.concatenate([np.arange(o, o + k) for o, k in part[:, [3, 2]].tolist()] or [np.zeros(0, np.int64)])
        part[:, 3] = np.cumsum(part[:, 2]) - part[:, 2]
        r_d, v_d = torch.from_numpy(part).to(dev), torch.from_numpy(np.ascontiguousarray(verts_h[idx])).to(dev)
        bufs = (u8(_capi.query("xv2_polygon_simplify_workspace", len(part), len(idx))), torch.empty_like(r_d),
                torch.empty_like(v_d), torch.empty((1,), dtype=torch.int64, device=dev))
        parts[name] = (len(part), len(idx))
        if len(part):
            legs[name] = (lambda r_d=r_d, v_d=v_d, bufs=bufs: _capi.call(
                "xv2_polygon_simplify", r_d, v_d, r_d.shape[0], v_d.shape[0], 16, bufs[0], bufs[1], bufs[2], bufs[3]))
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, a.iters))
    med = {k: statistics.median(times[k]) for k in legs}
    assert int(status.item()) == 0
    ok = True
    per_q = []
    tmp = tempfile.mkdtemp()
    rows, lab = buildings.building_table(pre, post, loc, return_labels=True)
    records = buildings.to_records(rows[0], H, W)

    def host(T):
        """(seconds in building_polygons, seconds in write_geojson, bytes) of the second call"""
        path = os.path.join(tmp, "scene_%g.geojson" % T)
        out = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            polys = polygons.building_polygons(pre, lab, T)[0]
            t1 = time.perf_counter()
            polygons.write_geojson(path, polys, records)
            out = (t1 - t0, time.perf_counter() - t1, os.path.getsize(path))
        os.remove(path)
        return out
    plain = host(0.0)
    for T, q in zip(TOLERANCES, qs):
        ks = kernel_times(legs["T = %g" % T])
        o_r, total = out_rings.cpu().numpy(), int(out_total.item())
        o_v = out_verts[:total].cpu().numpy()
        ok = check(rings_h, verts_h, o_r, o_v, q) and ok
        per_q.append((T, q, total, np.bincount(o_r[:, 7], minlength=3).tolist(), ks, host(T)))
    os.rmdir(tmp)
    lines = ["# Cost of simplifying the building outlines (`--polygons --simplify T`)", "",
             "One MI355X (%s), `python scripts/bench_simplify.py --iters %d --rounds %d`, one process.  Device events around %d "
             "calls after warm-up, the legs alternating within each round.  Recorded, not gated: the feature is off by default "
             "and a run that does not ask for it launches nothing new.  No cost was fixed in advance; the yardstick is the count "
             "and trace launches that the simplification follows, on the same label map in the same run."
             % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.iters), "",
             "## blob scene: B = %d, %d x %d" % (B, H, W), "",
             "Boundary edges %d, vertices %d, rings %d, buildings %d.  Vertices per ring: median %d, 99th percentile %d, largest "
             "%d; rings above 64 vertices (taken by a whole block): %d, above 1024 (state in global memory): %d."
             % (E, V, n, len(records), int(np.median(rings_h[:, 2])), int(np.percentile(rings_h[:, 2], 99)),
                int(rings_h[:, 2].max()), int((rings_h[:, 2] > 64).sum()), int((rings_h[:, 2] > 1024).sum())), "",
             "| leg | µs per call, %d rounds of %d calls | median | over count + trace |" % (a.rounds, a.iters),
             "|---|---|---|---|"]
    base = med["count"] + med["trace"]
    for k in legs:
        lines.append("| %s | %s | %.1f | %s |" % (k, ", ".join("%.1f" % t for t in times[k]), med[k],
                                                  "%.2f" % (med[k] / base) if k.startswith("T") else ""))
    lines += ["", "The two partial legs run the same three launches on a table of their own: %s."
              % "; ".join("`%s` %d rings with %d vertices" % (k, v[0], v[1]) for k, v in parts.items())]
    lines += ["", "| T (q) | vertices kept | of traced | rings by flag 0 / 1 / 2 | `building_polygons` ms | `write_geojson` ms | "
              "GeoJSON MB |", "|---|---|---|---|---|---|---|",
              "| off | %d | 1.000 | %d / 0 / 0 | %.1f | %.1f | %.2f |" % (V, n, 1e3 * plain[0], 1e3 * plain[1], plain[2] / 1e6)]
    for T, q, total, flags, ks, hst in per_q:
        lines.append("| %g (%d) | %d | %.3f | %d / %d / %d | %.1f | %.1f | %.2f |"
                     % (T, q, total, total / V, flags[0], flags[1], flags[2], 1e3 * hst[0], 1e3 * hst[1], hst[2] / 1e6))
    lines += ["", "The host columns are the second of two calls by the host clock: `building_polygons` is the labelled map to "
              "Python lists (count, trace, the simplify launches when asked for, the read-back, the grouping), `write_geojson` "
              "the JSON text of one feature per building with its table row.", ""]
    for T, q, total, flags, ks, hst in per_q:
        lines.append("Per kernel name at T = %g, one bracketed call (the brackets' events add their own overhead): %s."
                     % (T, ", ".join("`%s` %.1f µs" % (k, v[0]) for k, v in sorted(ks.items()))))
        lines.append("")
    lines.append("Checks at this size (offsets, first vertices, column 4 against the shoelace sum of the kept vertices on every "
                 "ring; the recursive restatement on every %d-th ring and on the longest): %s."
                 % (max(1, n // 400), "passed" if ok else "FAILED"))
    lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the simplified rings fail a check")


if __name__ == "__main__":
    main()
