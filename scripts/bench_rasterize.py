"""Cost of the polygon fill (csrc/rasterize.hip) next to its host packing and next to Pillow's ImageDraw.polygon on the host.

    timeout -k 10 900 python scripts/bench_rasterize.py [--iters 20] [--rounds 3] [--out profiles/rasterize_cost.md]
    python scripts/bench_rasterize.py --cpu-only        # the figures that need no GPU; the record says that no device run was made

One process.  Shapes: a generated xBD-like 1024 x 1024 tile of about 300 rotated quads and L-shapes (float vertices, values
1..4) at B = 1, 8 and 32 under rule "reference", and one 4096-vertex polygon that covers a 1024 x 1024 tile under rule "exact".
Per shape, event-timed after warm-up, the shapes alternating within every round: the whole call xv2_rasterize_polygons (host
validation of the tables, clear, cover, resolve) on resident tables and preallocated buffers.  Then once per shape the
launch-bracketing profiler's time per kernel, utils.rasterize.pack by the host clock, and the host alternative: one
ImageDraw.polygon per feature on the same rounded vertices.  The GPU map is compared with the numpy restatement
(tests/rasterize_ref.py) on tile 0, and on a 32-row strip of the large polygon.

CPU-only figures: the share of pixels on which rule "reference" differs from that Pillow fill on the bench tile, and the
differing pixels of 400 random small polygons (rotated quads and 3- to 8-gons, 4 to 30 px), with whether this project's rule
is a subset of Pillow's fill on every one.  Reads nothing outside the repository."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import buildings_ref as BR  # noqa: E402
import rasterize_ref as RR  # noqa: E402
from xview2_amd.utils import rasterize as RZ  # noqa: E402

SIZE = 1024


def _unit(seed, n):
    return BR._hash(seed, (n,), 1 << 20).astype(np.float64) / (1 << 20)


def xbd_tile(seed, n=300, size=SIZE):
    """about n rotated quads and L-shapes, 8 to 60 px, as (polygon, value) pairs with float vertices"""
    u = _unit(seed, 6 * n).reshape(n, 6)
    feats = []
    for i in range(n):
        cx, cy = size * u[i, 0], size * u[i, 1]
        a, b, th = 4 + 26 * u[i, 2], 4 + 26 * u[i, 3], np.pi * u[i, 4]
        if u[i, 5] < 0.7:
            local = [(-a, -b), (a, -b), (a, b), (-a, b)]
        else:
            local = [(-a, -b), (a, -b), (a, 0.1 * b), (0.2 * a, 0.1 * b), (0.2 * a, b), (-a, b)]
        c, s = np.cos(th), np.sin(th)
        feats.append(({"exterior": [[cx + c * x - s * y, cy + s * x + c * y] for x, y in local], "holes": []}, 1 + i % 4))
    return feats


def big_polygon(n=4096, size=SIZE):
    """a star of n vertices whose extent is the whole tile"""
    t = 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, 0.5 * size + 3.0, 0.33 * size)
    return [({"exterior": np.stack([size / 2 + r * np.cos(t), size / 2 + r * np.sin(t)], axis=1).tolist(), "holes": []}, 3)]


def small_polygons(n=400):
    """rotated quads and 3- to 8-gons of 4 to 30 px on 48 x 48 maps"""
    out = []
    for i in range(n):
        u = _unit(5000 + i, 24)
        if i % 2 == 0:
            a, b, th = 2 + 13 * u[0], 2 + 13 * u[1], np.pi * u[2]
            c, s = np.cos(th), np.sin(th)
            pts = [[24 + c * x - s * y, 24 + s * x + c * y] for x, y in ((-a, -b), (a, -b), (a, b), (-a, b))]
        else:
            m = 3 + int(u[0] * 6)
            ang = 2 * np.pi * np.sort(u[2:2 + m])
            rad = (2 + 13 * u[1]) * (0.5 + 0.5 * u[10:10 + m])
            pts = np.stack([24 + rad * np.cos(ang), 24 + rad * np.sin(ang)], axis=1).tolist()
        out.append({"exterior": pts, "holes": []})
    return out


def pillow_fill(feats, H, W):
    """the host alternative: one ImageDraw.polygon per feature on the exterior rounded as rule "reference" rounds it"""
    from PIL import Image, ImageDraw
    img = Image.new("L", (W, H), 0)
    draw = ImageDraw.Draw(img)
    for p, v in feats:
        draw.polygon([tuple(q) for q in RZ.quantise(p["exterior"], "reference").tolist()], fill=int(v))
    return np.asarray(img)


def cpu_figures(lines):
    feats = xbd_tile(900)
    pillow_fill(feats, SIZE, SIZE)                            # the first call pays Pillow's imports
    RZ.pack([feats], SIZE, SIZE, "reference")
    t0 = time.perf_counter()
    T = RZ.pack([feats], SIZE, SIZE, "reference")
    t_pack = time.perf_counter() - t0
    ours = RR.ref(T, SIZE, SIZE)[0]
    t0 = time.perf_counter()
    pil = pillow_fill(feats, SIZE, SIZE)
    t_pil = time.perf_counter() - t0
    diff = int((ours != pil).sum())
    lines += ["## Against Pillow on the host (no GPU needed)", "",
              "Bench tile (%d features, 1024 x 1024): rule `reference` differs from one `ImageDraw.polygon` per feature on %d "
              "pixels = %.3f %% of the tile, %.2f %% of Pillow's %d painted pixels; pixels this rule paints and Pillow does not: %d."
              % (len(feats), diff, 100.0 * diff / ours.size, 100.0 * diff / max(int((pil != 0).sum()), 1), int((pil != 0).sum()),
                 int(((ours != 0) & (pil == 0)).sum())), ""]
    n_diff = n_pil = 0
    subset = True
    polys = small_polygons()
    for p in polys:
        o = RR.ref(RZ.pack([[(p, 1)]], 48, 48, "reference"), 48, 48)[0]
        q = pillow_fill([(p, 1)], 48, 48)
        subset = subset and not ((o != 0) & (q == 0)).any()
        n_diff += int((o != q).sum())
        n_pil += int((q != 0).sum())
    lines += ["%d random small polygons (rotated quads and 3- to 8-gons, 4 to 30 px): %d differing pixels of Pillow's %d; this "
              "rule's fill a subset of Pillow's in every case: %s.  (Pillow, like cv2.fillPoly, also draws the edge lines; "
              "cv2 is not installed, so the difference against cv2 is not measured.)" % (len(polys), n_diff, n_pil, subset), "",
              "Host clock on this machine, bench tile, one call each: `pack` %.2f ms, Pillow fill %.2f ms." % (
                  1e3 * t_pack, 1e3 * t_pil), ""]


def gpu_figures(lines, iters, rounds):
    import torch
    from xview2_amd import _capi
    from bench_buildings import kernel_times, timed
    dev = torch.device("cuda", 0)
    shapes = []
    for B in (1, 8, 32):
        shapes.append(("xBD-like tiles, B = %d" % B, [xbd_tile(900 + 7 * b) for b in range(B)], "reference"))
    shapes.append(("one 4096-vertex polygon, B = 1", [big_polygon()], "exact"))
    legs, info = {}, {}
    pillow_fill(shapes[0][1][0], SIZE, SIZE)               # the first call pays Pillow's imports
    for name, tiles, rule in shapes:
        RZ.pack(tiles[:1], SIZE, SIZE, rule)
        t0 = time.perf_counter()
        T = RZ.pack(tiles, SIZE, SIZE, rule)
        t_pack = time.perf_counter() - t0
        t0 = time.perf_counter()
        for feats in tiles:
            pillow_fill(feats, SIZE, SIZE)
        t_pil = time.perf_counter() - t0
        buf = torch.from_numpy(T.tables).to(dev)
        ws = torch.empty(int(_capi.query("xv2_rasterize_workspace", T.B, SIZE, SIZE)), dtype=torch.uint8, device=dev)
        out = torch.empty((T.B, SIZE, SIZE), dtype=torch.uint8, device=dev)
        legs[name] = (lambda T=T, buf=buf, ws=ws, out=out: _capi.call(
            "xv2_rasterize_polygons", buf, T.tables.ctypes.data, T.n_edges, T.n_features, T.n_work, T.frac_bits, T.off, T.B,
            SIZE, SIZE, ws, out))
        info[name] = (T, out, t_pack, t_pil)
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    ok = True
    lines += ["## On the device", "",
              "| shape | features | edges | work items | µs per call, %d rounds of %d calls | median | `pack` on the host, ms | "
              "Pillow on the host, ms |" % (rounds, iters), "|---|---|---|---|---|---|---|---|"]
    notes = []
    for name, fn in legs.items():
        T, out, t_pack, t_pil = info[name]
        lines.append("| %s | %d | %d | %d | %s | %.1f | %.2f | %.1f |" % (
            name, T.n_features, T.n_edges, T.n_work, ", ".join("%.1f" % t for t in times[name]), statistics.median(times[name]),
            1e3 * t_pack, 1e3 * t_pil))
        ks = kernel_times(fn)
        got = out.cpu().numpy()
        if T.n_features == 1:                     # the large polygon: a 32-row strip of its box
            f = T.features.copy()
            f[0, 5], f[0, 7] = 480, 511
            strip = RZ.Tables(np.concatenate([T.tables[:4 * T.n_edges], f.reshape(-1)]).astype(np.int32), T.n_edges, 1, 0,
                              T.frac_bits, T.off, 1)
            equal = np.array_equal(got[0, 480:512], RR.ref(strip, SIZE, SIZE)[0, 480:512])
        else:
            first = T.features[:, 0] == 0
            one = RZ.Tables(np.concatenate([T.tables[:4 * T.n_edges], T.features[first].reshape(-1)]).astype(np.int32), T.n_edges,
                            int(first.sum()), 0, T.frac_bits, T.off, 1)
            equal = np.array_equal(got[0], RR.ref(one, SIZE, SIZE)[0])
        ok = ok and equal
        notes.append("%s: %s; painted %.1f %% of the pixels; equal to the numpy restatement (tile 0, or a 32-row strip of the "
                     "large polygon): %s." % (name, ", ".join("`%s` %.1f µs" % kv for kv in sorted(ks.items())),
                                              100.0 * float((got != 0).mean()), equal))
    lines += ["", "The call includes the host's validation pass over the tables.  Per kernel below: ONE bracketed call, not "
              "repeated and not a median; the brackets' events add their own overhead, so these figures are not comparable to "
              "the medians above and may exceed them (the clear is a memset and is not bracketed):", ""] + ["* " + n for n in notes] + [""]
    return ok


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--cpu-only", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "rasterize_cost.md"))
    a = p.parse_args()
    lines = ["# Cost of the polygon fill (`utils/rasterize.py`, `utils/convert2png.py`)", ""]
    ok = True
    if a.cpu_only:
        lines += ["`python scripts/bench_rasterize.py --cpu-only`.  No MI355X run was made for this record: it holds no device "
                  "figure.", ""]
    else:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("scripts/bench_rasterize.py measures on the MI355X; --cpu-only gives the figures that need none")
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        lines += ["One MI355X (%s), `python scripts/bench_rasterize.py --iters %d --rounds %d`, one process.  Device events around "
                  "%d calls after warm-up, the shapes alternating within each round.  Recorded, not gated: nothing in training "
                  "or inference calls the fill." % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.iters), ""]
        ok = gpu_figures(lines, a.iters, a.rounds)
    cpu_figures(lines)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU map differs from the restatement")


if __name__ == "__main__":
    main()
