"""Cost of registering the post scene to the pre scene (csrc/align.hip) next to the scene launches and forward passes
recorded in profiles/scene_cost.md, and next to the numpy restatement on the host.

    timeout -k 10 900 python scripts/bench_align.py [--iters 10] [--rounds 3] [--radii 8,16,32] [--out profiles/align_cost.md]

One process.  The pair is a 4096 x 4096 scene of uniform noise and the same scene moved by (3, -5) with +-6 of noise added
(the arithmetic does not depend on the content).  Per radius R with T = 128, event-timed after warm-up, the legs alternating
within every round:
  estimate   xv2_align_estimate on a resident workspace and resident outputs: three launches
  translate  xv2_translate_u8 of the post scene by the device shift the estimate wrote
Then the launch-bracketing profiler's time per kernel, scene.align_pair by the host clock, and the restatement of
tests/align_ref.py on a 512 x 512 crop of the pair, which the GPU tables of the same crop are compared with; its time is
scaled by the ratio of the shift-pixel products.  Writes the record as markdown to --out and prints it."""
import argparse
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import align_ref as AR  # noqa: E402
from bench_buildings import kernel_times, timed  # noqa: E402
from xview2_amd import _capi, ops, scene  # noqa: E402

T = 128
CROP = 512


def recorded_scene_cost():
    """(ms of the three scene launches, ms of the resnet50 forward passes) from profiles/scene_cost.md, or None"""
    try:
        text = open(os.path.join(ROOT, "profiles", "scene_cost.md")).read()
    except OSError:
        return None
    m = re.search(r"The three launches take ([0-9.]+) ms per scene next to ([0-9.]+) ms of network forward passes", text)
    return (float(m.group(1)), float(m.group(2))) if m else None


def bench_radius(pre, post, R, iters, rounds, lines):
    dev = pre.device
    B, H, W, _ = pre.shape
    D = 2 * R + 1
    nby, nbx = AR.grid(H, W, R, T)
    ws = torch.empty(int(_capi.query("xv2_align_workspace", B, H, W, R, T)), dtype=torch.uint8, device=dev)
    bs = torch.empty((B, nby, nbx, D, D), dtype=torch.int32, device=dev)
    sad = torch.empty((B, D, D), dtype=torch.int64, device=dev)
    bsh = torch.empty((B, nby, nbx, 2), dtype=torch.int32, device=dev)
    sh = torch.empty((B, 2), dtype=torch.int32, device=dev)
    out = torch.empty_like(post)

    def estimate():
        _capi.call("xv2_align_estimate", pre, post, B, H, W, R, T, ws, bs, sad, bsh, sh)

    def translate():
        _capi.call("xv2_translate_u8", post, B, H, W, 3, sh, out)

    legs = {"estimate": estimate, "translate": translate}
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    ks = kernel_times(estimate)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, info = scene.align_pair(pre[0], post[0], R, T)
    torch.cuda.synchronize()
    t_module = time.perf_counter() - t0
    assert torch.equal(info["shift"], sh) and torch.equal(info["sad"], sad)
    px = (H - 2 * R) * (W - 2 * R)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append("## R = %d (%d shifts, %d x %d tiles of %d)" % (R, D * D, nby, nbx, T))
    lines.append("")
    lines.append("Shift found: (%d, %d); %d of %d tiles agree." % (int(sh[0, 0]), int(sh[0, 1]),
                                                                  int((bsh == sh.view(B, 1, 1, 2)).all(dim=3).sum()), nby * nbx))
    lines.append("")
    lines.append("| leg | µs per call, %d rounds of %d calls | median | |" % (rounds, iters))
    lines.append("|---|---|---|---|")
    lines.append("| estimate | %s | %.1f | %.2f x 10^12 absolute differences per second |" % (
        ", ".join("%.1f" % t for t in times["estimate"]), med["estimate"], 1e-6 * px * D * D / med["estimate"]))
    lines.append("| translate | %s | %.1f | %.2f TB/s read and written |" % (
        ", ".join("%.1f" % t for t in times["translate"]), med["translate"], 1e-6 * 6.0 * H * W / med["translate"]))
    lines.append("")
    lines.append("Per kernel, one bracketed estimate (the brackets' events add their own overhead): " +
                 ", ".join("`%s` %.1f µs" % kv for kv in sorted(ks.items())) + ".")
    lines.append("")
    lines.append("`scene.align_pair` (allocations, estimate, translate), host clock, one call after those above: %.2f ms."
                 % (1e3 * t_module))
    # the restatement on a crop, and the GPU on the same crop
    cp, cq = pre[:, :CROP, :CROP].contiguous(), post[:, :CROP, :CROP].contiguous()
    t0 = time.perf_counter()
    want = AR.estimate(cp[0].cpu().numpy(), cq[0].cpu().numpy(), R, T)
    t_host = time.perf_counter() - t0
    got = ops.align_estimate(cp, cq, R, T)
    equal = all(np.array_equal(g[0].cpu().numpy().astype(np.int64), w) for g, w in zip(got, want))
    scale = px / float((CROP - 2 * R) ** 2)
    lines.append("")
    lines.append("numpy restatement (tests/align_ref.estimate) on a %d x %d crop, host: %.2f s; scaled by the interiors' ratio "
                 "(%.1f) to the scene: %.0f s, %.0f times the estimate.  GPU tables of the crop equal to it: %s."
                 % (CROP, CROP, t_host, scale, t_host * scale, 1e6 * t_host * scale / med["estimate"], equal))
    lines.append("")
    return equal, med


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--radii", default="8,16,32")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_align.py measures on the MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    H = W = 4096
    g = torch.Generator(device=dev).manual_seed(5)
    pre = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    jitter = torch.randint(-6, 7, (1, H, W, 3), dtype=torch.int16, device=dev, generator=g)
    post = (torch.roll(pre, (3, -5), (1, 2)).to(torch.int16) + jitter).clamp_(0, 255).to(torch.uint8)
    lines = ["# Cost of registering the post scene to the pre scene (`--align R`)", "",
             "One MI355X (%s), `python scripts/bench_align.py --iters %d --rounds %d --radii %s`, one process.  One %d x %d pair, "
             "T = %d.  Device events around %d calls after warm-up, the legs alternating within each round.  Recorded, not gated: "
             "the feature is off by default and a run that does not ask for it launches nothing new."
             % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.radii, H, W, T, a.iters), ""]
    ok, meds = True, {}
    for R in (int(v) for v in a.radii.split(",")):
        equal, meds[R] = bench_radius(pre, post, R, a.iters, a.rounds, lines)
        ok = ok and equal
    rec = recorded_scene_cost()
    lines.append("## Next to the scene")
    lines.append("")
    if rec is None:
        lines.append("profiles/scene_cost.md holds no record to compare with.")
    else:
        lines.append("profiles/scene_cost.md records %.3f ms for the three scene launches (gather, blend, finalize) and %.1f ms of "
                     "resnet50 forward passes over a scene of the same size." % rec)
        lines.append("")
        lines.append("| R | estimate + translate, ms | of the scene launches | of the forward passes |")
        lines.append("|---|---|---|---|")
        for R, m in meds.items():
            ms = 1e-3 * (m["estimate"] + m["translate"])
            lines.append("| %d | %.3f | %.2f x | %.2f %% |" % (R, ms, ms / rec[0], 100.0 * ms / rec[1]))
    lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU tables differ from the restatement")


if __name__ == "__main__":
    main()
