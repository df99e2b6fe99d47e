"""Cost of predicting a scene at other scales (csrc/resize.hip, scene.ScenePredictor.predict(scales=...)) next to the scene
launches and forward passes recorded in profiles/scene_cost.md, and next to Pillow on the host: a record, not a gate.

    timeout -k 10 900 python scripts/bench_resize.py [--iters 20] [--rounds 3] [--scales 0.5,0.75,1.25,2] [--no-model]
                                                     [--out profiles/resize_cost.md]

One process, one 4096 x 4096 pre/post pair of uniform noise (the arithmetic does not depend on the content), 5 map channels.
Per scale s, on resident tables and outputs, event-timed after warm-up, the legs alternating within every round:
  resize_u8     xv2_resize_u8 of one scene to scaled_size(4096, 4096, s): reads 3 H W bytes, writes 3 Hs Ws (a pair costs two)
  resize_f32    xv2_resize_f32 of the [5, Hs, Ws] maps onto the [5, 4096, 4096] sum in accumulate mode: reads 20 Hs Ws bytes,
                reads and writes 20 H W
and once per run xv2_translate_u8 of the same scene (reads and writes 3 H W bytes): the uint8 streaming yardstick.  Bytes are
algorithmic, computed from the shapes; rates are set against the HBM figures of the MI355X (8.0 TB/s peak, 6.3 TB/s achievable
by a float4 copy).  Then Pillow's Image.resize on the host for the same resize (host clock, one call), with the GPU image compared
byte for byte; and, unless --no-model, ScenePredictor.predict of the siamese resnet50 damage model (eval, --precision 16, window
1024, overlap 256, batch 4) at scales (1,) and (s,): the forward passes grow with s^2.  Writes the record as markdown and prints
it."""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_buildings import kernel_times, timed  # noqa: E402,F401
from xview2_amd import _capi, ops, resize, scene  # noqa: E402

C = 5
HBM_PEAK, HBM_COPY = 8.0, 6.3      # TB/s


def recorded_scene_cost():
    """(ms of the three scene launches, ms of the resnet50 forward passes) from profiles/scene_cost.md, or None"""
    try:
        text = open(os.path.join(ROOT, "profiles", "scene_cost.md")).read()
    except OSError:
        return None
    m = re.search(r"The three launches take ([0-9.]+) ms per scene next to ([0-9.]+) ms of network forward passes", text)
    return (float(m.group(1)), float(m.group(2))) if m else None


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--scales", default="0.5,0.75,1.25,2")
    p.add_argument("--no-model", action="store_true")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_cost.md"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scripts/bench_resize.py measures on the MI355X; there is no CPU fallback")
    from PIL import Image
    dev = torch.device("cuda", 0)
    H = W = 4096
    g = torch.Generator(device=dev).manual_seed(7)
    pre = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    post = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    pre_host = pre.cpu().numpy()
    total = torch.zeros((C, H, W), dtype=torch.float32, device=dev)
    scales = resize.check_scales(tuple(float(v) for v in a.scales.split(",")))

    # the uint8 yardstick of profiles/align_cost.md on this scene
    shift = torch.tensor([[3, -5]], dtype=torch.int32, device=dev)
    moved = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)

    def translate():
        _capi.call("xv2_translate_u8", pre, 1, H, W, 3, shift, moved)

    for _ in range(2):
        translate()
    torch.cuda.synchronize()
    t_tr = statistics.median(timed(translate, a.iters) for _ in range(a.rounds))
    r_tr = 1e-6 * 6.0 * H * W / t_tr

    model = None
    if not a.no_model:
        import main as cli
        from xview2_amd.lightning import Model
        from xview2_amd.weights import deterministic_init_
        ops.MATH_MODE = ops.MATH_BF16
        ops.set_storage_dtype(torch.bfloat16)
        torch.manual_seed(0)
        model = Model(cli.build_parser().parse_args(["--encoder", "resnet50", "--type", "post", "--dmg_model", "siamese",
                                                     "--loss_str", "focal+dice", "--results", "."]))
        deterministic_init_(model.model, 1)
        model.to(dev).eval()
        predictor = scene.ScenePredictor(model, window=1024, overlap=256, batch=4)
        predictor.predict(pre[:1024, :1024].contiguous(), post[:1024, :1024].contiguous())      # warm-up of every layer's shape
        predictor.predict(pre, post)
        t_native = min(host_clock(lambda: predictor.predict(pre, post))[0] for _ in range(2))

    lines = ["# Cost of predicting a scene at other scales (`--scales`)", "",
             "One MI355X (%s), `python scripts/bench_resize.py --iters %d --rounds %d --scales %s`, one process.  One %d x %d pair, "
             "%d map channels.  Device events around %d calls after warm-up, the legs alternating within each round; medians of "
             "the rounds.  Bytes are algorithmic.  Recorded, not gated: with the default `--scales 1` none of this runs."
             % (torch.cuda.get_device_name(0), a.iters, a.rounds, a.scales, H, W, C, a.iters), "",
             "`xv2_translate_u8` of the same scene (reads and writes 3 bytes per pixel): %.1f µs, %.2f TB/s - the uint8 streaming "
             "yardstick.  HBM: %.1f TB/s peak, %.1f TB/s achievable by a float4 copy." % (t_tr, r_tr, HBM_PEAK, HBM_COPY), "",
             "| s | size | leg | µs per call, every round | median | MB | achieved | of %.1f TB/s | of translate |" % HBM_COPY,
             "|---|---|---|---|---|---|---|---|---|"]
    host_lines, model_lines, ok = [], [], True
    for s in scales:
        Hs, Ws = scene.scaled_size(H, W, s)
        both = torch.from_numpy(np.concatenate([resize.axis_table_u8(W, Ws).ravel(), resize.axis_table_u8(H, Hs).ravel(),
                                                resize.axis_table_f32(Ws, W).ravel(), resize.axis_table_f32(Hs, H).ravel()])).to(dev)
        n = [Ws * 19, Hs * 19, W * 11, H * 11]
        xt8, yt8, xtf, ytf = torch.split(both, n)
        small = torch.empty((Hs, Ws, 3), dtype=torch.uint8, device=dev)
        maps = torch.rand((C, Hs, Ws), dtype=torch.float32, device=dev, generator=g)

        def resize_u8():
            _capi.call("xv2_resize_u8", pre, H, W, 3, xt8, yt8, Hs, Ws, small)

        def resize_f32():
            _capi.call("xv2_resize_f32", maps, C, Hs, Ws, xtf, ytf, H, W, 1, 1, total)

        legs = {"resize_u8": resize_u8, "resize_f32": resize_f32}
        nbytes = {"resize_u8": 3.0 * (H * W + Hs * Ws), "resize_f32": 4.0 * C * (Hs * Ws + 2 * H * W)}
        for fn in legs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, a.iters))
        for k in legs:
            med = statistics.median(times[k])
            rate = 1e-6 * nbytes[k] / med
            lines.append("| %g | %d x %d | %s | %s | %.1f | %.1f | %.2f TB/s | %.2f | %.2f |" % (
                s, Hs, Ws, k, ", ".join("%.1f" % t for t in times[k]), med, nbytes[k] / 1e6, rate, rate / HBM_COPY, rate / r_tr))
            print(lines[-1], flush=True)
        # Pillow on the host, and the same bytes from the GPU
        t0 = time.perf_counter()
        want = np.asarray(Image.fromarray(pre_host).resize((Ws, Hs), Image.BICUBIC))
        t_host = time.perf_counter() - t0
        equal = bool(np.array_equal(small.cpu().numpy(), want))
        ok = ok and equal
        host_lines.append("| %g | %.1f | %.0f | %s |" % (s, 1e3 * t_host, 1e6 * t_host / statistics.median(times["resize_u8"]), equal))
        if model is not None:
            predictor.predict(pre, post, scales=(s,))
            t_s = min(host_clock(lambda: predictor.predict(pre, post, scales=(s,)))[0] for _ in range(2))
            u8 = 2 * statistics.median(times["resize_u8"]) + statistics.median(times["resize_f32"])
            model_lines.append("| %g | %d | %.1f | %.2f | %.3f | %.2f %% |" % (
                s, scene.scene_windows(Hs, Ws, 1024, 256).shape[0], 1e3 * t_s, t_s / t_native, 1e-3 * u8, 0.1 * u8 / (1e3 * t_s)))
            print(model_lines[-1], flush=True)
        del small, maps, both
    lines += ["", "## Pillow on the host", "",
              "`Image.resize((w, h), Image.BICUBIC)` of the same 4096 x 4096 x 3 image, one call by the host clock (the scene "
              "would also cross PCIe twice).", "",
              "| s | Pillow, ms | times `xv2_resize_u8` | GPU bytes equal Pillow's |", "|---|---|---|---|"] + host_lines
    lines += ["", "## Next to the scene", ""]
    if model is not None:
        lines += ["`ScenePredictor.predict` of the siamese resnet50 damage model (eval, --precision 16, window 1024, overlap 256, "
                  "batch 4) by the host clock, the faster of two calls after one warm-up call.  At the native size: %.1f ms.  The forward passes grow "
                  "with the number of windows, about s^2; the three resize launches of a scale (two scenes down or up, one set "
                  "of maps back, from the medians above) stay a small share of it." % (1e3 * t_native), "",
                  "| s | windows | predict(scales=(s,)), ms | of the native prediction | two resize_u8 + one resize_f32, ms | share |",
                  "|---|---|---|---|---|---|"] + model_lines + [""]
    rec = recorded_scene_cost()
    if rec is not None:
        lines.append("profiles/scene_cost.md records %.3f ms for the three scene launches (gather, blend, finalize) and %.1f ms of "
                     "resnet50 forward passes over a scene of the native size." % rec)
    lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    if not ok:
        raise SystemExit("the GPU image differs from Pillow's")


if __name__ == "__main__":
    main()
