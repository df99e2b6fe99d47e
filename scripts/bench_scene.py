"""Cost of whole-scene prediction (csrc/scene.hip, xview2_amd/scene.py): a record, not a gate.

    python scripts/bench_scene.py [--size 4096] [--window 1024] [--overlap 256] [--batch 4] [--iters 20] [--rounds 3]
                                  [--out profiles/scene_cost.md] [--commit TEXT] [--no-model]

One 4096 x 4096 pre/post scene, 5 softmax channels.  Event-timed after warm-up, the legs alternating `--rounds` times:
  1. the three launches of a scene - the gather of every batch of windows, the blend of every batch (logits from a fixed
     random buffer) and the finalize - each alone and all together, with the bytes each must move (computed from the
     shapes below) over its time;
  2. xv2_bn_act_forward, the project's plain streaming kernel, on an fp32 tensor of a window batch's size in the same run:
     the bytes/s this box gives a kernel that reads and writes every element once;
  3. the forward passes of the siamese resnet50 damage model (eval, --precision 16) over the same batches of windows.
Writes the table as markdown and prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xview2_amd import _capi, ops, scene  # noqa: E402

C = 5


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters      # ms


def covered(tab, n, H, W):
    """scene pixels the windows of one call cover (the blend reads and writes their accumulators once)"""
    m = np.zeros((H, W), dtype=bool)
    for y0, x0 in tab:
        m[y0:y0 + n, x0:x0 + n] = True
    return int(m.sum())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=4096)
    p.add_argument("--window", type=int, default=1024)
    p.add_argument("--overlap", type=int, default=256)
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "scene_cost.md"))
    p.add_argument("--commit", type=str, default=None)
    p.add_argument("--no-model", action="store_true")
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scene: no GPU (timings are only meaningful on the MI355X)")
    dev = torch.device("cuda", 0)
    H = W = a.size
    n, ov, B = a.window, a.overlap, a.batch
    g = torch.Generator().manual_seed(1)
    pre = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    post = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    tab_h = scene.scene_windows(H, W, n, ov)
    tab = torch.from_numpy(tab_h).to(dev)
    K = tab.shape[0]
    batches = [(k0, min(B, K - k0)) for k0 in range(0, K, B)]
    wy = torch.from_numpy(scene.axis_normaliser(H, n, ov)).to(dev)
    wx = torch.from_numpy(scene.axis_normaliser(W, n, ov)).to(dev)
    wins = torch.empty((B, n, n, 6), dtype=torch.uint8, device=dev)
    logits = torch.randn((B, C, n, n), generator=g).to(dev)
    acc = torch.zeros((C, H, W), dtype=torch.float32, device=dev)

    def gather():
        for k0, m in batches:
            scene.gather_windows(pre, post, tab[k0:k0 + m], n, out=wins[:m])

    def blend():
        for k0, m in batches:
            scene.blend(logits[:m], scene.SOFTMAX, tab[k0:k0 + m], ov, acc)

    def finalize():
        scene.finalize(acc, wy, wx)

    def all_three():
        acc.zero_()
        for k0, m in batches:
            scene.gather_windows(pre, post, tab[k0:k0 + m], n, out=wins[:m])
            scene.blend(logits[:m], scene.SOFTMAX, tab[k0:k0 + m], ov, acc)
        scene.finalize(acc, wy, wx)

    npix, ch = B * n * n, 16      # the streaming yardstick: 2 x 4 bytes per element
    y = torch.randn((npix, ch), generator=g).to(dev)
    z = torch.empty_like(y)
    sc, sh = torch.ones(ch, device=dev), torch.zeros(ch, device=dev)

    def bn_act():
        _capi.call("xv2_bn_act_forward", y, ch, sc, sh, None, ch, ops.ACT_RELU, z, ch, npix, ch, ops._dt(y))

    bytes_ = {
        "gather": 2 * K * n * n * 6,
        "blend": sum(4 * m * C * n * n + 8 * C * covered(tab_h[k0:k0 + m], n, H, W) for k0, m in batches),
        "finalize": 8 * C * H * W + 4 * (H + W),
        "bn_act_fwd": 8 * npix * ch,
    }
    bytes_["all three"] = bytes_["gather"] + bytes_["blend"] + bytes_["finalize"] + 4 * C * H * W      # and the zeroing
    legs = [("gather", gather), ("blend", blend), ("finalize", finalize), ("all three", all_three), ("bn_act_fwd", bn_act)]
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
        gather()

        def forward():
            with torch.no_grad():
                for k0, m in batches:
                    model(ops.DeviceImage(wins[:m]))

        legs.append(("resnet50 forward", forward))
    rows = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            rows[name].append(timed(fn, 3 if name == "resnet50 forward" else a.iters))
            print("%-18s %.3f ms" % (name, rows[name][-1]), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    rate = {k: bytes_[k] / med[k] / 1e9 for k in bytes_}      # TB/s
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    lines = [
        "# Cost of whole-scene prediction (`xview2_amd.scene`)", "",
        "One MI355X, `python scripts/bench_scene.py`, taken at %s.  Recorded, not gated.  A %d x %d pre/post scene, window %d, "
        "overlap %d: %d windows in batches of %d, %d softmax channels.  Device events after warm-up, %d calls per timing "
        "(3 for the network), the legs alternating %d times.  Bytes are algorithmic: the gather reads and writes 6 bytes per "
        "window pixel; the blend reads every logit once and reads and writes the accumulators of the pixels a call covers; "
        "the finalize reads and writes every accumulator." % (commit, H, W, n, ov, K, B, C, a.iters, a.rounds), "",
        "| leg, per scene | ms, every round | MB | achieved |", "|---|---|---|---|"]
    for name, _ in legs:
        lines.append("| %s | %s | %s | %s |" % (
            name if name != "bn_act_fwd" else "`xv2_bn_act_forward`, %d x %d fp32 (one call)" % (npix, ch),
            ", ".join("%.3f" % v for v in rows[name]),
            "%.1f" % (bytes_[name] / 1e6) if name in bytes_ else "-",
            "%.2f TB/s" % rate[name] if name in rate else "-"))
    lines.append("")
    if model is not None:
        lines.append("The three launches take %.3f ms per scene next to %.1f ms of network forward passes over the same windows "
                     "(siamese resnet50 damage model, eval, --precision 16): %.2f %%." % (
                         med["all three"], med["resnet50 forward"], 100.0 * med["all three"] / med["resnet50 forward"]))
        lines.append("")
    for k in ("gather", "blend", "finalize"):
        lines.append("- %s: %.2f of `xv2_bn_act_forward`'s %.2f TB/s." % (k, rate[k] / rate["bn_act_fwd"], rate["bn_act_fwd"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    print(json.dumps({"commit": commit, "ms": rows, "median_ms": med, "bytes": bytes_, "tbytes_per_s": rate}))


if __name__ == "__main__":
    main()
