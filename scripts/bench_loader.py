"""Host time per batch of the training loader (data_module.DeviceAugLoader) with RandomScale on the device
(xv2_zoom_crop_u8, XV2_DEVICE_ZOOM=1) and on the host (XV2_DEVICE_ZOOM=0, the default: tile back from HBM, Pillow bicubic, crop, upload), in ONE run:

    python scripts/bench_loader.py [--tiles 32] [--batch 16] [--epochs 6] [--modes pre,post] [--probs 1.0,0.2] [--zoom device,host]

A tile tree of 1024^2 PNGs (random bytes, a few rectangular buildings per mask) is generated in a temporary directory; per mode
ONE loader decodes it once into its HBM cache (the first, untimed epoch) and every configuration then replays the same epochs
from the same random stream, so the device and the host branch take the same decisions and deliver the same bytes (checked on
the first timed batch).  Timed: the wall-clock of next(loader) on the consuming thread - what a training step waits for - and the
same plus a device synchronise (the launches' own time included); the two variants alternate epoch by epoch.  Prints one line
per configuration and a JSON summary.

Kernel durations from the trace (same batches; the device branch only, so that the trace holds no host-branch launches):
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
        python scripts/bench_loader.py --modes post --probs 1.0 --zoom device
The trace also holds the untimed first epoch (tiles / batch launches of xv2_augment_u8 at the real zoom probability, with the
few xv2_zoom_crop_u8 launches that draws): with the default 6 timed epochs that is 1 augment launch in 7.

`--autoaugment` runs another leg INSTEAD: batches per second of `--autoaugment` through the worker pipeline (DataLoader workers:
decode, crop, two PIL operations per image, upload - what DataModule builds by default) against the device path
(DeviceAugLoader(autoaugment=True): xv2_augment_u8 + xv2_autoaugment_u8, XV2_DEVICE_AUTOAUGMENT=1), same tile tree, same
`--num_workers` (worker processes there, decode threads here), for pre and post in one run:

    python scripts/bench_loader.py --autoaugment [--num_workers 8] [--tiles 32] [--batch 16] [--epochs 6] [--modes pre,post]

Timed: whole epochs on the consuming thread, a device synchronise after each batch (a training step would overlap it); the two
paths alternate epoch by epoch.  The worker path decodes its tiles every epoch and starts its workers every epoch - that is the
pipeline as it runs; the device path's first epoch (decode + upload into the HBM cache) is reported on its own line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xview2_amd.data_loading import data_module as dm, pytorch_loader as pl  # noqa: E402


def tile_tree(root, n, S=1024):
    rng = np.random.default_rng(0)
    for sub in ("images", "targets"):
        os.makedirs(os.path.join(root, "train", sub))
    for i in range(n):
        for kind in ("pre", "post"):
            img = rng.integers(1, 256, (S, S, 3), dtype=np.uint8)
            Image.fromarray(img).save(os.path.join(root, "train", "images", "t%03d_%s_disaster.png" % (i, kind)), compress_level=1)
            m = np.zeros((S, S), np.uint8)
            for _ in range(12):
                y, x = rng.integers(0, S - 60, 2)
                m[y:y + rng.integers(10, 60), x:x + rng.integers(10, 60)] = 1 if kind == "pre" else rng.integers(1, 5)
            Image.fromarray(m).save(os.path.join(root, "train", "targets", "t%03d_%s_disaster_target.png" % (i, kind)))
    csv = os.path.join(root, "index.csv")
    with open(csv, "w") as f:
        f.write("idx,1,2,3,4\n" + "".join("%d,1,0,0,0\n" % i for i in range(n)))
    return csv


def run(loader, epochs, prob, variants, seed=11):
    """-> {variant: (host seconds of every batch, host + drain seconds, the first batch's bytes, zoomed samples)}; the variants
    alternate epoch by epoch, each replaying the epoch from the same random stream"""
    draw, zoomed = pl.draw_scale, {v: 0 for v in variants}
    out = {v: ([], [], None) for v in variants}
    try:
        for epoch in range(1, epochs + 1):
            for v in variants:
                def forced(rng):
                    s = draw(rng, p=prob)
                    zoomed[v] += s is not None
                    return s
                pl.draw_scale, loader.device_zoom = forced, v == "device"
                loader.set_epoch(epoch)
                loader.rng = np.random.default_rng([seed, epoch])
                it = iter(loader)
                while True:
                    t0 = time.perf_counter()
                    b = next(it, None)
                    t1 = time.perf_counter()
                    if b is None:
                        break
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    out[v][0].append(t1 - t0)
                    out[v][1].append(t2 - t0)
                    if out[v][2] is None:
                        out[v] = out[v][:2] + ((b["image"].u8.cpu().numpy(), b["mask"].cpu().numpy()),)
    finally:
        pl.draw_scale = draw
    return {v: out[v] + (zoomed[v],) for v in variants}


def _epoch(loader):
    """-> (batches, seconds) of one epoch, the device drained after every batch"""
    t0, n = time.perf_counter(), 0
    for b in loader:
        torch.cuda.synchronize()
        n += 1
    return n, time.perf_counter() - t0


def autoaugment_leg(root, a):
    rows = []
    for mode in a.modes.split(","):
        path = os.path.join(root, "train")
        kwargs = {"batch_size": a.batch, "pin_memory": True, "num_workers": a.num_workers, "drop_last": True, "shuffle": True}
        worker = dm._OnDevice(pl.fetch_pytorch_loader(path, mode, True, kwargs, True, True), "cuda:0")
        ds = pl.fetch_pytorch_loader(path, mode, True, {"batch_size": 1}, False, True).dataset
        device = dm.DeviceAugLoader(ds, a.batch, "cuda:0", seed=3, threads=max(2, a.num_workers), autoaugment=True)
        device.set_epoch(0)
        n, first = _epoch(device)       # decode + upload every tile once
        tot = {"worker": [0, 0.0], "device": [0, 0.0]}
        for epoch in range(1, a.epochs + 1):
            device.set_epoch(epoch)
            for name, loader in (("worker", worker), ("device", device)):
                n, t = _epoch(loader)
                tot[name][0] += n
                tot[name][1] += t
        row = {"mode": mode, "batch": a.batch, "num_workers": a.num_workers, "epochs": a.epochs,
               "batches_per_epoch": tot["device"][0] // a.epochs,
               "device_first_epoch_batches_per_s": round(n / first, 2),
               "worker_batches_per_s": round(tot["worker"][0] / tot["worker"][1], 2),
               "device_batches_per_s": round(tot["device"][0] / tot["device"][1], 2)}
        rows.append(row)
        print("%-4s --autoaugment: worker pipeline (%d workers) %.2f batches / s, device path %.2f batches / s (its decoding first "
              "epoch: %.2f); batches of %d" % (mode, a.num_workers, row["worker_batches_per_s"], row["device_batches_per_s"],
                                               row["device_first_epoch_batches_per_s"], a.batch), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tiles", type=int, default=32)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--epochs", type=int, default=6)
    p.add_argument("--modes", default="pre,post")
    p.add_argument("--probs", default="1.0,0.2")
    p.add_argument("--zoom", default="device,host")
    p.add_argument("--autoaugment", action="store_true", help="the --autoaugment leg instead: worker pipeline against device path")
    p.add_argument("--num_workers", type=int, default=8)
    a = p.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as root:
        pl.DEFAULT_INDEX = tile_tree(root, a.tiles)
        if a.autoaugment:
            print(json.dumps({"device": torch.cuda.get_device_name(0), "autoaugment_rows": autoaugment_leg(root, a)}))
            return
        for mode in a.modes.split(","):
            ds = pl.fetch_pytorch_loader(os.path.join(root, "train"), mode, True, {"batch_size": 1}, False, True).dataset
            loader = dm.DeviceAugLoader(ds, a.batch, "cuda:0", seed=3, threads=4)
            loader.set_epoch(0)
            for _ in loader:        # decode + upload every tile once
                pass
            torch.cuda.synchronize()
            for prob in (float(v) for v in a.probs.split(",")):
                res = run(loader, a.epochs, prob, a.zoom.split(","))
                for zoom, (times, drained, _, zoomed) in res.items():
                    ms, msd = [1e3 * t for t in times], [1e3 * t for t in drained]
                    rows.append({"mode": mode, "p_zoom": prob, "zoom": zoom, "batch": a.batch, "batches": len(ms),
                                 "zoomed_samples": zoomed, "host_ms_per_batch_mean": round(statistics.fmean(ms), 3),
                                 "host_ms_per_batch_median": round(statistics.median(ms), 3),
                                 "host_ms_per_batch_max": round(max(ms), 3),
                                 "host_plus_drain_ms_per_batch_mean": round(statistics.fmean(msd), 3)})
                    print("%-4s p=%.1f zoom on %-6s: host %.2f ms / batch mean, %.2f median, %.2f max; %.2f with the device drained "
                          "(%d batches of %d, %d zoomed samples)"
                          % (mode, prob, zoom, rows[-1]["host_ms_per_batch_mean"], rows[-1]["host_ms_per_batch_median"],
                             rows[-1]["host_ms_per_batch_max"], rows[-1]["host_plus_drain_ms_per_batch_mean"], len(ms), a.batch,
                             zoomed), flush=True)
                if len(res) == 2:
                    same = all(np.array_equal(x, y) for x, y in zip(res["device"][2], res["host"][2]))
                    print("     first batch: device and host branch deliver %s bytes" % ("the same" if same else "DIFFERENT"), flush=True)
                    rows[-1]["same_bytes_as_host"] = rows[-2]["same_bytes_as_host"] = bool(same)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
