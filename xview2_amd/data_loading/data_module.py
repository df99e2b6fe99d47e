"""data_loading/data_module.py:DataModule with the same directory layout (<data>/train, <data>/test, <data>/holdout),
loader options (:15-28) and method names; batches are moved to the training device as they are yielded (pinned
host buffers, non-blocking copies) because the HIP path consumes device tensors."""
import os

import torch

from .pytorch_loader import fetch_pytorch_loader, seed_worker


class _OnDevice:
    def __init__(self, loader, device):
        self.loader, self.device = loader, device

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        sampler = getattr(self.loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)

    def __iter__(self):
        for batch in self.loader:
            out = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
            img = out.get("image")
            if torch.is_tensor(img) and img.dtype == torch.uint8 and img.is_cuda:
                # raw uint8 HWC tiles: normalised on the device straight into the stem's NHWC input
                from ..ops import DeviceImage
                out["image"] = DeviceImage(img)
            yield out


class DeviceAugLoader:
    """Training loader with the augmentation ON THE DEVICE (include/xv2.h xv2_augment_u8).

    Every tile is decoded once (PIL, a small thread pool running ahead of the consumer) and then lives in HBM as uint8
    (device_aug.DeviceTileCache: xBD's training set is 20 GB of 288); per sample the host only draws the decisions
    (device_aug.draw_params - the same stream, in the same order, as the worker path of pytorch_loader._TrainBase._augment,
    so both paths deliver the same bytes from the same seed) and ONE launch per batch crops, flips, adds the noise and applies
    the brightness / contrast tables to image and mask; the result goes to the network as an ops.DeviceImage.  RandomScale
    (p = 0.2, bicubic) runs on the device too with XV2_DEVICE_ZOOM=1: the host zooms only the mask (a gather, for the crop decision) and builds the
    coefficient tables of the crop window, and one more launch per batch (include/xv2.h xv2_zoom_crop_u8) resamples the windows
    of all its zoomed samples out of the cached tiles into one-off 512 x 512 sources - a twin of PILLOW's uint8 bicubic
    resampler (pytorch_loader.apply_scale), bit for bit (tests/test_zoom_cpu.py, tests/test_zoom_gpu.py); the reference's own
    cv2 INTER_CUBIC stays unpinned as before (VERDICT row f4).  XV2_DEVICE_ZOOM=0 is the host branch: the tile comes back
    from the cache, is zoomed and cropped by Pillow and uploaded.  It is the default: the same-run timing of the two branches
    on an MI355X that the default is to follow (scripts/bench_loader.py) is not recorded.  Sampling = DataLoader(shuffle=True, drop_last=True) /
    DistributedSampler semantics.

    autoaugment=True is `--autoaugment` on the device: per sample the host draws the crop (device_aug.draw_crop) and the 0 .. 2
    operations of one ImageNet sub-policy (autoaugment.draw_policy) - the worker path's stream, in its order; no zoom, flips or
    noise, as there - and a batch is the crop launch followed by ONE call (include/xv2.h xv2_autoaugment_u8) that runs every
    sample's operations in place: a twin of the bytes PILLOW produces for the ten operations of the POLICY table
    (device_autoaug.autoaug_numpy; tests/test_autoaug_cpu.py, tests/test_autoaug_gpu.py), no PIL operation runs on the host.
    DataModule chooses it for `--autoaugment` only with XV2_DEVICE_AUTOAUGMENT=1; the default 0 keeps the worker pipeline:
    one same-run timing of the two is recorded (scripts/bench_loader.py --autoaugment; DESIGN.md section 8,
    profiles/r08_autoaugment_loader.md) and the change of the default is left to a change that cites it."""

    def __init__(self, dataset, batch_size, device, rank=0, world_size=1, seed=0, threads=4, shuffle=True, autoaugment=False):
        from .device_aug import DeviceAugmenter, DeviceTileCache
        self.ds, self.bs, self.device = dataset, int(batch_size), torch.device(device)
        self.rank, self.world, self.seed, self.epoch, self.shuffle = rank, world_size, seed, 0, shuffle
        self.cache = DeviceTileCache(self.device)
        self.aug = DeviceAugmenter(self.cache)
        self.rows, self.host_masks = {}, {}
        self.threads = max(1, int(threads))
        self.autoaugment = bool(autoaugment)
        # XV2_DEVICE_ZOOM=1: RandomScale on the device; 0 (the default, see the class docstring): on the host (Pillow); a cache in
        # host memory has no kernel to run
        self.device_zoom = os.environ.get("XV2_DEVICE_ZOOM", "0") != "0" and self.device.type == "cuda"
        self._rng, self._rng_pinned, self._rng_epoch = None, False, None

    @property
    def rng(self):
        return self._rng

    @rng.setter
    def rng(self, g):                              # an assigned stream is kept as it is (replay tests)
        self._rng, self._rng_pinned = g, g is not None

    def __len__(self):
        return (len(self.ds) // self.world) // self.bs

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _order(self):
        import numpy as np
        n = len(self.ds)
        order = np.random.default_rng(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n)
        per = n // self.world                      # (DistributedSampler pads; drop_last training can simply truncate)
        return [int(i) for i in order[self.rank:per * self.world:self.world]]

    def _row(self, i, pending):
        k = self.ds.key(i)
        if k not in self.rows:
            img, lbl = pending.pop(i).result() if i in pending else self.ds.load(i)
            self.rows[k] = self.cache.add(img, lbl)
            self.host_masks[k] = lbl
        return self.rows[k], self.host_masks[k]

    def __iter__(self):
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from . import pytorch_loader as pl
        from .autoaugment import draw_policy
        from .device_aug import crop_params, draw_crop, draw_params, nearest_table, zoomed_size
        from ..ops import DeviceImage
        if self.rng is None or self._rng_epoch != self.epoch:
            # a private stream per (seed, rank, epoch): follows --seed, differs between the ranks of a data-parallel job
            # and does not restart from the same state after a resume (the worker path seeds per worker and rank from
            # torch.initial_seed(), pytorch_loader.seed_worker); tests that replay the worker path assign self.rng.
            if not self._rng_pinned:
                self._rng = np.random.default_rng([int(self.seed), int(self.rank), int(self.epoch)])
            self._rng_epoch = self.epoch
        order = self._order()
        ahead = 4 * self.bs
        with ThreadPoolExecutor(self.threads) as pool:
            pending = {}

            def prefetch(pos):
                for j in order[pos:pos + ahead]:
                    if self.ds.key(j) not in self.rows and j not in pending:
                        pending[j] = pool.submit(self.ds.load, j)
            for b in range(len(order) // self.bs):
                prefetch(b * self.bs)
                plist, rows, extra = [], [], []
                # every cache row of the batch is resolved BEFORE a one-off tile gets its index: cache.add() of a later,
                # not yet cached sample would otherwise shift len(cache) under an earlier zoomed sample's index
                resolved = [self._row(i, pending) for i in order[b * self.bs:(b + 1) * self.bs]]
                if self.autoaugment:     # crop + one sub-policy per sample: the crop launch, then xv2_autoaugment_u8
                    policies = []
                    for row, mask in resolved:
                        y0, x0 = draw_crop(self.rng, mask)
                        plist.append(crop_params(mask.shape[0], mask.shape[1], y0, x0, self.cache.imgs[row].shape[2] // 3))
                        rows.append(row)
                        policies.append(draw_policy(self.rng))
                    img, mask = self.aug.autoaugment(plist, rows, policies)
                    yield {"image": DeviceImage(img), "mask": mask}
                    continue
                base = len(self.cache)
                zlist = []
                for row, mask in resolved:
                    s = pl.draw_scale(self.rng)
                    if s is None:
                        plist.append(draw_params(self.rng, mask, self.cache.imgs[row].shape[2] // 3))
                        rows.append(row)
                        continue
                    if self.device_zoom:
                        # zoomed sample: only the MASK is zoomed on the host (a gather through Pillow's nearest tables - the
                        # crop decision needs it); the image window is resampled on the device from the cached tile
                        H, W = mask.shape[:2]
                        nh, nw = zoomed_size(H, W, s)
                        p = draw_params(self.rng, mask[nearest_table(H, nh)][:, nearest_table(W, nw)],
                                        self.cache.imgs[row].shape[2] // 3)
                        zlist.append((row, s, p["y0"], p["x0"]))
                        p.update(H=p["h"], W=p["w"], y0=0, x0=0)
                        plist.append(p)
                        rows.append(base + len(zlist) - 1)
                        continue
                    # XV2_DEVICE_ZOOM=0 (default): resize on the host, crop there, upload the window as a one-off source tile
                    img, zmask = pl.apply_scale(self.cache.imgs[row].cpu().numpy(), mask, s)
                    p = draw_params(self.rng, zmask, img.shape[2] // 3)
                    y0, x0 = p["y0"], p["x0"]
                    win = np.ascontiguousarray(img[y0:y0 + p["h"], x0:x0 + p["w"]])
                    wm = np.ascontiguousarray(zmask[y0:y0 + p["h"], x0:x0 + p["w"]])
                    p.update(H=p["h"], W=p["w"], y0=0, x0=0)
                    extra.append((torch.from_numpy(win).to(self.device), torch.from_numpy(wm).to(self.device)))
                    plist.append(p)
                    rows.append(base + len(extra) - 1)
                if zlist:       # every zoomed window of the batch: one table upload, one launch (xv2_zoom_crop_u8)
                    assert not extra, "one zoom branch per batch: the one-off rows are numbered by either list"
                    extra = self.aug.zoom(zlist, plist[0]["h"], plist[0]["w"])
                img, mask = self.aug(plist, rows, extra)
                yield {"image": DeviceImage(img), "mask": mask}


class DataModule:
    def __init__(self, args, device="cuda", rank=0, world_size=1):
        self.args, self.device, self.rank, self.world_size = args, device, rank, world_size
        self.train_path = os.path.join(args.data, "train")
        self.val_path = os.path.join(args.data, "test")
        self.test_path = os.path.join(args.data, "holdout")
        pin = str(device).startswith("cuda")
        # device-side input hand-over: workers deliver uint8 HWC tiles, the GPU normalises them into
        # NHWC (xv2_normalize_u8_to_nhwc).  XV2_HOST_NORMALIZE=1 restores the reference's host normalise + CHW transpose.
        self.raw_u8 = pin and os.environ.get("XV2_HOST_NORMALIZE", "0") != "1"
        self.train_loader_kwargs = {"batch_size": args.batch_size, "pin_memory": pin, "num_workers": args.num_workers,
                                    "drop_last": True, "shuffle": True}
        self.test_loader_kwargs = {"batch_size": args.val_batch_size, "pin_memory": pin,
                                   "num_workers": args.num_workers, "drop_last": False, "shuffle": False}

    def _loader(self, path, training, kwargs):
        kwargs = dict(kwargs)
        if self.world_size > 1:     # what PL's ddp accelerator adds: one shard of the dataset per rank
            from torch.utils.data.distributed import DistributedSampler
            # the dataset is built once and re-wrapped with the sampler (no second glob / index parse)
            probe = fetch_pytorch_loader(path, self.args.type, training, {"batch_size": 1},
                                         getattr(self.args, "autoaugment", False), self.raw_u8).dataset
            kwargs["sampler"] = DistributedSampler(probe, self.world_size, self.rank, shuffle=kwargs.pop("shuffle"))
            loader = torch.utils.data.DataLoader(probe, worker_init_fn=seed_worker, **kwargs)
        else:
            loader = fetch_pytorch_loader(path, self.args.type, training, kwargs,
                                          getattr(self.args, "autoaugment", False), self.raw_u8)
        return _OnDevice(loader, self.device)

    def train_dataloader(self):
        if getattr(self, "_train", None) is None:
            # augmentation on the device, tiles resident in HBM (DeviceAugLoader); XV2_DEVICE_AUG=0 or the host-normalise switch
            # keep the reference's worker pipeline, and so does --autoaugment (a PIL policy) unless XV2_DEVICE_AUTOAUGMENT=1
            # selects its device twin (default 0: DeviceAugLoader's docstring)
            auto = bool(getattr(self.args, "autoaugment", False))
            if (self.raw_u8 and os.environ.get("XV2_DEVICE_AUG", "1") != "0" and
                    (not auto or os.environ.get("XV2_DEVICE_AUTOAUGMENT", "0") != "0")):
                # (the dataset only decodes tiles here - load() / key() - so it is built without its PIL policy)
                ds = fetch_pytorch_loader(self.train_path, self.args.type, True, {"batch_size": 1}, False, True).dataset
                self._train = DeviceAugLoader(ds, self.args.batch_size, self.device, self.rank, self.world_size,
                                              seed=getattr(self.args, "seed", 0) or 0, threads=max(2, self.args.num_workers),
                                              autoaugment=auto)
            else:
                self._train = self._loader(self.train_path, True, self.train_loader_kwargs)
        return self._train

    def val_dataloader(self):
        return self._loader(self.val_path, False, self.test_loader_kwargs)

    def test_dataloader(self):
        return self._loader(self.test_path, False, self.test_loader_kwargs)
