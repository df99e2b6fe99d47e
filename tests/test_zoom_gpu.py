"""RandomScale on the device (include/xv2.h xv2_zoom_crop_u8): ONE launch resamples the crop windows of all zoomed samples of a
batch out of the tiles cached in HBM - Pillow's uint8 bicubic resize for the image, its nearest resize for the mask.  The bytes
must equal device_aug.zoom_crop_numpy (pinned against Pillow on the CPU, tests/test_zoom_cpu.py) AND Pillow itself
(pytorch_loader.apply_scale), and the training loader must deliver the worker path's samples without ever calling Pillow's
resize.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.test_zoom_cpu import _image

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 4096, 0xA5
FACTORS = (1.0, 1.17, 1.3)


@functools.lru_cache(maxsize=None)
def _case(H, W, C, kind):
    """(tile, mask, {factor: Pillow's zoomed (image, mask)}): computed once, shared, never written to"""
    from xview2_amd.data_loading import pytorch_loader as pl
    img, mask = _image(kind, H, W, C, seed=3)
    ref = {s: pl.apply_scale(img, mask, s) for s in FACTORS}
    for a in (img, mask) + tuple(x for r in ref.values() for x in r):
        a.setflags(write=False)
    return img, mask, ref


def _launch(cache, zlist, h, w, C):
    """DeviceAugmenter.zoom with outputs carved out of sentinel-filled buffers: -> (img, mask, the two whole buffers)"""
    from xview2_amd._capi import Ptr, call
    from xview2_amd.data_loading import device_aug as da
    Z = len(zlist)
    buf = torch.from_numpy(da.pack_zoom([(r, cache.imgs[r].shape[0], cache.imgs[r].shape[1], s, y0, x0)
                                         for r, s, y0, x0 in zlist], h, w)).to(DEV)
    bi = torch.full((2 * GUARD + Z * h * w * C,), SENTINEL, dtype=torch.uint8, device=DEV)
    bm = torch.full((2 * GUARD + Z * h * w,), SENTINEL, dtype=torch.uint8, device=DEV)
    pi, pm = cache.pointer_tables()
    call("xv2_zoom_crop_u8", buf, Ptr(buf, Z * 8), pi, pm, Z, C, h, w, Ptr(bi, GUARD), Ptr(bm, GUARD))
    bi, bm = bi.cpu().numpy(), bm.cpu().numpy()
    return bi[GUARD:-GUARD].reshape(Z, h, w, C), bm[GUARD:-GUARD].reshape(Z, h, w), bi, bm


# windows per launch: three samples, three factors (1.0 included); the origins put windows on every border of the zoomed tile -
# `start` clamped at 0 on the near side, fewer than four taps on the far side - and one in the interior
@pytest.mark.parametrize("H,W,h,w,C,kind,where", [
    (48, 40, 32, 32, 3, "random", ("tl", "br", "mid")),
    (48, 40, 32, 32, 6, "stripes", ("br", "tl", "tr")),
    (96, 80, 40, 72, 3, "stripes", ("tl", "br", "mid")),
    (96, 80, 40, 72, 6, "random", ("bl", "tr", "br")),
    (96, 80, 33, 17, 6, "stripes", ("tr", "bl", "br")),
    (96, 80, 33, 17, 3, "random", ("mid", "tl", "br")),
])
def test_kernel_equals_the_numpy_statement_and_pillow(H, W, h, w, C, kind, where):
    from xview2_amd.data_loading import device_aug as da
    img, mask, ref = _case(H, W, C, kind)
    other = _case(96, 80, C, "random") if (H, W) != (96, 80) else _case(48, 40, C, "random")
    cache = da.DeviceTileCache(DEV)
    cache.add(other[0].copy(), other[1].copy())          # row 0 is another tile of another size: `src` must select row 1
    cache.add(img.copy(), mask.copy())
    zlist = []
    for s, at in zip(FACTORS, where):
        nh, nw = da.zoomed_size(H, W, s)
        y0 = {"t": 0, "b": nh - h, "m": (nh - h) // 2}[at[0]]
        x0 = {"l": 0, "r": nw - w, "i": (nw - w) // 2}[at[1]]
        zlist.append((1, s, y0, x0))
    got_i, got_m, bi, bm = _launch(cache, zlist, h, w, C)
    for z, (_, s, y0, x0) in enumerate(zlist):
        want_i, want_m = da.zoom_crop_numpy(img, mask, s, y0, x0, h, w)
        assert np.array_equal(got_i[z], want_i), (z, s, y0, x0, int((got_i[z] != want_i).sum()))
        assert np.array_equal(got_m[z], want_m), (z, s, y0, x0)
        assert np.array_equal(got_i[z], ref[s][0][y0:y0 + h, x0:x0 + w]), (z, s, y0, x0)
        assert np.array_equal(got_m[z], ref[s][1][y0:y0 + h, x0:x0 + w]), (z, s, y0, x0)
    for b in (bi, bm):
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "the kernel wrote outside its outputs"


def test_entry_point_rejects_what_it_cannot_run():
    from xview2_amd._capi import call
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    o = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for args in ((t, t, t, t, 0, 3, 4, 4, o, o), (t, t, t, t, 1, 4, 4, 4, o, o), (t, t, t, t, 1, 3, 0, 4, o, o),
                 (t, t, t, t, 1, 3, 4, 0, o, o), (None, t, t, t, 1, 3, 4, 4, o, o), (t, None, t, t, 1, 3, 4, 4, o, o),
                 (t, t, None, t, 1, 3, 4, 4, o, o), (t, t, t, None, 1, 3, 4, 4, o, o), (t, t, t, t, 1, 3, 4, 4, None, o),
                 (t, t, t, t, 1, 3, 4, 4, o, None)):
        with pytest.raises(RuntimeError, match="zoom_crop_u8"):
            call("xv2_zoom_crop_u8", *args)


def test_zoom_and_augment_are_ordered_by_their_stream_alone():
    """everything on a side stream - table upload, zoom launch, augment launch, copy back - and no torch.cuda.synchronize():
    the result is right when it is read back through that stream alone, so the path relies on stream order, not on a
    device-wide wait (that the host never blocks is not something a test without timing can show)"""
    from xview2_amd.data_loading import device_aug as da
    img, mask, ref = _case(96, 80, 6, "random")
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        cache = da.DeviceTileCache(DEV)
        cache.add(img.copy(), mask.copy())
        aug = da.DeviceAugmenter(cache)
        rng = np.random.default_rng(4)
        plist, zlist, want = [], [], []
        for s in (1.3, 1.0, 1.17):
            p = da.draw_params(rng, ref[s][1], 2, 40, 40)
            p["hflip"] = s != 1.0
            want.append(da.apply_params_numpy(ref[s][0], ref[s][1], p))
            zlist.append((0, s, p["y0"], p["x0"]))
            p.update(H=40, W=40, y0=0, x0=0)
            plist.append(p)
        extra = aug.zoom(zlist, 40, 40)
        assert torch.cuda.current_stream() == side
        gi, gm = aug(plist, [1, 2, 3], extra)
        gi, gm = gi.cpu().numpy(), gm.cpu().numpy()
    for i, (wi, wm) in enumerate(want):
        assert np.array_equal(gi[i], wi) and np.array_equal(gm[i], wm), i


def _loader_against_the_worker_path(tmp_path, monkeypatch, host_zoom):
    """the existing device-loader test's loop (tests/test_augment_gpu.py): six epochs of DeviceAugLoader against ds[i] replayed
    from the same stream in the same order.  -> calls of pytorch_loader.apply_scale made while the LOADER ran"""
    from tests.test_data_cpu import _tile_tree
    from xview2_amd.data_loading import data_module as dm, pytorch_loader as pl
    root = str(tmp_path / "xbd")
    os.makedirs(root)
    monkeypatch.setattr(pl, "DEFAULT_INDEX", _tile_tree(root, n=4, S=640))
    real, calls = pl.apply_scale, []

    def watched(img, mask, s):
        calls.append(s)
        if not host_zoom:
            raise AssertionError("the device loader resized a tile on the host")
        return real(img, mask, s)
    for mode, C in (("pre", 3), ("post", 6)):
        ds = pl.fetch_pytorch_loader(os.path.join(root, "train"), mode, True, {"batch_size": 1}, False, True).dataset
        loader = dm.DeviceAugLoader(ds, 2, DEV, seed=3, threads=2)
        assert loader.device_zoom == (not host_zoom)
        zoomed = 0
        for epoch in range(6):
            loader.set_epoch(epoch)
            pl._rng_holder["rng"] = np.random.default_rng(100 + epoch)
            loader.rng = pl._rng()
            with monkeypatch.context() as m:
                m.setattr(pl, "apply_scale", watched)
                got = [(b["image"].u8.cpu().numpy(), b["mask"].cpu().numpy()) for b in loader]
            assert len(got) == len(loader) and got[0][0].shape == (2, 512, 512, C)
            pl._rng_holder["rng"] = np.random.default_rng(100 + epoch)      # replay: the worker path, same order, same stream
            order = loader._order()
            for b, (gi, gm) in enumerate(got):
                for j, i in enumerate(order[2 * b:2 * b + 2]):
                    probe = np.random.default_rng(0)
                    probe.bit_generator.state = pl._rng().bit_generator.state
                    zoomed += pl.draw_scale(probe) is not None
                    s = ds[i]
                    assert np.array_equal(gi[j], s["image"]) and np.array_equal(gm[j], s["mask"]), (mode, epoch, b, j)
        assert zoomed > 0, "no zoomed sample in 6 epochs"
        assert len(loader.cache) == len({ds.key(i) for i in range(len(ds))})      # every tile decoded and uploaded once
    return len(calls)


def test_device_loader_zooms_on_the_device_and_delivers_the_worker_paths_samples(tmp_path, monkeypatch):
    monkeypatch.setenv("XV2_DEVICE_ZOOM", "1")
    assert _loader_against_the_worker_path(tmp_path, monkeypatch, host_zoom=False) == 0


@pytest.mark.parametrize("value", ["0", None])
def test_device_zoom_switch_restores_the_host_branch(tmp_path, monkeypatch, value):
    """0, and the default while the two branches' timing on the GPU is unrecorded"""
    if value is None:
        monkeypatch.delenv("XV2_DEVICE_ZOOM", raising=False)
    else:
        monkeypatch.setenv("XV2_DEVICE_ZOOM", value)
    assert _loader_against_the_worker_path(tmp_path, monkeypatch, host_zoom=True) > 0
