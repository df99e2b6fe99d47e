"""`--autoaugment` on the device (include/xv2.h xv2_autoaugment_u8): ONE call runs the two-operation sub-policy of every sample
of a cropped batch in place - statistics, tables and the operations themselves never leave the GPU.  The bytes must equal
device_autoaug.autoaug_numpy (pinned against Pillow on the CPU, tests/test_autoaug_cpu.py) AND Pillow itself
(autoaugment.apply_op chained), and the training loader must deliver the worker path's samples without a PIL operation on the
host.  Every comparison is exact."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_autoaug_cpu import edge_inputs, edge_ops, pillow

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 4096, 0xA5


def _launch(imgs, masks, ops_list):
    """xv2_autoaugment_u8 on a batch (uint8 [N, h, w, C], [N, h, w]) placed inside sentinel-filled buffers, the workspace too:
    -> (images, masks) after the call; the guards on both sides of all three buffers must be intact"""
    from xview2_amd._capi import Ptr, call, query
    from xview2_amd.data_loading import device_autoaug as dv
    N, h, w, C = imgs.shape
    host = dv.pack_policy(ops_list, h, w)
    buf = torch.from_numpy(host).to(DEV)
    need = query("xv2_autoaugment_workspace", N, C, h, w)
    assert need >= N * h * w * (C + 1)
    bufs = [torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.uint8, device=DEV) for n in (imgs.size, masks.size, need)]
    bufs[0][GUARD:GUARD + imgs.size] = torch.from_numpy(imgs.copy()).to(DEV).reshape(-1)
    bufs[1][GUARD:GUARD + masks.size] = torch.from_numpy(masks.copy()).to(DEV).reshape(-1)
    call("xv2_autoaugment_u8", host.ctypes.data, buf, Ptr(buf, N * 2 * dv.ROW), N, C, h, w, Ptr(bufs[0], GUARD), Ptr(bufs[1], GUARD),
         Ptr(bufs[2], GUARD))
    bufs = [b.cpu().numpy() for b in bufs]
    for b in bufs:
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "the kernels wrote outside their buffers"
    return bufs[0][GUARD:-GUARD].reshape(N, h, w, C), bufs[1][GUARD:-GUARD].reshape(N, h, w)


def _check(imgs, masks, ops_list, against_pillow=True):
    from xview2_amd.data_loading import device_autoaug as dv
    gi, gm = _launch(imgs, masks, ops_list)
    for n, ops in enumerate(ops_list):
        wi, wm = dv.autoaug_numpy(imgs[n], masks[n], ops)
        assert np.array_equal(gi[n], wi), (n, ops, int((gi[n] != wi).sum()))
        assert np.array_equal(gm[n], wm), (n, ops, int((gm[n] != wm).sum()))
        if against_pillow:
            pi, pm = pillow(imgs[n], masks[n], ops)
            assert np.array_equal(gi[n], pi) and np.array_equal(gm[n], pm), (n, ops)
    return gi, gm


@functools.lru_cache(maxsize=None)
def _batch(N, h, w, C, seed=0):
    rng = np.random.default_rng([seed, N, h, w, C])
    imgs, masks = rng.integers(0, 256, (N, h, w, C), dtype=np.uint8), rng.integers(0, 5, (N, h, w), dtype=np.uint8)
    imgs.setflags(write=False)
    masks.setflags(write=False)
    return imgs, masks


@pytest.mark.parametrize("s1,s2", [(1, 1), (1, -1), (-1, 1), (-1, -1)])
@pytest.mark.parametrize("h,w,C", [(40, 33, 3), (33, 40, 6)])
def test_all_25_sub_policies_equal_the_numpy_statement_and_pillow(h, w, C, s1, s2):
    from xview2_amd.data_loading import autoaugment as aa
    imgs, masks = _batch(len(aa.POLICY), h, w, C)
    ops = [[(op1, aa.magnitude(op1, m1), s1), (op2, aa.magnitude(op2, m2), s2)] for _, op1, m1, _, op2, m2 in aa.POLICY]
    assert len(ops) == 25
    _check(imgs, masks, ops)


def test_a_mixed_batch_leaves_samples_without_an_operation_untouched():
    imgs, masks = _batch(7, 37, 53, 6, seed=1)
    ops = [[], [("rotate", 20.0, 1)], [("equalize", 0, 1), ("shearX", 0.3 * 5 / 9, -1)], [], [("sharpness", 0.7, 1)],
           [("contrast", 0.8, -1), ("solarize", 256 * 4 / 9, 1)], [("autocontrast", 0, 1)]]
    gi, gm = _check(imgs, masks, ops)
    for n in (0, 3):
        assert np.array_equal(gi[n], imgs[n]) and np.array_equal(gm[n], masks[n])
    gi, gm = _launch(imgs, masks, [[]] * 7)         # no operation at all: nothing is enqueued
    assert np.array_equal(gi, imgs) and np.array_equal(gm, masks)


def test_counts_at_full_size():
    """512 x 512, C = 6: up to 262 144 per histogram bin and 6.7e7 per sum of L; the second image is one flat value per channel
    (every pixel in ONE bin) with a second value in a corner so that equalize does not take its identity branch"""
    from xview2_amd.data_loading import autoaugment as aa
    imgs, masks = (a.copy() for a in _batch(3, 512, 512, 6, seed=2))
    imgs[0, :, :, 3:] = (255, 254, 253)
    imgs[0, :2, :2, 3:] = 0
    imgs[1, :, :, 3:] = 255                          # the largest sum of L
    ops = [[("equalize", 0, 1), ("equalize", 0, 1)],
           [("color", aa.magnitude("color", 4), 1), ("contrast", aa.magnitude("contrast", 8), -1)],
           [("rotate", aa.magnitude("rotate", 8), 1), ("color", aa.magnitude("color", 2), -1)]]
    _check(imgs, masks, ops)


@pytest.mark.parametrize("name", sorted(edge_inputs()))
def test_edge_inputs_through_the_kernel(name):
    img, mask, names = edge_inputs()[name]
    ops = [[op] for n in names for op in edge_ops(n)]
    ops += [[a[0], b[0]] for a, b in zip(ops[:-1], ops[1:])]          # and chained in pairs
    _check(np.repeat(img[None], len(ops), 0), np.repeat(mask[None], len(ops), 0), ops)


def test_crop_and_autoaugment_are_ordered_by_their_stream_alone():
    """everything on a side stream - tile upload, parameter uploads, crop launch, the autoaugment launches, copy back - and no
    torch.cuda.synchronize(): the result is right when it is read back through that stream alone"""
    from xview2_amd.data_loading import device_aug as da, device_autoaug as dv
    imgs, masks = _batch(1, 96, 80, 6, seed=3)
    img, mask = imgs[0], masks[0]
    ops = [[("equalize", 0, 1), ("rotate", 30.0, 1)], [("color", 0.4, 1), ("contrast", 0.8, 1)], [],
           [("shearX", 0.3 * 5 / 9, 1), ("equalize", 0, 1)]]
    origins = [(0, 0), (56, 40), (13, 7), (30, 21)]
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        cache = da.DeviceTileCache(DEV)
        cache.add(img.copy(), mask.copy())
        aug = da.DeviceAugmenter(cache)
        assert torch.cuda.current_stream() == side
        for _ in range(2):                           # the second batch reuses the first one's workspace
            gi, gm = aug.autoaugment([da.crop_params(96, 80, y0, x0, 2, 40, 40) for y0, x0 in origins], [0] * 4, ops)
            gi, gm = gi.cpu().numpy(), gm.cpu().numpy()
            for n, (y0, x0) in enumerate(origins):
                wi, wm = dv.autoaug_numpy(img[y0:y0 + 40, x0:x0 + 40], mask[y0:y0 + 40, x0:x0 + 40], ops[n])
                assert np.array_equal(gi[n], wi) and np.array_equal(gm[n], wm), n


def test_entry_point_rejects_what_it_cannot_run():
    from xview2_amd._capi import call, query
    from xview2_amd.data_loading import device_autoaug as dv
    host = dv.pack_policy([[("invert", 0, 1), ("equalize", 0, 1)]], 4, 4)      # every buffer is large enough for N=1 C=3 4x4
    bad_id, negative = host.copy(), host.copy()
    bad_id[8], negative[0] = 9, -1
    d = torch.from_numpy(host).to(DEV)
    luts = d[16:]
    img = torch.zeros(48, dtype=torch.uint8, device=DEV)
    mask = torch.zeros(16, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(query("xv2_autoaugment_workspace", 1, 3, 4, 4), dtype=torch.uint8, device=DEV)
    h = host.ctypes.data
    for args in ((h, d, luts, 0, 3, 4, 4, img, mask, ws), (h, d, luts, -1, 3, 4, 4, img, mask, ws),
                 (h, d, luts, 1, 4, 4, 4, img, mask, ws), (h, d, luts, 1, 1, 4, 4, img, mask, ws),
                 (h, d, luts, 1, 3, 0, 4, img, mask, ws), (h, d, luts, 1, 3, 4, 0, img, mask, ws),
                 (h, d, luts, 1, 3, -4, 4, img, mask, ws), (None, d, luts, 1, 3, 4, 4, img, mask, ws),
                 (h, None, luts, 1, 3, 4, 4, img, mask, ws), (h, d, luts, 1, 3, 4, 4, None, mask, ws),
                 (h, d, luts, 1, 3, 4, 4, img, None, ws), (h, d, luts, 1, 3, 4, 4, img, mask, None),
                 (h, d, None, 1, 3, 4, 4, img, mask, ws),          # a sample uses a host-built table and there is none
                 (bad_id.ctypes.data, d, luts, 1, 3, 4, 4, img, mask, ws), (negative.ctypes.data, d, luts, 1, 3, 4, 4, img, mask, ws)):
        with pytest.raises(RuntimeError, match="autoaugment_u8"):
            call("xv2_autoaugment_u8", *args)
    for shape in ((0, 3, 4, 4), (1, 4, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert query("xv2_autoaugment_workspace", *shape) == 0
    call("xv2_autoaugment_u8", h, d, luts, 1, 3, 4, 4, img, mask, ws)          # and the arguments themselves were fine
    torch.cuda.synchronize()


def test_device_loader_runs_the_policy_on_the_device_and_delivers_the_worker_paths_samples(tmp_path, monkeypatch):
    """six epochs of DeviceAugLoader(autoaugment=True) against ds[i] replayed from the same stream in the same order (the loop of
    tests/test_zoom_gpu.py), with autoaugment.apply_op raising while the LOADER runs"""
    from tests.test_data_cpu import _tile_tree
    from xview2_amd.data_loading import autoaugment as aa, data_module as dm, device_aug as da, pytorch_loader as pl
    monkeypatch.setenv("XV2_DEVICE_AUTOAUGMENT", "1")
    root = str(tmp_path / "xbd")
    os.makedirs(root)
    monkeypatch.setattr(pl, "DEFAULT_INDEX", _tile_tree(root, n=4, S=640))

    def no_pil(*a, **k):
        raise AssertionError("the device loader ran a PIL operation on the host")
    two = geometric = 0
    for mode, C in (("pre", 3), ("post", 6)):
        ds = pl.fetch_pytorch_loader(os.path.join(root, "train"), mode, True, {"batch_size": 1}, True, True).dataset
        loader = dm.DeviceAugLoader(ds, 2, DEV, seed=3, threads=2, autoaugment=True)
        for epoch in range(6):
            loader.set_epoch(epoch)
            pl._rng_holder["rng"] = np.random.default_rng(100 + epoch)
            loader.rng = pl._rng()
            with monkeypatch.context() as m:
                m.setattr(aa, "apply_op", no_pil)
                got = [(b["image"].u8.cpu().numpy(), b["mask"].cpu().numpy()) for b in loader]
            assert len(got) == len(loader) and got[0][0].shape == (2, 512, 512, C)
            pl._rng_holder["rng"] = np.random.default_rng(100 + epoch)      # replay: the worker path, same order, same stream
            order = loader._order()
            for b, (gi, gm) in enumerate(got):
                for j, i in enumerate(order[2 * b:2 * b + 2]):
                    probe = np.random.default_rng(0)
                    probe.bit_generator.state = pl._rng().bit_generator.state
                    da.draw_crop(probe, loader.host_masks[ds.key(i)])
                    ops = aa.draw_policy(probe)
                    two += len(ops) == 2
                    geometric += any(op in aa.GEOMETRIC for op, _, _ in ops)
                    s = ds[i]
                    assert np.array_equal(gi[j], s["image"]) and np.array_equal(gm[j], s["mask"]), (mode, epoch, b, j, ops)
        assert len(loader.cache) == len({ds.key(i) for i in range(len(ds))})      # every tile decoded and uploaded once
    assert two > 0 and geometric > 0, "six epochs must hold a sample with two operations and a geometric one"


@pytest.mark.parametrize("value", [None, "0", "1"])
def test_the_switch_defaults_to_the_worker_pipeline(tmp_path, monkeypatch, value):
    from tests.test_data_cpu import _tile_tree
    from xview2_amd.data_loading import data_module as dm, pytorch_loader as pl
    if value is None:
        monkeypatch.delenv("XV2_DEVICE_AUTOAUGMENT", raising=False)
    else:
        monkeypatch.setenv("XV2_DEVICE_AUTOAUGMENT", value)
    monkeypatch.delenv("XV2_DEVICE_AUG", raising=False)
    monkeypatch.delenv("XV2_HOST_NORMALIZE", raising=False)
    root = str(tmp_path / "xbd")
    os.makedirs(root)
    monkeypatch.setattr(pl, "DEFAULT_INDEX", _tile_tree(root, n=4, S=640))
    args = SimpleNamespace(data=root, type="post", batch_size=2, val_batch_size=2, num_workers=0, autoaugment=True, seed=1)
    loader = dm.DataModule(args, device=DEV).train_dataloader()
    if value == "1":
        assert isinstance(loader, dm.DeviceAugLoader) and loader.autoaugment
    else:
        assert isinstance(loader, dm._OnDevice) and not isinstance(loader, dm.DeviceAugLoader)
        assert loader.loader.dataset.use_autoaugment
    args.autoaugment = False                         # and without the flag the default recipe keeps its device loader
    plain = dm.DataModule(args, device=DEV).train_dataloader()
    assert isinstance(plain, dm.DeviceAugLoader) and not plain.autoaugment
