"""Whole-scene prediction: a trained model applied to imagery of any size, without labels.

A scene (uint8 [H, W, 3], pre and optionally post) stays in HBM.  It is cut into overlapping windows
(xv2_scene_windows_u8), the model runs on batches of them, and the per-window probabilities are blended back into
scene-sized maps with a separable ramp weight (xv2_scene_blend, xv2_scene_finalize; csrc/scene.hip) - no host round trip,
no atomics, the same bits however the windows are batched.

The geometry below is integer arithmetic in numpy, importable without a GPU, and is the specification of the kernels:

  window_origins(L, n, overlap)   origins along one axis: [0] when L <= n, else range(0, L - n, n - overlap) + [L - n] -
                                  the last window is moved back, never padded.  n % 32 == 0, 32 <= n <= 2048,
                                  0 <= overlap <= n // 2; then no position is covered by more than 3 windows per axis.
  windows of a scene              the product grid of the two axes, y outer, x inner: THE summation order everywhere.
  tri(i, L)                       padding exists only when L < n, on the far side: reflection without repeating the edge,
                                  iterated (period 2 (L - 1), tri(i, 1) = 0) = np.pad(mode="reflect").  Predictions at
                                  padded positions are discarded.
  ramp(n, overlap)                r(i) = min(i + 1, n - i, overlap + 1); window pixel (iy, ix) weighs r(iy) r(ix): an
                                  integer <= 1025^2, exact in fp32.
  axis_normaliser(L, n, overlap)  W[p] = the sum of r over the origins covering p.  The grid is a product, so the weight
                                  sum of scene pixel (y, x) is Wy[y] Wx[x] <= 9 * 1025^2 < 2^24: an exact fp32 integer,
                                  and no weight-sum buffer exists on the device.
  scaled_size(H, W, s)            the size the scene is predicted at under predict(scales=...): round(H s), round(W s), each
                                  at least 1 (xview2_amd/resize.py, with the coefficient tables of the two resize kernels).
"""
import numpy as np

from .resize import check_scales, scaled_size  # noqa: F401  (the geometry of predict(scales=...))

SIGMOID1, SOFTMAX, SIGMOID, RELU = 0, 1, 2, 3      # include/xv2.h XV2_SCENE_*
MAX_WINDOWS = 1024                                  # XV2_SCENE_MAX_WINDOWS: windows per kernel call


def check_window(n, overlap):
    if n % 32 != 0 or not 32 <= n <= 2048:
        raise ValueError("window side %d must be a multiple of 32 in 32..2048" % n)
    if not 0 <= overlap <= n // 2:
        raise ValueError("overlap %d must be in 0..%d (half the window)" % (overlap, n // 2))


def window_origins(L, n, overlap):
    check_window(n, overlap)
    if L < 1:
        raise ValueError("axis length %d must be positive" % L)
    if L <= n:
        return [0]
    return list(range(0, L - n, n - overlap)) + [L - n]


def tri(i, L):
    """source index of position i >= 0 on an axis of length L (i may be an array)"""
    i = np.asarray(i, dtype=np.int64)
    if L == 1:
        return np.zeros_like(i)
    p = 2 * (L - 1)
    m = i % p
    return np.where(m < L, m, p - m)


def ramp(n, overlap):
    i = np.arange(n, dtype=np.int64)
    return np.minimum(np.minimum(i + 1, n - i), overlap + 1)


def axis_normaliser(L, n, overlap):
    r = ramp(n, overlap)
    out = np.zeros(L, dtype=np.int64)
    for o in window_origins(L, n, overlap):
        m = min(n, L - o)
        out[o:o + m] += r[:m]
    return out.astype(np.int32)


def scene_windows(H, W, n, overlap):
    """int32 [K, 2] (y0, x0) of every window of an H x W scene, in summation order"""
    return np.array([(y, x) for y in window_origins(H, n, overlap) for x in window_origins(W, n, overlap)],
                    dtype=np.int32).reshape(-1, 2)


def kind_of(args):
    """the decode Model._decode chooses for a checkpoint's hyper-parameters"""
    if args.type == "pre":
        return SIGMOID1
    if args.loss_str == "coral":
        return SIGMOID
    if args.loss_str == "mse":
        return RELU
    return SOFTMAX


# ---- the kernels (the library is loaded on first use: there is no CPU path) -------------------------------------------

def gather_windows(pre_u8, post_u8, origins, n, out=None):
    """uint8 [K, n, n, 3 | 6] windows of the scene at the device table origins int32 [K, 2]"""
    import torch
    from ._capi import call
    H, W, _ = pre_u8.shape
    K = origins.shape[0]
    if out is None:
        out = torch.empty((K, n, n, 6 if post_u8 is not None else 3), dtype=torch.uint8, device=pre_u8.device)
    call("xv2_scene_windows_u8", pre_u8, post_u8, H, W, origins, K, n, n, out)
    return out


def blend(logits, kind, origins, overlap, acc):
    """acc [Cout, H, W] += the ramp-weighted decode of logits fp32 [K, C, n, n] (windows at origins, in index order)"""
    from ._capi import call
    K, C, h, w = logits.shape
    _, H, W = acc.shape
    call("xv2_scene_blend", logits, int(kind), C, origins, K, h, w, int(overlap), H, W, acc)


def finalize(acc, wy, wx):
    """acc[c, y, x] /= wy[y] * wx[x] in place"""
    from ._capi import call
    Cout, H, W = acc.shape
    call("xv2_scene_finalize", acc, Cout, H, W, wy, wx)


def _check_scene(name, t):
    import torch
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda:
        raise ValueError("%s: a uint8 [H, W, 3] device tensor expected, got %s" % (
            name, (t.dtype, tuple(t.shape), str(t.device)) if torch.is_tensor(t) else type(t)))
    return t.contiguous()


def align_pair(pre_u8, post_u8, radius, tile=128):
    """Register post to pre by the best whole-pixel translation within `radius` (include/xv2.h, "register the post image to
    the pre image"; utils/align.py): uint8 [H, W, 3] device scenes -> (post resampled by the global shift, info).  The shift
    goes from the estimate to the resampler on the device; info holds the estimate's device tables (block_sad, sad,
    block_shift, shift, each with a leading batch axis of 1) and radius / tile - utils.align.report_of(info, H, W) reads them
    back into the report."""
    from . import ops
    from .utils.align import check_radius, check_tile
    radius, tile = check_radius(radius), check_tile(tile)
    pre_u8, post_u8 = _check_scene("pre", pre_u8), _check_scene("post", post_u8)
    if post_u8.shape != pre_u8.shape or post_u8.device != pre_u8.device:
        raise ValueError("pre %s and post %s scenes differ" % (tuple(pre_u8.shape), tuple(post_u8.shape)))
    block_sad, sad, block_shift, shift = ops.align_estimate(pre_u8[None], post_u8[None], radius, tile)
    aligned = ops.translate_u8(post_u8[None], shift)[0]
    return aligned, {"radius": radius, "tile": tile, "block_sad": block_sad, "sad": sad, "block_shift": block_shift,
                     "shift": shift}


class ScenePredictor:
    """model: a lightning.Model in eval mode (its forward is called, so --tta works as in eval), or any callable
    DeviceImage -> fp32 logits [K, C, window, window].  kind: one of SIGMOID1 / SOFTMAX / SIGMOID / RELU; by default what
    Model._decode does for model.args."""

    def __init__(self, model, window=1024, overlap=256, batch=4, kind=None):
        check_window(window, overlap)
        if not 1 <= batch <= MAX_WINDOWS:
            raise ValueError("batch %d must be in 1..%d" % (batch, MAX_WINDOWS))
        if kind is None:
            if getattr(model, "args", None) is None:
                raise ValueError("ScenePredictor: kind= is required for a model without .args")
            kind = kind_of(model.args)
        if kind not in (SIGMOID1, SOFTMAX, SIGMOID, RELU):
            raise ValueError("ScenePredictor: unknown kind %r" % (kind,))
        self.model, self.window, self.overlap, self.batch, self.kind = model, window, overlap, batch, kind

    def predict(self, pre_u8, post_u8=None, scales=(1.0,)):
        """uint8 [H, W, 3] device scene(s) in stored (BGR) channel order -> fp32 [Cout, H, W] blended maps on the device.

        scales: the scene is predicted once per scale s, in list order - resized to scaled_size(H, W, s) as Pillow's bicubic
        resize does it (ops.resize_u8), predicted window by window at that size (a scaled scene smaller than the window takes
        the reflect padding), and the maps brought back to H x W with the bilinear resample of ops.resize_f32 - and the
        result is ((r1 + r2) + ... + rk) / k in fp32.  A scale of 1 contributes the maps as they are.  1 to 8 scales in
        [0.25, 4] without duplicates; scales=(1,) is the plain prediction, the same calls and the same bits."""
        pre_u8 = _check_scene("pre", pre_u8)
        if post_u8 is not None:
            post_u8 = _check_scene("post", post_u8)
            if post_u8.shape != pre_u8.shape or post_u8.device != pre_u8.device:
                raise ValueError("pre %s and post %s scenes differ" % (tuple(pre_u8.shape), tuple(post_u8.shape)))
        H, W, _ = pre_u8.shape
        if H * W >= 1 << 30:
            raise ValueError("scene %d x %d exceeds 2^30 pixels" % (H, W))
        scales = check_scales(scales)
        if scales == (1.0,):
            return self._predict_native(pre_u8, post_u8)
        from . import ops, resize
        sizes = [scaled_size(H, W, s) for s in scales]
        for s, (Hs, Ws) in zip(scales, sizes):          # every refusal before the first launch
            if Hs * Ws >= 1 << 30:
                raise ValueError("scene %d x %d at scale %g is %d x %d: 2^30 pixels or more" % (H, W, s, Hs, Ws))
            resize.check_axis(H, Hs)
            resize.check_axis(W, Ws)
        k, acc = len(scales), None
        for i, (s, (Hs, Ws)) in enumerate(zip(scales, sizes)):
            if s == 1.0:
                maps = self._predict_native(pre_u8, post_u8)
            else:
                maps = self._predict_native(ops.resize_u8(pre_u8, Hs, Ws),
                                            ops.resize_u8(post_u8, Hs, Ws) if post_u8 is not None else None)
            if i == 0:
                # the first term as it is: the predictor's own tensor at scale 1, else a plain write
                acc = maps if s == 1.0 else ops.resize_f32(maps, H, W)
            elif i < k - 1:
                ops.resize_f32(maps, H, W, out=acc, mode="accumulate")      # (scale 1: the identity tables, acc + maps)
            else:
                ops.resize_f32(maps, H, W, out=acc, mode="finish", k=k)
        return acc

    def _predict_native(self, pre_u8, post_u8):
        """the windowed prediction of checked scenes at the size they have"""
        import torch
        from . import ops
        H, W, _ = pre_u8.shape
        n, dev = self.window, pre_u8.device
        origins = torch.from_numpy(scene_windows(H, W, n, self.overlap)).to(dev)
        wy = torch.from_numpy(axis_normaliser(H, n, self.overlap)).to(dev)
        wx = torch.from_numpy(axis_normaliser(W, n, self.overlap)).to(dev)
        acc = None
        with torch.no_grad():
            for k0 in range(0, origins.shape[0], self.batch):
                tab = origins[k0:k0 + self.batch]
                logits = self.model(ops.DeviceImage(gather_windows(pre_u8, post_u8, tab, n)))
                if isinstance(logits, (tuple, list)):
                    logits = logits[0]
                if logits.dim() != 4 or logits.shape[0] != tab.shape[0] or tuple(logits.shape[2:]) != (n, n):
                    raise RuntimeError("ScenePredictor: the model returned %s for %d windows of %d x %d" % (
                        tuple(logits.shape), tab.shape[0], n, n))
                logits = logits.float().contiguous()
                if acc is None:
                    cout = 1 if self.kind == SIGMOID1 else logits.shape[1]
                    acc = torch.zeros((cout, H, W), dtype=torch.float32, device=dev)
                blend(logits, self.kind, tab, self.overlap, acc)
        finalize(acc, wy, wx)
        return acc


def decode_damage(maps, kind):
    """blended maps of a damage model -> what utils.post_process.post_process_tiles takes: softmax maps as they are (4 or 5
    channels), coral 1 + sum_k [p_k > 0.5], mse round(v) + 1 - the last two as int32 label maps (Model._decode)"""
    import torch
    if kind == SOFTMAX:
        return maps
    if kind == SIGMOID:
        return ((maps > 0.5).sum(dim=0) + 1).to(torch.int32)
    if kind == RELU:
        return (torch.round(maps[0]) + 1).to(torch.int32)
    raise ValueError("decode_damage: kind %r is no damage decode" % (kind,))


def predict_pair(loc, dmg, pre_u8, post_u8, components=False, dilate=False, dilation_rate=3, buildings=False):
    """loc, dmg: ScenePredictors of a localization and a damage model -> (uint8 [H, W] localization, uint8 [H, W] damage),
    through utils.post_process.post_process_tiles at scene size.  buildings=True: a third value, the int64 [n, 16] table of
    the buildings the two maps show (utils.buildings.building_table, confidence from the blended localization map)."""
    from .utils.post_process import post_process_tiles
    loc_map = loc.predict(pre_u8)[0]
    dmg_map = decode_damage(dmg.predict(pre_u8, post_u8), dmg.kind)
    pre, post = post_process_tiles(loc_map, dmg_map, components, dilate, dilation_rate)
    if not buildings:
        return pre, post
    from .utils.buildings import building_table
    return pre, post, building_table(pre, post, loc_map)
