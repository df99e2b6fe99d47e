"""`--autoaugment` split into DECISIONS and BYTES, like the default recipe (device_aug.py).

autoaugment.draw_policy draws the decisions of one sample: 0 .. 2 operations (op, magnitude, sign).  `autoaug_numpy` turns
(cropped uint8 tile, mask, decisions) into the bytes that ImageNetPolicy produces through Pillow - every one of the ten
operations of the POLICY table restated as integer, float32 or float64 arithmetic in Pillow's own order of operations
(tests/test_autoaug_cpu.py pins each against the installed Pillow, byte for byte) - and `pack_policy` packs the decisions of a
batch for include/xv2.h xv2_autoaugment_u8, which computes the same bytes on the GPU (tests/test_autoaug_gpu.py).

The tile's stored B,G,R bytes are handed to PIL as if they were "RGB" (pytorch_loader._TrainBase._augment), so everything here
follows the STORED channel order 0, 1, 2 of each 3-channel part.

    point tables   posterize, solarize, invert: 256-byte tables built on the host (ImageOps builds the same lists)
                   autocontrast, equalize: tables from the per-channel histogram (ImageOps.autocontrast / equalize)
    blends         color, contrast, sharpness: ImageEnhance = Image.blend(degenerate, image, f), float32 (libImaging/Blend.c)
    gathers        rotate: NEAREST affine gather in 16.16 fixed point, zero fill (libImaging/Geometry.c affine_fixed)
                   shearX: BICUBIC affine transform in float64, zero fill (Geometry.c affine_transform + bicubic_filter)

shearY, translateX, translateY and brightness do not occur in POLICY: ValueError."""
import math

import numpy as np

from .autoaugment import GEOMETRIC

# operation ids of a parameter row (csrc/autoaug.hip)
OP_NONE, OP_TABLE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_COLOR, OP_CONTRAST, OP_SHARPNESS, OP_ROTATE, OP_SHEARX = range(9)
ROW = 8                 # int32 per (sample, stage): {op, six operands, reserved}
_IDS = {"posterize": OP_TABLE, "solarize": OP_TABLE, "invert": OP_TABLE, "autocontrast": OP_AUTOCONTRAST,
        "equalize": OP_EQUALIZE, "color": OP_COLOR, "contrast": OP_CONTRAST, "sharpness": OP_SHARPNESS, "rotate": OP_ROTATE,
        "shearX": OP_SHEARX}
MAX_ROTATE = 4096       # a2 + a1 * y + a0 * x stays inside int32 (|a| <= 2^16, three terms <= 2^28 each)


def _known(op):
    if op not in _IDS:
        raise ValueError("AutoAugment operation %r has no device twin (it is not in the POLICY table)" % (op,))


def point_table(op, mag):
    """uint8 [256]: ImageOps.posterize / solarize / invert as the table they pass to Image.point"""
    i = np.arange(256)
    if op == "posterize":
        return (i & ~(2 ** (8 - int(mag)) - 1)).astype(np.uint8)
    if op == "solarize":
        return np.where(i < float(mag), i, 255 - i).astype(np.uint8)
    if op == "invert":
        return (255 - i).astype(np.uint8)
    raise ValueError("no host-built table for %r" % (op,))


def autocontrast_table(hist):
    """ImageOps.autocontrast(cutoff=0) of one channel: int64 [256] counts -> uint8 [256], or None (channel unchanged)"""
    nz = np.nonzero(hist)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return None
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.clip((np.arange(256, dtype=np.float64) * scale + offset).astype(np.int64), 0, 255).astype(np.uint8)


def equalize_table(hist):
    """ImageOps.equalize of one channel: int64 [256] counts -> uint8 [256], or None (channel unchanged).  Image.point clips the
    table to 255: in an image of fewer than ~65 000 pixels the last entries exceed it"""
    histo = hist[hist > 0]
    if histo.size <= 1:
        return None
    step = (int(histo.sum()) - int(histo[-1])) // 255
    if step == 0:
        return None
    n = step // 2 + np.concatenate(([0], np.cumsum(hist.astype(np.int64))[:-1]))
    return np.minimum(n // step, 255).astype(np.uint8)


def luma(part):
    """convert("L") of a 3-channel part (libImaging/Convert.c L24): uint8 [h, w]"""
    p = part.astype(np.int64)
    return ((p[:, :, 0] * 19595 + p[:, :, 1] * 38470 + p[:, :, 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, i, f):
    """Image.blend(d, i, f) on uint8 arrays (libImaging/Blend.c): float32 d + f * (i - d), truncated; clipped outside 0 <= f <= 1"""
    f = np.float32(f)
    d32 = d.astype(np.float32)
    t = d32 + f * (i.astype(np.float32) - d32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def smooth(part):
    """ImageFilter.SMOOTH (libImaging/Filter.c ImagingFilter3x3): float32, interior only, the 1-pixel border is copied"""
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)
    out = part.copy()
    h, w = part.shape[:2]
    if h < 3 or w < 3:
        return out
    a = part.astype(np.float32)
    ss = np.full((h - 2, w - 2) + part.shape[2:], 0.5, dtype=np.float32)
    for j, r in enumerate((2, 1, 0)):           # rows y + 1, y, y - 1
        rows = a[r:r + h - 2]
        ss = ss + ((rows[:, 0:w - 2] * k[3 * j] + rows[:, 1:w - 1] * k[3 * j + 1]) + rows[:, 2:w] * k[3 * j + 2])
    out[1:-1, 1:-1] = np.clip(np.floor(ss), 0, 255).astype(np.uint8)
    return out


def rotate_coeffs(angle, h, w):
    """Image.rotate(angle) as the six 16.16 fixed-point coefficients of Geometry.c affine_fixed: the matrix as PIL/Image.py
    builds it (rounded cosine / sine, centre (w / 2, h / 2)), the half-pixel offset folded into a2 and a5"""
    if max(h, w) > MAX_ROTATE:
        raise ValueError("rotate: %dx%d leaves the fixed-point range" % (h, w))
    angle = float(angle) % 360.0
    cx, cy = w / 2.0, h / 2.0
    rad = -math.radians(angle)
    m = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate(a, coeffs):
    """uint8 [h, w, ...] gathered through the fixed-point map, zero outside the image"""
    h, w = a.shape[:2]
    a0, a1, a2, a3, a4, a5 = coeffs
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xs, ys = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
    ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    out = a[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]
    out[~ok] = 0
    return out


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def shear_x(a, c):
    """transform(AFFINE, (1, c, 0, 0, 1, 0), BICUBIC, fillcolor=0) of uint8 [h, w, ...]: float64, taps clamped to the image,
    zero where the source point leaves it, truncated and clipped"""
    h, w = a.shape[:2]
    c = float(c)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    xin = 1.0 * (x + 0.5) + c * (y + 0.5) + 0.0
    yin = y + 0.5
    ok = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin, yin = xin - 0.5, yin - 0.5
    xb, yb = np.floor(xin), np.floor(yin)
    dx, dy = xin - xb, yin - yb
    xb, yb = xb.astype(np.int64) - 1, yb.astype(np.int64) - 1
    shape = (h, w) + (1,) * (a.ndim - 2)
    dx, dy = dx.reshape(shape), dy.reshape(shape)
    src = a.astype(np.float64)
    rows = []
    for j in range(4):
        r = np.clip(yb + j, 0, h - 1)
        rows.append(_cubic(*[src[r, np.clip(xb + i, 0, w - 1)] for i in range(4)], dx))
    v = _cubic(*rows, dy)
    out = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v)).astype(np.uint8)
    out[~ok] = 0
    return out


def _op_part(part, op, mag, sign):
    """one operation on one 3-channel part"""
    if op in ("posterize", "solarize", "invert"):
        return point_table(op, mag)[part]
    if op in ("autocontrast", "equalize"):
        out = part.copy()
        for c in range(part.shape[2]):
            hist = np.bincount(part[:, :, c].ravel(), minlength=256)
            lut = autocontrast_table(hist) if op == "autocontrast" else equalize_table(hist)
            if lut is not None:
                out[:, :, c] = lut[part[:, :, c]]
        return out
    f = 1 + mag * sign
    if op == "color":
        return blend(np.repeat(luma(part)[:, :, None], 3, 2), part, f)
    if op == "contrast":
        m = int(luma(part).astype(np.int64).sum() / (part.shape[0] * part.shape[1]) + 0.5)
        return blend(np.full_like(part, m), part, f)
    if op == "sharpness":
        return blend(smooth(part), part, f)
    if op == "rotate":
        return rotate(part, rotate_coeffs(mag, part.shape[0], part.shape[1]))
    return shear_x(part, mag * sign)


def autoaug_numpy(img, mask, ops):
    """(uint8 [h, w, 3 * parts], uint8 [h, w], [(op, magnitude, sign)]) -> (image, mask) after the operations in order: each on
    every 3-channel part, the geometric ones on the mask too (shearX INTERPOLATES the labels, as the reference does).  The
    numpy statement of xv2_autoaugment_u8, bit-equal to ImageNetPolicy through Pillow"""
    img, mask = np.ascontiguousarray(img), np.ascontiguousarray(mask)
    for op, mag, sign in ops:
        _known(op)
        img = np.concatenate([_op_part(img[:, :, i:i + 3], op, mag, sign) for i in range(0, img.shape[2], 3)], 2)
        if op in GEOMETRIC:
            mask = _op_part(mask[:, :, None], op, mag, sign)[:, :, 0]
    return np.ascontiguousarray(img), np.ascontiguousarray(mask)


def pack_policy(ops_list, h, w):
    """-> int32 [N * 2 * 8 + N * 2 * 64]: the parameter rows of xv2_autoaugment_u8 ([N][2] stages of {op, six operands, 0})
    followed by the [N][2][256] uint8 host-built point tables, ONE upload.  ops_list: per sample the 0 .. 2 decisions of
    draw_policy; a sample with one operation runs it in the first stage"""
    n = len(ops_list)
    buf = np.zeros(n * 2 * ROW + n * 2 * 64, dtype=np.int32)
    prm = buf[:n * 2 * ROW].reshape(n, 2, ROW)
    luts = buf[n * 2 * ROW:].view(np.uint8).reshape(n, 2, 256)
    for i, ops in enumerate(ops_list):
        if len(ops) > 2:
            raise ValueError("a sub-policy has two operations, sample %d has %d" % (i, len(ops)))
        for s, (op, mag, sign) in enumerate(ops):
            _known(op)
            prm[i, s, 0] = _IDS[op]
            if _IDS[op] == OP_TABLE:
                luts[i, s] = point_table(op, mag)
            elif op in ("color", "contrast", "sharpness"):
                prm[i, s, 1:2].view(np.float32)[0] = np.float32(1 + mag * sign)
            elif op == "rotate":
                prm[i, s, 1:7] = rotate_coeffs(mag, h, w)
            elif op == "shearX":
                prm[i, s, 2:4].view(np.float64)[0] = float(mag * sign)
    return buf
