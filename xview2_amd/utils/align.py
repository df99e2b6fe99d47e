"""Register a post image to its pre image by an integer translation, and report how well a translation can do it.

Every damage model reads a pair pixel against pixel, and two acquisitions of one place are rarely registered to the pixel.
The rule (include/xv2.h, "register the post image to the pre image") on the MI355X (csrc/align.hip): luma of both images, the
sum of absolute differences S(d) between pre(p) and post(p + d) over the interior of the scene for every shift |dy|, |dx| <= R,
the shift with the smallest sum (ties to the shortest shift), and a resampling of post by that shift that reflects at the
border.  The same table per tile of T x T pixels says whether one translation fits the whole pair: tiles that disagree with
the global shift are parallax or a warp, which are reported and not corrected.  Shifts are whole pixels; there is no rotation
and no scale; no radius is recommended.

    python -m xview2_amd.utils.align PRE POST OUT [--radius R] [--tile T] [--json J]

PRE / POST / OUT are files, or directories paired by sorted order as xview2_amd.predict pairs them.  OUT receives the aligned
post image(s) under the post images' names, J (by default <OUT stem>_alignment.json, or OUT/alignment.json for a directory)
the report; for a directory the report holds one entry per pair and a histogram of the shifts found, which is the tool for
asking how misregistered a dataset is.  This module imports without a GPU; only align_scene and the command line need one."""
import json
import os
from argparse import ArgumentParser

import numpy as np

TILES = (32, 64, 128)


def check_radius(radius):
    r = int(radius)
    if not 1 <= r <= 32:
        raise ValueError("the alignment radius must lie in 1..32, got %d" % r)
    return r


def check_tile(tile):
    t = int(tile)
    if t not in TILES:
        raise ValueError("the alignment tile must be one of %s, got %d" % (TILES, t))
    return t


def _fixed(num, den):
    """num / den rounded half up to six decimals, by integer arithmetic: the same characters everywhere"""
    q = (2 * 10 ** 6 * int(num) + int(den)) // (2 * int(den))
    return "%d.%06d" % divmod(q, 10 ** 6)


def summarise(block_sad, sad, block_shift, shift, R, T, H, W):
    """The report of one pair from the four tables of xv2_align_estimate (arrays of one image: [nby,nbx,D,D], [D,D],
    [nby,nbx,2], [2]).  Integers, exact ratios as strings and fixed-format decimals as strings: the same input gives the same
    bytes through dumps()."""
    block_sad, sad = np.asarray(block_sad).astype(np.int64), np.asarray(sad).astype(np.int64)
    block_shift, shift = np.asarray(block_shift).astype(np.int64), np.asarray(shift).astype(np.int64)
    R, T, H, W = int(R), int(T), int(H), int(W)
    D = 2 * R + 1
    nby, nbx = -(-(H - 2 * R) // T), -(-(W - 2 * R) // T)
    if block_sad.shape != (nby, nbx, D, D) or sad.shape != (D, D) or block_shift.shape != (nby, nbx, 2) or shift.shape != (2,):
        raise ValueError("summarise: tables %s %s %s %s do not belong to R=%d T=%d H=%d W=%d" % (
            block_sad.shape, sad.shape, block_shift.shape, shift.shape, R, T, H, W))
    dy, dx = int(shift[0]), int(shift[1])
    pixels = (H - 2 * R) * (W - 2 * R)
    zero, best = int(sad[R, R]), int(sad[dy + R, dx + R])
    flat = block_sad.max(axis=(2, 3)) == block_sad.min(axis=(2, 3))
    diff = np.abs(block_shift - shift).max(axis=2)
    return {
        "radius": R, "tile": T, "shift": [dy, dx], "pixels": pixels,
        "sad_zero": zero, "sad_best": best,
        "mean_abs_zero": _fixed(zero, pixels), "mean_abs_zero_exact": "%d/%d" % (zero, pixels),
        "mean_abs_best": _fixed(best, pixels), "mean_abs_best_exact": "%d/%d" % (best, pixels),
        "at_limit": bool(abs(dy) == R or abs(dx) == R),
        "blocks": {
            "grid": [nby, nbx],
            "shifts": block_shift.tolist(),
            "flat": int(flat.sum()),
            "agree": int((diff == 0).sum()),
            "spread": int(diff[~flat].max()) if (~flat).any() else 0,
        },
    }


def dumps(report):
    return json.dumps(report, indent=1, sort_keys=True) + "\n"


def histogram(reports):
    """[[dy, dx, pairs]] over the reports' global shifts, sorted by (dy, dx)"""
    counts = {}
    for r in reports:
        counts[tuple(r["shift"])] = counts.get(tuple(r["shift"]), 0) + 1
    return [[dy, dx, n] for (dy, dx), n in sorted(counts.items())]


def report_of(info, H, W):
    """summarise() of what scene.align_pair returned as info (device tables of one pair): the read-back"""
    t = [info[k][0].cpu().numpy() for k in ("block_sad", "sad", "block_shift", "shift")]
    return summarise(t[0], t[1], t[2], t[3], info["radius"], info["tile"], H, W)


def get_parser():
    p = ArgumentParser(prog="python -m xview2_amd.utils.align",
                       description="shift the post image by the whole-pixel translation that matches it best to the pre image")
    p.add_argument("pre", help="pre image, or a directory of them")
    p.add_argument("post", help="post image or directory (paired with pre by sorted order)")
    p.add_argument("out", help="aligned post image, or the directory they are written to")
    p.add_argument("--radius", type=int, default=8, help="search radius R in pixels (1..32): shifts up to R in either direction "
                   "are compared; a result with at_limit set may be a larger true offset.  No value is recommended; the default "
                   "only bounds the search")
    p.add_argument("--tile", type=int, default=128, choices=list(TILES), help="side of the tiles whose own best shifts are reported")
    p.add_argument("--json", type=str, default=None, help="the report (default <out stem>_alignment.json, or out/alignment.json)")
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    R, T = check_radius(a.radius), check_tile(a.tile)
    import torch
    from PIL import Image
    from .. import scene
    from ..predict import pair_inputs, read_bgr
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.align runs on the MI355X only; there is no CPU fallback")
    pairs = pair_inputs(a.pre, a.post)
    many = os.path.isdir(a.pre)
    if many:
        os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    reports = {}
    for pre_path, post_path in pairs:
        pre, post = read_bgr(pre_path), read_bgr(post_path)
        if pre.shape != post.shape:
            raise ValueError("%s is %d x %d but %s is %d x %d" % (pre_path, pre.shape[0], pre.shape[1], post_path,
                                                                   post.shape[0], post.shape[1]))
        aligned, info = scene.align_pair(torch.from_numpy(pre).to(dev), torch.from_numpy(post).to(dev), R, T)
        target = os.path.join(a.out, os.path.basename(post_path)) if many else a.out
        Image.fromarray(np.ascontiguousarray(aligned.cpu().numpy()[:, :, ::-1])).save(target)
        reports[os.path.splitext(os.path.basename(pre_path))[0]] = report_of(info, pre.shape[0], pre.shape[1])
    if many:
        report = {"pairs": reports, "histogram": histogram(reports.values())}
        path = a.json or os.path.join(a.out, "alignment.json")
    else:
        report = next(iter(reports.values()))
        path = a.json or os.path.splitext(a.out)[0] + "_alignment.json"
    with open(path, "w") as f:
        f.write(dumps(report))
    return len(pairs)


if __name__ == "__main__":
    print("aligned %d pairs" % main())
