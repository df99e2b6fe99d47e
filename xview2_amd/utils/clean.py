"""Fill small holes in buildings and drop small buildings: every output after the network takes a 4-connected component of the
localization map for a building, so one false-positive pixel is a table row, a polygon and a false positive of the
object-level score, and a one-pixel dropout inside a roof is a hole ring in the GeoJSON.

The rule (include/xv2.h, "clean buildings") on the MI355X (csrc/clean.hip), in two stages.  Fill: a hole is an 8-connected
component of background that does not touch the tile's outer frame; a hole of at most --fill_holes pixels becomes building
(pre = 1) and takes the voted damage class of the building around it.  Drop: in the filled map a 4-connected building of
fewer than --min_area pixels becomes background in both maps.  Every other pixel keeps its bytes.  The result is a pair of
maps again: everything that reads the two PNGs (utils.split, utils.buildings, utils.polygons, utils.building_metrics) works on
it unchanged.  Background goes by 8-connectivity, so a courtyard joined to the outside only through a diagonal step is no
hole, and a hole on the frame is never filled.  Both values default to 0 = off; no value is recommended.

    python -m xview2_amd.utils.clean PRE.png POST.png OUT_PRE.png OUT_POST.png --min_area A --fill_holes M
"""
from argparse import ArgumentParser

import numpy as np

STAT_KEYS = ("holes_filled", "pixels_filled", "buildings_dropped", "pixels_dropped")


def _check(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError("%s must be an integer >= 0, got %r" % (name, value))
    if value < 0:
        raise ValueError("%s must be an integer >= 0, got %d" % (name, value))
    return int(value)


def check_min_area(min_area):
    """the smallest area in pixels a building keeps: an integer >= 0, 0 and 1 drop nothing"""
    return _check("min_area", min_area)


def check_fill_holes(fill_holes):
    """the largest hole in pixels that is filled: an integer >= 0, 0 fills nothing"""
    return _check("fill_holes", fill_holes)


def clean_maps(pre, post, min_area=0, fill_holes=0, return_stats=False):
    """pre, post: uint8 [H,W] or [B,H,W] device maps (the label maps of the two PNGs).  Returns (pre', post'): holes of at
    most fill_holes pixels filled, then buildings of fewer than min_area pixels dropped; with return_stats also the device
    int64 [B,4] (or [4]) of STAT_KEYS."""
    from .. import ops
    a, m = check_min_area(min_area), check_fill_holes(fill_holes)
    single = pre.dim() == 2
    if single:
        pre, post = pre.unsqueeze(0), post.unsqueeze(0)
    if pre.shape != post.shape:
        raise ValueError("clean_maps: pre and post must have one shape, got %s and %s" % (tuple(pre.shape), tuple(post.shape)))
    pre2, post2, stats = ops.clean_buildings(pre, post, a, m)
    if single:
        pre2, post2, stats = pre2[0], post2[0], stats[0]
    return (pre2, post2, stats) if return_stats else (pre2, post2)


def totals(stats):
    """device stats [B,4] or [4] -> {STAT_KEYS: Python int}, summed over the tiles (one copy to the host)"""
    s = stats.reshape(-1, 4).sum(0).cpu().tolist()
    return {k: int(v) for k, v in zip(STAT_KEYS, s)}


def get_parser():
    p = ArgumentParser(description="fill small holes in the buildings of the localization PNG, drop small buildings, and "
                       "carry both changes into the damage PNG")
    p.add_argument("pre")
    p.add_argument("post")
    p.add_argument("out_pre")
    p.add_argument("out_post")
    p.add_argument("--min_area", type=int, default=0, metavar="A", help="drop buildings of fewer than A pixels, 0 = off")
    p.add_argument("--fill_holes", type=int, default=0, metavar="M", help="fill holes of at most M pixels, 0 = off")
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    min_area, fill_holes = check_min_area(a.min_area), check_fill_holes(a.fill_holes)
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.clean runs on the MI355X only; there is no CPU fallback")
    pre, post = (np.asarray(Image.open(p)) for p in (a.pre, a.post))
    if pre.ndim != 2 or pre.shape != post.shape or pre.dtype != np.uint8 or post.dtype != np.uint8:
        raise ValueError("%s and %s must be 8-bit single-channel images of one size" % (a.pre, a.post))
    dev = torch.device("cuda", torch.cuda.current_device())
    pre2, post2, stats = clean_maps(torch.from_numpy(pre.copy()).to(dev), torch.from_numpy(post.copy()).to(dev), min_area,
                                    fill_holes, return_stats=True)
    Image.fromarray(pre2.cpu().numpy()).save(a.out_pre)
    Image.fromarray(post2.cpu().numpy()).save(a.out_post)
    return totals(stats)


if __name__ == "__main__":
    t = main()
    print("%d holes filled (%d pixels), %d buildings dropped (%d pixels)" % tuple(t[k] for k in STAT_KEYS))
