"""Split buildings that touch: a row of houses predicted without gaps is one 4-connected component, so it is one row of
the table, one polygon and one voted damage class.  This step cuts such a blob where it is narrow.

The rule (include/xv2.h, "split touching buildings") on the MI355X (csrc/split.hip): erode the localization mask by a disc
of radius R (an exact squared distance, d^2 > R^2), take the surviving cores as seeds, grow them back inside the mask by
4-connected geodesic distance, and cut a 1-pixel line of background where two grown pieces meet.  A building with at most one
core is returned untouched, so thin and small buildings stay as they are.  The result is a mask again: everything that reads
the two PNGs (utils.buildings, utils.polygons, utils.building_metrics) works on it unchanged.  A straight neck n pixels wide
is cut iff ceil(n / 2) <= R.

    python -m xview2_amd.utils.split PRE.png POST.png OUT_PRE.png OUT_POST.png --radius R
"""
from argparse import ArgumentParser

import numpy as np


def check_radius(radius):
    r = int(radius)
    if not 1 <= r <= 63:
        raise ValueError("the split radius must lie in 1..63, got %d" % r)
    return r


def split_maps(pre, post, radius):
    """pre, post: uint8 [H,W] or [B,H,W] device maps (the label maps of the two PNGs).  Returns (pre', post') with
    pre' = pre cut where buildings touch (r2 = radius^2) and post' = post * (pre' != 0)."""
    from .. import ops
    r = check_radius(radius)
    single = pre.dim() == 2
    if single:
        pre, post = pre.unsqueeze(0), post.unsqueeze(0)
    if pre.shape != post.shape:
        raise ValueError("split_maps: pre and post must have one shape, got %s and %s" % (tuple(pre.shape), tuple(post.shape)))
    pre2, _ = ops.split_buildings(pre, r * r)
    post2 = post * (pre2 != 0).to(post.dtype)
    return (pre2[0], post2[0]) if single else (pre2, post2)


def get_parser():
    p = ArgumentParser(description="cut the localization PNG where buildings touch and mask the damage PNG with the result")
    p.add_argument("pre")
    p.add_argument("post")
    p.add_argument("out_pre")
    p.add_argument("out_post")
    p.add_argument("--radius", type=int, required=True, help="erosion radius R in pixels (1..63): necks up to 2 R wide are cut")
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.split runs on the MI355X only; there is no CPU fallback")
    pre, post = (np.asarray(Image.open(p)) for p in (a.pre, a.post))
    if pre.ndim != 2 or pre.shape != post.shape or pre.dtype != np.uint8 or post.dtype != np.uint8:
        raise ValueError("%s and %s must be 8-bit single-channel images of one size" % (a.pre, a.post))
    dev = torch.device("cuda", torch.cuda.current_device())
    pre2, post2 = split_maps(torch.from_numpy(pre.copy()).to(dev), torch.from_numpy(post.copy()).to(dev), a.radius)
    Image.fromarray(pre2.cpu().numpy()).save(a.out_pre)
    Image.fromarray(post2.cpu().numpy()).save(a.out_post)
    return int((pre2 != torch.from_numpy(pre.copy()).to(dev)).sum().item())


if __name__ == "__main__":
    print("%d pixels cut" % main())
