"""The border weight map of the ``wce`` loss term for one target PNG, to look at before training with it.

The map (include/xv2.h, "wce") on the MI355X (csrc/wce.hip): for a background pixel, d1 and d2 are the distances to the nearest
and the second-nearest 4-connected component of label > 0 within ``--radius`` pixels, and the weight is
``weight * exp(-(d1 + d2)^2 / (2 sigma^2))`` (Ronneberger et al., U-Net, 2015); 0 on buildings and where fewer than two
buildings are within reach.  It is the map ``--loss_str wce --border_weight W --border_sigma S --border_radius R`` adds to the
class weight of every pixel, evaluated by the same device function.  Labelled buildings that touch are one component and get no
border between them.

    python -m xview2_amd.utils.border_map TARGET.png OUT.npy [--weight 10 --sigma 5 --radius 0]
"""
import math
from argparse import ArgumentParser

import numpy as np


def default_radius(sigma):
    """--border_radius 0: where the map has fallen to exp(-4.5) of its weight even for d2 = 0, capped at the kernel's 32"""
    return min(32, max(1, math.ceil(3.0 * sigma)))


def border_map(target, weight, sigma, radius=0):
    """target: uint8 [H,W] or [B,H,W] device label map -> fp32 map of the same shape"""
    from .. import ops
    single = target.dim() == 2
    t = target.unsqueeze(0) if single else target
    d1, d2 = ops.border_distances(t, radius or default_radius(sigma))
    out = ops.border_weights(d1, d2, weight, sigma)
    return out[0] if single else out


def get_parser():
    p = ArgumentParser(description="write the fp32 border weight map of one target PNG as .npy")
    p.add_argument("target")
    p.add_argument("out")
    p.add_argument("--weight", type=float, default=10.0, help="w0 of the map (--border_weight)")
    p.add_argument("--sigma", type=float, default=5.0, help="sigma in pixels (--border_sigma)")
    p.add_argument("--radius", type=int, default=0, help="search radius 1..32 (--border_radius; 0: min(32, ceil(3 sigma)))")
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.border_map runs on the MI355X only; there is no CPU fallback")
    t = np.asarray(Image.open(a.target))
    if t.ndim != 2 or t.dtype != np.uint8:
        raise ValueError("%s must be an 8-bit single-channel image" % a.target)
    dev = torch.device("cuda", torch.cuda.current_device())
    m = border_map(torch.from_numpy(t.copy()).to(dev), a.weight, a.sigma, a.radius).cpu().numpy()
    np.save(a.out, m)
    return m


if __name__ == "__main__":
    m = main()
    print("%d of %d pixels weighted, max %.4g" % (int((m > 0).sum()), m.size, float(m.max())))
