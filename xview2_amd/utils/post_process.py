"""Post-processing of the evaluation outputs (reference utils/post_process.py) on the MI355X.

`main.py --exec_mode eval` writes probs/test_{localization,damage}_NNNNN.npy; this step fuses each pair, optionally
replaces every predicted building's damage by its majority class (--components) and dilates both maps (--dilate), and
writes predictions/test_{localization,damage}_NNNNN_prediction.png.  The work runs in the HIP kernels of
csrc/postproc.hip (xv2_postprocess), a batch of tiles per launch sequence; there is no host path.

Semantics are the reference's (post_process.py:27-47), bit for bit, with these deliberate departures:
  1. five-channel damage probabilities (a softmax that carries a background channel first) use
     post = argmax(dmg[1:5]) + 1: the background channel is dropped and the four-channel rule applies.  The reference
     raises IndexError on this input.  Four-channel input and label maps behave as in the reference;
  2. the dilation rate must be odd (>= 1): an even rate raises ValueError (skimage's centring of even footprints has
     changed between releases);
  3. tiles of any H x W are accepted (the reference hard-codes 1024 x 1024);
  4. the CLI takes --results DIR (default /results, the reference's fixed root) and --batch N;
  5. label maps (coral / mse decodes) are converted to int32.  Values dropped by the fusion are never looked at, so
     an unclamped mse decode on background behaves as in the reference.  A value that survives it must fit the
     output: 0..255 without --components, 1..4 with it (the vote keeps four classes per building); otherwise
     ValueError, where the reference would vote over it and write a PNG its scorer rejects.

    python -m xview2_amd.utils.post_process --results R [--components] [--dilate [--dilation_rate 3]] [--split R]
                                            [--min_area A] [--fill_holes M] [--buildings] [--polygons [--simplify T]]

--buildings also writes buildings/test_buildings_NNNNN.csv per pair: one row per predicted building of the two PNGs
(xview2_amd.utils.buildings), its confidence from the localization probabilities.  --polygons (which implies --buildings)
adds buildings/test_buildings_NNNNN.geojson: the outline of every building, traced from the same label map
(xview2_amd.utils.polygons); --simplify T reduces those outlines by Douglas-Peucker with a tolerance of T pixels and changes the
GeoJSON only.  --split R cuts the localization map where buildings touch (xview2_amd.utils.split: erosion
by a disc of radius R, cores grown back, a 1-pixel cut where they meet) and masks the damage map with it.  The order is fuse,
dilate, split, vote: a dilation after the split would close the cuts again, and the vote of --components is then taken per
split piece.  The PNGs, the CSV and the GeoJSON all come from the split maps.  --fill_holes M fills holes of at most M pixels
inside buildings and --min_area A then drops buildings of fewer than A pixels (xview2_amd.utils.clean), both before the split:
the order is fuse, dilate, clean, split, vote.  Both default to 0 = off, and then no call and no byte changes.
--loc_threshold A, --loc_threshold_dmg B and --class_scale s1,s2,s3,s4 (utils/fusion.py) replace the fusion's constants:
pre = (loc > A) | ((loc > B) & (post > 1)), post = argmax(s * dmg) + 1; --calibration FILE.json takes them from a report of
xview2_amd.utils.calibrate, explicit flags winning.  Without any of them the reference's 0.3 / 0.1 / no scales apply through
the call that was always made.
"""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser, ArgumentTypeError
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np
import torch

from .. import ops
from . import fusion


def _check_rate(dilate, dilation_rate):
    if not dilate:
        return 0
    r = int(dilation_rate)
    if r < 1 or r % 2 == 0:
        raise ValueError("dilation_rate must be odd and >= 1, got %d" % r)
    return r


def post_process_tiles(loc, dmg, components=False, dilate=False, dilation_rate=3, workspace=None, split=0, min_area=0,
                       fill_holes=0, return_stats=False, loc_threshold=None, dmg_threshold=None, class_scale=None):
    """uint8 (pre, post) on the device.  loc: fp32 [H,W] or [B,H,W]; dmg: [4|5,H,W] / [B,4|5,H,W] probabilities or an
    [H,W] / [B,H,W] label map.  Unbatched input gives unbatched output.  split > 0: fuse and dilate first, cut pre where
    buildings touch (utils.split.split_maps with that radius) and mask post with it, and only then, with components, vote
    per split piece: a second pass over the split maps (pre' as the localization, post' as a label map, no dilation).
    min_area > 0 or fill_holes > 0: utils.clean.clean_maps after the dilation and before the split, so that filled roofs
    erode as solid shapes and the pieces a split makes are not deleted afterwards; the vote is then taken on the cleaned
    maps by the same second pass.  return_stats: a third value, the device int64 [B,4] (or [4]) of clean_maps, None
    when neither is set.  loc_threshold, dmg_threshold, class_scale (ops.postprocess) apply to the fusing pass only: the
    second pass reads a 0/1 map as its localization and keeps the defaults."""
    # only what was given: with the defaults ops.postprocess gets the call it always got
    fuse_kw = {k: v for k, v in (("loc_threshold", loc_threshold), ("dmg_threshold", dmg_threshold),
                                ("class_scale", class_scale)) if v is not None}
    rate = _check_rate(dilate, dilation_rate)
    single = loc.dim() == 2
    if single:
        loc, dmg = loc.unsqueeze(0), dmg.unsqueeze(0)
    stats = None
    if split or min_area or fill_holes:
        pre, post = ops.postprocess(loc, dmg, components=False, rate=rate, workspace=workspace, **fuse_kw)
        if min_area or fill_holes:
            from .clean import clean_maps
            pre, post, stats = clean_maps(pre, post, min_area, fill_holes, return_stats=True)
        if split:
            from .split import split_maps
            pre, post = split_maps(pre, post, split)
        if components:
            pre, post = ops.postprocess(pre.float(), post.to(torch.int32), components=True, rate=0, workspace=workspace)
    else:
        pre, post = ops.postprocess(loc, dmg, components=components, rate=rate, workspace=workspace, **fuse_kw)
    if single:
        pre, post, stats = pre[0], post[0], (stats[0] if stats is not None else None)
    return (pre, post, stats) if return_stats else (pre, post)


def connected_components(mask):
    """int32 labels of the 4-connected components of mask != 0 ([H,W] or [B,H,W], on the device): 1 + the smallest
    linear index of the component within its tile, 0 for background.  np.unique(labels, return_inverse=True) gives
    scipy.ndimage.label's numbering."""
    single = mask.dim() == 2
    lab = ops.label_components(mask.unsqueeze(0) if single else mask)
    return lab[0] if single else lab


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.post_process runs on the MI355X only; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=False)


def _save(img, path):
    from PIL import Image
    Image.fromarray(img).save(path)


def _out_name(path):
    return os.path.basename(path).replace(".npy", "_prediction.png")


def _buildings_name(pre_path):
    base = os.path.basename(pre_path)
    return (base[:-4] if base.endswith(".npy") else base).replace("localization", "buildings") + ".csv"


def post_process(args, pre_path, post_path):
    """one pair of .npy files -> two prediction PNGs under <args.results>/predictions (reference signature)"""
    results = getattr(args, "results", "/results")
    dev = _device()
    loc, dmg = _to_device(np.load(pre_path), dev), _to_device(np.load(post_path), dev)
    pre, post = post_process_tiles(loc, dmg, args.components, args.dilate, args.dilation_rate,
                                   split=getattr(args, "split", 0), min_area=getattr(args, "min_area", 0),
                                   fill_holes=getattr(args, "fill_holes", 0), **fusion.resolve(args))
    _save(pre.cpu().numpy(), os.path.join(results, "predictions", _out_name(pre_path)))
    _save(post.cpu().numpy(), os.path.join(results, "predictions", _out_name(post_path)))


def prob_pairs(results):
    """(localization files, damage files) under <results>/probs, sorted: the k-th of each is one pair (as the reference)"""
    pre_paths = sorted(glob(os.path.join(results, "probs", "*localization*")))
    post_paths = sorted(glob(os.path.join(results, "probs", "*damage*")))
    if len(pre_paths) != len(post_paths):
        raise ValueError("%d localization files but %d damage files" % (len(pre_paths), len(post_paths)))
    return pre_paths, post_paths


def geometry_groups(locs, dmgs):
    """(loc shape, dmg shape, dmg dtype) -> indices: one launch per input geometry"""
    groups = {}
    for k, (l, d) in enumerate(zip(locs, dmgs)):
        groups.setdefault((l.shape, d.shape, d.dtype.str), []).append(k)
    return groups


def run(args):
    """the CLI: every probs/*localization* with its probs/*damage* partner (sorted pairing, as the reference), --batch
    pairs per GPU call, PNGs written from a small thread pool"""
    rate = _check_rate(args.dilate, args.dilation_rate)
    split = getattr(args, "split", 0)
    if split:
        from .split import check_radius
        split = check_radius(split)
    min_area, fill_holes = getattr(args, "min_area", 0), getattr(args, "fill_holes", 0)
    if min_area or fill_holes:
        from .clean import check_fill_holes, check_min_area
        min_area, fill_holes = check_min_area(min_area), check_fill_holes(fill_holes)
    if args.batch < 1:
        raise ValueError("--batch must be >= 1, got %d" % args.batch)
    simplify = getattr(args, "simplify", 0.0)
    if simplify:
        from .polygons import quantise_tolerance
        quantise_tolerance(simplify)
    fuse_kw = fusion.resolve(args)
    pred_dir = os.path.join(args.results, "predictions")
    os.makedirs(pred_dir, exist_ok=True)
    pre_paths, post_paths = prob_pairs(args.results)
    dev = _device()
    workspace = {}
    with ThreadPoolExecutor(max_workers=4) as pool:
        pending = []
        for i in range(0, len(pre_paths), args.batch):
            pairs = list(zip(pre_paths[i:i + args.batch], post_paths[i:i + args.batch]))
            locs = [np.load(a) for a, _ in pairs]
            dmgs = [np.load(b) for _, b in pairs]
            for (lshape, _, _), ks in geometry_groups(locs, dmgs).items():
                loc = _to_device(np.stack([locs[k] for k in ks]), dev)
                dmg = _to_device(np.stack([dmgs[k] for k in ks]), dev)
                key = (len(ks),) + tuple(lshape)
                if key not in workspace and (args.components or rate):
                    workspace[key] = ops.postprocess_workspace(len(ks), lshape[0], lshape[1], args.components, dev)
                pre, post = post_process_tiles(loc, dmg, args.components, args.dilate, args.dilation_rate,
                                               workspace.get(key), split=split, min_area=min_area, fill_holes=fill_holes,
                                               **fuse_kw)
                want_polygons = getattr(args, "polygons", False)
                if getattr(args, "buildings", False) or want_polygons:
                    from . import buildings
                    os.makedirs(os.path.join(args.results, "buildings"), exist_ok=True)
                    tables, labels = buildings.building_table(pre, post, loc, return_labels=True)
                    if want_polygons:
                        from . import polygons
                        outlines = polygons.building_polygons(pre, labels, simplify)
                    for j, rows in enumerate(tables):
                        recs = buildings.to_records(rows, lshape[0], lshape[1])
                        name = os.path.join(args.results, "buildings", _buildings_name(pairs[ks[j]][0]))
                        pending.append(pool.submit(buildings.write_csv, name, recs))
                        if want_polygons:
                            pending.append(pool.submit(polygons.write_geojson, name[:-4] + ".geojson", outlines[j], recs))
                pre, post = pre.cpu().numpy(), post.cpu().numpy()
                for j, k in enumerate(ks):
                    a, b = pairs[k]
                    pending.append(pool.submit(_save, pre[j], os.path.join(pred_dir, _out_name(a))))
                    pending.append(pool.submit(_save, post[j], os.path.join(pred_dir, _out_name(b))))
        for f in pending:
            f.result()
    return len(pre_paths)


def _positive_int(text):
    v = int(text)
    if v < 1:
        raise ArgumentTypeError("must be >= 1, got %d" % v)
    return v


def get_parser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter)
    arg = parser.add_argument
    arg("--components", action="store_true", help="Enable connected component analysis for post disaster")
    arg("--dilate", action="store_true", help="Dilate pre and post images")
    arg("--dilation_rate", type=int, default=3, help="Dilation rate (odd)")
    arg("--results", type=str, default="/results", help="Directory holding probs/; predictions/ is written there")
    arg("--batch", type=_positive_int, default=8, help="Tiles per GPU call")
    arg("--buildings", action="store_true", help="Also write buildings/<name>.csv per pair: one row per predicted building")
    arg("--polygons", action="store_true", help="Also write buildings/<name>.geojson per pair: one outline per predicted "
        "building (implies --buildings)")
    arg("--simplify", type=float, default=0.0, metavar="T", help="With --polygons: drop outline vertices that lie within T "
        "pixels of what is left (Douglas-Peucker per ring, 0 <= T < 4096); 0 = off.  No value is recommended")
    arg("--split", type=int, default=0, metavar="R", help="Cut buildings that touch: erosion radius in pixels, 0 = off.  "
        "Applied after --dilate (a dilation after it would close the cuts again) and before the vote of --components")
    arg("--min_area", type=int, default=0, metavar="A", help="Drop predicted buildings of fewer than A pixels, 0 = off.  "
        "Applied after --fill_holes and before --split.  No value is recommended")
    arg("--fill_holes", type=int, default=0, metavar="M", help="Fill holes of at most M pixels inside predicted buildings (a "
        "hole is 8-connected background that does not touch the tile's frame), 0 = off.  No value is recommended")
    fusion.add_flags(arg)
    return parser


if __name__ == "__main__":
    n = run(get_parser().parse_args())
    print("post-processed %d tile pairs" % n)
