"""Apply a trained pair of checkpoints to imagery of any size that has no labels.

    python -m xview2_amd.predict --ckpt_loc loc.ckpt --ckpt_dmg dmg.ckpt --pre pre.png --post post.png --out DIR

--pre / --post take a file or a directory; directories are paired by sorted order and must hold equally many files.  Each
pair is predicted window by window on the GPU (xview2_amd.scene) and written as <stem>_localization_prediction.png and
<stem>_damage_prediction.png, <stem> being the pre image's; --save_probs adds the blended maps as .npy.  With only one
checkpoint only its map is written: the localization map is then the 0.3 threshold of post-processing, the damage map the
decoded class of every pixel.  --buildings adds <stem>_buildings.csv (one row per predicted building: box, area, centroid,
damage class, pixel counts, confidence) and <stem>_buildings.json (totals), computed on the GPU (xview2_amd.utils.buildings).
--polygons adds <stem>_buildings.geojson: the outline of every building with its holes, traced on the GPU from the same label
map (xview2_amd.utils.polygons), with the table's row as properties; it implies --buildings.  --simplify T
reduces those outlines by Douglas-Peucker with a tolerance of T pixels, on the GPU; it changes the GeoJSON only.  --split R cuts the localization
map where buildings touch (xview2_amd.utils.split) before any of these outputs is made: the PNGs, the table and the outlines
all come from the split maps.  --fill_holes M and --min_area A (xview2_amd.utils.clean) fill holes of at most M pixels inside
buildings and then drop buildings of fewer than A pixels, before the split: the PNGs, the table, its JSON (which then lists what
was filled and dropped under "clean") and the outlines all come from the cleaned maps.  --align R registers the post scene to the pre scene first (xview2_amd.utils.align): the
best whole-pixel translation within R pixels is found and applied on the GPU before the damage model sees the pair, and
<stem>_alignment.json reports the shift, the residuals and how far the tiles of the scene agree with it.  --scales s1,s2,...
predicts every scene once per scale and averages the maps (xview2_amd.scene, predict(scales=...)): the scene is resized on the
GPU as Pillow's bicubic resize does it, predicted at that size, and the maps are brought back to the native grid, where the
post-processing and every output stay; --save_probs writes the averaged maps.  One value other than 1 predicts imagery of
another ground resolution (a model trained at 0.5 m per pixel reads a 0.3 m scene at --scales 0.6); --align runs before it, at
the native size.  --loc_threshold A, --loc_threshold_dmg B and --class_scale s1,s2,s3,s4 replace the constants of the fusion
(a building where loc > A, or loc > B with a damage class above 1; the damage class the argmax of s * probabilities), and
--calibration FILE.json takes them from a report of xview2_amd.utils.calibrate, explicit flags winning; scales need a softmax
damage checkpoint.  Without them the reference's 0.3 / 0.1 / plain argmax apply, through the call that was always made."""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")


def get_parser():
    parser = ArgumentParser(prog="python -m xview2_amd.predict", formatter_class=ArgumentDefaultsHelpFormatter)
    arg = parser.add_argument
    arg("--ckpt_loc", type=str, default=None, help="localization checkpoint (--type pre)")
    arg("--ckpt_dmg", type=str, default=None, help="damage checkpoint (--type post)")
    arg("--pre", type=str, required=True, help="pre-disaster image, or a directory of them")
    arg("--post", type=str, default=None, help="post-disaster image or directory (required with --ckpt_dmg)")
    arg("--out", type=str, required=True, help="directory the predictions are written to")
    arg("--window", type=int, default=1024, help="window side (a multiple of 32, 32..2048)")
    arg("--overlap", type=int, default=256, help="pixels two neighbouring windows share (at most half the window)")
    arg("--batch", type=int, default=4, help="windows per model call")
    arg("--tta", action="store_true", help="average every window over the identity and three flips")
    arg("--precision", type=int, default=16, choices=[16, 32], help="32: exact fp32; 16: bf16 matrix math")
    arg("--ema", action="store_true", help="load the checkpoints' averaged weights (ema_state_dict)")
    arg("--components", action="store_true", help="majority damage class per connected building")
    arg("--dilate", action="store_true", help="dilate both maps")
    arg("--dilation_rate", type=int, default=3, help="dilation rate (odd)")
    arg("--save_probs", action="store_true", help="also write the blended probability maps as .npy")
    arg("--buildings", action="store_true", help="also write <stem>_buildings.csv / .json: one row per predicted building")
    arg("--polygons", action="store_true", help="also write <stem>_buildings.geojson: one outline per predicted building "
        "(implies --buildings)")
    arg("--simplify", type=float, default=0.0, metavar="T", help="with --polygons: drop outline vertices that lie within T "
        "pixels of what is left (Douglas-Peucker per ring, 0 <= T < 4096); 0 = off.  No value is recommended")
    arg("--split", type=int, default=0, metavar="R", help="cut buildings that touch: erosion radius in pixels, 0 = off; applied "
        "after --dilate (a dilation after it would close the cuts again) and before the vote of --components")
    arg("--min_area", type=int, default=0, metavar="A", help="drop predicted buildings of fewer than A pixels, 0 = off; applied "
        "after --fill_holes and before --split.  No value is recommended")
    arg("--fill_holes", type=int, default=0, metavar="M", help="fill holes of at most M pixels inside predicted buildings (a "
        "hole is 8-connected background that does not touch the scene's frame), 0 = off.  No value is recommended")
    arg("--align", type=int, default=0, metavar="R", help="register the post scene to the pre scene before the damage model "
        "reads the pair: the best whole-pixel translation with |dy|, |dx| <= R (1..32) is applied to the post scene and "
        "<stem>_alignment.json is written; 0 = off.  A shift found at the limit R (at_limit in the report) means the true "
        "offset may be larger than the search.  Needs --post.  No radius is recommended")
    arg("--align_tile", type=int, default=128, choices=[32, 64, 128], help="with --align: side of the tiles whose own best "
        "shifts the report lists")
    arg("--scales", type=parse_scales, default="1", metavar="S1,S2,...", help="predict every scene once per scale and average "
        "the maps in this order: 1 to 8 values in [0.25, 4], no duplicates.  The scene is resized on the GPU (bicubic, as "
        "Pillow), predicted at that size and the maps resampled back (bilinear); all outputs stay on the native grid.  One "
        "value is a ground-resolution correction: the ratio of the scene's metres per pixel to the training data's.  No "
        "value is recommended")
    from .utils import fusion
    fusion.add_flags(arg)
    return parser


def parse_scales(text):
    """'0.75,1,1.25' -> (0.75, 1.0, 1.25), checked (resize.check_scales); ValueError for anything else"""
    from .resize import check_scales
    parts = [p.strip() for p in str(text).split(",")]
    if not all(parts):
        raise ValueError("--scales: an empty entry in %r" % (text,))
    return check_scales(tuple(float(p) for p in parts))


def _listing(path):
    if os.path.isdir(path):
        return sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(IMAGE_SUFFIXES))
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return [path]


def pair_inputs(pre, post=None):
    """[(pre file, post file | None)]: directories are paired by sorted order with equal counts"""
    pres = _listing(pre)
    if not pres:
        raise ValueError("no image under %s" % pre)
    if post is None:
        return [(p, None) for p in pres]
    posts = _listing(post)
    if len(pres) != len(posts):
        raise ValueError("%d pre images under %s but %d post images under %s" % (len(pres), pre, len(posts), post))
    return list(zip(pres, posts))


def read_bgr(path):
    """cv2.imread semantics, as data_loading/pytorch_loader.py load_pair: 8-bit B, G, R"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def _load(path, ema, tta, device):
    from .lightning import Model
    model = Model.load_from_checkpoint(path, ema=ema)
    model.args.tta = tta
    return model.to(device).eval()


def main(argv=None):
    args = get_parser().parse_args(argv)
    if args.align:
        from .utils.align import check_radius
        check_radius(args.align)
        if args.post is None:
            raise ValueError("--align needs --post")
    if args.ckpt_loc is None and args.ckpt_dmg is None:
        raise ValueError("give --ckpt_loc, --ckpt_dmg or both")
    if args.ckpt_dmg is not None and args.post is None:
        raise ValueError("--ckpt_dmg needs --post")
    import torch
    from PIL import Image
    from . import ops, scene
    from .utils.post_process import post_process_tiles
    scene.check_window(args.window, args.overlap)
    if args.simplify:
        from .utils.polygons import quantise_tolerance
        quantise_tolerance(args.simplify)
    if args.min_area or args.fill_holes:
        from .utils.clean import check_fill_holes, check_min_area
        check_min_area(args.min_area)
        check_fill_holes(args.fill_holes)
    from .utils import fusion
    fuse_kw = fusion.resolve(args)
    pairs = pair_inputs(args.pre, args.post if args.ckpt_dmg is not None or args.align else None)
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.predict runs on the MI355X only; there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    # the arithmetic mode, as Trainer.__init__ sets it
    ops.MATH_MODE = ops.MATH_BF16 if args.precision == 16 else ops.fp32_math()
    ops.set_storage_dtype(torch.bfloat16 if args.precision == 16 else None)
    loc = dmg = None
    if args.ckpt_loc is not None:
        loc = scene.ScenePredictor(_load(args.ckpt_loc, args.ema, args.tta, device), args.window, args.overlap, args.batch)
        if loc.kind != scene.SIGMOID1:
            raise ValueError("%s is no localization (--type pre) checkpoint" % args.ckpt_loc)
    if args.ckpt_dmg is not None:
        dmg = scene.ScenePredictor(_load(args.ckpt_dmg, args.ema, args.tta, device), args.window, args.overlap, args.batch)
        if dmg.kind == scene.SIGMOID1:
            raise ValueError("%s is no damage (--type post) checkpoint" % args.ckpt_dmg)
        if fuse_kw["class_scale"] is not None and dmg.kind != scene.SOFTMAX:
            raise ValueError("--class_scale multiplies the damage probabilities before their argmax, but %s is a coral / mse "
                             "checkpoint, which decodes to a label map with no per-class probabilities to scale"
                             % args.ckpt_dmg)
    os.makedirs(args.out, exist_ok=True)
    for pre_path, post_path in pairs:
        pre = read_bgr(pre_path)
        post = read_bgr(post_path) if post_path is not None else None
        if post is not None and post.shape != pre.shape:
            raise ValueError("%s is %d x %d but %s is %d x %d" % (pre_path, pre.shape[0], pre.shape[1], post_path,
                                                                   post.shape[0], post.shape[1]))
        stem = os.path.join(args.out, os.path.splitext(os.path.basename(pre_path))[0])
        pre_d = torch.from_numpy(pre).to(device)
        post_d = torch.from_numpy(post).to(device) if post is not None else None
        H, W, _ = pre.shape
        if args.align:
            from .utils import align
            post_d, info = scene.align_pair(pre_d, post_d, args.align, args.align_tile)
            with open(stem + "_alignment.json", "w") as f:
                f.write(align.dumps(align.report_of(info, H, W)))
        loc_maps = loc.predict(pre_d, scales=args.scales) if loc is not None else None
        dmg_maps = dmg.predict(pre_d, post_d, scales=args.scales) if dmg is not None else None
        # a missing partner is neutral in the fusion: every pixel a building / no pixel damaged beyond class 1
        loc_map = loc_maps[0] if loc is not None else torch.ones((H, W), dtype=torch.float32, device=device)
        dmg_map = (scene.decode_damage(dmg_maps, dmg.kind) if dmg is not None
                   else torch.ones((H, W), dtype=torch.int32, device=device))
        pre_png, post_png, clean_stats = post_process_tiles(loc_map, dmg_map, args.components and dmg is not None, args.dilate,
                                                            args.dilation_rate, split=args.split, min_area=args.min_area,
                                                            fill_holes=args.fill_holes, return_stats=True, **fuse_kw)
        if loc is not None:
            Image.fromarray(pre_png.cpu().numpy()).save(stem + "_localization_prediction.png")
        if dmg is not None:
            Image.fromarray(post_png.cpu().numpy()).save(stem + "_damage_prediction.png")
        if args.buildings or args.polygons:
            # from the maps the PNGs show (after --components and --dilate); confidence only with a localization model
            from .utils import buildings
            rows, labels = buildings.building_table(pre_png, post_png, loc_map if loc is not None else None,
                                                    return_labels=True)
            records = buildings.to_records(rows, H, W, confidence=loc is not None)
            buildings.write_csv(stem + "_buildings.csv", records)
            if clean_stats is not None:      # only with --min_area / --fill_holes: the JSON is otherwise what it was
                import json
                from .utils import clean
                doc = buildings.summary(records)
                doc["clean"] = clean.totals(clean_stats)
                with open(stem + "_buildings.json", "w") as f:
                    json.dump(doc, f, indent=1, sort_keys=True)
                    f.write("\n")
            else:
                buildings.write_summary(stem + "_buildings.json", records)
            if args.polygons:
                from .utils import polygons
                polygons.write_geojson(stem + "_buildings.geojson", polygons.building_polygons(pre_png, labels, args.simplify),
                                       records)
        if args.save_probs:
            if loc is not None:
                np.save(stem + "_localization_probs.npy", loc_maps.cpu().numpy())
            if dmg is not None:
                np.save(stem + "_damage_probs.npy", dmg_maps.cpu().numpy())
    return len(pairs)


if __name__ == "__main__":
    print("predicted %d scenes" % main())
