"""Pick the fusion's thresholds and class scales on a hold-out set: the full grid, swept on the MI355X.

`main.py --exec_mode eval` writes probs/ and targets/; utils.post_process fuses each pair with
    post_raw = argmax(s * dmg) + 1,   pre = (loc > A) | ((loc > B) & (post_raw > 1)),   post = pre ? post_raw : 0
and the reference fixes A = 0.3, B = 0.1, s = 1.  This tool scores every (A, B) = (T_i, T_j), j <= i, of a threshold grid T
for every scale vector of a list, and writes the best point as a report that `utils.post_process --calibration` and
`predict --calibration` read.

    python -m xview2_amd.utils.calibrate --results R [--targets DIR] [--grid 0.01]
        [--scale_grid 0.5,1,2 | --class_scales "1,1,1,1;1,2,2,2"] [--batch 8] [--out R/calibration.json] [--table OUT.npy]
        [--components] [--dilate] [--dilation_rate 3] [--split R] [--min_area A] [--fill_holes M]

How: the fusion is per pixel, so the scorer's 15 counts at every grid point are integer functions of one joint histogram
hist[s][k][r][t][d] (k = #{ j : loc > T_j }, r = post_raw - 1, t = lt > 0, d = dt; csrc/calibrate.hip, one pass over the
probabilities per 64 scale vectors).  With G[i] = sum over k > i of hist[k], the set "pre" at (T_i, T_j) is G[i] where r = 0
and G[j] where r >= 1, and the counts are sums of it (derive()).  The score is xview2_metrics' own arithmetic on those counts.
Ties go to the first point in the order (scale index, i, j).

The sweep sees the per-pixel fusion only.  --components, --dilate, --split, --min_area and --fill_holes act after it and can
move the optimum; the report's `verified` runs the default and the best point through the real post_process_tiles with those
flags and scores both with the scorer's kernel, so both numbers stand side by side.  Without such flags `verified` equals the
swept numbers exactly.

Calibrate on a hold-out set, never on the set you report: the best point of a set is fitted to it.  No value is recommended.
"""
import json
import math
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

MAX_THRESHOLDS, MAX_SCALES = 128, 64
ONES = (1.0, 1.0, 1.0, 1.0)
REF_T = (np.float32(0.1), np.float32(0.3))     # the reference's (B, A): the `default` point's own two-threshold table
SCORE_KEYS = ("score", "damage_f1", "localization_f1", "damage_f1_no_damage", "damage_f1_minor_damage",
              "damage_f1_major_damage", "damage_f1_destroyed")


# ---- the grid and the scale list (host, no GPU) ---------------------------------------------------------------------------
def threshold_grid(step):
    """T_j = float32(j * step), j = 0 .. ceil(1 / step) - 1; at most 128 of them"""
    g = float(step)
    if not (math.isfinite(g) and 0 < g <= 1):
        raise ValueError("--grid must be in (0, 1], got %r" % (step,))
    n = int(math.ceil(1.0 / g - 1e-9))
    if n > MAX_THRESHOLDS:
        raise ValueError("--grid %r gives %d thresholds, at most %d fit one sweep" % (step, n, MAX_THRESHOLDS))
    t = np.array([np.float32(j * g) for j in range(n)], dtype=np.float32)
    if n > 1 and not (np.diff(t) > 0).all():
        raise ValueError("--grid %r is too fine for float32" % (step,))
    return t


def scale_product(values):
    """--scale_grid: every combination of the values for classes 2..4, class 1 fixed at 1 (argmax is invariant to a
    common factor)"""
    v = [float(x) for x in values]
    if not v or not all(math.isfinite(x) and x > 0 for x in v):
        raise ValueError("--scale_grid: finite factors > 0 expected, got %r" % (values,))
    return [(1.0, a, b, c) for a in v for b in v for c in v]


def parse_scale_list(text):
    """--class_scales '1,1,1,1;1,2,2,2' -> [(1,1,1,1), (1,2,2,2)]"""
    from .fusion import parse_class_scale
    rows = [r for r in str(text).split(";") if r.strip()]
    if not rows:
        raise ValueError("--class_scales: no scale vector in %r" % (text,))
    return [tuple(float(np.float32(x)) for x in parse_class_scale(r)) for r in rows]


def scale_list(scale_grid=None, class_scales=None):
    if scale_grid is not None and class_scales is not None:
        raise ValueError("give --scale_grid or --class_scales, not both")
    if scale_grid is not None:
        rows = scale_product([x for x in str(scale_grid).split(",") if x.strip()])
    elif class_scales is not None:
        rows = parse_scale_list(class_scales)
    else:
        rows = [ONES]
    return [tuple(float(np.float32(x)) for x in r) for r in rows]


# ---- histogram -> counts -> scores (host, int64 / float64 numpy) ----------------------------------------------------------
def derive(hist):
    """int64 [S, n, n, 15]: the scorer's counts [lTP, lFN, lFP, (TP, FN, FP) x classes 1..4] at (A, B) = (T_i, T_j) for
    hist [S, n+1, 4, 2, 5]; entries with j > i are computed too but mean nothing (B <= A is the fusion's contract).  Every
    count is f(i) + g(j) + const, because pre is G[i] on r = 0 and G[j] on r >= 1."""
    h = np.asarray(hist, dtype=np.int64)
    S, n1 = h.shape[0], h.shape[1]
    n = n1 - 1
    assert h.shape[2:] == (4, 2, 5) and n >= 1
    # G[:, i] = sum over k > i
    G = np.flip(np.cumsum(np.flip(h, axis=1), axis=1), axis=1)[:, 1:]          # [S, n, 4, 2, 5]
    tot = h.sum(axis=(1, 2))                                                   # [S, 2, 5]
    fi = np.zeros((S, n, 15), dtype=np.int64)     # the part that follows i (r = 0)
    gj = np.zeros((S, n, 15), dtype=np.int64)     # the part that follows j (r >= 1)
    const = np.zeros((S, 15), dtype=np.int64)
    fi[:, :, 0] = G[:, :, 0, 1, :].sum(axis=-1)
    gj[:, :, 0] = G[:, :, 1:, 1, :].sum(axis=(-1, -2))
    fi[:, :, 2] = G[:, :, 0, 0, :].sum(axis=-1)
    gj[:, :, 2] = G[:, :, 1:, 0, :].sum(axis=(-1, -2))
    const[:, 1] = tot[:, 1, :].sum(axis=-1)
    for c in range(1, 5):
        part = fi if c == 1 else gj
        sel = G[:, :, c - 1].sum(axis=2)                                       # [S, n, 5] over t
        part[:, :, 3 * c] = sel[:, :, c]
        part[:, :, 3 * c + 2] = sel[:, :, 1:].sum(axis=-1) - sel[:, :, c]
        const[:, 3 * c + 1] = tot[:, :, c].sum(axis=-1)
    out = fi[:, :, None, :] + gj[:, None, :, :]
    for k in (1, 4, 7, 10, 13):     # FN = all - TP
        out[..., k] = const[:, None, None, k] - out[..., k - 1]
    return out


def point_scores(counts):
    """the seven scores of 15 summed counts, by xview2_metrics' own F1Recorder and harmonic mean"""
    from .xview2_metrics import F1Recorder
    c = [int(x) for x in counts]
    lf1 = F1Recorder(c[0], c[2], c[1]).f1
    df1s = [F1Recorder(c[3 * k], c[3 * k + 2], c[3 * k + 1]).f1 for k in range(1, 5)]
    df1 = len(df1s) / sum((x + 1e-6) ** -1 for x in df1s)
    vals = (0.3 * lf1 + 0.7 * df1, df1, lf1) + tuple(df1s)
    return {k: float(v) for k, v in zip(SCORE_KEYS, vals)}


def _f1(tp, fn, fp):
    tp, fn, fp = (np.asarray(x, dtype=np.float64) for x in (tp, fn, fp))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(tp == 0, 0.0, tp / (tp + fp))
        r = np.where(tp == 0, 0.0, tp / (tp + fn))
        return np.where((p == 0) | (r == 0), 0.0, (2 * p * r) / (p + r))


def score_table(counts):
    """float64 [S, n, n] scores of derive()'s counts, NaN where j > i.  The same formulas as point_scores over whole arrays;
    best() settles near-ties with point_scores itself."""
    c = np.asarray(counts)
    lf1 = _f1(c[..., 0], c[..., 1], c[..., 2])
    inv = 0.0
    for k in range(1, 5):
        inv = inv + 1.0 / (_f1(c[..., 3 * k], c[..., 3 * k + 1], c[..., 3 * k + 2]) + 1e-6)
    table = 0.3 * lf1 + 0.7 * (4 / inv)
    n = c.shape[1]
    table[:, np.triu(np.ones((n, n), dtype=bool), 1)] = np.nan
    return table


def best(counts, table=None):
    """(s, i, j) of the maximum score, the first in the order (scale index, i, j) among equals.  Candidates come from the
    array table; every one within 1e-9 of its maximum is scored again by point_scores, so the choice never hangs on a last
    bit that two ways of writing the same formula could round differently."""
    table = score_table(counts) if table is None else table
    m = np.nanmax(table)
    top, arg = None, None
    for s, i, j in zip(*np.nonzero(table >= m - 1e-9)):      # np.nonzero walks in row-major order: (s, i, j)
        v = point_scores(counts[s, i, j])["score"]
        if top is None or v > top:
            top, arg = v, (int(s), int(i), int(j))
    return arg


def point(thresholds, scales, counts, s, i, j):
    return {"index": [int(s), int(i), int(j)], "loc_threshold": float(thresholds[i]), "loc_threshold_dmg": float(thresholds[j]),
            "class_scale": [float(x) for x in scales[s]], "counts": [int(x) for x in counts],
            "scores": point_scores(counts)}


def build_report(thresholds, scales, hist, default_hist, tiles, pixels, bad, step=None):
    """the report without `verified`, and the score table.  hist [S, n+1, 4, 2, 5] over `scales`; default_hist
    [1, 3, 4, 2, 5], the unscaled histogram over REF_T that the reference's point is read from whatever the grid is."""
    counts = derive(hist)
    table = score_table(counts)
    s, i, j = best(counts, table)
    per_scale = []
    for k in range(len(scales)):
        _, bi, bj = best(counts[k:k + 1], table[k:k + 1])
        per_scale.append(point(thresholds, scales, counts[k, bi, bj], k, bi, bj))
    dflt = point(REF_T, [ONES], derive(default_hist)[0, 1, 0], 0, 1, 0)
    del dflt["index"]
    on_grid = [int(np.nonzero(thresholds == t)[0][0]) if (thresholds == t).any() else None for t in (REF_T[1], REF_T[0])]
    dflt["grid_index"] = on_grid if None not in on_grid else None
    doc = {
        "grid": {"step": None if step is None else float(step), "thresholds": [float(t) for t in thresholds]},
        "class_scales": [[float(x) for x in r] for r in scales],
        "tiles": int(tiles), "pixels": int(pixels), "bad": int(bad),
        "default": dflt,
        "best": point(thresholds, scales, counts[s, i, j], s, i, j),
        "best_per_scale": per_scale,
        "note": "The sweep scores the per-pixel fusion only; --components, --dilate, --split, --min_area and --fill_holes act "
                "after it and can move the optimum: `verified` holds both points run through the real post-processing with "
                "the flags given.  Calibrate on a hold-out set, not on the set you report.",
    }
    return doc, table


def dumps(doc):
    return json.dumps(doc, indent=1, sort_keys=True) + "\n"


# ---- the GPU passes -------------------------------------------------------------------------------------------------------
def _target_path(targets, prob_path):
    base = os.path.basename(prob_path)
    return os.path.join(targets, (base[:-4] if base.endswith(".npy") else base) + "_target.png")


def _load_target(path, shape):
    from PIL import Image
    if not os.path.exists(path):
        raise FileNotFoundError("calibrate: target %s is missing" % path)
    a = np.asarray(Image.open(path))
    if a.ndim != 2 or a.dtype != np.uint8 or a.shape != tuple(shape):
        raise ValueError("calibrate: target %s is %s %s, expected uint8 %s" % (path, a.dtype, a.shape, tuple(shape)))
    return a


def batches(results, targets, batch):
    """yields device (loc, dmg, lt, dt) per geometry group of every --batch pairs, in post_process.run's order and
    grouping"""
    from . import post_process as pp
    dev = pp._device()
    pre_paths, post_paths = pp.prob_pairs(results)
    for i in range(0, len(pre_paths), batch):
        pairs = list(zip(pre_paths[i:i + batch], post_paths[i:i + batch]))
        locs = [np.load(a) for a, _ in pairs]
        dmgs = [np.load(b) for _, b in pairs]
        for (lshape, _, _), ks in pp.geometry_groups(locs, dmgs).items():
            lt = np.stack([_load_target(_target_path(targets, pairs[k][0]), lshape) for k in ks])
            dt = np.stack([_load_target(_target_path(targets, pairs[k][1]), lshape) for k in ks])
            yield (pp._to_device(np.stack([locs[k] for k in ks]), dev), pp._to_device(np.stack([dmgs[k] for k in ks]), dev),
                   pp._to_device(lt, dev), pp._to_device(dt, dev))


def sweep(results, targets, thresholds, scales, batch=8):
    """(hist [S, n+1, 4, 2, 5], default_hist [1, 3, 4, 2, 5], tiles, pixels, bad) as numpy / ints: one pass over the data,
    one histogram launch per 64 scale vectors plus the reference point's own"""
    import torch
    from .. import ops
    chunks = [scales[k:k + MAX_SCALES] for k in range(0, len(scales), MAX_SCALES)]
    plain = list(scales) == [ONES]
    hists, dflt, bad, again = [None] * len(chunks), None, None, None     # again: the same bad pixels, counted per chunk
    tiles = pixels = 0
    for loc, dmg, lt, dt in batches(results, targets, batch):
        if dmg.dim() == 3 and not plain:
            raise ValueError("calibrate: class scales need damage probabilities, but the damage files hold label maps "
                             "(a coral or mse model); sweep the thresholds alone")
        dflt, bad = ops.calibrate_hist(loc, dmg, lt, dt, REF_T, None, dflt, bad)
        for c, rows in enumerate(chunks):
            hists[c], again = ops.calibrate_hist(loc, dmg, lt, dt, thresholds, None if plain else rows, hists[c], again)
        tiles += loc.shape[0]
        pixels += loc.numel()
    if tiles == 0:
        raise ValueError("calibrate: no localization / damage pair under %s" % os.path.join(results, "probs"))
    hist = torch.cat(hists, dim=0).cpu().numpy()
    return hist, dflt.cpu().numpy(), tiles, pixels, int(bad.item())


def verify(results, targets, points, batch=8, **post_flags):
    """each point's 15 counts through the real post_process_tiles with the post-processing flags given, scored by
    ops.xview2_counts: one pass over the data per point"""
    import torch
    from .. import ops
    from .post_process import post_process_tiles
    out = []
    for p in points:
        scale = None if tuple(p["class_scale"]) == ONES else p["class_scale"]
        total = torch.zeros(16, dtype=torch.int64)
        for loc, dmg, lt, dt in batches(results, targets, batch):
            pre, post = post_process_tiles(loc, dmg, loc_threshold=p["loc_threshold"], dmg_threshold=p["loc_threshold_dmg"],
                                           class_scale=scale, **post_flags)
            total += ops.xview2_counts(pre, post, lt, dt).sum(dim=0).cpu()
        counts = [int(x) for x in total[:15]]
        out.append({"counts": counts, "scores": point_scores(counts), "bad": int(total[15])})
    return out


def run(args):
    from .post_process import _check_rate
    thresholds = threshold_grid(args.grid)
    scales = scale_list(args.scale_grid, args.class_scales)
    if args.batch < 1:
        raise ValueError("--batch must be >= 1, got %d" % args.batch)
    _check_rate(args.dilate, args.dilation_rate)
    targets = args.targets if args.targets is not None else os.path.join(args.results, "targets")
    hist, dflt, tiles, pixels, bad = sweep(args.results, targets, thresholds, scales, args.batch)
    doc, table = build_report(thresholds, scales, hist, dflt, tiles, pixels, bad, args.grid)
    flags = dict(components=args.components, dilate=args.dilate, dilation_rate=args.dilation_rate, split=args.split,
                 min_area=args.min_area, fill_holes=args.fill_holes)
    v_default, v_best = verify(args.results, targets, [doc["default"], doc["best"]], args.batch, **flags)
    doc["verified"] = {"flags": {k: (bool(v) if isinstance(v, bool) else int(v)) for k, v in flags.items()},
                       "default": v_default, "best": v_best}
    out = args.out if args.out is not None else os.path.join(args.results, "calibration.json")
    with open(out, "w") as f:
        f.write(dumps(doc))
    if args.table:
        np.save(args.table, table)
    return doc


def get_parser():
    parser = ArgumentParser(prog="python -m xview2_amd.utils.calibrate", formatter_class=ArgumentDefaultsHelpFormatter)
    arg = parser.add_argument
    arg("--results", type=str, default="/results", help="directory holding probs/ (and targets/)")
    arg("--targets", type=str, default=None, help="directory of test_{localization,damage}_NNNNN_target.png; default "
        "<results>/targets, where the evaluation writes them")
    arg("--grid", type=float, default=0.01, help="threshold step g: T_j = float32(j * g), at most 128 thresholds")
    arg("--scale_grid", type=str, default=None, metavar="v1,v2,...", help="sweep every combination of these factors for "
        "damage classes 2..4 (class 1 stays 1)")
    arg("--class_scales", type=str, default=None, metavar="'a,b,c,d;...'", help="sweep exactly these scale vectors")
    arg("--batch", type=int, default=8, help="tiles per GPU call")
    arg("--out", type=str, default=None, help="the report; default <results>/calibration.json")
    arg("--table", type=str, default=None, metavar="OUT.npy", help="also write the float64 [S, n, n] score table (NaN "
        "where the damage-gated threshold would exceed the localization threshold)")
    arg("--components", action="store_true", help="for `verified`: as utils.post_process")
    arg("--dilate", action="store_true", help="for `verified`: as utils.post_process")
    arg("--dilation_rate", type=int, default=3, help="for `verified`: as utils.post_process")
    arg("--split", type=int, default=0, metavar="R", help="for `verified`: as utils.post_process")
    arg("--min_area", type=int, default=0, metavar="A", help="for `verified`: as utils.post_process")
    arg("--fill_holes", type=int, default=0, metavar="M", help="for `verified`: as utils.post_process")
    return parser


if __name__ == "__main__":
    d = run(get_parser().parse_args())
    print("swept %d tiles: default %.6f, best %.6f at (%g, %g) x %s" % (
        d["tiles"], d["default"]["scores"]["score"], d["best"]["scores"]["score"], d["best"]["loc_threshold"],
        d["best"]["loc_threshold_dmg"], d["best"]["class_scale"]))
