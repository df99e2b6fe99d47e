"""Score a prediction per BUILDING: how many labelled buildings were found, how many reported buildings are real, and
how the damage class voted for a found building compares with the labelled one.

The buildings of a map are the 4-connected components of its localization PNG (utils/buildings.py), their damage class the
vote over the damage PNG.  Predicted and labelled buildings are matched on the MI355X (csrc/match.hip,
xv2_building_match): a pair is matched when each is the other's best partner by intersection over union and the IoU
reaches the threshold, which is at least 1/2 so that the matched set does not depend on a matching rule.  Everything the
score is made of is an integer; the F1 arithmetic runs through xview2_metrics.F1Recorder on the summed integers, so the
JSON depends on the integers alone.

What this does not do:
  * Labelled buildings that touch in the raster are ONE building here: the target PNG carries no instance ids.
    --split_targets R cuts them apart by shape (utils/split.py) before they are labelled, --split R does the same to the
    prediction; neither knows the labelled instances.
  * The minimum-area filter is off unless asked for: by default a one-pixel component is a building on either side.
    --min_area A / --fill_holes M clean the predicted pair (utils/clean.py: holes of at most M pixels filled, then
    buildings below A pixels dropped) and --min_area_targets A drops small labelled buildings, each before the split.
  * There is no georeferencing: boxes and ids are pixel coordinates and row numbers of the tile.

    python -m xview2_amd.utils.building_metrics PRED_DIR TARG_DIR OUT_JSON [--iou 1/2] [--per_building DIR] [--batch 16]
                                                [--split R] [--split_targets R] [--min_area A] [--fill_holes M]
                                                [--min_area_targets A]
"""
import json
import os
from argparse import ArgumentParser, ArgumentTypeError
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from decimal import Decimal, InvalidOperation
from fractions import Fraction
from pathlib import Path

import numpy as np

from .buildings import COLS, first_capacity
from .xview2_metrics import F1Recorder, XviewMetrics

MATCH_COLS = 8
CLASS_KEYS = ("no_damage", "minor_damage", "major_damage", "destroyed")
CSV_FIELDS = ("side", "id", "y0", "x0", "y1", "x1", "area", "damage", "partner", "intersection", "union", "matched", "partners")

# the two tables (int64 [n, 16]) and the two match arrays (int64 [n, 8]) of one tile, as numpy
TileMatch = namedtuple("TileMatch", "table_p table_t match_p match_t")


def parse_iou(text):
    """'N/D' or a decimal -> (num, den) in lowest terms: an exact fraction with den <= 65536 and 1/2 <= num/den <= 1"""
    try:
        if "/" in text:
            n, d = text.split("/")
            f = Fraction(int(n), int(d))
        else:
            f = Fraction(Decimal(text))
    except (ValueError, ZeroDivisionError, InvalidOperation, OverflowError):
        raise ValueError("--iou %r is neither N/D nor a decimal" % (text,))
    if f.denominator > 65536:
        raise ValueError("--iou %s is no exact fraction with a denominator of at most 65536" % text)
    if not (Fraction(1, 2) <= f <= 1):
        raise ValueError("--iou %s must lie in 1/2 .. 1: below 1/2 the matched set would depend on a matching rule" % text)
    return f.numerator, f.denominator


def _pad(tables, device):
    """list of [n_b, 16] host tables -> (rows int64 [B, max(1, max n_b), 16], count int32 [B]) on the device"""
    import torch
    n = [int(t.shape[0]) for t in tables]
    rows = np.zeros((len(tables), max(1, max(n)), COLS), dtype=np.int64)
    for b, t in enumerate(tables):
        rows[b, :n[b]] = t
    return torch.from_numpy(rows).to(device), torch.tensor(n, dtype=torch.int32, device=device)


def match_maps(pre_p, post_p, pre_t, post_t, iou=(1, 2), loc=None, max_pieces=None):
    """pre_p, post_p: the prediction's two label maps, pre_t, post_t: the target's; uint8 [H,W] or [B,H,W] on the device.
    loc: fp32 localization probabilities of the prediction or None (column 14 of its table).  max_pieces: first capacity of
    overlap pieces per tile (default first_capacity(H, W)); a tile with more makes the match run once more with the capacity
    its count asks for.  Returns one TileMatch per tile (a list; one TileMatch for unbatched input).
    building_table brings both tables to the host (they are part of the result), and they are padded and uploaded again for
    the match: that round trip and the copies of the result, not the launches, are most of this call's time
    (profiles/match_cost.md: 1.9 ms against 0.5 ms of launches on a 4096 x 4096 scene)."""
    from .. import ops
    from .buildings import building_table
    single = pre_p.dim() == 2
    if single:
        pre_p, post_p, pre_t, post_t = (m.unsqueeze(0) for m in (pre_p, post_p, pre_t, post_t))
        loc = loc.unsqueeze(0) if loc is not None else None
    if pre_t.shape != pre_p.shape:
        raise ValueError("match_maps: prediction and target maps must have one shape, got %s and %s"
                         % (tuple(pre_p.shape), tuple(pre_t.shape)))
    tables_p, labels_p = building_table(pre_p, post_p, loc, return_labels=True)
    tables_t, labels_t = building_table(pre_t, post_t, None, return_labels=True)
    B, H, W = pre_p.shape
    rows_p, count_p = _pad(tables_p, pre_p.device)
    rows_t, count_t = _pad(tables_t, pre_p.device)
    cap = first_capacity(H, W) if max_pieces is None else int(max_pieces)
    match_p, match_t, pieces = ops.building_match(labels_p, rows_p, count_p, labels_t, rows_t, count_t, iou, cap)
    most = int(pieces.cpu().numpy().max())          # the only host decision, after the last launch
    if most > cap:
        match_p, match_t, pieces = ops.building_match(labels_p, rows_p, count_p, labels_t, rows_t, count_t, iou, most)
    mp, mt = match_p.cpu().numpy(), match_t.cpu().numpy()
    out = [TileMatch(tables_p[b], tables_t[b], np.ascontiguousarray(mp[b, :tables_p[b].shape[0]]),
                     np.ascontiguousarray(mt[b, :tables_t[b].shape[0]])) for b in range(B)]
    return out[0] if single else out


def tile_counts(tm):
    """The integers of one tile (Python ints): object-level TP / FP / FN (matched, unmatched predicted, unmatched labelled),
    confusion[target class][predicted class] over the matched pairs (voted classes 0..4, column 13 of the tables), the
    buildings per voted class on either side, and the predicted buildings that cover several labelled ones (merged) and the
    labelled buildings covered by several predicted ones (split): column 4 > 1."""
    tp_, tt, mp, mt = (np.asarray(a, dtype=np.int64) for a in tm)
    tp_, tt = tp_.reshape(-1, COLS), tt.reshape(-1, COLS)
    mp, mt = mp.reshape(-1, MATCH_COLS), mt.reshape(-1, MATCH_COLS)
    if mp.shape[0] != tp_.shape[0] or mt.shape[0] != tt.shape[0]:
        raise ValueError("tile_counts: %d / %d match rows for %d / %d buildings" % (mp.shape[0], mt.shape[0], tp_.shape[0],
                                                                                  tt.shape[0]))
    TP = int(mp[:, 3].sum())
    if TP != int(mt[:, 3].sum()):
        raise ValueError("tile_counts: %d matched predictions but %d matched labels" % (TP, int(mt[:, 3].sum())))
    confusion = [[0] * 5 for _ in range(5)]
    for r in np.nonzero(mp[:, 3])[0].tolist():
        confusion[int(tt[mp[r, 0], 13])][int(tp_[r, 13])] += 1
    return {"TP": TP, "FP": int(mp.shape[0]) - TP, "FN": int(mt.shape[0]) - TP, "confusion": confusion,
            "pred_per_class": np.bincount(tp_[:, 13], minlength=5)[:5].tolist(),
            "targ_per_class": np.bincount(tt[:, 13], minlength=5)[:5].tolist(),
            "merged": int((mp[:, 4] > 1).sum()), "split": int((mt[:, 4] > 1).sum())}


def sum_counts(counts):
    """the field-wise sum of tile_counts dicts (zeros for an empty list)"""
    tot = {"TP": 0, "FP": 0, "FN": 0, "confusion": [[0] * 5 for _ in range(5)], "pred_per_class": [0] * 5,
           "targ_per_class": [0] * 5, "merged": 0, "split": 0}
    for c in counts:
        for k in ("TP", "FP", "FN", "merged", "split"):
            tot[k] += c[k]
        for k in ("pred_per_class", "targ_per_class"):
            tot[k] = [a + b for a, b in zip(tot[k], c[k])]
        tot["confusion"] = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(tot["confusion"], c["confusion"])]
    return tot


def damage_recorders(tot):
    """per class c = 1..4: TP_c matched pairs with both voted c, FP_c predicted buildings voted c that are not TP_c, FN_c
    labelled buildings of class c that are not TP_c"""
    out = []
    for c in range(1, 5):
        tp = tot["confusion"][c][c]
        out.append(F1Recorder(tp, tot["pred_per_class"][c] - tp, tot["targ_per_class"][c] - tp, XviewMetrics.dmg2str[c]))
    return out


def score_dict(tot, iou, tiles):
    """the JSON of compute_score from summed integers"""
    loc = F1Recorder(tot["TP"], tot["FP"], tot["FN"], "Buildings")
    recs = damage_recorders(tot)
    d = {"object_localization_precision": loc.P, "object_localization_recall": loc.R, "object_localization_f1": loc.f1}
    for key, rec in zip(CLASS_KEYS, recs):
        d["object_damage_f1_" + key] = rec.f1
    d["object_damage_f1"] = len(recs) / sum((rec.f1 + 1e-6) ** -1 for rec in recs)
    d["confusion"] = tot["confusion"]
    d["totals"] = {k: tot[k] for k in ("TP", "FP", "FN", "pred_per_class", "targ_per_class", "merged", "split")}
    d["totals"]["predicted"] = tot["TP"] + tot["FP"]
    d["totals"]["labelled"] = tot["TP"] + tot["FN"]
    d["totals"]["tiles"] = int(tiles)
    d["iou"] = [int(iou[0]), int(iou[1])]
    return d


def to_records(tm):
    """one dict per predicted ('p') and per labelled ('t') building: id and partner are 1-based row numbers of the side's own
    and of the other side's table, partner 0 when there is none"""
    out = []
    for side, table, match in (("p", tm.table_p, tm.match_p), ("t", tm.table_t, tm.match_t)):
        rows = np.asarray(table, dtype=np.int64).reshape(-1, COLS).tolist()
        for i, (r, m) in enumerate(zip(rows, np.asarray(match, dtype=np.int64).reshape(-1, MATCH_COLS).tolist())):
            out.append({"side": side, "id": i + 1, "y0": r[2], "x0": r[3], "y1": r[4], "x1": r[5], "area": r[1], "damage": r[13],
                        "partner": m[0] + 1, "intersection": m[1], "union": m[2], "matched": m[3], "partners": m[4]})
    return out


def write_csv(path, records):
    """one header line, then one line per building; the side as its letter, every number as repr: the bytes repeat"""
    with open(path, "w", newline="\n") as f:
        f.write(",".join(CSV_FIELDS) + "\n")
        for r in records:
            f.write(",".join(r[k] if k == "side" else repr(r[k]) for k in CSV_FIELDS) + "\n")


def read_csv(path):
    """the records write_csv wrote"""
    with open(path) as f:
        fields = f.readline().rstrip("\n").split(",")
        return [{k: (v if k == "side" else int(v)) for k, v in zip(fields, line.rstrip("\n").split(","))}
                for line in f if line.strip()]


def _load(ph):
    """the four uint8 maps of a tile, with the loader's checks and the 0..4 value check of the pixel score"""
    maps = ph.load_images()
    bad = sum(int((m > 4).sum()) for m in maps)
    if bad:
        raise ValueError("prediction / target values must be ints 0-4: %d pixels hold a larger value" % bad)
    return maps


class BuildingMetrics:
    """object-level metrics of a directory of predictions against a directory of targets, named as for XviewMetrics:
    {test,hold}_{localization,damage}_NNNNN_{prediction,target}.png"""

    get_path_handlers = XviewMetrics.get_path_handlers      # the same file naming, through the same PathHandler

    def __init__(self, pred_dir, targ_dir, iou=(1, 2), batch=16, split=0, split_targets=0, min_area=0, fill_holes=0,
                 min_area_targets=0):
        self.pred_dir, self.targ_dir = Path(pred_dir), Path(targ_dir)
        assert self.pred_dir.is_dir(), "Could not find prediction directory: '%s'" % pred_dir
        assert self.targ_dir.is_dir(), "Could not find target directory: '%s'" % targ_dir
        self.iou, self.batch = (int(iou[0]), int(iou[1])), batch
        self.split, self.split_targets = int(split), int(split_targets)
        self.min_area, self.fill_holes, self.min_area_targets = min_area, fill_holes, min_area_targets
        if min_area or fill_holes or min_area_targets:
            from .clean import check_fill_holes, check_min_area
            self.min_area, self.fill_holes = check_min_area(min_area), check_fill_holes(fill_holes)
            self.min_area_targets = check_min_area(min_area_targets)
        self.get_path_handlers()
        self.get_matches()
        self.counts = [tile_counts(tm) for tm in self.matches]
        self.totals = sum_counts(self.counts)

    def __repr__(self):
        d = self.score_dict()
        s = "Buildings (IoU >= %d/%d):\n    precision: %.4f, recall: %.4f, f1: %.4f\n\nDamage per building:\n" % (
            self.iou + (d["object_localization_precision"], d["object_localization_recall"], d["object_localization_f1"]))
        for rec in damage_recorders(self.totals):
            s += "    %s\n" % rec
        return s + "    Harmonic mean dmgs | f1: %.4f" % d["object_damage_f1"]

    def get_matches(self):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        self.matches = []
        with ThreadPoolExecutor(max_workers=8) as pool:
            for i in range(0, len(self.path_handlers), self.batch):
                tiles = list(pool.map(_load, self.path_handlers[i:i + self.batch]))
                lp, dp, lt, dt = (torch.from_numpy(np.stack([t[k] for t in tiles])).to(dev) for k in range(4))
                if self.min_area or self.fill_holes or self.min_area_targets:
                    from .clean import clean_maps
                    if self.min_area or self.fill_holes:
                        lp, dp = clean_maps(lp, dp, self.min_area, self.fill_holes)
                    if self.min_area_targets:
                        lt, dt = clean_maps(lt, dt, self.min_area_targets, 0)
                if self.split or self.split_targets:
                    from .split import split_maps
                    if self.split:
                        lp, dp = split_maps(lp, dp, self.split)
                    if self.split_targets:
                        lt, dt = split_maps(lt, dt, self.split_targets)
                self.matches.extend(match_maps(lp, dp, lt, dt, self.iou))

    def score_dict(self):
        return score_dict(self.totals, self.iou, len(self.matches))

    def write_per_building(self, out_dir):
        """one CSV per tile, <split>_buildings_<id>_match.csv"""
        os.makedirs(str(out_dir), exist_ok=True)
        paths = []
        for ph, tm in zip(self.path_handlers, self.matches):
            split, _, img_id, _ = ph.lt.name[:-len(".png")].split("_")
            paths.append(os.path.join(str(out_dir), "%s_buildings_%s_match.csv" % (split, img_id)))
            write_csv(paths[-1], to_records(tm))
        return paths

    @classmethod
    def compute_score(cls, pred_dir, targ_dir, out_fp, iou=(1, 2), per_building=None, batch=16, split=0, split_targets=0,
                      min_area=0, fill_holes=0, min_area_targets=0):
        """write the object-level metrics JSON to out_fp (and the per-building CSVs into per_building, when given); batch:
        tiles per call of the kernels; split, split_targets: radius of utils.split on the predicted and on the labelled pair
        before the buildings are labelled (0 = off); min_area, fill_holes: utils.clean on the predicted pair, min_area_targets:
        its minimum area on the labelled pair, each before the split (0 = off)"""
        self = cls(pred_dir, targ_dir, iou, batch, split, split_targets, min_area, fill_holes, min_area_targets)
        d = self.score_dict()
        with open(out_fp, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
            f.write("\n")
        if per_building is not None:
            self.write_per_building(per_building)
        print("Wrote building metrics to %s" % out_fp)
        return d


compute_score = BuildingMetrics.compute_score


def _iou_arg(text):
    try:
        return parse_iou(text)
    except ValueError as e:
        raise ArgumentTypeError(str(e))


def get_parser():
    p = ArgumentParser(description="object-level (per-building) metrics of a prediction directory against a target directory")
    p.add_argument("pred_dir")
    p.add_argument("targ_dir")
    p.add_argument("out_fp")
    p.add_argument("--iou", type=_iou_arg, default=(1, 2), help="IoU threshold of a match, N/D or a decimal, at least 1/2")
    p.add_argument("--per_building", default=None, metavar="DIR", help="write one CSV per tile with one line per building")
    p.add_argument("--batch", type=int, default=16, help="tiles per call of the kernels")
    p.add_argument("--split", type=int, default=0, metavar="R", help="cut predicted buildings that touch before labelling them: "
                   "erosion radius in pixels, 0 = off")
    p.add_argument("--split_targets", type=int, default=0, metavar="R", help="the same for the labelled buildings, so that "
                   "touching labelled buildings count separately")
    p.add_argument("--min_area", type=int, default=0, metavar="A", help="drop predicted buildings of fewer than A pixels before "
                   "labelling (and before --split), 0 = off")
    p.add_argument("--fill_holes", type=int, default=0, metavar="M", help="fill holes of at most M pixels inside predicted "
                   "buildings first, 0 = off")
    p.add_argument("--min_area_targets", type=int, default=0, metavar="A", help="drop labelled buildings of fewer than A pixels "
                   "before labelling (and before --split_targets), 0 = off")
    return p


if __name__ == "__main__":
    a = get_parser().parse_args()
    compute_score(os.path.expanduser(a.pred_dir), os.path.expanduser(a.targ_dir), os.path.expanduser(a.out_fp), a.iou,
                  os.path.expanduser(a.per_building) if a.per_building else None, a.batch, a.split, a.split_targets,
                  a.min_area, a.fill_holes, a.min_area_targets)
