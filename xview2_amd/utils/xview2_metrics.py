"""The xView2 competition score (reference utils/xview2_metrics.py) with the per-tile counts on the MI355X.

    score = 0.3 * F1(localization) + 0.7 * harmonic_mean(F1(damage class 1..4))

Per tile, the HIP kernel xv2_xview2_counts (csrc/postproc.hip) produces [lTP, lFN, lFP] of the building masks and
[TP, FN, FP] of each damage class where the damage target is a building, plus the number of pixels holding a value
above 4 (the value check of the reference's loader, without a second pass).  The F1 arithmetic runs in Python floats on
the summed int64 counts, exactly as the reference's, so the JSON written by compute_score is bit-equal to the
reference's.  `ldf` / `ddf` are pandas DataFrames when pandas can be imported, int64 numpy arrays otherwise.

Departure: the CLI uses argparse with the reference's three positionals (fire is not a dependency).

    python -m xview2_amd.utils.xview2_metrics PRED_DIR TARG_DIR OUT_JSON
"""
import json
import os
from argparse import ArgumentParser
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from .. import ops

LCOLUMNS = ["lTP", "lFN", "lFP"]
DCOLUMNS = ["dTP1", "dFN1", "dFP1", "dTP2", "dFN2", "dFP2", "dTP3", "dFN3", "dFP3", "dTP4", "dFN4", "dFP4"]
TILE = (1024, 1024)


def score_tiles(lp, dp, lt, dt):
    """int64 [B,15] per-tile rows (LCOLUMNS + DCOLUMNS) of four uint8 [B,H,W] device maps; raises ValueError when a
    map holds a value above 4"""
    counts = ops.xview2_counts(lp, dp, lt, dt).cpu()
    bad = int(counts[:, 15].sum())
    if bad:
        raise ValueError("prediction / target values must be ints 0-4: %d pixels hold a larger value" % bad)
    return counts[:, :15]


class PathHandler:
    """the four PNG paths of one tile id ('test' or 'hold' split)"""

    def __init__(self, pred_dir, targ_dir, img_id, test_hold):
        for d in (pred_dir, targ_dir):
            if not isinstance(d, Path) or not d.is_dir():
                raise AssertionError("'%s' must be an existing directory given as a Path" % (d,))
        if test_hold not in ("test", "hold"):
            raise AssertionError("test_hold '%s' was not one of 'test' or 'hold'" % test_hold)
        self.lp = pred_dir / ("%s_localization_%s_prediction.png" % (test_hold, img_id))
        self.dp = pred_dir / ("%s_damage_%s_prediction.png" % (test_hold, img_id))
        self.lt = targ_dir / ("%s_localization_%s_target.png" % (test_hold, img_id))
        self.dt = targ_dir / ("%s_damage_%s_target.png" % (test_hold, img_id))
        self.paths = (self.lp, self.dp, self.lt, self.dt)

    def load_and_validate_image(self, path):
        """uint8 1024 x 1024 array; the 0..4 value check is the count kernel's 16th slot"""
        from PIL import Image
        if not path.is_file():
            raise AssertionError("file '%s' does not exist or is not a file" % path)
        img = np.array(Image.open(path))
        if img.dtype != np.uint8:
            raise AssertionError("%s is of wrong format %s - should be np.uint8" % (path.name, img.dtype))
        if img.shape != TILE:
            raise AssertionError("%s must be a 1024x1024 image" % path)
        return img

    def load_images(self):
        return [self.load_and_validate_image(p) for p in self.paths]


class RowPairCalculator:
    """[lTP, lFN, lFP] and [TP, FN, FP] x 4 of tiles, counted on the device"""

    @staticmethod
    def rows(tiles):
        """tiles: list of (lp, dp, lt, dt) uint8 host arrays -> int64 numpy [n, 15]"""
        dev = torch.device("cuda", torch.cuda.current_device())
        maps = [torch.from_numpy(np.stack([t[k] for t in tiles])).to(dev) for k in range(4)]
        return score_tiles(*maps).numpy()

    @classmethod
    def get_row_pair(cls, ph):
        row = cls.rows([ph.load_images()])[0].tolist()
        return row[:3], row[3:]


class F1Recorder:
    """precision, recall and F1 of summed counts; P or R is 0 when TP is 0, F1 is 0 when P or R is 0"""

    def __init__(self, TP, FP, FN, name=""):
        self.TP, self.FN, self.FP, self.name = TP, FN, FP, name
        self.P = self.precision()
        self.R = self.recall()
        self.f1 = self.f1()

    def __repr__(self):
        return "%s | f1: %.4f, precision: %.4f, recall: %.4f" % (self.name, self.f1, self.P, self.R)

    def precision(self):
        assert self.TP >= 0 and self.FP >= 0
        return 0 if self.TP == 0 else self.TP / (self.TP + self.FP)

    def recall(self):
        assert self.TP >= 0 and self.FN >= 0
        return 0 if self.TP == 0 else self.TP / (self.TP + self.FN)

    def f1(self):
        assert 0 <= self.P <= 1 and 0 <= self.R <= 1
        return 0 if self.P == 0 or self.R == 0 else (2 * self.P * self.R) / (self.P + self.R)


def _frame(rows, columns):
    try:
        import pandas as pd
    except ImportError:
        return rows
    return pd.DataFrame(rows, columns=columns)


class XviewMetrics:
    """xView2 metrics of a directory of predictions against a directory of targets, named
    {test,hold}_{localization,damage}_NNNNN_{prediction,target}.png"""

    dmg2str = {1: "No damage     (1) ", 2: "Minor damage  (2) ", 3: "Major damage  (3) ", 4: "Destroyed     (4) "}

    def __init__(self, pred_dir, targ_dir, batch=16):
        self.pred_dir, self.targ_dir = Path(pred_dir), Path(targ_dir)
        assert self.pred_dir.is_dir(), "Could not find prediction directory: '%s'" % pred_dir
        assert self.targ_dir.is_dir(), "Could not find target directory: '%s'" % targ_dir
        self.batch = batch
        self.get_path_handlers()
        self.get_dfs()
        self.get_lf1r()
        self.get_df1rs()

    def __repr__(self):
        s = "Localization:\n    %s\n\nDamage:\n" % self.lf1r
        for rec in self.df1rs:
            s += "    %s\n" % rec
        s += "    Harmonic mean dmgs | f1: %.4f\n" % self.df1
        s += "\nScore:\n    Score | f1: %.4f\n" % self.score
        return s.rstrip()

    def get_path_handlers(self):
        self.path_handlers = []
        for path in sorted(self.targ_dir.glob("*.png")):
            parts = path.name[:-len(".png")].split("_")
            assert len(parts) == 4, "target filename %s is not <split>_<task>_<id>_target.png" % path.name
            test_hold, loc_dmg, img_id, target = parts
            assert loc_dmg in ("localization", "damage"), \
                "target filenames must have 'localization' or 'damage' in filename, got %s" % path
            assert target == "target", "%s should equal 'target' when getting path handlers" % target
            if loc_dmg == "localization":
                self.path_handlers.append(PathHandler(self.pred_dir, self.targ_dir, img_id, test_hold))

    def get_dfs(self):
        rows = []
        with ThreadPoolExecutor(max_workers=8) as pool:
            for i in range(0, len(self.path_handlers), self.batch):
                tiles = list(pool.map(PathHandler.load_images, self.path_handlers[i:i + self.batch]))
                rows.append(RowPairCalculator.rows(tiles))
        rows = np.concatenate(rows) if rows else np.zeros((0, 15), dtype=np.int64)
        self.lrows, self.drows = rows[:, :3], rows[:, 3:]
        self.ldf = _frame(self.lrows, LCOLUMNS)
        self.ddf = _frame(self.drows, DCOLUMNS)

    def _sum(self, rows, k):
        return int(rows[:, k].sum())

    def get_lf1r(self):
        self.lf1r = F1Recorder(self._sum(self.lrows, 0), self._sum(self.lrows, 2), self._sum(self.lrows, 1), "Buildings")

    @property
    def lf1(self):
        return self.lf1r.f1

    def get_df1rs(self):
        self.df1rs = [F1Recorder(self._sum(self.drows, 3 * i), self._sum(self.drows, 3 * i + 2),
                                 self._sum(self.drows, 3 * i + 1), self.dmg2str[i + 1]) for i in range(4)]

    @property
    def df1s(self):
        return [rec.f1 for rec in self.df1rs]

    @property
    def df1(self):
        """harmonic mean of the four damage F1s, each offset by 1e-6"""
        xs = self.df1s
        return len(xs) / sum((x + 1e-6) ** -1 for x in xs)

    @property
    def score(self):
        return 0.3 * self.lf1 + 0.7 * self.df1

    @classmethod
    def compute_score(cls, pred_dir, targ_dir, out_fp):
        """write the metrics JSON (score, damage_f1, localization_f1 and the four per-class damage F1s) to out_fp"""
        self = cls(pred_dir, targ_dir)
        d = {"score": self.score, "damage_f1": self.df1, "localization_f1": self.lf1}
        d["damage_f1_no_damage"] = self.df1s[0]
        d["damage_f1_minor_damage"] = self.df1s[1]
        d["damage_f1_major_damage"] = self.df1s[2]
        d["damage_f1_destroyed"] = self.df1s[3]
        with open(out_fp, "w") as f:
            json.dump(d, f)
        print("Wrote metrics to %s" % out_fp)
        return d


compute_score = XviewMetrics.compute_score


if __name__ == "__main__":
    p = ArgumentParser(description="xView2 score of a prediction directory against a target directory")
    p.add_argument("pred_dir")
    p.add_argument("targ_dir")
    p.add_argument("out_fp")
    a = p.parse_args()
    compute_score(os.path.expanduser(a.pred_dir), os.path.expanduser(a.targ_dir), os.path.expanduser(a.out_fp))
