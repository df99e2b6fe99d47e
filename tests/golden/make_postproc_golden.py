"""Regenerate tests/golden/postproc_golden.json from the reference's own offline scripts (CPU only).

    python tests/golden/make_postproc_golden.py REFERENCE_CHECKOUT

REFERENCE_CHECKOUT is a checkout of the reference repository (michal2409/xView2).  Its utils/post_process.py and
utils/xview2_metrics.py are imported at run time, nothing of them is stored: the fixture holds sha256 digests of the
output arrays, per-tile count rows and the metrics dictionary.  skimage is replaced by what skimage's dilation computes
for an odd square footprint, scipy.ndimage.grey_dilation with footprint ones((r, r)); the reference's `save` is
replaced by a capture of the array it would write.

Component voting runs through the reference where its per-building loop (one full-tile scan per component) finishes
in reasonable time: cases with more than MAX_COMPONENTS components are recorded without the components variants."""
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import postproc_ref as R  # noqa: E402

RATES = (0, 1, 3, 5)
MAX_COMPONENTS = 3000


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _stub_modules():
    import scipy.ndimage as nd
    sk = types.ModuleType("skimage")
    morph = types.ModuleType("skimage.morphology")
    morph.square = lambda r: np.ones((r, r), dtype=np.uint8)
    morph.dilation = lambda img, fp: nd.grey_dilation(img, footprint=fp)
    sk.morphology = morph
    sys.modules.setdefault("skimage", sk)
    sys.modules.setdefault("skimage.morphology", morph)
    for name in ("joblib", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.Parallel = m.delayed = m.tqdm = None
            sys.modules[name] = m


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod   # the metrics' process pool pickles its classes by module name
    spec.loader.exec_module(mod)
    return mod


def postproc_digests(ref_dir):
    _stub_modules()
    pp = _load(os.path.join(ref_dir, "utils", "post_process.py"), "ref_post_process")
    captured = {}
    pp.save = lambda img, d, fname: captured.__setitem__(fname, img.astype(np.uint8))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (loc, dmg) in sorted(R.cases().items()):
            # five-channel input: the reference applied to the four damage channels (this project's documented rule)
            ref_dmg = dmg[1:5] if dmg.ndim == 3 and dmg.shape[0] == 5 else dmg
            lp, dp = os.path.join(tmp, "test_localization_00000.npy"), os.path.join(tmp, "test_damage_00000.npy")
            np.save(lp, loc)
            np.save(dp, ref_dmg)
            _, post = R.fuse(loc, dmg)
            lab = R.label_min_index(post > 0)
            ncomp = len(np.unique(lab[lab > 0]))
            rec = {"components": ncomp}
            for comp in (False, True):
                if comp and ncomp > MAX_COMPONENTS:
                    continue
                for rate in RATES:
                    captured.clear()
                    args = SimpleNamespace(components=comp, dilate=rate > 0, dilation_rate=rate)
                    pp.post_process(args, lp, dp)
                    pre = captured["test_localization_00000_prediction.png"]
                    pst = captured["test_damage_00000_prediction.png"]
                    rec["c%d_r%d" % (comp, rate)] = [digest(pre), digest(pst)]
            out[name] = rec
            print(name, ncomp, flush=True)
    return out


def metrics_record(ref_dir):
    from PIL import Image
    xm = _load(os.path.join(ref_dir, "utils", "xview2_metrics.py"), "ref_xview2_metrics")
    tiles = R.metric_tiles()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        pred, targ = os.path.join(tmp, "predictions"), os.path.join(tmp, "targets")
        os.makedirs(pred)
        os.makedirs(targ)
        for k, (lp, dp, lt, dt) in enumerate(tiles):
            for d, kind, suffix, a in ((pred, "localization", "prediction", lp), (pred, "damage", "prediction", dp),
                                       (targ, "localization", "target", lt), (targ, "damage", "target", dt)):
                Image.fromarray(a).save(os.path.join(d, "test_%s_%05d_%s.png" % (kind, k, suffix)))
            ph = xm.PathHandler(xm.Path(pred), xm.Path(targ), "%05d" % k, "test")
            lrow, drow = xm.RowPairCalculator.get_row_pair(ph)
            rows.append([int(v) for v in lrow + drow])
        out_fp = os.path.join(tmp, "metrics.json")
        xm.XviewMetrics.compute_score(pred, targ, out_fp)
        with open(out_fp) as f:
            text = f.read()
    return {"rows": rows, "json": text, "dict": json.loads(text)}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = sys.argv[1]
    gold = {"postprocess": postproc_digests(ref_dir), "metrics": metrics_record(ref_dir)}
    with open(os.path.join(HERE, "postproc_golden.json"), "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
