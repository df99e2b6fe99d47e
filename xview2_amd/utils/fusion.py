"""The fusion's parameters on a command line: --loc_threshold, --loc_threshold_dmg, --class_scale and --calibration, shared by
utils.post_process and predict.  numpy-free and torch-free, so a parser can be built without either.

The fusion is pre = (loc > A) | ((loc > B) & (post > 1)), post = argmax(s * dmg) + 1 where pre.  The reference fixes A = 0.3,
B = 0.1 and no scales; with no flag given nothing here changes that, and no new call is made."""
import json
import math

FLAGS = ("loc_threshold", "loc_threshold_dmg", "class_scale")


def parse_class_scale(text):
    """'1,2,2,1.5' -> (1.0, 2.0, 2.0, 1.5): four finite factors > 0; ValueError otherwise"""
    parts = [p.strip() for p in str(text).split(",")]
    if len(parts) != 4 or not all(parts):
        raise ValueError("--class_scale: four comma-separated factors expected, got %r" % (text,))
    v = tuple(float(p) for p in parts)
    if not all(math.isfinite(x) and x > 0 for x in v):
        raise ValueError("--class_scale: every factor must be finite and > 0, got %r" % (text,))
    return v


def add_flags(arg):
    arg("--loc_threshold", type=float, default=None, metavar="A", help="a pixel is a building where the localization "
        "probability exceeds A (the reference's 0.3 when neither this nor --calibration is given).  No value is recommended: "
        "xview2_amd.utils.calibrate picks one on a hold-out set")
    arg("--loc_threshold_dmg", type=float, default=None, metavar="B", help="... or exceeds B <= A where the damage class is "
        "above 1 (the reference's 0.1)")
    arg("--class_scale", type=parse_class_scale, default=None, metavar="s1,s2,s3,s4", help="multiply the four damage "
        "probabilities by these factors before the argmax (softmax models only)")
    arg("--calibration", type=str, default=None, metavar="FILE.json", help="take the three values above from the `best` "
        "point of a report of xview2_amd.utils.calibrate; a flag given explicitly wins over the file")


def load_calibration(path):
    """(A, B, scales) of a calibrate report's best point"""
    with open(path) as f:
        doc = json.load(f)
    try:
        best = doc["best"]
        return float(best["loc_threshold"]), float(best["loc_threshold_dmg"]), parse_class_scale(
            ",".join(repr(float(x)) for x in best["class_scale"]))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s is no report of xview2_amd.utils.calibrate: %s" % (path, e))


def resolve(args):
    """dict(loc_threshold=, dmg_threshold=, class_scale=) for post_process_tiles from parsed flags: every value None unless a
    flag or --calibration sets it; explicit flags win over the file.  A report's all-ones scales stay None (multiplying by one
    changes nothing, and label maps take no scales)."""
    a, b, s = (getattr(args, k, None) for k in FLAGS)
    path = getattr(args, "calibration", None)
    if path is not None:
        ca, cb, cs = load_calibration(path)
        a = ca if a is None else a
        b = cb if b is None else b
        if s is None and cs != (1.0, 1.0, 1.0, 1.0):
            s = cs
    if a is not None or b is not None:
        ra, rb = (0.3 if a is None else a), (0.1 if b is None else b)
        if not (math.isfinite(ra) and math.isfinite(rb)):
            raise ValueError("--loc_threshold / --loc_threshold_dmg must be finite")
        if rb > ra:
            raise ValueError("--loc_threshold_dmg %r must not exceed --loc_threshold %r" % (rb, ra))
    return {"loc_threshold": a, "dmg_threshold": b, "class_scale": s}
