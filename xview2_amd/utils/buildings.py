"""A prediction as a list of buildings: where each one is, how big it is, its damage class and the model's confidence.

The table is computed on the MI355X (csrc/buildings.hip, xv2_building_table) from the two label maps the prediction PNGs
are written from: the 4-connected components of pre != 0 are the buildings, post gives the damage pixels, and the
localization probabilities (when there are any) the confidence.  Every column of a row is an integer (include/xv2.h lists
them), so the table, and the CSV written from it, has the same bytes on every run.

    python -m xview2_amd.utils.buildings PRE.png POST.png OUT.csv
"""
import json

import numpy as np

COLS = 16
MIN_ROWS = 1024          # first row capacity per tile: max(MIN_ROWS, H * W // PIXELS_PER_ROW)
PIXELS_PER_ROW = 256
FIELDS = ("id", "y0", "x0", "y1", "x1", "area", "cy", "cx", "damage", "n1", "n2", "n3", "n4", "n_other", "confidence")


def first_capacity(H, W):
    return max(MIN_ROWS, H * W // PIXELS_PER_ROW)


def building_table(pre, post, loc=None, capacity=None, return_labels=False):
    """pre, post: uint8 [H,W] or [B,H,W] device maps (the label maps of the two PNGs); loc: fp32 probabilities of the same
    shape or None.  Returns numpy int64 [n_b, 16] per tile (a list; one array for unbatched input), rows in
    scipy.ndimage.label's order.  capacity: first row capacity per tile (default first_capacity(H, W)); a tile with more
    buildings makes the kernels run once more with the capacity its count asks for.  return_labels: also return the int32
    device labels of pre != 0 the table was built from (utils.polygons traces the outlines from them)."""
    import torch
    from .. import ops
    single = pre.dim() == 2
    if single:
        pre, post = pre.unsqueeze(0), post.unsqueeze(0)
        loc = loc.unsqueeze(0) if loc is not None else None
    if pre.dtype != torch.uint8 or post.dtype != torch.uint8 or pre.shape != post.shape or pre.dim() != 3:
        raise ValueError("building_table: pre and post must be uint8 maps of one shape [H,W] or [B,H,W], got %s %s and %s %s"
                         % (pre.dtype, tuple(pre.shape), post.dtype, tuple(post.shape)))
    if loc is not None:
        loc = loc.float()
    B, H, W = pre.shape
    labels = ops.label_components(pre)
    cap = first_capacity(H, W) if capacity is None else int(capacity)
    rows, count = ops.building_table(labels, post, loc, cap)
    n = count.cpu().numpy()          # the only host decision, after the last launch
    if int(n.max()) > cap:
        rows, count = ops.building_table(labels, post, loc, int(n.max()))
        n = count.cpu().numpy()
    host = rows[:, :int(n.max())].cpu().numpy()
    out = [np.ascontiguousarray(host[b, :int(n[b])]) for b in range(B)]
    if return_labels:
        return (out[0], labels[0]) if single else (out, labels)
    return out[0] if single else out


def to_records(rows, H, W, confidence=True):
    """one dict per row: id (1-based, row order), the inclusive box, area, the centroid (cy, cx) as Python floats from the
    integer sums, the voted damage class, the pixel counts per class and (unless confidence is False: no localization
    probabilities went in) the mean quantised probability"""
    out = []
    for i, r in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, COLS).tolist()):
        area = r[1]
        if not (0 <= r[0] < H * W and area >= 1 and 0 <= r[2] <= r[4] < H and 0 <= r[3] <= r[5] < W):
            raise ValueError("row %d is no building of a %d x %d map: %s" % (i, H, W, r))
        rec = {"id": i + 1, "y0": r[2], "x0": r[3], "y1": r[4], "x1": r[5], "area": area, "cy": r[6] / area,
               "cx": r[7] / area, "damage": r[13], "n1": r[8], "n2": r[9], "n3": r[10], "n4": r[11], "n_other": r[12]}
        if confidence:
            rec["confidence"] = r[14] / (65535 * area)
        out.append(rec)
    return out


def write_csv(path, records):
    """one header line, then one line per building; floats as repr, so the file is a function of the integers alone"""
    fields = [f for f in FIELDS if f != "confidence" or any("confidence" in r for r in records)]
    with open(path, "w", newline="\n") as f:
        f.write(",".join(fields) + "\n")
        for r in records:
            f.write(",".join(repr(r[k]) for k in fields) + "\n")


def read_csv(path):
    """the records write_csv wrote (ints stay ints, floats round-trip through repr)"""
    with open(path) as f:
        fields = f.readline().rstrip("\n").split(",")
        return [{k: (float(v) if k in ("cy", "cx", "confidence") else int(v)) for k, v in zip(fields, line.rstrip("\n").split(","))}
                for line in f if line.strip()]


def summary(records):
    """the number of buildings, buildings per voted damage class 0..4 and pixels per damage class (0 = n_other)"""
    per_class = [0] * 5
    pixels = [0] * 5
    for r in records:
        per_class[r["damage"]] += 1
        for c, k in enumerate(("n_other", "n1", "n2", "n3", "n4")):
            pixels[c] += r[k]
    return {"buildings": len(records), "buildings_per_damage": per_class, "pixels_per_damage": pixels}


def write_summary(path, records):
    with open(path, "w") as f:
        json.dump(summary(records), f, indent=1, sort_keys=True)
        f.write("\n")


def main(argv=None):
    import sys
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 3:
        raise SystemExit("usage: python -m xview2_amd.utils.buildings PRE.png POST.png OUT.csv")
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.buildings runs on the MI355X only; there is no CPU fallback")
    pre, post = (np.asarray(Image.open(p)) for p in argv[:2])
    if pre.ndim != 2 or pre.shape != post.shape or pre.dtype != np.uint8 or post.dtype != np.uint8:
        raise ValueError("%s and %s must be 8-bit single-channel images of one size" % (argv[0], argv[1]))
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = building_table(torch.from_numpy(pre.copy()).to(dev), torch.from_numpy(post.copy()).to(dev))
    records = to_records(rows, pre.shape[0], pre.shape[1], confidence=False)
    write_csv(argv[2], records)
    return len(records)


if __name__ == "__main__":
    print("%d buildings" % main())
