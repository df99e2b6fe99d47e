"""A prediction as building outlines: one polygon per building, with its holes, in files a GIS opens.

The rings are traced on the MI355X (csrc/polygons.hip, xv2_polygon_count and xv2_polygon_trace) from the label map of the
localization PNG: the boundary of every 4-connected component of pre != 0, ordered into closed rings of lattice corners
(include/xv2.h states the contract).  Pixel (y, x) covers [x, x + 1] x [y, y + 1], so coordinates run 0..W and 0..H, y down.
Collinear points are dropped and, unless a tolerance is given, nothing else is simplified.  Read as plain (x, y) pairs the
exterior rings have positive and the holes negative signed area.  Every value is an integer, so the files have the same bytes
on every run.

With a tolerance T > 0 in pixels (`simplify=T`, `--simplify T`) every ring, exterior or hole, is then reduced on the MI355X by
Douglas-Peucker in exact integers (csrc/simplify.hip, xv2_polygon_simplify; include/xv2.h states the rule): a vertex survives
iff it lies more than T from the chord of its chain, T quantised to sixteenths of a pixel.  Every dropped vertex lies within
T of the ring that is left, every coordinate stays an integer corner, and no ring is lost (a ring that would collapse below
three vertices is kept as traced).  Rings are simplified one by one: neighbouring outlines, or a hole and its exterior, may
cross afterwards, a ring may cut itself, and the table's area stays the pixel area.  No tolerance is recommended: there is
no xBD imagery at hand to score one.

One known property: a hole ring may touch itself at a corner (two hole pixels that meet diagonally are one ring that
passes the shared corner twice).  That is topologically right, but strict OGC validators call such a ring non-simple.

    python -m xview2_amd.utils.polygons PRE.png POST.png OUT.geojson [--simplify T]
"""
import json
import math
import os

import numpy as np

RING_COLS = 8
DAMAGE_NAMES = ("un-classified", "no-damage", "minor-damage", "major-damage", "destroyed")


def group_rings(rings, verts):
    """the ring rows of ONE tile (int64 [n, 8]) and the vertex array their column 3 indexes -> one dict
    per building in ascending root: {"root", "exterior": [[x, y], ...], "holes": [[[x, y], ...], ...]}, holes in ascending
    leader.  A ring is its component's exterior iff its leader is 4 * root."""
    out = {}
    if not isinstance(verts, list):          # (a caller with many tiles converts the shared vertex array once)
        verts = np.asarray(verts).tolist()
    for r in np.asarray(rings, dtype=np.int64).reshape(-1, RING_COLS).tolist():
        pts = verts[r[3]:r[3] + r[2]]
        poly = out.setdefault(r[0], {"root": r[0], "exterior": None, "holes": []})
        if r[1] == 4 * r[0]:
            poly["exterior"] = pts
        else:
            poly["holes"].append(pts)
    polys = [out[k] for k in sorted(out)]
    for p in polys:
        if p["exterior"] is None:
            raise ValueError("the rings of root %d hold no exterior (no ring led by edge %d)" % (p["root"], 4 * p["root"]))
    return polys


def quantise_tolerance(T):
    """the tolerance in pixels -> q = round(16 T) (halves up), the integer the rule of include/xv2.h is stated in; 0 <= T <
    4096, and the few T just below 4096 that would round to 65536 give 65535"""
    T = float(T)
    if not 0.0 <= T < 4096.0:                # (NaN fails both comparisons)
        raise ValueError("the simplification tolerance must satisfy 0 <= T < 4096 pixels, got %r" % T)
    return min(int(math.floor(16.0 * T + 0.5)), 65535)


def building_polygons(pre, labels=None, simplify=0.0):
    """pre: uint8 [H,W] or [B,H,W] device map (the label map of the localization PNG).  Returns per tile (a list of lists;
    one list for unbatched input) the polygons of its buildings in the building table's row order.  labels: the int32
    labels of pre != 0 when the caller has them already (utils.buildings.building_table(..., return_labels=True)).
    simplify: the tolerance T in pixels; with quantise_tolerance(T) == 0 nothing new is launched, otherwise the traced rings
    are simplified on the device, only the simplified table and its vertices are read back, and every polygon carries
    "simplified": q."""
    import torch
    from .. import ops
    q = quantise_tolerance(simplify)
    single = pre.dim() == 2
    if single:
        pre = pre.unsqueeze(0)
        labels = labels.unsqueeze(0) if labels is not None and labels.dim() == 2 else labels
    if pre.dtype != torch.uint8 or pre.dim() != 3:
        raise ValueError("building_polygons: pre must be a uint8 map [H,W] or [B,H,W], got %s %s" % (pre.dtype, tuple(pre.shape)))
    if labels is None:
        labels = ops.label_components(pre)
    elif labels.shape != pre.shape:
        raise ValueError("building_polygons: labels %s do not fit pre %s" % (tuple(labels.shape), tuple(pre.shape)))
    counts = ops.polygon_count(labels).cpu().numpy()      # the only read-back before the last launch: it sizes the rest
    rings, verts, ring_count = ops.polygon_trace(labels, int(counts[:, 0].sum()), int(counts[:, 1].sum()))
    n = ring_count.cpu().numpy().astype(np.int64)
    if q:
        rings, verts, total = ops.polygon_simplify(rings, verts, int(n.sum()), q, checked=True)
        verts = verts[:int(total.item())]
    rings, verts = rings[:int(n.sum())].cpu().numpy(), verts.cpu().numpy().tolist()
    ends = np.cumsum(n)
    out = [group_rings(rings[e - k:e], verts) for k, e in zip(n.tolist(), ends.tolist())]
    if q:
        for tile in out:
            for p in tile:
                p["simplified"] = q
    return out[0] if single else out


def _closed(ring):
    return [[int(x), int(y)] for x, y in ring] + [[int(ring[0][0]), int(ring[0][1])]]


def to_wkt(polygon):
    """POLYGON ((x y, ...), (...)): the exterior, then the holes, every ring closed by repeating its first vertex"""
    return "POLYGON (%s)" % ", ".join("(%s)" % ", ".join("%d %d" % (x, y) for x, y in _closed(r))
                                      for r in [polygon["exterior"]] + list(polygon["holes"]))


def _match(polygons, records):
    """records (utils.buildings.to_records rows, or None) in the polygons' order: equally many, and every record's box is
    its polygon's extent.  A polygon that carries "simplified": q may have lost the vertices that touched the box: its
    extent must lie inside the box and fall short of it by at most ceil(q / 16) pixels on each side."""
    if records is None:
        return [None] * len(polygons)
    if len(records) != len(polygons):
        raise ValueError("%d polygons but %d building records" % (len(polygons), len(records)))
    for i, (p, r) in enumerate(zip(polygons, records)):
        xs, ys = [v[0] for v in p["exterior"]], [v[1] for v in p["exterior"]]
        ext, box = (min(ys), min(xs), max(ys), max(xs)), (r["y0"], r["x0"], r["y1"] + 1, r["x1"] + 1)
        slack = (int(p["simplified"]) + 15) // 16 if "simplified" in p else 0
        if not all(0 <= s * (e - b) <= slack for e, b, s in zip(ext, box, (1, 1, -1, -1))):
            raise ValueError("record %d (id %s) is not the building of polygon %d (root %d): the records must be in the "
                             "polygons' order" % (i, r.get("id"), i, p["root"]))
    return records


def _dumps(obj):
    return json.dumps(obj, separators=(", ", ": "))      # insertion order; floats as repr, like buildings.write_csv


def write_geojson(path, polygons, records=None):
    """a FeatureCollection, one Polygon feature per line; properties: the matching record (id, box, area, centroid, damage,
    pixel counts, confidence) when records are given, else id and root"""
    records = _match(polygons, records)
    lines = []
    for i, (p, r) in enumerate(zip(polygons, records)):
        props = {"id": i + 1, "root": int(p["root"])} if r is None else dict(r, damage_name=DAMAGE_NAMES[r["damage"]])
        geom = {"type": "Polygon", "coordinates": [_closed(ring) for ring in [p["exterior"]] + list(p["holes"])]}
        lines.append(_dumps({"type": "Feature", "properties": props, "geometry": geom}))
    with open(path, "w", newline="\n") as f:
        f.write('{"type": "FeatureCollection", "features": [\n' + ",\n".join(lines) + ("\n" if lines else "") + "]}\n")


def write_xbd_json(path, polygons, records):
    """the layout of the xBD label files: features.xy[*] = {"properties": {"feature_type", "subtype", "uid"}, "wkt"}, the
    subtype from the voted damage class, the uid from the file's stem and the record's id"""
    records = _match(polygons, records)
    if polygons and records[0] is None:
        raise ValueError("write_xbd_json needs the building records (the damage class is the subtype)")
    stem = os.path.splitext(os.path.basename(path))[0]
    lines = [_dumps({"properties": {"feature_type": "building", "subtype": DAMAGE_NAMES[r["damage"]],
                                    "uid": "%s-%d" % (stem, r["id"])}, "wkt": to_wkt(p)})
             for p, r in zip(polygons, records)]
    with open(path, "w", newline="\n") as f:
        f.write('{"features": {"xy": [\n' + ",\n".join(lines) + ("\n" if lines else "") + "]}}\n")


def get_parser():
    from argparse import ArgumentParser
    usage = "python -m xview2_amd.utils.polygons PRE.png POST.png OUT.geojson [--simplify T]"

    class Parser(ArgumentParser):
        def error(self, message):            # the usage line is the exit message, as before there were options
            raise SystemExit("usage: %s\n%s" % (usage, message))
    parser = Parser(prog="python -m xview2_amd.utils.polygons", usage=usage)
    parser.add_argument("pre", metavar="PRE.png")
    parser.add_argument("post", metavar="POST.png")
    parser.add_argument("out", metavar="OUT.geojson")
    parser.add_argument("--simplify", type=float, default=0.0, metavar="T", help="drop outline vertices that lie within T "
                        "pixels of what is left (Douglas-Peucker per ring, 0 <= T < 4096); 0 = off")
    return parser


def main(argv=None):
    args = get_parser().parse_args(argv)
    quantise_tolerance(args.simplify)
    argv = [args.pre, args.post, args.out]
    import torch
    from PIL import Image
    from . import buildings
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.polygons runs on the MI355X only; there is no CPU fallback")
    pre, post = (np.asarray(Image.open(p)) for p in argv[:2])
    if pre.ndim != 2 or pre.shape != post.shape or pre.dtype != np.uint8 or post.dtype != np.uint8:
        raise ValueError("%s and %s must be 8-bit single-channel images of one size" % (argv[0], argv[1]))
    dev = torch.device("cuda", torch.cuda.current_device())
    pre_d = torch.from_numpy(pre.copy()).to(dev)
    rows, labels = buildings.building_table(pre_d, torch.from_numpy(post.copy()).to(dev), return_labels=True)
    records = buildings.to_records(rows, pre.shape[0], pre.shape[1], confidence=False)
    write_geojson(argv[2], building_polygons(pre_d, labels, args.simplify), records)
    return len(records)


if __name__ == "__main__":
    print("%d buildings" % main())
