"""Building polygons as label maps: xBD label files, or the files `--polygons` writes, painted into uint8 masks.

The fill runs on the MI355X (csrc/rasterize.hip, xv2_rasterize_polygons; include/xv2.h states the contract): a pixel is
covered by a feature when its sample point lies on one of the feature's edges or an odd number of edges cross the ray to its
right (even-odd over all rings, closed boundary), and the features of a tile are painted in file order, the last one winning.
The host only parses, rounds and packs tables; it loops over no pixel.

Three rules say where a pixel is sampled and how vertices are rounded:
    reference  the exterior ring only, vertices rounded half to even to whole pixels and read as pixel indices, the pixel
               sampled at its lattice point: the conventions of the reference's label conversion (cv2.fillPoly on rounded
               vertices).  The fill itself is this project's rule, NOT pinned to cv2: like Pillow's ImageDraw.polygon, fillPoly
               also draws the edge lines, which adds pixels up to half a pixel outside slanted edges, so these targets are
               slightly thinner along slanted edges.  Axis-aligned rectangles agree exactly with Pillow.
    corner     integer corner coordinates, holes kept, pixels sampled at their centres: the exact inverse of `--polygons`
               (utils/polygons.py), where pixel (y, x) covers [x, x + 1] x [y, y + 1].
    exact      coordinates rounded half to even to 1/256 pixel, holes kept, pixels sampled at their centres.

    python -m xview2_amd.utils.rasterize IN.{geojson,json} PRE.png POST.png [--size H W] [--rule reference|corner|exact]
"""
import collections
import json
import re

import numpy as np

from .polygons import DAMAGE_NAMES

WINDOW = 32                       # a work item is one WINDOW x WINDOW stretch of a feature's clipped box
COORD_MAX = 1 << 24
RULES = {"reference": (0, 0, False), "corner": (1, 1, True), "exact": (8, 128, True)}     # frac_bits, off, holes kept
SUBTYPE_VALUES = {name: (255 if i == 0 else i) for i, name in enumerate(DAMAGE_NAMES)}

Tables = collections.namedtuple("Tables", "tables n_edges n_features n_work frac_bits off B")
Tables.edges = property(lambda t: t.tables[:4 * t.n_edges].reshape(-1, 4))
Tables.features = property(lambda t: t.tables[4 * t.n_edges:4 * t.n_edges + 8 * t.n_features].reshape(-1, 8))
Tables.work = property(lambda t: t.tables[4 * t.n_edges + 8 * t.n_features:].reshape(-1, 4))

_NUMBER = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_RING = re.compile(r"\(([^()]*)\)")
_POINT = re.compile(r"^\s*(%s)\s+(%s)(?:\s+%s)*\s*$" % (_NUMBER, _NUMBER, _NUMBER))


# ---- reading -------------------------------------------------------------------------------------------------------------
def parse_wkt(text):
    """'POLYGON ((x y, ...), (...))' -> {"exterior": [[x, y], ...], "holes": [[[x, y], ...], ...]} as floats, the closing
    repeat of a ring's first vertex dropped; 'POLYGON EMPTY' -> None (no feature).  MULTIPOLYGON, any other text, or a ring
    with fewer than 3 vertices raises ValueError that names the text."""
    m = re.match(r"^\s*POLYGON\s*(?:Z\s*)?(EMPTY|\((.*)\))\s*$", text, flags=re.I | re.S)
    if m is None:
        raise ValueError("not a WKT POLYGON: %r" % text)
    if m.group(2) is None:
        return None
    body = m.group(2)
    rings = []
    for r in _RING.finditer(body):
        pts = []
        for p in r.group(1).split(","):
            q = _POINT.match(p)
            if q is None:
                raise ValueError("bad vertex %r in WKT polygon %r" % (p.strip(), text))
            pts.append([float(q.group(1)), float(q.group(2))])
        if len(pts) > 1 and pts[0] == pts[-1]:
            pts.pop()
        if len(pts) < 3:
            raise ValueError("a ring with fewer than 3 vertices in WKT polygon %r" % text)
        rings.append(pts)
    if not rings or _RING.sub("", body).replace(",", "").strip():
        raise ValueError("not a WKT POLYGON: %r" % text)
    return {"exterior": rings[0], "holes": rings[1:]}


def read_xbd_json(path, mode):
    """the (polygon, value) pairs of an xBD label file's features.xy, in file order.  mode "pre": every feature 1; "post":
    no-damage 1, minor-damage 2, major-damage 3, destroyed 4, un-classified 255.  A missing or unknown subtype raises
    ValueError naming file and uid."""
    if mode not in ("pre", "post"):
        raise ValueError("read_xbd_json: mode must be 'pre' or 'post', got %r" % (mode,))
    with open(path) as f:
        doc = json.load(f)
    out = []
    for feat in doc["features"]["xy"]:
        props = feat.get("properties", {})
        value = 1
        if mode == "post":
            sub = props.get("subtype")
            if sub not in SUBTYPE_VALUES:
                raise ValueError("%s: feature %s has subtype %r, not one of %s" % (path, props.get("uid"), sub,
                                                                                  ", ".join(DAMAGE_NAMES)))
            value = SUBTYPE_VALUES[sub]
        poly = parse_wkt(feat["wkt"])
        if poly is not None:
            out.append((poly, value))
    return out


def _open_ring(ring):
    pts = [[float(p[0]), float(p[1])] for p in ring]
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts.pop()
    if len(pts) < 3:
        raise ValueError("a ring with fewer than 3 vertices: %r" % (ring,))
    return pts


def read_geojson(path):
    """the (polygon, value) pairs of a FeatureCollection as polygons.write_geojson writes it, in file order: the `damage`
    property is the value (1 where a feature has none), holes kept"""
    with open(path) as f:
        doc = json.load(f)
    out = []
    for i, feat in enumerate(doc["features"]):
        geom = feat["geometry"]
        if geom["type"] != "Polygon":
            raise ValueError("%s: feature %d is a %s, not a Polygon" % (path, i, geom["type"]))
        rings = [_open_ring(r) for r in geom["coordinates"]]
        if not rings:
            continue
        value = int((feat.get("properties") or {}).get("damage", 1))
        if not 0 <= value <= 255:
            raise ValueError("%s: feature %d has damage %d outside 0..255" % (path, i, value))
        out.append(({"exterior": rings[0], "holes": rings[1:]}, value))
    return out


# ---- packing -------------------------------------------------------------------------------------------------------------
def quantise(coords, rule):
    """float coordinates -> the rule's int64 units of 2^-frac_bits pixel, half to even (np.round)"""
    k = RULES[rule][0]
    v = np.asarray(coords, dtype=np.float64)
    if rule == "corner":
        q = np.round(v)
        if not np.array_equal(q, v):
            raise ValueError("rule 'corner' takes integer corner coordinates (the files --polygons writes)")
        return q.astype(np.int64) << k
    return np.round(v * (1 << k)).astype(np.int64)         # (a power of two: the product is exact)


def _gather(tiles, rings_of):
    """one pass over the features: all vertices as one Python list, and per ring / per feature the lengths that cut it"""
    pts, ring_len, feat_rings, feat_tile, feat_value = [], [], [], [], []
    for b, feats in enumerate(tiles):
        for shape, value in feats:
            if not 0 <= int(value) <= 255:
                raise ValueError("feature value %r outside 0..255" % (value,))
            rings = [r for r in rings_of(shape) if len(r)]
            if not rings:
                continue
            for r in rings:
                pts.extend(r)
                ring_len.append(len(r))
            feat_rings.append(len(rings))
            feat_tile.append(b)
            feat_value.append(int(value))
    return pts, ring_len, feat_rings, feat_tile, feat_value


def _tables(a, ring_len, feat_rings, feat_tile, feat_value, B, H, W, k, off):
    """a: int64 [n, 2] vertices of all rings in order -> Tables; numpy over vertices, features and windows, no pixel loop"""
    k, off, H, W = int(k), int(off), int(H), int(W)
    if len(a) == 0:
        return Tables(np.zeros(0, dtype=np.int32), 0, 0, 0, k, off, B)
    if int(np.abs(a).max()) > COORD_MAX:
        raise ValueError("a coordinate exceeds 2^24 units of 2^-%d pixel" % k)
    ring_len = np.asarray(ring_len, dtype=np.int64)
    ring_start = np.cumsum(ring_len) - ring_len
    nxt = np.arange(len(a)) + 1                                        # the next vertex of the same ring
    nxt[ring_start + ring_len - 1] = ring_start
    edges = np.concatenate([a, a[nxt]], axis=1)
    feat_rings = np.asarray(feat_rings, dtype=np.int64)
    first_ring = np.cumsum(feat_rings) - feat_rings
    e_first = ring_start[first_ring]
    e_count = np.add.reduceat(ring_len, first_ring)
    lo = np.minimum.reduceat(a, e_first, axis=0)
    hi = np.maximum.reduceat(a, e_first, axis=0)
    # pixels whose sample (p << k) + off lies in [lo, hi]: ceil((lo - off) / 2^k) .. floor((hi - off) / 2^k)
    p0 = -((off - lo) >> k)
    p1 = (hi - off) >> k
    x0, y0 = np.maximum(p0[:, 0], 0), np.maximum(p0[:, 1], 0)
    x1, y1 = np.minimum(p1[:, 0], W - 1), np.minimum(p1[:, 1], H - 1)
    keep = (x0 <= x1) & (y0 <= y1)
    feats = np.stack([np.asarray(feat_tile), np.asarray(feat_value), e_first, e_count, x0, y0, x1, y1], axis=1)[keep]
    nwx = (feats[:, 6] - feats[:, 4]) // WINDOW + 1
    n_win = nwx * ((feats[:, 7] - feats[:, 5]) // WINDOW + 1)
    owner = np.repeat(np.arange(len(feats)), n_win)
    local = np.arange(int(n_win.sum())) - np.repeat(np.cumsum(n_win) - n_win, n_win)
    work = np.stack([owner, feats[owner, 4] + WINDOW * (local % nwx[owner]), feats[owner, 5] + WINDOW * (local // nwx[owner]),
                     np.zeros_like(owner)], axis=1)
    tables = np.concatenate([edges.reshape(-1), feats.reshape(-1), work.reshape(-1)]).astype(np.int32)
    return Tables(tables, len(edges), len(feats), len(work), k, off, B)


def pack_rings(tiles, H, W, frac_bits, off):
    """tiles: per tile a list of (rings, value), rings a list of integer (x, y) vertex lists in units of 2^-frac_bits pixel
    -> Tables, the buffer xv2_rasterize_polygons takes.  A feature's box is the pixels whose sample point lies in the
    feature's extent, clipped to the tile; features whose box is empty are dropped; every box is cut into 32 x 32 windows."""
    pts, *cuts = _gather(tiles, lambda rings: rings)
    return _tables(np.asarray(pts, dtype=np.int64).reshape(-1, 2), *cuts, len(tiles), H, W, frac_bits, off)


def pack(tiles, H, W, rule="reference"):
    """tiles: per tile a list of (polygon, value) pairs in file order, polygon = {"exterior": [[x, y], ...], "holes": [...]}
    -> Tables under the rule (see the module text).  Features whose box misses the tile are dropped here."""
    if rule not in RULES:
        raise ValueError("unknown rule %r (one of %s)" % (rule, ", ".join(sorted(RULES))))
    k, off, holes = RULES[rule]
    pts, *cuts = _gather(tiles, (lambda p: [p["exterior"]] + list(p["holes"])) if holes else (lambda p: [p["exterior"]]))
    return _tables(quantise(np.asarray(pts, dtype=np.float64).reshape(-1, 2), rule), *cuts, len(tiles), H, W, k, off)


def rasterize_tables(t, H, W):
    from .. import ops
    return ops.rasterize_polygons(t.tables, t.n_edges, t.n_features, t.n_work, t.frac_bits, t.off, t.B, H, W)


def rasterize(tiles, H, W, rule="reference"):
    """the uint8 [B,H,W] device map of `tiles` (as pack takes them) under the rule"""
    return rasterize_tables(pack(tiles, H, W, rule), H, W)


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def read_features(path):
    """-> (features of the PRE map, features of the POST map, the file is an xBD-layout label JSON and no GeoJSON)"""
    with open(path) as f:
        doc = json.load(f)
    if isinstance(doc.get("features"), dict):
        pre = read_xbd_json(path, "pre")
        # a pre-disaster label file carries no subtype at all: its POST map is its PRE map
        graded = any("subtype" in f.get("properties", {}) for f in doc["features"]["xy"])
        return pre, (read_xbd_json(path, "post") if graded else pre), True
    post = read_geojson(path)
    return [(p, 1) for p, _ in post], post, False


def write_png(path, array):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(array, dtype=np.uint8)).save(path, compress_level=9)


def get_parser():
    from argparse import ArgumentParser
    p = ArgumentParser(description="Paint building polygons into a PRE / POST pair of 8-bit label PNGs on the GPU.  The fill "
                       "rule is this project's own (include/xv2.h): it is not pinned to cv2.fillPoly, and rule 'reference' "
                       "gives slightly thinner buildings along slanted edges than a fill that also draws the edge lines.")
    p.add_argument("input", help="GeoJSON as --polygons writes it, or an xBD-layout label JSON")
    p.add_argument("pre", help="PNG to write: every feature painted 1")
    p.add_argument("post", help="PNG to write: every feature painted its damage value (1 for a label file without subtypes)")
    p.add_argument("--size", type=int, nargs=2, default=(1024, 1024), metavar=("H", "W"))
    p.add_argument("--rule", choices=sorted(RULES), default=None,
                   help="default: corner for GeoJSON (the inverse of --polygons), reference for label JSON")
    return p


def main(argv=None):
    args = get_parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("xview2_amd.utils.rasterize runs on the MI355X only; there is no CPU fallback")
    pre, post, is_xbd = read_features(args.input)
    rule = args.rule or ("reference" if is_xbd else "corner")
    H, W = args.size
    maps = rasterize([pre, post], H, W, rule).cpu().numpy()
    write_png(args.pre, maps[0])
    write_png(args.post, maps[1])
    return len(post)


if __name__ == "__main__":
    print("%d features" % main())
