"""Host restatement of the building outlines (include/xv2.h xv2_polygon_count / xv2_polygon_trace): a sequential tracer
written from the header's contract, an even-odd rasteriser that is independent of it, and the case table of
tests/test_polygons_cpu.py and tests/test_polygons_gpu.py.  Every value is an integer, so every comparison is ==."""
import numpy as np
from scipy import ndimage

import buildings_ref as BR

RING_COLS = 8
DX = (1, 0, -1, 0)          # directions 0 E, 1 S, 2 W, 3 N on screen (y down); side s heads in direction s
DY = (0, 1, 0, -1)
EIGHT = np.ones((3, 3), dtype=int)


def _left(d):
    return (d + 3) % 4


def _fg(lab, y, x):
    H, W = lab.shape
    return 0 <= y < H and 0 <= x < W and lab[y, x] != 0


def boundary_edges(lab):
    """ascending ids 4 (y W + x) + s of the boundary edges of one tile"""
    H, W = lab.shape
    out = []
    for y in range(H):
        for x in range(W):
            if lab[y, x] == 0:
                continue
            for s in range(4):
                n = _left(s)                       # the neighbour across side s lies to the left of the edge
                if not _fg(lab, y + DY[n], x + DX[n]):
                    out.append(4 * (y * W + x) + s)
    return out


def successor(lab, eid):
    """the three-pixel rule"""
    W = lab.shape[1]
    p, s = divmod(eid, 4)
    y, x = divmod(p, W)
    ay, ax = y + DY[s], x + DX[s]
    ly, lx = ay + DY[_left(s)], ax + DX[_left(s)]
    if not _fg(lab, ay, ax):
        return 4 * p + (s + 1) % 4
    if not _fg(lab, ly, lx):
        return 4 * (ay * W + ax) + s
    return 4 * (ly * W + lx) + (s + 3) % 4


def end_corner(W, eid):
    p, s = divmod(eid, 4)
    y, x = divmod(p, W)
    return ((x + 1, y), (x + 1, y + 1), (x, y + 1), (x, y))[s]


def shoelace(pts):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]))


def trace_tile(lab, tile=0, first_vertex=0):
    """(rings int64 [R,8], verts int32 [V,2], edges) of one tile: walks the successor map from every unvisited edge in
    ascending id, so rings come out in ascending leader"""
    lab = np.asarray(lab)
    W = lab.shape[1]
    edges = boundary_edges(lab)
    eset = set(edges)
    seen = set()
    rings, verts = [], []
    for lead in edges:
        if lead in seen:
            continue
        pts, n, e = [], 0, lead
        while True:
            assert e in eset and e not in seen, "the successor map is no permutation of the boundary edges"
            seen.add(e)
            n += 1
            nxt = successor(lab, e)
            if nxt % 4 != e % 4:
                pts.append(end_corner(W, e))
            e = nxt
            if e == lead:
                break
            assert n <= len(edges), "a cycle does not close"
        py, px = divmod(lead // 4, W)
        rings.append([int(lab[py, px]) - 1, lead, len(pts), first_vertex + len(verts), shoelace(pts), n, tile, 0])
        verts.extend(pts)
    return (np.array(rings, dtype=np.int64).reshape(-1, RING_COLS), np.array(verts, dtype=np.int32).reshape(-1, 2),
            len(edges))


def trace(labels):
    """what the device returns for int32 [B,H,W]: counts int64 [B,2], rings [R,8], verts [V,2], ring_count int32 [B]"""
    labels = np.asarray(labels)
    counts, rings, verts, rc = [], [], [], []
    nv = 0
    for b in range(labels.shape[0]):
        r, v, ne = trace_tile(labels[b], b, nv)
        counts.append([ne, len(v)])
        rings.append(r)
        verts.append(v)
        rc.append(len(r))
        nv += len(v)
    return (np.array(counts, dtype=np.int64).reshape(-1, 2), np.concatenate(rings), np.concatenate(verts),
            np.array(rc, dtype=np.int32))


def rasterise(rings, verts, H, W):
    """even-odd fill at pixel centres from the vertical ring edges alone: a centre (x + 0.5, y + 0.5) is inside when an odd
    number of vertical edges that span its row lie to its left"""
    out = np.zeros((H, W), dtype=bool)
    for r in np.asarray(rings).reshape(-1, RING_COLS):
        pts = np.asarray(verts)[r[3]:r[3] + r[2]].tolist()
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if x0 == x1 and y0 != y1:
                out[min(y0, y1):max(y0, y1), x0:] ^= True
    return out


def polygons(rings, verts):
    """one tile's ring rows -> [{"root", "exterior", "holes"}] in ascending root, holes in ascending leader"""
    out = {}
    for r in np.asarray(rings).reshape(-1, RING_COLS).tolist():
        pts = np.asarray(verts)[r[3]:r[3] + r[2]].tolist()
        poly = out.setdefault(r[0], {"root": r[0], "exterior": None, "holes": []})
        if r[1] == 4 * r[0]:
            poly["exterior"] = pts
        else:
            poly["holes"].append(pts)
    return [out[k] for k in sorted(out)]


def expected_ring_count(mask):
    """4-connected foreground components + 8-connected components of the background padded by one pixel - 1"""
    mask = np.asarray(mask) != 0
    n4 = ndimage.label(mask, structure=BR.FOUR)[1]
    n8 = ndimage.label(~np.pad(mask, 1), structure=EIGHT)[1]
    return n4 + n8 - 1


def labels_of(mask):
    return BR.label_min_index(mask)


# ---- cases --------------------------------------------------------------------------------------------------------------
def serpentine(n=96):
    """even rows full, odd rows joined alternately at the right and the left end: one component, one ring"""
    m = np.zeros((n, n), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, n, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = True
    return m


def nested():
    """building, hole, island, hole"""
    m = np.zeros((17, 17), dtype=bool)
    m[1:16, 1:16] = True
    m[3:14, 3:14] = False
    m[5:12, 5:12] = True
    m[7:10, 7:10] = False
    return m


def diagonal_holes():
    m = np.ones((4, 4), dtype=bool)
    m[1, 1] = m[2, 2] = False
    return m


def random_mask(seed, H, W, percent):
    return BR._hash(seed, (H, W), 100) < percent


def row(n):
    m = np.zeros((3, n + 2), dtype=bool)
    m[1, 1:n + 1] = True
    return m


def all_borders():
    """one component that touches all four borders, with a hole and a separate island in it"""
    m = np.zeros((9, 11), dtype=bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    m[4, 4:7] = True
    return m


def shape_cases():
    """name -> bool mask [H,W]"""
    corner = np.zeros((2, 2), dtype=bool)
    corner[0, 0] = corner[1, 1] = True
    return {
        "one_fg": np.ones((1, 1), dtype=bool),
        "one_bg": np.zeros((1, 1), dtype=bool),
        "full_1x7": np.ones((1, 7), dtype=bool),
        "full_7x1": np.ones((7, 1), dtype=bool),
        "full_64": np.ones((64, 64), dtype=bool),
        "full_65x63": np.ones((65, 63), dtype=bool),
        "row_126": row(126),
        "row_127": row(127),
        "row_128": row(128),
        "checker_8": np.add.outer(np.arange(8), np.arange(8)) % 2 == 0,
        "diagonal_holes": diagonal_holes(),
        "corner_touch": corner,
        "nested_17": nested(),
        "serpentine_96": serpentine(96),
        "random_33x47_p10": random_mask(11, 33, 47, 10),
        "random_33x47_p50": random_mask(12, 33, 47, 50),
        "random_33x47_p90": random_mask(13, 33, 47, 90),
        "all_borders": all_borders(),
    }


def batch_case():
    """B = 3 with an empty tile in the middle and a tile that touches all four borders"""
    full = np.zeros((9, 11), dtype=bool)
    full[2:7, 3:9] = True
    full[4, 5] = False
    return np.stack([full, np.zeros((9, 11), dtype=bool), all_borders()])


# the sizes the CPU test sweeps (the issue's own check: 1 x 1 up to 33 x 47, p = 0.1, 0.5, 0.9)
SWEEP_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (8, 8), (13, 7), (33, 47)]
SWEEP_PERCENT = (10, 50, 90)
