"""Host restatement of the tolerance simplification (include/xv2.h xv2_polygon_simplify), written from the header's text as
the RECURSIVE form of Douglas-Peucker with Python integers, and the case table of tests/test_simplify_cpu.py and
tests/test_simplify_gpu.py.  The kernel is level-synchronous (every open segment of a ring picks its farthest vertex in the
same round), so the two are independent formulations of one rule.  Every value is an integer and every comparison is ==.

One remark on the rule's first key line (L2 == 0, a segment whose two ends are one point): a vertex that coincides with an
end of its segment has key 0, and 0 is never above the threshold, so a vertex is never kept next to a kept copy of itself
and the line cannot be reached from the two anchors.  The restatement keeps it as the header states it; `revisit` is the
ring that passes one corner twice."""
import functools
import sys

import numpy as np

import polygons_ref as R

RING_COLS = 8
QS = (0, 8, 16, 24, 64)
EXT_MAX = 32767
GROUPS, LDS_MAX = (8, 16, 32, 64), 1024          # the ring sizes at which csrc/simplify.hip changes its path


# ---- the rule ------------------------------------------------------------------------------------------------------------
def key_scale(A, B, P):
    dx, dy = B[0] - A[0], B[1] - A[1]
    vx, vy = P[0] - A[0], P[1] - A[1]
    L2 = dx * dx + dy * dy
    if L2 == 0:
        return vx * vx + vy * vy, 1
    t = vx * dx + vy * dy
    if t <= 0:
        return (vx * vx + vy * vy) * L2, L2
    if t >= L2:
        wx, wy = P[0] - B[0], P[1] - B[1]
        return (wx * wx + wy * wy) * L2, L2
    c = vx * dy - vy * dx
    return c * c, L2


def within(A, B, P, q):
    """dist(P, segment A B) <= T, in exact integers"""
    k, s = key_scale(A, B, P)
    return k <= (q * q * s) >> 8


def _chain(v, a, b, q, keep, depth, tie_high=False):
    """the open chain v[a..b] (v has v[n] = v[0] appended): marks what is kept strictly inside it; returns the depth"""
    best, at = -1, -1
    for i in range(a + 1, b):
        k, _ = key_scale(v[a], v[b], v[i])
        if k > best or (tie_high and k == best):
            best, at = k, i
    if at < 0:
        return depth
    _, s = key_scale(v[a], v[b], v[at])
    if best > (q * q * s) >> 8:
        keep[at] = True
        return max(_chain(v, a, at, q, keep, depth + 1, tie_high), _chain(v, at, b, q, keep, depth + 1, tie_high))
    return depth


def simplify_ring(pts, q, tie_high=False):
    """pts: [(x, y), ...] -> (kept points, flag, rounds): rounds is the depth of the recursion, which is the number of
    rounds in which the level-synchronous form splits something"""
    pts = [(int(x), int(y)) for x, y in pts]
    n = len(pts)
    if n and (max(p[0] for p in pts) - min(p[0] for p in pts) > EXT_MAX or max(p[1] for p in pts) - min(p[1] for p in pts) > EXT_MAX):
        return pts, 2, 0
    if n < 3:
        return pts, 1, 0
    d2 = [(p[0] - pts[0][0]) ** 2 + (p[1] - pts[0][1]) ** 2 for p in pts]
    m = d2.index(max(d2))
    if d2[m] == 0:
        return pts, 1, 0
    v = pts + pts[:1]
    keep = [False] * (n + 1)
    keep[0] = keep[m] = True
    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, n + 200))
    try:
        depth = max(_chain(v, 0, m, q, keep, 0, tie_high), _chain(v, m, n, q, keep, 0, tie_high))
    finally:
        sys.setrecursionlimit(old)
    out = [p for p, k in zip(pts, keep) if k]
    if len(out) < 3:
        return pts, 1, depth
    return out, 0, depth


def simplify_table(rings, verts, q):
    """what xv2_polygon_simplify writes: (out_rings int64 [R,8], out_verts int32 [out_total,2], out_total)"""
    rings = np.asarray(rings, dtype=np.int64).reshape(-1, RING_COLS)
    verts = np.asarray(verts, dtype=np.int32).reshape(-1, 2)
    out_r, out_v = rings.copy(), []
    vl = verts.tolist()
    for i, r in enumerate(rings.tolist()):
        kept, flag, _ = simplify_ring(vl[r[3]:r[3] + r[2]], q)
        out_r[i, 2], out_r[i, 3], out_r[i, 4], out_r[i, 7] = len(kept), len(out_v), R.shoelace(kept), flag
        out_v.extend(kept)
    return out_r, np.array(out_v, dtype=np.int32).reshape(-1, 2), len(out_v)


# ---- tables without a mask -------------------------------------------------------------------------------------------------
def table_of(point_lists):
    """ring rows and the vertex array of a list of rings: root i, leader 4 i, the ring's own 2A and vertex count as its
    perimeter, tile 0"""
    rings, verts = [], []
    for i, pts in enumerate(point_lists):
        pts = [(int(x), int(y)) for x, y in pts]
        rings.append([i, 4 * i, len(pts), len(verts), R.shoelace(pts), len(pts), 0, 0])
        verts.extend(pts)
    return np.array(rings, dtype=np.int64).reshape(-1, RING_COLS), np.array(verts, dtype=np.int32).reshape(-1, 2)


def square_spiral(n=200):
    """n corners of a square spiral that winds outwards: legs of 2, 2, 4, 4, 6, 6, ... (closed by the chord to its start)"""
    pts, x, y = [], 0, 0
    for k in range(n):
        pts.append((x, y))
        step = 2 * (k // 2 + 1)
        x, y = x + (step, 0, -step, 0)[k % 4], y + (0, step, 0, -step)[k % 4]
    return pts


def zigzag(n=300):
    """a zigzag of growing amplitude along x, closed below it: the farthest vertex of what is left is always the last tooth,
    so the level-synchronous form needs about n rounds"""
    return [(0, -4 * n)] + [(3 * i, (i + 2) * (i + 2) * (1 if i % 2 else -1) // 8 + 3 * n) for i in range(1, n)]


def zigzag_linear(n=1100):
    """the same with teeth that grow by a constant, so that more than LDS_MAX vertices stay inside the extent limit: about n
    rounds on the path that keeps its state in global memory"""
    return [(0, -4 * n)] + [(3 * i, (i + 2) * 12 * (1 if i % 2 else -1) + 14000) for i in range(1, n)]


def circle(n, radius, seed, jitter=3, centre=(0, 0)):
    """n points on a circle with a few pixels of jitter, counter-clockwise on screen coordinates read as plain (x, y)"""
    rng = np.random.RandomState(seed)
    a = 2 * np.pi * np.arange(n) / n
    x = np.rint(radius * np.cos(a)).astype(np.int64) + rng.randint(-jitter, jitter + 1, n) + centre[0]
    y = np.rint(radius * np.sin(a)).astype(np.int64) + rng.randint(-jitter, jitter + 1, n) + centre[1]
    return list(zip(x.tolist(), y.tolist()))


def tie_ring():
    """vertices 1 and 2 are equally far (6) from the chord of their chain, and which of them is taken first decides whether
    the other one survives at q = 64 (tests/test_simplify_cpu.py checks that the other tie rule gives another ring)"""
    return [(0, 0), (3, 6), (30, 6), (60, 0), (30, -40)]


def revisit_ring():
    """passes the corner (10, 10) twice, as a hole of two pixels that meet diagonally does"""
    return [(0, 0), (10, 0), (10, 10), (20, 10), (20, 20), (10, 20), (10, 10), (0, 10)]


def threshold_rings():
    """k - 1, k and k + 1 vertices around both path thresholds of the kernel (circle_5000 lies well above the second)"""
    return ([circle(n, 10 * k, 100 + n, 2, (1000, 500)) for k in GROUPS for n in (k - 1, k, k + 1)]
            + [circle(n, 3000, 200 + n, 2, (-500, 7000)) for n in (LDS_MAX - 1, LDS_MAX, LDS_MAX + 1)])


def tiny_rings():
    """n = 1, 2, 3, an empty row between them, all vertices equal, and a degenerate collinear ring"""
    return [[(5, 7)], [(1, 1), (4, 5)], [], [(0, 0), (4, 0), (0, 3)], [(3, 3)] * 5, [(0, 0), (5, 0), (9, 0), (2, 0)]]


def extent_rings():
    """extent exactly 32767 in x and in y (simplified), 32768 in x, 32768 in y (flag 2), with vertices worth dropping"""
    def box(w, h):
        return [(-7, 11), (w // 2 - 7, 12), (w - 7, 11), (w - 7, h // 2 + 11), (w - 7, h + 11), (w // 3 - 7, h + 10), (-7, h + 11)]
    return [box(32767, 32767), box(32768, 100), box(100, 32768), box(32767, 5), box(32768, 32768)]


def translate(point_lists, dx, dy):
    return [[(x + dx, y + dy) for x, y in pts] for pts in point_lists]


def mixed_masks():
    """six tiles of 33 x 47, two of them empty: several hundred rings, most of them small"""
    z = np.zeros((33, 47), dtype=bool)
    return [R.random_mask(12, 33, 47, 50), z, R.random_mask(11, 33, 47, 10), R.BR.blobs(14, 33, 47), z, R.random_mask(13, 33, 47, 90)]


TRANSLATED = ("tie", "revisit", "circle_65")          # name -> name + "_far" is the same table moved by (2^20, 2^20)
FAR = 1 << 20


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (rings int64 [R,8], verts int32 [V,2], traced): traced tables come from polygons_ref's tracer"""
    out = {}
    for name, mask in R.shape_cases().items():
        r, v, _ = R.trace_tile(R.labels_of(mask))
        out["shape_" + name] = (r, v, True)
    _, r, v, _ = R.trace(np.stack([R.labels_of(m) for m in R.batch_case()]))
    out["batch"] = (r, v, True)
    _, r, v, _ = R.trace(np.stack([R.labels_of(m) for m in mixed_masks()]))
    out["mixed"] = (r, v, True)
    synth = {
        "spiral_200": [square_spiral(200)],
        "zigzag_300": [zigzag(300)],
        "zigzag_1100": [zigzag_linear(1100)],
        "circle_5000": [circle(5000, 16000, 7)],
        "thresholds": threshold_rings(),
        "tie": [tie_ring()],
        "revisit": [revisit_ring()],
        "circle_65": [circle(65, 40, 3, 2)],
        "tiny": tiny_rings(),
        "extent": extent_rings(),
    }
    for k in TRANSLATED:
        synth[k + "_far"] = translate(synth[k], FAR, FAR)
    for name, lists in synth.items():
        out[name] = table_of(lists) + (False,)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, q):
    """the restatement's result for a case of the table, computed once and shared (treat it as read-only)"""
    rings, verts, _ = cases()[name]
    return simplify_table(rings, verts, q)


def polygons_of(rings, verts, q):
    """polygons_ref.polygons of a simplified tile, each with "simplified": q, as utils.polygons.building_polygons returns"""
    out_r, out_v, _ = simplify_table(rings, verts, q)
    polys = R.polygons(out_r, out_v)
    for p in polys:
        p["simplified"] = q
    return polys
