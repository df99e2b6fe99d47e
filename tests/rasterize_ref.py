"""The polygon fill of include/xv2.h (xv2_rasterize_polygons) restated twice on the host, and the cases both test files share.

ref     numpy int64, per edge over the feature's clipped box, from the packed tables (it follows the boxes, not the windows)
brute   pure Python integers, every pixel of the tile against every edge of every feature, from the integer rings: it shares
        neither the packing nor any fixed-width arithmetic with the kernel

Rings are integer (x, y) lists in units of 2^-k pixel; pixel (y, x) is sampled at ((x << k) + off, (y << k) + off)."""
import numpy as np

SAMPLINGS = [(0, 0), (1, 1)]          # (frac_bits, off): lattice points as the reference's rule, pixel centres as "corner"


def ref(T, H, W):
    """uint8 [B,H,W] of a utils.rasterize.Tables"""
    out = np.zeros((T.B, H, W), dtype=np.uint8)
    k, off = T.frac_bits, T.off
    edges = T.edges.astype(np.int64)
    for b, value, e0, ne, x0, y0, x1, y1 in T.features.tolist():
        sy, sx = np.meshgrid((np.arange(y0, y1 + 1, dtype=np.int64) << k) + off,
                             (np.arange(x0, x1 + 1, dtype=np.int64) << k) + off, indexing="ij")
        par = np.zeros(sy.shape, dtype=bool)
        on = np.zeros(sy.shape, dtype=bool)
        for ax, ay, bx, by in edges[e0:e0 + ne].tolist():
            cr = (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)
            on |= (cr == 0) & (sx >= min(ax, bx)) & (sx <= max(ax, bx)) & (sy >= min(ay, by)) & (sy <= max(ay, by))
            if by != ay:
                par ^= (sy >= min(ay, by)) & (sy < max(ay, by)) & ((cr > 0) if by > ay else (cr < 0))
        out[b, y0:y1 + 1, x0:x1 + 1][par | on] = value
    return out


def covered(rings, sx, sy):
    """the contract for one feature and one sample point, in Python integers"""
    crossings = 0
    for ring in rings:
        n = len(ring)
        for i in range(n):
            (ax, ay), (bx, by) = ring[i], ring[(i + 1) % n]
            ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
            cr = (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)
            if cr == 0 and min(ax, bx) <= sx <= max(ax, bx) and min(ay, by) <= sy <= max(ay, by):
                return True
            if min(ay, by) <= sy < max(ay, by) and (cr > 0 if by > ay else cr < 0):
                crossings += 1
    return crossings % 2 == 1


def brute(tiles, H, W, k, off):
    """uint8 [B,H,W]: tiles as utils.rasterize.pack_rings takes them"""
    out = np.zeros((len(tiles), H, W), dtype=np.uint8)
    for b, feats in enumerate(tiles):
        for y in range(H):
            for x in range(W):
                sx, sy = (x << k) + off, (y << k) + off
                for rings, value in feats:
                    if covered(rings, sx, sy):
                        out[b, y, x] = value
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------
def cases(H, W, k, off):
    """name -> tiles.  Coordinates are placed relative to sample points, S(x, y) being the sample point of pixel (y, x), so
    that "on a sample row" and "on a vertex" hold under either sampling; d is a sub-pixel step where the grid has one."""
    u = 1 << k
    d = 1 if k else 0

    def S(x, y, dx=0, dy=0):
        return [x * u + off + dx, y * u + off + dy]

    def X(f):
        return int(f * (W - 1))

    def Y(f):
        return int(f * (H - 1))

    def one(*rings, value=7):
        return [[(list(rings), value)]]

    ring = [S(X(.2), Y(.15)), S(X(.8), Y(.3), d), S(X(.7), Y(.85), 0, d), S(X(.3), Y(.7))]
    rect = [S(X(.1), Y(.1)), S(X(.9), Y(.1)), S(X(.9), Y(.9)), S(X(.1), Y(.9))]
    inner = [S(X(.3), Y(.3)), S(X(.6), Y(.3)), S(X(.6), Y(.7)), S(X(.3), Y(.7))]
    touching = [S(X(.1), Y(.3)), S(X(.5), Y(.3)), S(X(.5), Y(.6)), S(X(.1), Y(.6))]       # its left edge lies on rect's
    tri = [S(X(.1), Y(.1), d, d), S(X(.9), Y(.3), -d), S(X(.4), Y(.9), d, -d)]
    out = {
        "triangle": one(tri),
        "vertex_on_sample": one([S(X(.1), Y(.1)), S(X(.9), Y(.3)), S(X(.4), Y(.9))]),
        "ring_cw": one(ring),
        "ring_ccw": one(ring[::-1]),
        "bow_tie": one([S(X(.1), Y(.1)), S(X(.9), Y(.9)), S(X(.9), Y(.1)), S(X(.1), Y(.9))]),
        "hole": one(rect, inner),
        "hole_touching": one(rect, touching),
        "collinear": one([S(1, 1), S(5, 3), S(9, 5)]),
        "spike": one([S(X(.2), Y(.2)), S(X(.6), Y(.2)), S(X(.6), Y(.6)), S(X(.95), Y(.95), d), S(X(.6), Y(.6))]),
        "horizontal_on_row": one([S(2, 3), S(W - 3, 3), S(W - 6, H - 4, d, d), S(4, H - 4, 0, d)]),
        "diamond": one([S(X(.5), 1), S(X(.5) + 6, 7), S(X(.5), 13), S(X(.5) - 6, 7)]),
        "beyond_borders": one([S(-5, -7), S(W + 6, Y(.3)), S(X(.7), H + 9), S(-3, Y(.6))]),
        "whole_tile": one([S(-1, -1), S(W, -1), S(W, H), S(-1, H)]),
        "outside": one([S(W + 3, 2), S(W + 9, 2), S(W + 9, 8), S(W + 3, 8)]),
        "empty_middle": [[([tri], 5)], [], [([rect], 9)]],
    }
    return out


def comb(n_edges, k=8):
    """one ring of n_edges edges inside a 64 x 64 tile: a zigzag of n_edges - 2 teeth ends closed along the bottom"""
    u = 1 << k
    n = n_edges - 2
    x0, span = u + 44, 62 * u - 100
    pts = [[x0 + (i * span) // (n - 1), (5 * u + 3) if i % 2 == 0 else (40 * u + 77)] for i in range(n)]
    return [[([pts + [[pts[-1][0], 60 * u + 9], [pts[0][0], 60 * u + 9]]], 3)]]


def far_triangle(k, off):
    """vertices near +-2^24 whose slanted edge crosses a 64 x 64 tile: its cross products need more than 32 bits"""
    m = 1 << 24
    return [[([[[-m, -m + 5], [m, m - 3 + off], [m, -m]]], 2)]]


def painter_overlap():
    """three overlapping features with values 3, 255, 1 in that order, corner units (k = 1)"""
    def box(x0, y0, x1, y1):
        return [[2 * x0, 2 * y0], [2 * x1, 2 * y0], [2 * x1, 2 * y1], [2 * x0, 2 * y1]]
    return [[([box(2, 2, 30, 20)], 3), ([box(10, 8, 40, 30)], 255), ([box(5, 12, 25, 36)], 1)]]


def painter_twins():
    ring = [[6, 4], [70, 20], [30, 66]]
    return [[([ring], 4), ([ring], 200)]]


def painter_pixels(n=5000, H=96, W=80):
    """n one-pixel squares (corner units) at positions that repeat, values cycling 1..4: later ones overwrite earlier ones"""
    feats = []
    for i in range(n):
        p = (i * 37) % 3000
        x, y = p % W, p // W
        feats.append(([[[2 * x, 2 * y], [2 * x + 2, 2 * y], [2 * x + 2, 2 * y + 2], [2 * x, 2 * y + 2]]], 1 + i % 4))
    return [feats]


def window_boxes():
    """on a 40 x 70 tile (corner units): a 65 x 1 pixel box (a degenerate ring along one sample row), a 33 x 31 pixel box, and a
    box cut by the right and the lower tile edge"""
    return [[([[[7, 11], [135, 11]]], 6),
             ([[[60, 16], [126, 16], [126, 78], [60, 78]]], 2),
             ([[[100, 50], [180, 50], [180, 120], [100, 120]]], 9)]]
