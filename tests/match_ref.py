"""Host restatement of the building match (include/xv2.h xv2_building_match) and of the object-level score
(xview2_amd/utils/building_metrics.py), a brute-force dense version that checks the restatement itself on tiny tiles, and
the planted cases of tests/test_match_gpu.py with their hand-derived answers.

Labels and tables come from tests/buildings_ref.py; the pair intersections from np.unique over the stacked label pair of
the overlap pixels; the best partner from Fractions of Python ints; the piece count from scipy.ndimage.label of the overlap
mask.  Every value is an integer, so the comparison is ==."""
from fractions import Fraction

import numpy as np
from scipy import ndimage

import buildings_ref as R

COLS = 8


def piece_count(labels_p, labels_t):
    """the number of 4-connected components of the overlap mask"""
    return int(ndimage.label((np.asarray(labels_p) != 0) & (np.asarray(labels_t) != 0), structure=R.FOUR)[1])


def _ranks(labels, rows):
    """per pixel: the row whose column 0 is label - 1, or -1 (background, or a label that names no usable row)"""
    labels = np.asarray(labels).astype(np.int64)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 16)
    hw = labels.size
    out = np.full(labels.shape, -1, dtype=np.int64)
    usable = np.nonzero((rows[:, 0] >= 0) & (rows[:, 0] < hw) & (rows[:, 1] >= 1) & (rows[:, 1] <= hw))[0]
    if len(usable) == 0:
        return out
    roots = rows[usable, 0]
    assert np.all(np.diff(roots) > 0), "tables have ascending roots"
    at = np.minimum(np.searchsorted(roots, labels - 1), len(roots) - 1)
    hit = (labels > 0) & (roots[at] == labels - 1)
    out[hit] = usable[at[hit]]
    return out


def _side(n, areas, roots_other, areas_other, pairs, me):
    """[n, 8] without column 3: pairs is {(a, b): I} keyed (own row, other row) when me == 0, (other, own) when me == 1"""
    out = np.zeros((n, COLS), dtype=np.int64)
    partners = [[] for _ in range(n)]
    for key, inter in pairs.items():
        partners[key[me]].append((key[1 - me], inter))
    for a in range(n):
        best = None
        for b, inter in partners[a]:
            union = areas[a] + areas_other[b] - inter
            cand = (Fraction(inter, union), -roots_other[b], b, inter, union)
            if best is None or cand[:2] > best[:2]:
                best = cand
        out[a, 4] = len(partners[a])
        if best is None:
            out[a, :3] = (-1, 0, areas[a])
        else:
            out[a, :3] = (best[2], best[3], best[4])
    return out


def match_tables(labels_p, rows_p, labels_t, rows_t, iou=(1, 2)):
    """(match_p [n_p, 8], match_t [n_t, 8]) of one tile from its two label maps (1 + smallest index) and tables"""
    rows_p, rows_t = (np.asarray(r, dtype=np.int64).reshape(-1, 16) for r in (rows_p, rows_t))
    rp, rt = _ranks(labels_p, rows_p), _ranks(labels_t, rows_t)
    both = (rp >= 0) & (rt >= 0)
    pairs = {}
    if both.any():
        uniq, cnt = np.unique(np.stack([rp[both], rt[both]], axis=1), axis=0, return_counts=True)
        pairs = {(int(a), int(b)): int(c) for (a, b), c in zip(uniq.tolist(), cnt.tolist())}
    ap, at = rows_p[:, 1].tolist(), rows_t[:, 1].tolist()
    mp = _side(len(ap), ap, rows_t[:, 0].tolist(), at, pairs, 0)
    mt = _side(len(at), at, rows_p[:, 0].tolist(), ap, pairs, 1)
    num, den = iou
    for a in range(len(ap)):
        b = int(mp[a, 0])
        if b >= 0 and int(mt[b, 0]) == a and int(mp[a, 1]) * den >= num * int(mp[a, 2]):
            mp[a, 3] = 1
            mt[b, 3] = 1
    # the target's side of the flag, derived on its own (the loop above must agree)
    for b in range(len(at)):
        a = int(mt[b, 0])
        want = int(a >= 0 and int(mp[a, 0]) == b and int(mt[b, 1]) * den >= num * int(mt[b, 2]))
        assert want == int(mt[b, 3]), (b, a, want)
    return mp, mt


def match(pre_p, post_p, pre_t, post_t, iou=(1, 2)):
    """dict of one tile from its four maps: table_p, table_t, match_p, match_t, piece_count, labels_p, labels_t"""
    lp, lt = R.label_min_index(np.asarray(pre_p) != 0), R.label_min_index(np.asarray(pre_t) != 0)
    tp, tt = R.table(np.asarray(pre_p) != 0, post_p), R.table(np.asarray(pre_t) != 0, post_t)
    mp, mt = match_tables(lp, tp, lt, tt, iou)
    return {"table_p": tp, "table_t": tt, "match_p": mp, "match_t": mt, "piece_count": piece_count(lp, lt),
            "labels_p": lp, "labels_t": lt}


# ---- the dense brute force: one flood fill per building, an n_p x n_t intersection matrix ----------------------------------
def _flood_masks(mask):
    """boolean masks of the components in raster order of their first pixel"""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    seen = np.zeros((H, W), dtype=bool)
    out = []
    for y in range(H):
        for x in range(W):
            if not mask[y, x] or seen[y, x]:
                continue
            m = np.zeros((H, W), dtype=bool)
            stack = [(y, x)]
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                m[cy, cx] = True
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and mask[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            out.append(m)
    return out


def dense_match(mask_p, mask_t, iou=(1, 2)):
    """(match_p, match_t, piece_count) with nothing shared with match_tables but the contract"""
    P, T = _flood_masks(mask_p), _flood_masks(mask_t)
    inter = [[int((p & t).sum()) for t in T] for p in P]
    area_p, area_t = [int(p.sum()) for p in P], [int(t.sum()) for t in T]

    def best(a, areas_a, areas_b, get, nb):
        k, top = -1, None
        for b in range(nb):                       # raster order of first pixels = ascending root: the first maximum wins
            i = get(a, b)
            if i == 0:
                continue
            u = areas_a[a] + areas_b[b] - i
            if top is None or i * top[1] > top[0] * u:
                k, top = b, (i, u)
        return k, top

    num, den = iou
    mp, mt = np.zeros((len(P), COLS), dtype=np.int64), np.zeros((len(T), COLS), dtype=np.int64)
    bp = [best(a, area_p, area_t, lambda a, b: inter[a][b], len(T)) for a in range(len(P))]
    bt = [best(b, area_t, area_p, lambda b, a: inter[a][b], len(P)) for b in range(len(T))]
    for out, bests, other, areas in ((mp, bp, bt, area_p), (mt, bt, bp, area_t)):
        for a, (k, top) in enumerate(bests):
            if k < 0:
                out[a, :3] = (-1, 0, areas[a])
            else:
                out[a, :3] = (k, top[0], top[1])
                out[a, 3] = int(other[k][0] == a and top[0] * den >= num * top[1])
    for a in range(len(P)):
        mp[a, 4] = sum(1 for b in range(len(T)) if inter[a][b])
    for b in range(len(T)):
        mt[b, 4] = sum(1 for a in range(len(P)) if inter[a][b])
    return mp, mt, len(_flood_masks((np.asarray(mask_p) != 0) & (np.asarray(mask_t) != 0)))


# ---- the score -----------------------------------------------------------------------------------------------------------
def tile_counts(table_p, table_t, match_p, match_t):
    tp = int(sum(1 for m in match_p.tolist() if m[3]))
    conf = [[0] * 5 for _ in range(5)]
    for r, m in enumerate(match_p.tolist()):
        if m[3]:
            conf[int(table_t[m[0], 13])][int(table_p[r, 13])] += 1
    return {"TP": tp, "FP": len(match_p) - tp, "FN": len(match_t) - tp, "confusion": conf,
            "pred_per_class": [int((table_p[:, 13] == c).sum()) for c in range(5)],
            "targ_per_class": [int((table_t[:, 13] == c).sum()) for c in range(5)],
            "merged": int(sum(1 for m in match_p.tolist() if m[4] > 1)),
            "split": int(sum(1 for m in match_t.tolist() if m[4] > 1))}


def _prf(tp, fp, fn):
    p = 0 if tp == 0 else tp / (tp + fp)
    r = 0 if tp == 0 else tp / (tp + fn)
    return p, r, (0 if p == 0 or r == 0 else (2 * p * r) / (p + r))


def score(counts, iou=(1, 2)):
    """the JSON of BuildingMetrics.compute_score from a list of tile_counts dicts"""
    add = lambda k: sum(c[k] for c in counts)
    vec = lambda k: [sum(c[k][i] for c in counts) for i in range(5)]
    conf = [[sum(c["confusion"][i][j] for c in counts) for j in range(5)] for i in range(5)]
    TP, FP, FN = add("TP"), add("FP"), add("FN")
    ppc, tpc = vec("pred_per_class"), vec("targ_per_class")
    p, r, f = _prf(TP, FP, FN)
    d = {"object_localization_precision": p, "object_localization_recall": r, "object_localization_f1": f}
    f1s = []
    for c, key in zip(range(1, 5), ("no_damage", "minor_damage", "major_damage", "destroyed")):
        f1s.append(_prf(conf[c][c], ppc[c] - conf[c][c], tpc[c] - conf[c][c])[2])
        d["object_damage_f1_" + key] = f1s[-1]
    d["object_damage_f1"] = 4 / sum((x + 1e-6) ** -1 for x in f1s)
    d["confusion"] = conf
    d["totals"] = {"TP": TP, "FP": FP, "FN": FN, "pred_per_class": ppc, "targ_per_class": tpc, "merged": add("merged"),
                   "split": add("split"), "predicted": TP + FP, "labelled": TP + FN, "tiles": len(counts)}
    d["iou"] = [int(iou[0]), int(iou[1])]
    return d


# ---- planted cases -----------------------------------------------------------------------------------------------------------
def _rect(shape, *boxes):
    m = np.zeros(shape, dtype=bool)
    for y0, y1, x0, x1 in boxes:              # inclusive
        m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def planted():
    """name -> (mask_p, mask_t, want) with want = dict(match_p, match_t, piece_count), derived by hand (see each comment)"""
    out = {}
    # u_over_bar, 40 x 90: a U (two legs 28 x 1 at x = 5 and x = 80, bottom 1 x 76 at y = 29; area 28 + 28 + 74 = 130) over a
    # horizontal bar y = 10..12, x = 0..89 (area 270).  The legs cross the bar in two 3 x 1 pieces: I = 6, U = 130 + 270 - 6.
    u = _rect((40, 90), (2, 29, 5, 5), (2, 29, 80, 80), (29, 29, 5, 80))
    bar = _rect((40, 90), (10, 12, 0, 89))
    out["u_over_bar"] = (u, bar, {"match_p": [[0, 6, 394, 0, 1, 0, 0, 0]], "match_t": [[0, 6, 394, 0, 1, 0, 0, 0]],
                                  "piece_count": 2})
    # crossing_bars, 70 x 70: predicted rows y = 10..12 and y = 40..42 (x = 5..64, area 180 each) across labelled columns
    # x = 20..22 and x = 50..52 (y = 5..64, area 180 each).  Four 3 x 3 pieces, four pairs, I = 9, U = 351 everywhere: every
    # building has 2 partners at equal IoU and picks the smaller root (row 0 of the other table); 9 / 351 < 1/2: none matched.
    hb = _rect((70, 70), (10, 12, 5, 64), (40, 42, 5, 64))
    vb = _rect((70, 70), (5, 64, 20, 22), (5, 64, 50, 52))
    row = [0, 9, 351, 0, 2, 0, 0, 0]
    out["crossing_bars"] = (hb, vb, {"match_p": [row, row], "match_t": [row, row], "piece_count": 4})
    # one_sided, 8 x 12.  Row 1: predicted 1 x 4 at x = 1..4 over a labelled 1 x 2 at x = 1..2: I = 2, U = 4, exactly 1/2 and
    # mutual: matched at 1/2 (pins >=).  A second labelled 1 x 2 at x = 4..5 shares one pixel with the same prediction:
    # I = 1, U = 4 + 2 - 1 = 5; its only (so best) partner is the prediction, whose best is the first label: not mutual.
    # Row 5: two 1 x 2 rectangles sharing one pixel, predicted x = 1..2, labelled x = 2..3: I = 1, U = 3, mutual, below 1/2.
    p1 = _rect((8, 12), (1, 1, 1, 4), (5, 5, 1, 2))
    t1 = _rect((8, 12), (1, 1, 1, 2), (1, 1, 4, 5), (5, 5, 2, 3))
    out["one_sided"] = (p1, t1, {"match_p": [[0, 2, 4, 1, 2, 0, 0, 0], [2, 1, 3, 0, 1, 0, 0, 0]],
                                 "match_t": [[0, 2, 4, 1, 1, 0, 0, 0], [0, 1, 5, 0, 1, 0, 0, 0], [1, 1, 3, 0, 1, 0, 0, 0]],
                                 "piece_count": 3})
    # disjoint, 20 x 30: a predicted 3 x 4 block (area 12) and a labelled 2 x 5 block (area 10) that share no pixel
    out["disjoint"] = (_rect((20, 30), (2, 4, 3, 6)), _rect((20, 30), (10, 11, 20, 24)),
                       {"match_p": [[-1, 0, 12, 0, 0, 0, 0, 0]], "match_t": [[-1, 0, 10, 0, 0, 0, 0, 0]], "piece_count": 0})
    # the three empty combinations (a 2 x 3 block of area 6 on the side that has one)
    blk, none = _rect((9, 70), (3, 4, 60, 62)), np.zeros((9, 70), dtype=bool)
    lone = [[-1, 0, 6, 0, 0, 0, 0, 0]]
    out["empty_p"] = (none, blk, {"match_p": [], "match_t": lone, "piece_count": 0})
    out["empty_t"] = (blk, none, {"match_p": lone, "match_t": [], "piece_count": 0})
    out["empty_both"] = (none, none, {"match_p": [], "match_t": [], "piece_count": 0})
    for k, (a, b, w) in out.items():
        w["match_p"] = np.array(w["match_p"], dtype=np.int64).reshape(-1, COLS)
        w["match_t"] = np.array(w["match_t"], dtype=np.int64).reshape(-1, COLS)
    return out


def two_halves():
    """(mask_labels, mask_rows, mask_other, want): the one input on which the mutual-best condition of column 3 decides.
    With tables that are the labels' own it cannot: two partners b1, b2 of a that both reach 1/2 have I1, I2 >= |a| / 2
    and I1 + I2 <= |a|, so both are exactly half of a, lie inside it and tile it; then some pixel of b1 is 4-adjacent to
    one of b2 (a is connected), and they would be ONE component.  So the case takes a table from another map: the labels of
    a 1 x 5 building (x = 1..5) with the row of a 1 x 4 one at the same root (x = 1..4, area 4), over two 1 x 2 buildings
    at x = 1..2 and x = 4..5.  Both pairs have I = 2 and U = 4 + 2 - 2 = 4, exactly 1/2.  The long building's tie goes to the
    smaller root, short building 0, and that pair is mutual and matched.  Short building 1 passes 1/2 too and its only, so
    best, partner is the long building, whose best partner is short building 0: it stays unmatched.  want: the rows of the
    long side and of the short side, and the piece count."""
    labels_of, rows_of = _rect((6, 10), (2, 2, 1, 5)), _rect((6, 10), (2, 2, 1, 4))
    short = _rect((6, 10), (2, 2, 1, 2), (2, 2, 4, 5))
    want = {"long": np.array([[0, 2, 4, 1, 2, 0, 0, 0]], dtype=np.int64),
            "short": np.array([[0, 2, 4, 1, 1, 0, 0, 0], [0, 2, 4, 0, 1, 0, 0, 0]], dtype=np.int64), "piece_count": 2}
    return labels_of, rows_of, short, want


def checker(H, W):
    return np.add.outer(np.arange(H), np.arange(W)) % 2 == 0


def town(seed, H, W, cell=56, jitter=0):
    """rectangular 'buildings', one per cell x cell block of the tile, origin and size hashed from seed; some reach into the
    next block and fuse with its building.  jitter != 0: every origin and size moved by -3..3 pixels and one building in
    eight left out, hashed from jitter (a prediction of the map with jitter 0)"""
    ny, nx = H // cell, W // cell
    g = R._hash(seed, (ny, nx, 4), 1 << 16)
    j = R._hash(jitter, (ny, nx, 4), 7) - 3 if jitter else np.zeros((ny, nx, 4), dtype=np.int64)
    keep = R._hash(jitter + 1, (ny, nx), 8) != 0 if jitter else np.ones((ny, nx), dtype=bool)
    m = np.zeros((H, W), dtype=bool)
    for iy in range(ny):
        for ix in range(nx):
            if not keep[iy, ix]:
                continue
            y0 = iy * cell + g[iy, ix, 0] % (cell // 3) + j[iy, ix, 0]
            x0 = ix * cell + g[iy, ix, 1] % (cell // 3) + j[iy, ix, 1]
            h = 10 + g[iy, ix, 2] % (cell - 14) + j[iy, ix, 2]
            w = 10 + g[iy, ix, 3] % (cell - 14) + j[iy, ix, 3]
            m[max(y0, 0):max(y0 + h, 0), max(x0, 0):max(x0 + w, 0)] = True
    return m
