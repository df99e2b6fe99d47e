"""Host restatement of the rule of include/xv2.h, "clean buildings" (csrc/clean.hip, xview2_amd/utils/clean.py): plain numpy
and Python, flood fill with explicit neighbour lists, no scipy.  Everything is an integer, so the tests compare with ==."""
import numpy as np

N4 = ((0, -1), (-1, 0), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def components(mask, neighbours):
    """mask bool [H,W] -> (labels int64 [H,W], list of components); label k + 1 marks the pixels of components[k], a list of
    (y, x).  Components are numbered by their first pixel in raster order, which is also the first entry of each list."""
    H, W = mask.shape
    m = np.asarray(mask, dtype=bool).tolist()          # (Python lists: the loops below index single pixels)
    labels = [[0] * W for _ in range(H)]
    comps = []
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0][x0] or labels[y0][x0]:
                continue
            k = len(comps) + 1
            labels[y0][x0] = k
            stack, px = [(y0, x0)], [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in neighbours:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and m[v][u] and not labels[v][u]:
                        labels[v][u] = k
                        stack.append((v, u))
                        px.append((v, u))
            comps.append(px)
    return np.array(labels, dtype=np.int64).reshape(H, W), comps


_memo = {}


def _unfilled(pre):
    """(labels, components) of the buildings and the holes of an input map, kept per map: the tests run many (min_area,
    max_hole) pairs on the same tiles"""
    key = (pre.shape, pre.tobytes())
    if key not in _memo:
        H, W = pre.shape
        _, comps = components(pre == 0, N8)
        found = [c for c in comps if not any(y == 0 or x == 0 or y == H - 1 or x == W - 1 for y, x in c)]
        _memo[key] = components(pre != 0, N4) + (found,)
    return _memo[key]


def holes(pre):
    """the holes of pre != 0: 8-connected background components without a pixel on the outer frame, as lists of (y, x),
    in raster order of their first pixels"""
    return _unfilled(np.ascontiguousarray(pre, dtype=np.uint8))[2]


def vote(classes):
    """the class 1..4 with the most entries, ties to the smaller class, 0 without any entry in 1..4"""
    best, n = 0, 0
    for c in (1, 2, 3, 4):
        k = int(np.count_nonzero(classes == c))
        if k > n:
            best, n = c, k
    return best


def clean(pre, post, min_area, max_hole):
    """pre uint8 [H,W], post uint8 [H,W] or None -> (pre', post' or None, stats int64 [4]: holes filled, pixels filled,
    buildings dropped, pixels dropped)"""
    pre = np.ascontiguousarray(pre, dtype=np.uint8)
    if min_area < 0 or max_hole < 0:
        raise ValueError("min_area and max_hole must not be negative")
    out = pre.copy()
    pout = None if post is None else np.asarray(post, dtype=np.uint8).copy()
    stats = np.zeros(4, dtype=np.int64)
    # stage 1: fill, every decision taken on the unfilled maps
    flab, fcomps, found = _unfilled(pre)
    votes = {}
    for hole in found:
        if not 1 <= len(hole) <= max_hole:
            continue
        y, x = min(hole)                       # the first pixel in raster order
        assert pre[y, x - 1] != 0
        owner = int(flab[y, x - 1])
        if owner not in votes:                  # (many holes share one owner)
            votes[owner] = 0 if post is None else vote(np.asarray(post)[flab == owner])
        cls = votes[owner]
        for v, u in hole:
            out[v, u] = 1
            if pout is not None:
                pout[v, u] = cls
        stats[0] += 1
        stats[1] += len(hole)
    # stage 2: drop, on the filled map
    comps = components(out != 0, N4)[1] if stats[0] else fcomps
    for comp in comps:
        if len(comp) < min_area:
            for v, u in comp:
                out[v, u] = 0
                if pout is not None:
                    pout[v, u] = 0
            stats[2] += 1
            stats[3] += len(comp)
    return out, pout, stats


def random_pair(seed, H, W, density):
    """a random uint8 mask with the given share of building pixels (values 1 and, rarely, 7) and a post map with every value
    0..6 on it, from a fixed generator"""
    rng = np.random.RandomState(seed)
    pre = (rng.rand(H, W) < density).astype(np.uint8)
    pre[(rng.rand(H, W) < 0.05) & (pre != 0)] = 7
    post = rng.randint(0, 7, size=(H, W)).astype(np.uint8)
    return pre, post
