"""Host restatement of the splitting rule (include/xv2.h, "split touching buildings"), written from the rule: a
brute-force capped squared distance, seeds by threshold, growth in synchronous rounds, the cut; a second, closed-form
growth from per-seed breadth-first distances (small tiles) that checks the rounds; and the masks the tests share.
Every value is an integer, so every comparison is ==."""
import numpy as np

from buildings_ref import blobs, label_min_index

BIG = np.int64(1) << 40


def cap_of(r2):
    """floor(sqrt(r2)) + 1 in integers"""
    s = 0
    while (s + 1) * (s + 1) <= r2:
        s += 1
    return s + 1


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that is outside the tile"""
    H, W = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        b[yd, xd] = a[ys, xs]
    return b


def edt_sq(mask, cap):
    """int64 [H,W]: min(cap^2, the squared distance to the nearest pixel of the tile with mask == 0); every offset below cap
    is tried on its own, pixels outside the tile are no background"""
    zero = np.asarray(mask) == 0
    d2 = np.full(zero.shape, cap * cap, dtype=np.int64)
    for dy in range(-(cap - 1), cap):
        for dx in range(-(cap - 1), cap):
            if dy * dy + dx * dx < cap * cap:
                near = _shift(zero, dy, dx, False)
                d2[near] = np.minimum(d2[near], dy * dy + dx * dx)
    return d2


def seeds(mask, r2):
    """(bool S, int32 seed labels): S = M & (d2 > r2), labels 1 + the smallest linear index of the seed's component"""
    M = np.asarray(mask) != 0
    S = M & (edt_sq(M, cap_of(r2)) > r2)
    return S, label_min_index(S)


def grow_rounds(mask, seed_labels):
    """(L int64 [H,W], rounds): every unlabelled pixel of M with a labelled 4-neighbour takes the smallest label among those
    neighbours, all at once, until a round changes nothing; rounds counts the rounds that changed something"""
    M = np.asarray(mask) != 0
    L = np.asarray(seed_labels).astype(np.int64).copy()
    rounds = 0
    while True:
        cand = np.where(L > 0, L, BIG)
        best = np.minimum(np.minimum(_shift(cand, 1, 0, BIG), _shift(cand, -1, 0, BIG)),
                          np.minimum(_shift(cand, 0, 1, BIG), _shift(cand, 0, -1, BIG)))
        take = M & (L == 0) & (best < BIG)
        if not take.any():
            return L, rounds
        L[take] = best[take]
        rounds += 1


def grow_closed_form(mask, seed_labels):
    """L from the definition: per seed label l a breadth-first geodesic distance g_l inside M, g = min over l,
    L = min{l : g_l = g}; 0 where no seed reaches (small tiles only)"""
    M = np.asarray(mask) != 0
    H, W = M.shape
    lab = np.asarray(seed_labels).astype(np.int64)
    best_g = np.full((H, W), BIG, dtype=np.int64)
    best_l = np.zeros((H, W), dtype=np.int64)
    for l in np.unique(lab[lab > 0]).tolist():       # ascending: a later label must be strictly nearer to win
        g = np.full((H, W), BIG, dtype=np.int64)
        front = [(int(y), int(x)) for y, x in zip(*np.nonzero(lab == l))]
        for y, x in front:
            g[y, x] = 0
        while front:
            nxt = []
            for y, x in front:
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < H and 0 <= nx < W and M[ny, nx] and g[ny, nx] == BIG:
                        g[ny, nx] = g[y, x] + 1
                        nxt.append((ny, nx))
            front = nxt
        win = g < best_g
        best_g[win] = g[win]
        best_l[win] = l
    return best_l


def cut(L):
    """bool [H,W]: L(p) > 0 and some 4-neighbour q with 0 < L(q) < L(p)"""
    L = np.asarray(L).astype(np.int64)
    cand = np.where(L > 0, L, BIG)
    low = np.minimum(np.minimum(_shift(cand, 1, 0, BIG), _shift(cand, -1, 0, BIG)),
                     np.minimum(_shift(cand, 0, 1, BIG), _shift(cand, 0, -1, BIG)))
    return (L > 0) & (low < L)


def split(mask, r2):
    """(out uint8 [H,W] with the mask's own values kept, L int32 [H,W], rounds) of one tile"""
    mask = np.asarray(mask)
    _, lab = seeds(mask, r2)
    L, rounds = grow_rounds(mask, lab)
    out = np.where(cut(L), 0, mask.astype(np.uint8)).astype(np.uint8)
    return out, L.astype(np.int32), rounds


# ---- masks -------------------------------------------------------------------------------------------------------------
def dumbbell(n, neck_len=7, body=14, margin=3):
    """two body x body squares joined by a straight horizontal neck n pixels wide, `margin` pixels of background around
    (uint8 0 / 1).  Returns (mask, first neck column, first neck row)."""
    H, W = body + 2 * margin, 2 * body + neck_len + 2 * margin
    m = np.zeros((H, W), dtype=np.uint8)
    m[margin:margin + body, margin:margin + body] = 1
    m[margin:margin + body, margin + body + neck_len:margin + 2 * body + neck_len] = 1
    top = margin + (body - n) // 2
    m[top:top + n, margin + body:margin + body + neck_len] = 1
    return m, margin + body, top


def serpentine(H=131, W=131, body=12):
    """a wide body in the top left corner feeding a 1-pixel corridor that runs left and right across the whole map, two rows
    further down each time, into a second body in the bottom corner where it ends (uint8 0 / 1)"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0:body, 0:body] = 1
    y, right = body + 1, True
    m[body:y + 1, 1] = 1                                   # down from the body
    last = H - body - 2
    while y <= last:
        m[y, 1:W - 1] = 1
        if y + 2 <= last:
            m[y:y + 3, W - 2 if right else 1] = 1
        y, right = y + 2, not right
    y -= 2
    x = W - 2 if not right else 1                          # the end the last run stopped at
    m[y:H - body + 1, x] = 1
    if x == 1:
        m[H - body:H, 0:body] = 1
    else:
        m[H - body:H, W - body:W] = 1
    return m


def blob_mask(seed, H, W, values=False):
    """random blobs (buildings_ref.blobs with a wide box, so that bodies survive an erosion) as uint8: 0 / 1, or with
    `values` 0 and the values 1..255 in patches"""
    m = blobs(seed, H, W, thresh=0.5, box=9).astype(np.uint8)
    if values:
        yy, xx = np.mgrid[0:H, 0:W]
        m = m * (1 + ((yy // 5) * 7 + (xx // 3) * 13 + seed) % 255).astype(np.uint8)
    return m
