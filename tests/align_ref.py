"""Host restatement of the registration rule (include/xv2.h, "register the post image to the pre image"), in int64 numpy,
straight from the definitions: luma, the tables of sums of absolute differences, the best shift of a table, and the
reflecting resampler.  What the kernels of csrc/align.hip are compared with, by ==."""
import numpy as np


def luma(img):
    """uint8 [..., 3] in stored channel order -> int64 [...] in 0..255"""
    c = np.asarray(img).astype(np.int64)
    return (29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2] + 128) >> 8


def grid(H, W, R, T):
    """(nby, nbx)"""
    return -(-(H - 2 * R) // T), -(-(W - 2 * R) // T)


def block_sad(pre, post, R, T):
    """pre, post uint8 [H, W, 3] -> int64 [nby, nbx, D, D], indexed [by, bx, dy + R, dx + R]"""
    yp, yq = luma(pre), luma(post)
    H, W = yp.shape
    assert H > 2 * R and W > 2 * R
    nby, nbx = grid(H, W, R, T)
    D = 2 * R + 1
    out = np.zeros((nby, nbx, D, D), dtype=np.int64)
    inner = yp[R:H - R, R:W - R]
    ys, xs = np.arange(0, H - 2 * R, T), np.arange(0, W - 2 * R, T)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            a = np.abs(inner - yq[R + dy:H - R + dy, R + dx:W - R + dx])
            out[:, :, dy + R, dx + R] = np.add.reduceat(np.add.reduceat(a, ys, axis=0), xs, axis=1)
    return out


def best(table):
    """int64 [D, D] -> (dy, dx): the smallest S, then the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx"""
    table = np.asarray(table)
    D = table.shape[0]
    R = D // 2
    cands = [(int(table[dy + R, dx + R]), dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    return min(cands)[2:]


def estimate(pre, post, R, T):
    """one image pair -> (block_sad [nby,nbx,D,D], sad [D,D], block_shift [nby,nbx,2], shift [2]), all int64"""
    bs = block_sad(pre, post, R, T)
    sad = bs.sum(axis=(0, 1))
    nby, nbx = bs.shape[:2]
    bshift = np.array([[best(bs[y, x]) for x in range(nbx)] for y in range(nby)], dtype=np.int64).reshape(nby, nbx, 2)
    return bs, sad, bshift, np.array(best(sad), dtype=np.int64)


def tri(i, L):
    """reflection without repeating the edge for any integer index (floor modulo)"""
    i = np.asarray(i, dtype=np.int64)
    if L == 1:
        return np.zeros_like(i)
    p = 2 * (L - 1)
    m = np.mod(i, p)
    return np.where(m < L, m, p - m)


def translate(src, dy, dx):
    """src [H, W, ...] -> out[y][x] = src[tri(y + dy, H)][tri(x + dx, W)]"""
    src = np.asarray(src)
    H, W = src.shape[:2]
    return src[tri(np.arange(H) + int(dy), H)][:, tri(np.arange(W) + int(dx), W)]


def planted(seed, H, W, d):
    """uniform noise pre and post = np.roll(pre, d, (0, 1)): S(d) == 0 on the interior"""
    pre = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return pre, np.roll(pre, d, (0, 1))
