"""The registration rule's host restatement (tests/align_ref.py) against a brute force and against its own definition, the
report, the command lines, and what of the ABI needs no GPU."""
import ctypes

import numpy as np
import pytest

import align_ref as A

PLANTED = [(37, 41, 3, (2, -3)), (70, 67, 5, (-5, 5)), (131, 203, 16, (7, -16)), (200, 197, 32, (-32, 31)), (3, 3, 1, (0, 0))]


def _noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_luma_range_and_weights():
    assert A.luma(np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)).tolist() == [
        0, 255, (29 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (77 * 255 + 128) >> 8]


def test_restatement_against_a_triple_loop():
    H, W, R, T = 9, 11, 2, 32
    pre, post = _noise(1, H, W), _noise(2, H, W)
    yp, yq = A.luma(pre), A.luma(post)
    want = np.zeros((5, 5), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            for y in range(R, H - R):
                for x in range(R, W - R):
                    want[dy + R, dx + R] += abs(int(yp[y, x]) - int(yq[y + dy, x + dx]))
    bs, sad, bshift, shift = A.estimate(pre, post, R, T)
    assert bs.shape == (1, 1, 5, 5) and np.array_equal(bs[0, 0], want) and np.array_equal(sad, want)
    flat = [(int(want[dy + R, dx + R]), dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    assert tuple(shift) == min(flat)[2:] == tuple(bshift[0, 0])


@pytest.mark.parametrize("H,W,R,d", PLANTED)
def test_planted_shift_is_found_with_zero_residual(H, W, R, d):
    pre, post = A.planted(H + W, H, W, d)
    sad = A.block_sad(pre, post, R, 128).sum(axis=(0, 1))
    assert sad[d[0] + R, d[1] + R] == 0 and A.best(sad) == d


def test_constant_image_gives_no_shift():
    img = np.full((20, 23, 3), 77, np.uint8)
    bs, sad, bshift, shift = A.estimate(img, img, 4, 32)
    assert tuple(shift) == (0, 0) and not sad.any() and not bshift.any()
    assert A.best(np.full((9, 9), 5, np.int64)) == (0, 0)


def test_tile_tables_sum_to_the_global_one():
    H, W, R = 70, 67, 5
    pre, post = _noise(3, H, W), _noise(4, H, W)
    one = A.block_sad(pre, post, R, 128)
    for T in (32, 64):
        bs = A.block_sad(pre, post, R, T)
        assert bs.shape[:2] == A.grid(H, W, R, T) and np.array_equal(bs.sum(axis=(0, 1)), one[0, 0])
    bs = A.block_sad(pre, post, R, 32)
    yp, yq = A.luma(pre), A.luma(post)
    # tile (1, 1) at shift (-2, 3): rows R + 32 ... R + 59 (partial), columns R + 32 ... R + 56 (partial)
    want = np.abs(yp[R + 32:H - R, R + 32:W - R] - yq[R + 30:H - R - 2, R + 35:W - R + 3]).sum()
    assert bs[1, 1, R - 2, R + 3] == want


def test_tie_rule():
    t = np.full((3, 3), 9, np.int64)
    t[1, 2] = t[2, 1] = t[1, 0] = t[0, 1] = 4          # (0, 1), (1, 0), (0, -1), (-1, 0)
    assert A.best(t) == (-1, 0)
    t = np.full((3, 3), 9, np.int64)
    t[2, 2] = t[1, 2] = 4                               # (1, 1), (0, 1)
    assert A.best(t) == (0, 1)
    t = np.full((5, 5), 9, np.int64)
    t[2, 2] = 5
    t[0, 0] = 4                                         # a smaller sum beats a shorter shift
    assert A.best(t) == (-2, -2)


def test_translate_against_numpy_reflect():
    src = _noise(5, 13, 17)
    for dy, dx in ((0, 0), (3, 5), (-3, 5), (4, -6), (-12, -16), (12, 16)):
        pad = np.pad(src, ((12, 12), (16, 16), (0, 0)), mode="reflect")
        want = pad[12 + dy:12 + dy + 13, 16 + dx:16 + dx + 17]
        assert np.array_equal(A.translate(src, dy, dx), want), (dy, dx)
    small = _noise(6, 3, 4)
    pad = np.pad(small, ((32, 32), (0, 0), (0, 0)), mode="reflect")       # numpy iterates the reflection
    assert np.array_equal(A.translate(small, 32, 0), pad[64:67])
    assert np.array_equal(A.translate(small, -32, 0), pad[0:3])
    assert np.array_equal(A.translate(small[:1], 7, -2)[0], A.translate(small[:1], 0, -2)[0])   # tri(i, 1) = 0
    from xview2_amd import scene
    i = np.arange(0, 40)
    for L in (1, 2, 3, 7):
        assert np.array_equal(A.tri(i, L), scene.tri(i, L))


# ---- the report ----------------------------------------------------------------------------------------------------------
def test_summarise_on_a_hand_made_table():
    from xview2_amd.utils import align
    R, T, H, W = 1, 32, 36, 66                       # interior 34 x 64: a 2 x 2 grid of tiles
    bs = np.zeros((2, 2, 3, 3), np.int64)
    bs[0, 0] = [[9, 9, 9], [9, 5, 1], [9, 9, 9]]     # best (0, 1)
    bs[0, 1] = [[9, 9, 9], [9, 6, 2], [9, 9, 9]]     # best (0, 1)
    bs[1, 0] = 7                                     # flat: (0, 0), not counted in the spread
    bs[1, 1] = [[3, 9, 9], [9, 8, 9], [9, 9, 9]]     # best (-1, -1)
    sad = bs.sum(axis=(0, 1))
    bshift = np.array([[A.best(bs[y, x]) for x in range(2)] for y in range(2)])
    shift = np.array(A.best(sad))
    assert tuple(shift) == (0, 1)
    rep = align.summarise(bs, sad, bshift, shift, R, T, H, W)
    assert rep == {
        "radius": 1, "tile": 32, "shift": [0, 1], "pixels": 34 * 64, "sad_zero": 26, "sad_best": 19,
        "mean_abs_zero": "0.011949", "mean_abs_zero_exact": "26/2176", "mean_abs_best": "0.008732",
        "mean_abs_best_exact": "19/2176", "at_limit": True,
        "blocks": {"grid": [2, 2], "shifts": [[[0, 1], [0, 1]], [[0, 0], [-1, -1]]], "flat": 1, "agree": 2, "spread": 2}}
    text = align.dumps(rep)
    assert text == align.dumps(align.summarise(bs, sad, bshift, shift, R, T, H, W)) and text.endswith("\n")
    import json
    assert json.loads(text) == rep
    inner = align.summarise(np.zeros((1, 1, 5, 5)), np.zeros((5, 5)), np.zeros((1, 1, 2)), np.zeros(2), 2, 32, 9, 11)
    assert inner["at_limit"] is False and inner["blocks"] == {"grid": [1, 1], "shifts": [[[0, 0]]], "flat": 1, "agree": 1, "spread": 0}
    with pytest.raises(ValueError):
        align.summarise(bs, sad, bshift, shift, R, T, H, W + 64)
    assert align.histogram([{"shift": [0, 1]}, {"shift": [-1, 2]}, {"shift": [0, 1]}]) == [[-1, 2, 1], [0, 1, 2]]


# ---- command lines -------------------------------------------------------------------------------------------------------
def test_command_lines():
    from xview2_amd import predict
    from xview2_amd.utils import align
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o"])
    assert a.align == 0 and a.align_tile == 128
    assert predict.get_parser().parse_args(["--pre", "p", "--post", "q", "--out", "o", "--align", "3"]).align == 3
    with pytest.raises(ValueError, match="--align needs --post"):
        predict.main(["--pre", "p", "--out", "o", "--ckpt_loc", "c", "--align", "3"])
    with pytest.raises(ValueError, match="1..32"):
        predict.main(["--pre", "p", "--post", "q", "--out", "o", "--ckpt_loc", "c", "--align", "33"])
    assert "may be larger than the search" in " ".join(predict.get_parser().format_help().split())
    a = align.get_parser().parse_args(["a.png", "b.png", "c.png"])
    assert (a.pre, a.post, a.out, a.tile, a.json) == ("a.png", "b.png", "c.png", 128, None) and 1 <= a.radius <= 32
    a = align.get_parser().parse_args(["A", "B", "C", "--radius", "16", "--tile", "64", "--json", "r.json"])
    assert (a.radius, a.tile, a.json) == (16, 64, "r.json")
    with pytest.raises(SystemExit):
        align.get_parser().parse_args(["A", "B", "C", "--tile", "48"])
    for bad in (0, -1, 33):
        with pytest.raises(ValueError):
            align.check_radius(bad)
    assert align.check_radius(32) == 32 and align.check_radius(1) == 1
    assert "may be a larger true offset" in " ".join(align.get_parser().format_help().split())
    import inspect
    from xview2_amd import scene
    assert inspect.signature(scene.align_pair).parameters["tile"].default == 128


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    assert protos["xv2_align_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert protos["xv2_align_estimate"] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 6)
    assert protos["xv2_translate_u8"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3)
    assert "align.hip" in _lib.SOURCES


def test_workspace_query():
    from xview2_amd import _capi, _lib
    _lib.build()
    q = lambda *a: _capi.query("xv2_align_workspace", *a)
    assert q(1, 3, 3, 1, 32) >= 8 * 9 and q(1, 3, 3, 1, 32) % 256 == 0
    # 4096^2 at R = 16, T = 128: 32 x 32 tiles in 32 chunks of 32
    assert q(1, 4096, 4096, 16, 128) >= 8 * 32 * 33 * 33
    assert q(2, 70, 67, 5, 32) >= 2 * 8 * 121 and q(65535, 3, 3, 1, 64) > 0 and q(1, 65, 65, 32, 128) > 0
    for bad in ((0, 9, 9, 1, 32), (65536, 9, 9, 1, 32), (1, 9, 9, 0, 32), (1, 99, 99, 33, 32), (1, 9, 9, 1, 48), (1, 9, 9, 1, 0),
                (1, 2, 9, 1, 32), (1, 9, 2, 1, 32), (1, 64, 99, 32, 32), (1, 99, 64, 32, 32), (1, 1 << 15, 1 << 15, 1, 128),
                (1, -5, 9, 1, 32)):
        assert q(*bad) == 0, bad


def test_every_argument_check_is_reachable_without_a_gpu():
    from xview2_amd import _capi, _lib
    _lib.build()
    one = ctypes.c_void_p(256)
    err = lambda: _lib.lib().xv2_last_error()

    def run(name, order, kw, msg):
        a = dict(pre=one, post=one, src=one, B=1, H=9, W=9, R=2, T=32, C=3, ws=one, block_sad=one, sad=one, block_shift=one,
                 shift=one, out=ctypes.c_void_p(4096), stream=None)
        a.update(kw)
        assert _capi._func(name)(*[a[k] for k in order]) == 1 and msg in err(), (name, kw, err())

    est = ("pre", "post", "B", "H", "W", "R", "T", "ws", "block_sad", "sad", "block_shift", "shift", "stream")
    odd = ctypes.c_void_p(258)
    for kw, msg in [(dict(B=0), b"positive"), (dict(H=0), b"positive"), (dict(W=-1), b"positive"), (dict(R=0), b"radius"),
                    (dict(R=33, H=99, W=99), b"radius"), (dict(T=48), b"tile"), (dict(T=0), b"tile"), (dict(H=4), b"interior"),
                    (dict(W=4), b"interior"), (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"),
                    (dict(pre=None), b"null"), (dict(post=None), b"null"), (dict(block_sad=None), b"null"),
                    (dict(sad=None), b"null"), (dict(block_shift=None), b"null"), (dict(shift=None), b"null"),
                    (dict(ws=None), b"workspace"), (dict(ws=ctypes.c_void_p(264)), b"16-byte"), (dict(block_sad=odd), b"aligned"),
                    (dict(sad=ctypes.c_void_p(260)), b"aligned"), (dict(block_shift=odd), b"aligned"), (dict(shift=odd), b"aligned")]:
        run("xv2_align_estimate", est, kw, msg)
    tr = ("src", "B", "H", "W", "C", "shift", "out", "stream")
    for kw, msg in [(dict(B=0), b"positive"), (dict(H=-2), b"positive"), (dict(W=0), b"positive"), (dict(C=0), b"channels"),
                    (dict(C=9), b"channels"), (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"),
                    (dict(src=None), b"null"), (dict(shift=None), b"null"), (dict(out=None), b"null"), (dict(shift=odd), b"aligned"),
                    (dict(out=one), b"overlap"), (dict(out=ctypes.c_void_p(256 + 242)), b"overlap"),
                    (dict(src=ctypes.c_void_p(4096 + 242)), b"overlap")]:
        run("xv2_translate_u8", tr, kw, msg)
