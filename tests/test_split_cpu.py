"""The splitting rule's host restatement (tests/split_ref.py) against scipy and against its own definition, the
consequences include/xv2.h lists, the command lines, and what of the ABI needs no GPU."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import split_ref as S
from buildings_ref import FOUR, label_min_index

R2S = (1, 2, 4, 5, 8, 9)


def _blob_cases():
    return [S.blob_mask(seed, H, W) for seed, H, W in ((1, 40, 52), (2, 37, 41), (3, 64, 30), (4, 33, 33), (5, 50, 45))]


# ---- distance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 2, 3, 8])
def test_distance_against_scipy_on_the_mask_padded_with_ones(cap):
    masks = [S.blob_mask(seed, 45, 38) for seed in range(4)] + [np.ones((9, 7), np.uint8), np.zeros((5, 6), np.uint8)]
    corner = np.ones((12, 10), np.uint8)
    corner[0, 0] = 0
    for m in masks + [corner]:
        edt = ndimage.distance_transform_edt(np.pad(m, cap, constant_values=1))[cap:-cap, cap:-cap]
        want = np.minimum(np.rint(edt ** 2).astype(np.int64), cap * cap)
        assert np.array_equal(S.edt_sq(m, cap), want)
    assert np.all(S.edt_sq(np.ones((9, 7), np.uint8), cap) == cap * cap)       # the tile edge is no background


def test_cap():
    assert [S.cap_of(r2) for r2 in (1, 2, 3, 4, 8, 9, 15, 16, 4095)] == [2, 2, 2, 3, 3, 4, 4, 5, 64]


# ---- growth: the rounds are the closed form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", [1, 2, 4, 9])
def test_rounds_equal_the_closed_form(r2):
    for m in _blob_cases()[:3] + [S.dumbbell(3)[0], S.dumbbell(4, neck_len=6)[0]]:
        _, lab = S.seeds(m, r2)
        L, _ = S.grow_rounds(m, lab)
        assert np.array_equal(L, S.grow_closed_form(m, lab))


def test_label_tie_goes_to_the_smaller_label():
    m = np.ones((1, 7), np.uint8)
    lab = np.zeros((1, 7), np.int32)
    lab[0, 0], lab[0, 6] = 1, 7
    L, rounds = S.grow_rounds(m, lab)
    assert L.tolist() == [[1, 1, 1, 1, 7, 7, 7]] and rounds == 3
    assert S.cut(L).tolist() == [[False] * 4 + [True] + [False] * 2]
    assert np.array_equal(L, S.grow_closed_form(m, lab))


# ---- the five consequences ---------------------------------------------------------------------------------------------------
def _check_consequences(m, r2):
    out, L, _ = S.split(m, r2)
    M = m != 0
    assert np.all((out == m) | (out == 0)) and np.all(out <= m)                                  # out <= mask
    comp_m = label_min_index(M)
    comp_o, n = ndimage.label(out != 0, structure=FOUR)
    for c in range(1, n + 1):                             # a piece lies in one component of mask and carries one L
        sel = comp_o == c
        assert len(np.unique(comp_m[sel])) == 1 and len(np.unique(L[sel])) == 1
    O = np.where(out != 0, L, 0).astype(np.int64)
    for a, b in ((O[1:], O[:-1]), (O[:, 1:], O[:, :-1])):                                        # no two labels adjacent in out
        assert not np.any((a > 0) & (b > 0) & (a != b))
    _, seed_lab = S.seeds(m, r2)
    for c in np.unique(comp_m[M]).tolist():                                                       # at most one seed: untouched
        sel = comp_m == c
        if len(np.unique(seed_lab[sel & (seed_lab > 0)])) <= 1:
            assert np.array_equal(out[sel], m[sel])
    assert np.all(L[~M] == 0) and np.all((L > 0) | (seed_lab == 0))
    return out


@pytest.mark.parametrize("r2", R2S)
def test_consequences_on_blobs(r2):
    cut = 0
    for m in _blob_cases():
        cut += int((_check_consequences(m, r2) != m).sum())
    assert cut > 0
    _check_consequences(S.blob_mask(7, 40, 40, values=True), r2)


@pytest.mark.parametrize("n", range(1, 7))
@pytest.mark.parametrize("r2", R2S)
def test_dumbbell_neck_is_cut_iff_half_its_width_fits_the_radius(n, r2):
    for neck_len in (6, 7):
        m, col, top = S.dumbbell(n, neck_len)
        out = _check_consequences(m, r2)
        want = m.copy()
        if ((n + 1) // 2) ** 2 <= r2:
            want[top:top + n, col + (neck_len + 1) // 2] = 0      # the first neck column nearer to the right body
        assert np.array_equal(out, want)


def test_thin_and_small_buildings_stay():
    m = np.zeros((20, 30), np.uint8)
    m[2, 1:29] = 1
    m[5:8, 3:6] = 3
    m[10:12, 10:28] = 1
    out, L, rounds = S.split(m, 4)
    assert np.array_equal(out, m) and not L.any() and rounds == 0


def test_serpentine_needs_more_than_a_thousand_rounds():
    m = S.serpentine()
    assert m.shape == (131, 131)
    assert ndimage.label(m, structure=FOUR)[1] == 1
    out, L, rounds = S.split(m, 4)
    assert rounds > 1000 and len(np.unique(L)) == 3 and int((out != m).sum()) == 1


# ---- command lines -----------------------------------------------------------------------------------------------------------
def test_the_three_command_lines_take_split_and_default_to_off():
    from xview2_amd import predict
    from xview2_amd.utils import building_metrics, post_process, split
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o"]).split == 0
    assert predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--split", "3"]).split == 3
    assert post_process.get_parser().parse_args([]).split == 0
    assert post_process.get_parser().parse_args(["--split", "2", "--components"]).split == 2
    a = building_metrics.get_parser().parse_args(["P", "T", "o.json"])
    assert a.split == 0 and a.split_targets == 0
    a = building_metrics.get_parser().parse_args(["P", "T", "o.json", "--split", "2", "--split_targets", "3"])
    assert a.split == 2 and a.split_targets == 3
    a = split.get_parser().parse_args(["a.png", "b.png", "c.png", "d.png", "--radius", "2"])
    assert a.radius == 2 and (a.pre, a.post, a.out_pre, a.out_post) == ("a.png", "b.png", "c.png", "d.png")
    with pytest.raises(SystemExit):
        split.get_parser().parse_args(["a.png", "b.png", "c.png", "d.png"])
    for bad in (0, -1, 64):
        with pytest.raises(ValueError):
            split.check_radius(bad)
    assert split.check_radius(63) == 63
    for parser in (predict.get_parser(), post_process.get_parser()):
        assert "close the cuts" in " ".join(parser.format_help().split())
    import inspect
    assert inspect.signature(post_process.post_process_tiles).parameters["split"].default == 0


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_five_entry_points():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    assert protos["xv2_edt_sq"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2)
    assert protos["xv2_split_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert protos["xv2_split_seed"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2)
    assert protos["xv2_split_grow"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3)
    assert protos["xv2_split_finish"] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4)
    assert "split.hip" in _lib.SOURCES


def test_workspace_query():
    from xview2_amd import _capi, _lib
    _lib.build()
    q = lambda *a: _capi.query("xv2_split_workspace", *a)
    assert q(2, 100, 70) >= 2 * 8 * 2 * 100 * 70 + 4 * 2 * 2 * 2 and q(2, 100, 70) % 256 == 0
    assert q(1, 1, 1) > 0 and q(65535, 1, 1) > 0
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, 0) == 0
    assert q(1, 1 << 15, 1 << 15) == 0 and q(65536, 4, 4) == 0


def test_every_argument_check_is_reachable_without_a_gpu():
    from xview2_amd import _capi, _lib
    _lib.build()
    one = ctypes.c_void_p(256)
    err = lambda: _lib.lib().xv2_last_error()

    def run(name, order, kw, msg):
        a = dict(mask=one, B=1, H=4, W=4, cap=2, r2=4, sweeps=1, ws=one, d2=one, pending=one, out=one, labels=None, stream=None)
        a.update(kw)
        assert _capi._func(name)(*[a[k] for k in order]) == 1 and msg in err(), (name, kw, err())

    sizes = [(dict(B=0), b"positive"), (dict(H=0), b"positive"), (dict(W=-1), b"positive"),
             (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"), (dict(mask=None), b"null")]
    ws = [(dict(ws=None), b"workspace"), (dict(ws=ctypes.c_void_p(264)), b"aligned")]
    edt = ("mask", "B", "H", "W", "cap", "d2", "stream")
    for kw, msg in sizes + [(dict(cap=0), b"cap"), (dict(cap=65), b"cap"), (dict(d2=None), b"null")]:
        run("xv2_edt_sq", edt, kw, msg)
    seed = ("mask", "B", "H", "W", "r2", "ws", "stream")
    for kw, msg in sizes + ws + [(dict(r2=0), b"r2"), (dict(r2=4096), b"r2"), (dict(r2=-3), b"r2")]:
        run("xv2_split_seed", seed, kw, msg)
    grow = ("mask", "B", "H", "W", "sweeps", "ws", "pending", "stream")
    for kw, msg in sizes + ws + [(dict(sweeps=0), b"sweeps"), (dict(sweeps=-1), b"sweeps"), (dict(pending=None), b"null")]:
        run("xv2_split_grow", grow, kw, msg)
    finish = ("mask", "B", "H", "W", "ws", "out", "labels", "stream")
    for kw, msg in sizes + ws + [(dict(out=None), b"null")]:
        run("xv2_split_finish", finish, kw, msg)
