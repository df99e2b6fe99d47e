"""The rule of include/xv2.h, "clean buildings", as restated by tests/clean_ref.py: pinned against hand-drawn expectations and
against scipy.ndimage, plus everything about the feature that needs no GPU (argument checks, parser defaults, the ABI, and
that the defaults route to the code path that was there before)."""
import ctypes
import inspect
import sys

import numpy as np
import pytest
from scipy import ndimage

import clean_ref as C

EIGHT = np.ones((3, 3), dtype=int)


def _draw(*rows):
    return np.array([[0 if ch == "." else int(ch) for ch in r] for r in rows], dtype=np.uint8)


# ---- hand-drawn ------------------------------------------------------------------------------------------------------------
def test_a_one_pixel_hole_is_filled_with_the_owners_class():
    pre = _draw(".....",
                ".111.",
                ".1.1.",
                ".111.",
                ".....")
    post = _draw("66666",
                 "62216",
                 "62516",
                 "61056",
                 "66666")           # the owner's classes: 2 x 3, 1 x 3 -> a tie, the smaller class wins
    out, pout, stats = C.clean(pre, post, 0, 1)
    want = pre.copy()
    want[2, 2] = 1
    wpost = post.copy()
    wpost[2, 2] = 1
    assert np.array_equal(out, want) and np.array_equal(pout, wpost) and stats.tolist() == [1, 1, 0, 0]
    out, pout, stats = C.clean(pre, post, 0, 0)
    assert np.array_equal(out, pre) and np.array_equal(pout, post) and stats.tolist() == [0, 0, 0, 0]
    out, pout, stats = C.clean(pre, None, 0, 5)
    assert np.array_equal(out, want) and pout is None


def test_a_diagonal_way_out_is_a_way_out():
    pre = _draw("......",
                ".111..",
                ".1.1..",
                ".11.1.",
                "......")           # the pocket at (2,2) leaves through (3,3): 8-connected background
    assert C.holes(pre) == []
    out, _, stats = C.clean(pre, None, 0, 99)
    assert np.array_equal(out, pre) and stats.tolist() == [0, 0, 0, 0]
    # the same pocket reaching the frame only through a diagonal step is not a hole either; one pixel inside the frame it is
    frame = _draw("11.1",
                  "1.11",
                  "1111")
    assert C.holes(frame) == []
    inside = _draw("1111",
                   "1.11",
                   "1111")
    assert C.holes(inside) == [[(1, 1)]]


def test_thresholds_hold_at_equality():
    pre = np.zeros((12, 20), dtype=np.uint8)
    pre[1:7, 1:8] = 1
    pre[2:4, 2:4] = 0                # a hole of 4
    pre[2:4, 5:7] = 0
    pre[4, 5] = 0                    # a hole of 5
    pre[9, 1:4] = 1                  # a building of 3
    pre[9, 6:10] = 1                 # a building of 4
    out, _, stats = C.clean(pre, None, 4, 4)
    want = pre.copy()
    want[2:4, 2:4] = 1
    want[9, 1:4] = 0
    assert np.array_equal(out, want) and stats.tolist() == [1, 4, 1, 3]


def test_island_merges_with_its_owner_and_nested_holes_go_by_their_own_area():
    pre = np.zeros((11, 11), dtype=np.uint8)
    pre[1:10, 1:10] = 1
    pre[2:9, 2:9] = 0                # the outer hole: a ring of 49 - 9 = 40 pixels around ...
    pre[4:7, 4:7] = 2                # ... an island of 9 - 1 = 8 pixels ...
    pre[5, 5] = 0                    # ... with its own hole of 1 pixel
    post = np.where(pre == 1, 3, np.where(pre == 2, 4, 0)).astype(np.uint8)
    assert sorted(len(h) for h in C.holes(pre)) == [1, 40]
    inner, pin, s = C.clean(pre, post, 0, 1)
    assert inner[5, 5] == 1 and pin[5, 5] == 4 and int((inner != pre).sum()) == 1 and s.tolist() == [1, 1, 0, 0]
    both, pboth, s = C.clean(pre, post, 0, 40)
    assert (both[1:10, 1:10] != 0).all() and s.tolist() == [2, 41, 0, 0]
    assert pboth[2, 2] == 3 and pboth[5, 5] == 4 and both[4, 4] == 2 and both[2, 2] == 1
    # the island alone (8 pixels, 9 with its hole filled) would be dropped at A = 10; merged with the filled ring it stays
    alone, _, s = C.clean(pre, post, 10, 1)
    assert not alone[4:7, 4:7].any() and s.tolist() == [1, 1, 1, 9]
    kept, _, s = C.clean(pre, post, 10, 40)
    assert (kept[1:10, 1:10] != 0).all() and s.tolist() == [2, 41, 0, 0]
    # the owner (32 pixels) is lifted over A = 81 by the ring, the island and its hole together, and no further
    assert C.clean(pre, post, 81, 40)[2].tolist() == [2, 41, 0, 0]
    assert C.clean(pre, post, 82, 40)[2].tolist() == [2, 41, 1, 81]


def test_an_owner_without_a_class_gives_zero():
    pre = _draw("111",
                "1.1",
                "111")
    post = _draw("057",
                 "030",
                 "600")
    out, pout, _ = C.clean(pre, post, 0, 1)
    assert out[1, 1] == 1 and pout[1, 1] == 0
    assert C.vote(np.array([0, 5, 9])) == 0 and C.vote(np.array([4, 4, 2, 2, 7])) == 2 and C.vote(np.array([], dtype=int)) == 0


# ---- scipy -----------------------------------------------------------------------------------------------------------------
CASES = [(seed, H, W, d) for seed, (H, W) in enumerate(((1, 1), (1, 7), (7, 1), (3, 3), (20, 31), (33, 17), (40, 40)))
         for d in (0.1, 0.5, 0.9)]


@pytest.mark.parametrize("seed,H,W,density", CASES)
def test_fill_everything_is_binary_fill_holes(seed, H, W, density):
    pre, post = C.random_pair(seed, H, W, density)
    out, _, stats = C.clean(pre, post, 0, H * W)
    want = ndimage.binary_fill_holes(pre != 0, structure=EIGHT)
    assert np.array_equal(out != 0, want)
    assert stats[1] == int(want.sum()) - int((pre != 0).sum()) and np.array_equal(out[pre != 0], pre[pre != 0])


@pytest.mark.parametrize("seed,H,W,density", CASES)
def test_hole_areas_are_those_of_the_eight_connected_background(seed, H, W, density):
    pre, _ = C.random_pair(seed, H, W, density)
    lab, n = ndimage.label(pre == 0, structure=EIGHT)
    frame = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
    want = sorted(int((lab == k).sum()) for k in range(1, n + 1) if k not in frame)
    assert sorted(len(h) for h in C.holes(pre)) == want


@pytest.mark.parametrize("seed,H,W,density", CASES)
@pytest.mark.parametrize("A", [1, 2, 5])
def test_drop_alone_keeps_the_components_of_at_least_min_area(seed, H, W, density, A):
    pre, post = C.random_pair(seed, H, W, density)
    out, pout, stats = C.clean(pre, post, A, 0)
    lab, n = ndimage.label(pre != 0)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = (area >= A)[lab] & (lab > 0)
    assert np.array_equal(out, np.where(keep, pre, 0)) and np.array_equal(pout, np.where((lab > 0) & ~keep, 0, post))
    assert stats.tolist() == [0, 0, int(((area < A)[1:]).sum()), int(area[1:][area[1:] < A].sum())]


def test_zero_and_zero_is_the_identity():
    pre, post = C.random_pair(3, 30, 30, 0.6)
    out, pout, stats = C.clean(pre, post, 0, 0)
    assert np.array_equal(out, pre) and np.array_equal(pout, post) and not stats.any()
    with pytest.raises(ValueError):
        C.clean(pre, post, -1, 0)


# ---- arguments and command lines -------------------------------------------------------------------------------------------
def test_argument_checks():
    from xview2_amd.utils import clean
    assert clean.check_min_area(0) == 0 and clean.check_min_area(np.int64(7)) == 7 and clean.check_fill_holes(1 << 40) == 1 << 40
    for check in (clean.check_min_area, clean.check_fill_holes):
        for bad in (-1, 1.5, "3", None, True):
            with pytest.raises(ValueError, match="integer >= 0"):
                check(bad)
    assert clean.STAT_KEYS == ("holes_filled", "pixels_filled", "buildings_dropped", "pixels_dropped")


def test_the_four_command_lines_default_to_off():
    from xview2_amd import predict
    from xview2_amd.utils import building_metrics, clean, post_process
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o"])
    assert a.min_area == 0 and a.fill_holes == 0
    a = predict.get_parser().parse_args(["--pre", "p", "--out", "o", "--min_area", "16", "--fill_holes", "9"])
    assert a.min_area == 16 and a.fill_holes == 9
    a = post_process.get_parser().parse_args([])
    assert a.min_area == 0 and a.fill_holes == 0
    a = post_process.get_parser().parse_args(["--min_area", "4", "--fill_holes", "2", "--split", "1"])
    assert (a.min_area, a.fill_holes, a.split) == (4, 2, 1)
    a = building_metrics.get_parser().parse_args(["P", "T", "o.json"])
    assert a.min_area == 0 and a.fill_holes == 0 and a.min_area_targets == 0
    a = building_metrics.get_parser().parse_args(["P", "T", "o.json", "--min_area", "2", "--fill_holes", "3", "--min_area_targets", "4"])
    assert (a.min_area, a.fill_holes, a.min_area_targets) == (2, 3, 4)
    a = clean.get_parser().parse_args(["a.png", "b.png", "c.png", "d.png"])
    assert a.min_area == 0 and a.fill_holes == 0 and (a.pre, a.post, a.out_pre, a.out_post) == ("a.png", "b.png", "c.png", "d.png")
    a = clean.get_parser().parse_args(["a.png", "b.png", "c.png", "d.png", "--min_area", "5", "--fill_holes", "6"])
    assert a.min_area == 5 and a.fill_holes == 6
    with pytest.raises(ValueError, match="integer >= 0"):
        clean.main(["a.png", "b.png", "c.png", "d.png", "--min_area", "-2"])
    for parser in (predict.get_parser(), post_process.get_parser()):
        assert "No value is recommended" in " ".join(parser.format_help().split())


def test_trailing_keywords_default_to_zero():
    from xview2_amd.utils import building_metrics, clean, post_process
    p = list(inspect.signature(post_process.post_process_tiles).parameters.items())
    assert [n for n, _ in p[:7]] == ["loc", "dmg", "components", "dilate", "dilation_rate", "workspace", "split"]
    assert (p[7][0], p[7][1].default, p[8][0], p[8][1].default) == ("min_area", 0, "fill_holes", 0)
    for fn in (building_metrics.BuildingMetrics.__init__, building_metrics.compute_score):
        q = inspect.signature(fn).parameters
        assert list(q)[-3:] == ["min_area", "fill_holes", "min_area_targets"] and all(q[k].default == 0 for k in list(q)[-3:])
    q = inspect.signature(clean.clean_maps).parameters
    assert list(q)[:4] == ["pre", "post", "min_area", "fill_holes"]
    assert "minimum-area" in building_metrics.__doc__ and "off unless asked for" in building_metrics.__doc__


class _Map:
    """stands for a device tensor: post_process_tiles only asks for its rank and hands it on"""
    def __init__(self, rank):
        self.rank = rank

    def dim(self):
        return self.rank

    def unsqueeze(self, _):
        return _Map(self.rank + 1)

    def __getitem__(self, _):
        return _Map(self.rank - 1)


def test_the_defaults_make_the_call_that_was_made_before(monkeypatch):
    from xview2_amd import ops
    from xview2_amd.utils import post_process
    calls = []

    def fake(loc, dmg, components=False, rate=0, workspace=None):
        calls.append((components, rate, workspace))
        return _Map(3), _Map(3)

    def boom(*a, **k):
        raise AssertionError("clean_buildings must not be called with the defaults")

    monkeypatch.setattr(ops, "postprocess", fake)
    monkeypatch.setattr(ops, "clean_buildings", boom)
    monkeypatch.delitem(sys.modules, "xview2_amd.utils.clean", raising=False)
    monkeypatch.delitem(sys.modules, "xview2_amd.utils.split", raising=False)
    for kw in ({}, dict(min_area=0, fill_holes=0), dict(split=0, min_area=0, fill_holes=0)):
        out = post_process.post_process_tiles(_Map(3), _Map(4), True, True, 5, "ws", **kw)
        assert len(out) == 2
    assert calls == [(True, 5, "ws")] * 3
    assert "xview2_amd.utils.clean" not in sys.modules and "xview2_amd.utils.split" not in sys.modules
    out = post_process.post_process_tiles(_Map(2), _Map(3), return_stats=True)
    assert len(out) == 3 and out[2] is None and out[0].rank == 2


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_entry_points():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    assert protos["xv2_clean_workspace"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert protos["xv2_clean_buildings"] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_int64] * 2
                                             + [ctypes.c_void_p] * 5)
    assert "clean.hip" in _lib.SOURCES


def test_workspace_query():
    from xview2_amd import _capi, _lib
    _lib.build()
    q = lambda *a: _capi.query("xv2_clean_workspace", *a)
    assert q(2, 100, 70) >= 20 * 2 * 100 * 70 and q(2, 100, 70) % 256 == 0
    assert q(1, 1, 1) > 0 and q(65535, 1, 1) > 0
    assert q(0, 4, 4) == 0 and q(1, 0, 4) == 0 and q(1, 4, 0) == 0
    assert q(1, 1 << 15, 1 << 15) == 0 and q(65536, 4, 4) == 0


def test_every_argument_check_is_reachable_without_a_gpu():
    from xview2_amd import _capi, _lib
    _lib.build()
    one, two, three, four = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    err = lambda: _lib.lib().xv2_last_error()
    order = ("pre", "post", "B", "H", "W", "A", "M", "ws", "pre_out", "post_out", "stats", "stream")
    for kw, msg in [(dict(B=0), b"positive"), (dict(H=0), b"positive"), (dict(W=-1), b"positive"),
                    (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"), (dict(A=-1), b"negative"),
                    (dict(M=-1), b"negative"), (dict(pre=None), b"null"), (dict(pre_out=None), b"null"),
                    (dict(stats=None), b"null"), (dict(post=None), b"both"), (dict(post_out=None), b"both"),
                    (dict(pre_out=one), b"alias"), (dict(post_out=two), b"alias"), (dict(post_out=one), b"alias"),
                    (dict(ws=None), b"workspace"), (dict(ws=ctypes.c_void_p(264)), b"aligned")]:
        a = dict(pre=one, post=two, B=1, H=4, W=4, A=2, M=2, ws=one, pre_out=three, post_out=four, stats=one, stream=None)
        a.update(kw)
        assert _capi._func("xv2_clean_buildings")(*[a[k] for k in order]) == 1 and msg in err(), (kw, err())
