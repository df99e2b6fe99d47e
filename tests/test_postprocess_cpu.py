"""CPU checks of the offline post-processing / scoring feature: the numpy restatement (tests/postproc_ref.py) against
the fixture recorded from the reference's own scripts, its connected components against scipy, the documented
departures, and argument validation of the new C-ABI entry points (no GPU needed)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import postproc_ref as R

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postproc_golden.json")))


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def cases():
    return R.cases()


def test_fixture_covers_every_case(cases):
    assert set(GOLD["postprocess"]) == set(cases)
    with_vote = [n for n, rec in GOLD["postprocess"].items() if "c1_r0" in rec]
    assert {"buildings_4ch", "buildings_5ch", "buildings_int_label", "vote_ties", "mask_spiral", "mse_unclamped",
            "wide_label"} <= set(with_vote)


def test_unclamped_label_maps_keep_reference_values():
    """an mse decode with values above 4 on background loses them in the fusion; values that survive stay as they are"""
    case = R.cases()
    loc, dmg = case["mse_unclamped"]
    assert dmg.max() > 4 and not (dmg[loc > np.float32(0.1)] > 4).any()
    for comp in (False, True):
        pre, post = R.post_process(loc, dmg, components=comp, rate=3)
        assert post.max() <= 4
    loc, dmg = case["wide_label"]
    _, post = R.post_process(loc, dmg)
    assert post.max() == 9


@pytest.mark.parametrize("name", sorted(GOLD["postprocess"]))
def test_restatement_reproduces_reference_digests(cases, name):
    loc, dmg = cases[name]
    rec = GOLD["postprocess"][name]
    for key, val in sorted(rec.items()):
        if key == "components":
            continue
        dpre, dpost = val
        comp, rate = int(key[1]), int(key.split("_r")[1])
        pre, post = R.post_process(loc, dmg, components=bool(comp), rate=rate)
        assert (_digest(pre), _digest(post)) == (dpre, dpost), (name, key)


def test_restatement_reproduces_reference_metrics():
    rows = [R.tile_row(*t) for t in R.metric_tiles()]
    assert rows == GOLD["metrics"]["rows"]
    d = R.score(rows)
    assert d == GOLD["metrics"]["dict"]
    assert json.dumps(d) == GOLD["metrics"]["json"]


@pytest.mark.parametrize("shape", [(1024, 1024), (1000, 777), (1, 1), (3, 130)])
def test_restatement_components_equal_scipy(shape):
    nd = pytest.importorskip("scipy.ndimage")
    masks = R.adversarial_masks(*shape)
    for name, m in masks.items():
        ref, n = nd.label(m)
        lab = R.label_min_index(m)
        assert np.array_equal(R.scipy_numbering(lab), ref), name
        if n:
            idx = np.arange(m.size).reshape(m.shape)
            mins = np.asarray(nd.minimum(idx, ref, index=np.arange(1, n + 1)), dtype=np.int64)
            assert np.array_equal(lab[m], mins[ref[m] - 1] + 1), name


def test_five_channel_rule_drops_background_channel():
    loc = np.full((2, 3), 0.5, dtype=np.float32)
    dmg = np.zeros((5, 2, 3), dtype=np.float32)
    dmg[0] = 9.0                      # background channel: the largest everywhere, ignored
    dmg[3, 0, 0] = 1.0                # damage channel 3 -> class 3
    dmg[1, 1, 2] = dmg[2, 1, 2] = 1.0  # tie between classes 1 and 2 -> the first
    _, post = R.post_process(loc, dmg)
    assert post[0, 0] == 3 and post[1, 2] == 1 and post[0, 1] == 1
    _, post4 = R.post_process(loc, dmg[1:5])
    assert np.array_equal(post, post4)


def test_thresholds_compare_in_float32():
    t3, t1 = np.float32(0.3), np.float32(0.1)
    loc = np.array([[t3, np.nextafter(t3, np.float32(1)), t1, np.nextafter(t1, np.float32(1))]], dtype=np.float32)
    lab = np.array([[1, 1, 2, 2]])
    pre, post = R.post_process(loc, lab)
    assert pre.tolist() == [[0, 1, 0, 1]] and post.tolist() == [[0, 1, 0, 2]]


def test_even_rate_is_rejected():
    loc = np.zeros((4, 4), dtype=np.float32)
    with pytest.raises(ValueError):
        R.post_process(loc, np.zeros((4, 4, 4), dtype=np.float32).reshape(4, 4, 4), rate=2)
    from xview2_amd.utils import post_process as pp
    with pytest.raises(ValueError):
        pp._check_rate(True, 4)
    assert pp._check_rate(False, 4) == 0 and pp._check_rate(True, 3) == 3


def test_entry_points_validate_arguments_without_gpu():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    for name in ("xv2_postprocess", "xv2_postprocess_workspace", "xv2_label_components", "xv2_xview2_counts"):
        assert name in protos
    assert protos["xv2_postprocess_workspace"][0] is ctypes.c_size_t
    assert _capi.query("xv2_postprocess_workspace", 2, 1024, 1024, 1) >= 22 * 2 * 1024 * 1024
    assert _capi.query("xv2_postprocess_workspace", 2, 1024, 1024, 0) >= 2 * 2 * 1024 * 1024
    L = _lib.lib()
    err = lambda: L.xv2_last_error().decode()   # noqa: E731
    pp = _capi._func("xv2_postprocess")
    dummy = 256   # never dereferenced: validation returns before any launch
    assert pp(dummy, dummy, 0, 1, 64, 64, 1, 2, dummy, dummy, dummy, None, None) == 1 and "rate 2" in err()
    assert pp(dummy, dummy, 7, 1, 64, 64, 0, 0, None, dummy, dummy, None, None) == 1 and "dmg_kind=7" in err()
    assert pp(dummy, dummy, 0, 0, 64, 64, 0, 0, None, dummy, dummy, None, None) == 1 and "positive" in err()
    assert pp(dummy, dummy, 0, 1, 64, 64, 1, 3, None, dummy, dummy, None, None) == 1 and "workspace" in err()
    assert pp(dummy, dummy, 2, 1, 64, 64, 0, 0, None, dummy, dummy, None, None) == 1 and "status" in err()
    lc = _capi._func("xv2_label_components")
    assert lc(dummy, 1, -5, 64, None, dummy, None) == 1 and "positive" in err()
    xc = _capi._func("xv2_xview2_counts")
    assert xc(dummy, dummy, dummy, dummy, 1, 0, dummy, None) == 1 and "positive" in err()
