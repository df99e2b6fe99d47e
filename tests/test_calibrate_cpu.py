"""Everything about the threshold / class-scale sweep that needs no GPU: the restatement of tests/calibrate_ref.py against the
brute force, the host derivation of utils/calibrate.py against it, the grid, the tie rule, the report's bytes, the flags of
both parsers, and every argument check of xv2_calibrate_hist and xv2_postprocess_ex."""
import ctypes
import json

import numpy as np
import pytest

import calibrate_ref as C
import postproc_ref as R

T7 = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.75, 0.9], dtype=np.float32)


@pytest.fixture(scope="module")
def small():
    """four 48 x 40 tiles, their histogram over T7 x C.SCALES by the restatement"""
    tl = C.tiles(900, 4, 48, 40, T7)
    cols = list(zip(*tl))
    h, bad = C.hist(*cols, T7, C.SCALES)
    assert bad == 0 and h.sum() == 3 * 4 * 48 * 40
    return cols, h


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_derive_equals_the_brute_force_at_every_grid_point(small):
    from xview2_amd.utils import calibrate
    cols, h = small
    fast = calibrate.derive(h)
    assert fast.shape == (3, 7, 7, 15) and fast.dtype == np.int64
    for s, scale in enumerate(C.SCALES):
        for i in range(7):
            for j in range(i + 1):
                want = C.brute(*cols, T7[i], T7[j], scale)
                assert C.derive(h[s], i, j) == want, (s, i, j)
                assert fast[s, i, j].tolist() == want, (s, i, j)


def test_scales_flip_the_argmax_and_tie_exactly(small):
    cols, h = small
    d = cols[1][0]
    plain, a, b = (C.decode_post(d, s) for s in C.SCALES)
    assert (plain != a).any() and (plain != b).any()
    prod = np.stack([np.float32(C.SCALES[1][c]) * d[c] for c in range(4)])
    top = prod.max(axis=0)
    assert ((prod == top).sum(axis=0) > 1).any()          # exact product ties: the first maximum must win
    assert np.array_equal(a, np.argmax(prod, axis=0) + 1)


def test_the_restatement_at_the_reference_point_is_the_reference_fusion():
    for name, (loc, dmg) in (("thresholds", (R.threshold_loc(21, (96, 80)), R.probs_from_classes(22, 1 + R.hash_int(23, (96, 80), 4), 4))),
                             ("five", (R.threshold_loc(24, (96, 80)), R.probs_from_classes(25, R.hash_int(26, (96, 80), 5), 5))),
                             ("label", (R.threshold_loc(27, (96, 80)), R.hash_int(28, (96, 80), 5)))):
        want_pre, want_post = R.fuse(loc, dmg)
        for scale in (None, C.ONES) if name != "label" else (None,):
            pre, post = C.fuse(loc, dmg, 0.3, 0.1, scale)
            assert np.array_equal(pre, want_pre) and np.array_equal(post, want_post), name


def test_bins_send_wide_targets_and_labels_to_bad():
    loc = C.edge_loc(5, (20, 30), T7)
    lt, dt = C.targets(6, (20, 30))
    lab = R.hash_int(7, (20, 30), 7) - 1                   # -1..5
    h, bad = C.hist(loc, lab, lt, dt, T7)
    ok = (lt <= 4) & (dt <= 4) & (lab >= 1) & (lab <= 4)
    assert bad == int((~ok).sum()) > 0 and h.sum() == int(ok.sum())
    assert np.isnan(loc).any() and h[0, 0].sum() >= int((np.isnan(loc) & ok).sum())


# ---- grid, scale list, tie rule --------------------------------------------------------------------------------------------
def test_the_reference_point_lies_on_the_default_grid():
    from xview2_amd.utils import calibrate
    t = calibrate.threshold_grid(0.01)
    assert t.dtype == np.float32 and len(t) == 100 and (np.diff(t) > 0).all()
    assert t[30] == np.float32(0.3) and t[10] == np.float32(0.1)
    assert np.float32(30 / 100.0) == np.float32(0.3) and np.float32(10 / 100.0) == np.float32(0.1)
    assert t[0] == 0 and t[-1] == np.float32(99 * 0.01)
    assert len(calibrate.threshold_grid(1 / 128.0)) == 128 and len(calibrate.threshold_grid(0.3)) == 4


@pytest.mark.parametrize("g", [0.005, 1 / 129.0, 0.0, -0.1, float("nan"), 2.0])
def test_a_grid_of_more_than_128_thresholds_is_refused(g):
    from xview2_amd.utils import calibrate
    with pytest.raises(ValueError):
        calibrate.threshold_grid(g)


def test_scale_lists():
    from xview2_amd.utils import calibrate
    assert calibrate.scale_list() == [C.ONES]
    grid = calibrate.scale_list(scale_grid="0.5,1,2")
    assert len(grid) == 27 and all(r[0] == 1.0 for r in grid) and grid[0] == (1.0, 0.5, 0.5, 0.5) and grid[13] == C.ONES
    assert calibrate.scale_list(class_scales="1,1,1,1;1,2,2,0.1") == [C.ONES, (1.0, 2.0, 2.0, float(np.float32(0.1)))]
    for kw in (dict(scale_grid="1", class_scales="1,1,1,1"), dict(scale_grid="0"), dict(class_scales="1,1,1"),
               dict(class_scales="1,1,1,-1"), dict(class_scales=";")):
        with pytest.raises(ValueError):
            calibrate.scale_list(**kw)


def test_best_is_the_restatements_best(small):
    from xview2_amd.utils import calibrate
    _, h = small
    top, arg = C.best(h)
    counts = calibrate.derive(h)
    assert calibrate.best(counts) == arg
    assert calibrate.point_scores(counts[arg])["score"] == top
    table = calibrate.score_table(counts)
    assert table.shape == (3, 7, 7) and np.isnan(table[:, 0, 1:]).all() and not np.isnan(table[:, 6, :]).any()
    assert abs(np.nanmax(table) - top) < 1e-12
    for s, i, j in ((0, 3, 1), (2, 6, 6), (1, 0, 0)):
        assert calibrate.point_scores(counts[s, i, j]) == R.score([counts[s, i, j].tolist()])


def test_ties_go_to_the_first_point_in_scale_i_j_order():
    from xview2_amd.utils import calibrate
    # every pixel at loc = 0.55 with a right damage answer: every (i, j) with T_i < 0.55 scores the same, in both scale rows
    h = np.zeros((2, 8, 4, 2, 5), dtype=np.int64)
    h[:, 5, 0, 1, 1] = 10
    h[:, 5, 1, 1, 2] = 10
    h[:, 5, 2, 1, 3] = 10
    h[:, 5, 3, 1, 4] = 10
    counts = calibrate.derive(h)
    assert calibrate.best(counts) == (0, 0, 0) == C.best(h)[1]
    # a background pixel just above T_0 that class 1 would claim: (0, 0) loses it, the first winner is (1, 0)
    h[:, 1, 0, 0, 0] = 3
    assert calibrate.best(calibrate.derive(h)) == (0, 1, 0) == C.best(h)[1]
    # the second scale vector strictly better: it wins over every earlier point
    h[0, 5, 0, 1, 1] = 9
    h[0, 5, 1, 1, 1] += 1
    assert calibrate.best(calibrate.derive(h)) == (1, 1, 0) == C.best(h)[1]


def test_the_report_has_the_same_bytes_on_every_run(small):
    from xview2_amd.utils import calibrate
    _, h = small
    dh = np.zeros((1, 3, 4, 2, 5), dtype=np.int64)
    dh[0, 2, 0, 1, 1] = 7
    dh[0, 1, 2, 1, 3] = 5
    dh[0, 0, 0, 0, 0] = 100
    docs = [calibrate.build_report(T7, C.SCALES, h.copy(), dh.copy(), 4, 4 * 48 * 40, 0, None)[0] for _ in range(2)]
    a, b = (calibrate.dumps(d) for d in docs)
    assert a == b and a.endswith("\n") and json.loads(a) == docs[0]
    doc = docs[0]
    assert a == json.dumps(doc, indent=1, sort_keys=True) + "\n"
    assert doc["default"]["loc_threshold"] == float(np.float32(0.3)) and doc["default"]["loc_threshold_dmg"] == float(np.float32(0.1))
    assert doc["default"]["counts"] == C.derive(dh[0], 1, 0) and doc["default"]["grid_index"] == [3, 1]
    top, arg = C.best(h)
    assert doc["best"]["index"] == list(arg) and doc["best"]["scores"]["score"] == top
    assert doc["best"]["scores"] == R.score([doc["best"]["counts"]])
    assert len(doc["best_per_scale"]) == 3 and [p["index"][0] for p in doc["best_per_scale"]] == [0, 1, 2]
    assert max(p["scores"]["score"] for p in doc["best_per_scale"]) == top
    assert sorted(doc["best"]["scores"]) == sorted(calibrate.SCORE_KEYS) and len(doc["best"]["counts"]) == 15


# ---- flags -----------------------------------------------------------------------------------------------------------------
def _report(tmp_path, a=0.42, b=0.17, scale=(1.0, 2.0, 0.5, 1.5)):
    p = tmp_path / "calibration.json"
    p.write_text(json.dumps({"best": {"loc_threshold": a, "loc_threshold_dmg": b, "class_scale": list(scale)}}))
    return str(p)


def _parsers():
    from xview2_amd import predict
    from xview2_amd.utils import post_process
    return [(post_process.get_parser(), []), (predict.get_parser(), ["--pre", "a", "--out", "b"])]


def test_defaults_leave_the_fusion_alone():
    from xview2_amd.utils import fusion
    for parser, need in _parsers():
        args = parser.parse_args(need)
        assert (args.loc_threshold, args.loc_threshold_dmg, args.class_scale, args.calibration) == (None,) * 4
        assert fusion.resolve(args) == {"loc_threshold": None, "dmg_threshold": None, "class_scale": None}


def test_explicit_flags_win_over_the_calibration_file(tmp_path):
    from xview2_amd.utils import fusion
    rep = _report(tmp_path)
    for parser, need in _parsers():
        got = fusion.resolve(parser.parse_args(need + ["--calibration", rep]))
        assert got == {"loc_threshold": 0.42, "dmg_threshold": 0.17, "class_scale": (1.0, 2.0, 0.5, 1.5)}
        got = fusion.resolve(parser.parse_args(need + ["--calibration", rep, "--loc_threshold", "0.5"]))
        assert got == {"loc_threshold": 0.5, "dmg_threshold": 0.17, "class_scale": (1.0, 2.0, 0.5, 1.5)}
        got = fusion.resolve(parser.parse_args(need + ["--calibration", rep, "--loc_threshold_dmg", "0.05", "--class_scale",
                                                       "1,1,3,1"]))
        assert got == {"loc_threshold": 0.42, "dmg_threshold": 0.05, "class_scale": (1.0, 1.0, 3.0, 1.0)}
        got = fusion.resolve(parser.parse_args(need + ["--loc_threshold", "0.6", "--class_scale", "2,1,1,1"]))
        assert got == {"loc_threshold": 0.6, "dmg_threshold": None, "class_scale": (2.0, 1.0, 1.0, 1.0)}
        with pytest.raises(ValueError):      # B from the file above the explicit A
            fusion.resolve(parser.parse_args(need + ["--calibration", rep, "--loc_threshold", "0.1"]))
        with pytest.raises(ValueError):
            fusion.resolve(parser.parse_args(need + ["--loc_threshold_dmg", "0.4"]))
        with pytest.raises(SystemExit):
            parser.parse_args(need + ["--class_scale", "1,2,3"])


def test_a_report_with_unit_scales_passes_no_scales(tmp_path):
    from xview2_amd.utils import fusion, post_process
    rep = _report(tmp_path, scale=(1.0, 1.0, 1.0, 1.0))
    got = fusion.resolve(post_process.get_parser().parse_args(["--calibration", rep]))
    assert got == {"loc_threshold": 0.42, "dmg_threshold": 0.17, "class_scale": None}
    bad = tmp_path / "other.json"
    bad.write_text("{}")
    with pytest.raises(ValueError, match="no report"):
        fusion.resolve(post_process.get_parser().parse_args(["--calibration", str(bad)]))


def test_defaults_route_to_the_call_that_was_always_made(monkeypatch):
    import torch
    from xview2_amd import ops
    calls = []
    scales = []      # read while the call runs: the host array lives no longer than that

    def record(name, *a):
        calls.append((name, a))
        if name == "xv2_postprocess_ex" and a[14] is not None:
            scales.append((ctypes.c_float * 4).from_address(a[14])[:])

    monkeypatch.setattr(ops, "call", record)
    monkeypatch.setattr(ops, "_need_cuda", lambda t: None)
    loc, dmg = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 4)
    ops.postprocess(loc, dmg)
    ops.postprocess(loc, dmg, loc_threshold=0.3, dmg_threshold=0.1, class_scale=(1, 1, 1, 1))
    ops.postprocess(loc, dmg, dmg_threshold=0.2)
    assert [c[0] for c in calls] == ["xv2_postprocess", "xv2_postprocess_ex", "xv2_postprocess_ex"]
    assert len(calls[0][1]) == 12
    a = calls[1][1]
    assert a[2:9] == calls[0][1][2:9] and a[12] == float(np.float32(0.3)) and a[13] == float(np.float32(0.1))
    assert scales == [[1.0] * 4]
    assert calls[2][1][12:] == (float(np.float32(0.3)), float(np.float32(0.2)), None)
    for kw in (dict(loc_threshold=0.1, dmg_threshold=0.2), dict(loc_threshold=float("nan")), dict(class_scale=(1, 1, 1)),
               dict(class_scale=(1, 0, 1, 1)), dict(class_scale=(1, float("inf"), 1, 1))):
        with pytest.raises(ValueError):
            ops.postprocess(loc, dmg, **kw)
    with pytest.raises(ValueError, match="label map"):
        ops.postprocess(loc, torch.ones(1, 4, 4, dtype=torch.int32), class_scale=(1, 2, 1, 1))


def test_threshold_tables_are_checked_on_the_host():
    """xv2_calibrate_hist takes its table in device memory, so its order is ops' to check (include/xv2.h says so)"""
    from xview2_amd import ops
    assert ops.check_thresholds([0.0, 0.5]).dtype == np.float32
    for t in ([], list(range(129)), [0.1, 0.1], [0.2, 0.1], [0.0, float("nan")], [0.0, float("inf")],
              [0.1, 0.1 + 1e-12]):     # equal once rounded to float32
        with pytest.raises(ValueError):
            ops.check_thresholds(t)
    assert len(ops.check_thresholds(np.arange(128) / 128.0)) == 128


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    from xview2_amd import _capi, _lib
    protos = _capi._parse_header()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["xv2_postprocess_ex"] == (I, protos["xv2_postprocess"][1][:-1] + [F, F, P, P])
    assert protos["xv2_calibrate_hist"] == (I, [P, P, I, P, P, I, I, I, P, I, P, I, P, P, P])
    assert "calibrate.hip" in _lib.SOURCES
    assert {"xv2_postprocess_ex", "xv2_calibrate_hist"} <= set(_lib.declared_symbols())


def test_every_argument_check_is_reachable_without_a_gpu():
    from xview2_amd import _capi, _lib
    _lib.build()
    one, two, three, four = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    err = lambda: _lib.lib().xv2_last_error()
    order = ("loc", "dmg", "kind", "lt", "dt", "B", "H", "W", "thresholds", "n", "scales", "S", "hist", "bad", "stream")
    for kw, msg in [(dict(n=0), b"thresholds"), (dict(n=129), b"thresholds"), (dict(S=65, scales=one), b"scale vectors"),
                    (dict(S=0), b"scale vectors"), (dict(S=2), b"without a scale table"),
                    (dict(kind=2, scales=one), b"label map"), (dict(kind=3), b"unsupported"), (dict(B=0), b"positive"),
                    (dict(H=1 << 15, W=1 << 15), b"2^30"), (dict(B=65536), b"too large"), (dict(loc=None), b"null"),
                    (dict(lt=None), b"null"), (dict(thresholds=None), b"null"), (dict(hist=None), b"null"),
                    (dict(bad=None), b"null")]:
        a = dict(loc=one, dmg=two, kind=0, lt=three, dt=four, B=1, H=4, W=4, thresholds=one, n=4, scales=None, S=1, hist=two,
                 bad=three, stream=None)
        a.update(kw)
        assert _capi._func("xv2_calibrate_hist")(*[a[k] for k in order]) == 1 and msg in err(), (kw, err())
    order = ("loc", "dmg", "kind", "B", "H", "W", "comp", "rate", "ws", "pre", "post", "status", "t_loc", "t_dmg", "scale",
             "stream")
    good = (ctypes.c_float * 4)(1, 2, 3, 4)
    for kw, msg in [(dict(t_loc=0.1, t_dmg=0.2), b"must not exceed"), (dict(t_loc=float("nan")), b"finite"),
                    (dict(t_dmg=float("-inf")), b"finite"), (dict(t_loc=float("inf")), b"finite"),
                    (dict(kind=2, scale=good, status=one), b"label map"),
                    (dict(scale=(ctypes.c_float * 4)(1, 0, 1, 1)), b"class scale 2"),
                    (dict(scale=(ctypes.c_float * 4)(1, 1, -2, 1)), b"class scale 3"),
                    (dict(scale=(ctypes.c_float * 4)(1, 1, 1, float("nan"))), b"class scale 4"),
                    (dict(scale=(ctypes.c_float * 4)(float("inf"), 1, 1, 1)), b"class scale 1"),
                    (dict(B=0), b"positive"), (dict(rate=2), b"odd"), (dict(kind=5), b"unsupported"), (dict(pre=None), b"null")]:
        a = dict(loc=one, dmg=two, kind=0, B=1, H=4, W=4, comp=0, rate=0, ws=None, pre=three, post=four, status=None,
                 t_loc=0.3, t_dmg=0.1, scale=None, stream=None)
        a.update(kw)
        if a["scale"] is not None:
            a["scale"] = ctypes.cast(a["scale"], ctypes.c_void_p)
        assert _capi._func("xv2_postprocess_ex")(*[a[k] for k in order]) == 1 and msg in err(), (kw, err())
