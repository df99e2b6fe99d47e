"""The restatement of the ``wce`` term (tests/wce_ref.py) pinned on the CPU: the loss and gradient against torch's weighted
cross-entropy, the streaming distance rule against the per-component definition, the fixture condition that keeps an
all-0xFFFF kernel from passing, and the host layers' handling of the new name, flags and symbols."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wce_ref as R
from tests.golden.cases import ARGS


@pytest.mark.parametrize("shape,post,cw", [((2, 2, 13, 17), False, (1.0, 3.0)), ((2, 2, 9, 8), False, (0.0, 2.5)),
                                            ((2, 4, 16, 15), True, (0.5, 1.0, 4.0, 8.0)), ((1, 4, 12, 12), True, (1.0, 0.0, 2.0, 3.0))])
def test_without_a_border_the_term_is_torchs_weighted_cross_entropy(shape, post, cw):
    x, y = R.case(shape, 11 + shape[2], post)
    x = x.double().requires_grad_(True)
    loss, _ = R.forward(x, y, cw, post)
    loss.backward()
    x2 = x.detach().clone().requires_grad_(True)
    C = shape[1]
    if post:      # over the label > 0 pixels with label - 1
        keep = y > 0
        want = F.cross_entropy(x2.permute(0, 2, 3, 1)[keep], (y[keep].long() - 1), weight=torch.tensor(cw, dtype=torch.float64))
    else:
        want = F.cross_entropy(x2, y.long(), weight=torch.tensor(cw, dtype=torch.float64))
    want.backward()
    loss, want = float(loss.detach()), float(want.detach())
    assert abs(loss - want) <= 1e-13 * max(1.0, abs(want))
    assert (x.grad - x2.grad).abs().max() <= 1e-15
    assert (R.backward(x, y, cw, post) - x2.grad).abs().max() <= 1e-15
    assert (R.backward(x, y, cw, post, gscale=0.25) - 0.25 * x2.grad).abs().max() <= 1e-15
    assert C == len(cw)


def test_label_stride_border_and_empty_sets():
    x, y = R.case((2, 2, 8, 8), 5, lshape=(2, 16, 16))
    b = torch.rand(2, 16, 16, dtype=torch.float64)
    l2, (S0, S1) = R.forward(x, y, (1.0, 2.0), ls=2, bmap=b)
    w = torch.tensor([1.0, 2.0], dtype=torch.float64)[y[:, ::2, ::2].long()] + b[:, ::2, ::2]
    ce = F.cross_entropy(x.double(), y[:, ::2, ::2].long(), reduction="none")
    assert abs(float(l2) - float((w * ce).sum() / w.sum())) <= 1e-13 and abs(float(S1) - float(w.sum())) <= 1e-12
    # post with no building pixel, and every present class weighted 0: sum w == 0, loss 0, gradient 0
    xp, _ = R.case((1, 4, 6, 6), 6, True)
    zero = torch.zeros(1, 6, 6, dtype=torch.uint8)
    assert float(R.forward(xp, zero, (1.0,) * 4, True)[0]) == 0.0 and not R.backward(xp, zero, (1.0,) * 4, True).any()
    ones = torch.ones(2, 8, 8, dtype=torch.uint8)
    assert float(R.forward(x, ones, (1.0, 0.0))[0]) == 0.0 and not R.backward(x, ones, (1.0, 0.0)).any()
    assert R.bounds(x, ones, (1.0, 0.0))["loss"] == 0.0


@pytest.mark.parametrize("name", list(R.RANDOM) + list(R.SPECIAL))
def test_the_streaming_rule_agrees_with_the_per_component_definition(name):
    make, rad = {**R.RANDOM, **R.SPECIAL}[name]
    m = make()
    D1, D2 = R.distances(m, rad)
    S1, S2 = R.distances_stream(m, rad)
    assert np.array_equal(D1, S1) and np.array_equal(D2, S2)
    # the scan order does not matter
    order = R.disc(rad)
    np.random.RandomState(7).shuffle(order)
    P1, P2 = R.distances_stream(m, rad, order)
    assert np.array_equal(D1, P1) and np.array_equal(D2, P2)
    bld = m > 0
    assert (D1[bld] == R.NONE).all() and (D2[bld] == R.NONE).all()
    seen = D1[D1 != R.NONE]
    assert ((seen >= 1) & (seen <= rad * rad)).all() and (D2 >= D1).all()


@pytest.mark.parametrize("name", list(R.RANDOM) + ["big"])
def test_random_fixtures_have_a_second_building_in_reach_of_a_tenth_of_the_background(name):
    make, rad = R.BIG if name == "big" else R.RANDOM[name]
    m = make()
    _, D2 = R.distances(m, rad)
    share = (D2 != R.NONE).sum() / (m == 0).sum()
    print("%s: D2 set on %.1f %% of the background" % (name, 100 * share))
    assert share >= 0.10


def test_special_fixtures_are_what_their_names_say():
    D1, D2 = R.distances(*_fx("smaller_than_the_window"))
    assert (D2 == R.NONE).all() and (D1 != R.NONE).sum() == 20 - 4
    D1, D2 = R.distances(*_fx("equidistant"))
    assert D1[4, 7] == 16 and D2[4, 7] == 16 and ((D1 == D2) & (D1 != R.NONE)).sum() >= 3
    for n in ("empty", "full"):
        D1, D2 = R.distances(*_fx(n))
        assert (D1 == R.NONE).all() and (D2 == R.NONE).all()
    m, _ = _fx("straddles_four_tiles")
    assert m[31, 31] and m[31, 32] and m[32, 31] and m[32, 32] and R.components(m)[1] == 2


def _fx(name):
    make, rad = R.SPECIAL[name]
    return make(), rad


def test_border_map_values_and_bound():
    D1 = np.array([[1, 4, 16, 1024, 9, R.NONE]])
    D2 = np.array([[1, 9, 16, 1024, R.NONE, R.NONE]])
    b, bound = R.border_map(D1, D2, 10.0, 5.0)
    want = [10 * np.exp(-4 / 50), 10 * np.exp(-25 / 50), 10 * np.exp(-64 / 50), 10 * np.exp(-4096 / 50), 0.0, 0.0]
    assert np.allclose(b[0], want, rtol=1e-14, atol=0) and (b[0, 4:] == 0).all() and (bound[0, 4:] == 0).all()
    assert (bound[0, :4] > 0).all() and (bound[0, :4] <= 400 * R.U * b[0, :4] + R.TINY).all()
    # an fp32 transcription of the stated order stays inside the bound
    f = np.float32
    a1, a2 = D1[0, :4].astype(f), D2[0, :4].astype(f)
    s = (a1 + a2) + f(2) * np.sqrt(a1 * a2)
    got = f(10) * np.exp(-(s / (f(2) * (f(5) * f(5))))).astype(f)
    assert (np.abs(got.astype(np.float64) - b[0, :4]) <= bound[0, :4]).all()


def test_criterion_accepts_wce_and_refuses_bad_weights():
    from xview2_amd import criterion
    for s in ("wce", "wce+dice", "lovasz+wce", "wce+wce"):
        assert "wce" in criterion.Loss(ARGS(type="pre", loss_str=s)).names
    assert "wce" in criterion.Loss(ARGS(type="post", loss_str="wce+dice")).names
    assert criterion.Loss(ARGS(type="pre", loss_str="wce+wce")).names == ["wce", "wce"]
    # golden argument objects carry none of the new attributes: the defaults
    d = criterion.Loss(ARGS(type="post", loss_str="wce"))
    assert d.class_weights == [1.0] * 4 and d.border_weight == 0.0 and d.border_sigma == 5.0 and not d.wants_border
    a = criterion.Loss(ARGS(type="pre", loss_str="wce+dice", class_weights="1,3", border_weight=10.0, border_sigma=2.0))
    assert a.class_weights == [1.0, 3.0] and a.wants_border and a.border_radius == 6
    assert criterion.Loss(ARGS(type="pre", loss_str="wce", border_weight=1.0, border_sigma=20.0)).border_radius == 32
    assert criterion.Loss(ARGS(type="pre", loss_str="wce", border_weight=1.0, border_radius=9)).border_radius == 9
    assert not criterion.Loss(ARGS(type="pre", loss_str="dice", border_weight=1.0)).wants_border
    with pytest.raises(ValueError, match="--border_weight"):
        criterion.Loss(ARGS(type="post", loss_str="wce", border_weight=1.0))
    for bad, t in (("1,2,3", "pre"), ("1,2", "post"), ("1", "pre")):
        with pytest.raises(ValueError, match="--class_weights"):
            criterion.Loss(ARGS(type=t, loss_str="wce", class_weights=bad))
    for bad in ("1,-1", "nan,1", "inf,1", "0,0", "a,b"):
        with pytest.raises(ValueError, match="--class_weights"):
            criterion.Loss(ARGS(type="pre", loss_str="wce", class_weights=bad))
    with pytest.raises(ValueError, match="--border_sigma"):
        criterion.Loss(ARGS(type="pre", loss_str="wce", border_sigma=0.0))
    with pytest.raises(ValueError, match="--border_radius"):
        criterion.Loss(ARGS(type="pre", loss_str="wce", border_radius=33))
    with pytest.raises(ValueError, match="--border_weight"):
        criterion.Loss(ARGS(type="pre", loss_str="wce", border_weight=-1.0))
    with pytest.raises(KeyError):
        criterion.Loss(ARGS(type="pre", loss_str="wce_hard"))
    # wce composes with mse / coral no more than any other term
    for combo in ("wce+mse", "coral+wce"):
        loss = criterion.Loss(ARGS(type="post", loss_str=combo))
        with pytest.raises(RuntimeError):
            loss(torch.zeros(1, 4, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))
    # no CPU fallback: the term needs the device
    with pytest.raises(RuntimeError):
        criterion.Loss(ARGS(type="pre", loss_str="wce"))(torch.zeros(1, 2, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))


def test_cli_has_the_flags_and_their_defaults_change_nothing():
    import main as cli
    from argparse import ArgumentParser
    from tests.test_abi_cpu import test_cli_flags_match_reference_defaults
    from xview2_amd.model.plt import Model
    a = cli.build_parser().parse_args(["--type", "pre"])
    assert (a.class_weights, a.border_weight, a.border_sigma, a.border_radius) == (None, 0.0, 5.0, 0)
    b = cli.build_parser().parse_args(["--type", "pre", "--loss_str", "wce+dice", "--class_weights", "1,3", "--border_weight", "10",
                                       "--border_sigma", "2.5", "--border_radius", "7"])
    assert (b.loss_str, b.class_weights, b.border_weight, b.border_sigma, b.border_radius) == ("wce+dice", "1,3", 10.0, 2.5, 7)
    # launcher flags, not the reference's model flags; every other default is where it was
    p = Model.add_model_specific_args(ArgumentParser())
    m = p.parse_args([])
    for f in ("class_weights", "border_weight", "border_sigma", "border_radius"):
        assert not hasattr(m, f)
    assert "wce" in p.format_help()
    test_cli_flags_match_reference_defaults()
    assert (a.exec_mode, a.data, a.results, a.gpus, a.num_workers, a.batch_size, a.val_batch_size, a.precision, a.epochs,
            a.patience, a.ckpt, a.logname, a.ckpt_pre, a.seed, a.gradient_clip_val, a.skip_nonfinite, a.ema_decay,
            a.accumulate_grad_batches, a.loss_str) == (
        "train", "/data", "/results", 1, 8, 16, 13, 16, 250, 100, None, "logs", None, 1, 0.0, False, 0.0, 1, "focal+dice")
    # the parsed defaults build the loss that the golden argument objects build
    from xview2_amd import criterion
    d = criterion.Loss(a)
    assert d.names == ["focal", "dice"] and d.class_weights == [1.0, 1.0] and not d.wants_border
    from xview2_amd.utils import border_map
    v = border_map.get_parser().parse_args(["t.png", "o.npy", "--weight", "3", "--sigma", "2", "--radius", "4"])
    assert (v.weight, v.sigma, v.radius) == (3.0, 2.0, 4) and border_map.default_radius(5.0) == 15 == R.default_radius(5.0)


def test_the_symbols_are_declared_exported_and_bound():
    import ctypes
    from xview2_amd import _capi, _lib
    names = ("xv2_border_workspace", "xv2_border_distances", "xv2_border_weights", "xv2_wce_workspace", "xv2_wce_forward",
             "xv2_wce_backward")
    assert "wce.hip" in _lib.SOURCES
    protos = _capi._parse_header()
    lib = _lib.lib()
    for n in names:
        assert n in protos and n in _lib.declared_symbols() and hasattr(lib, n)
    assert len(protos["xv2_wce_forward"][1]) == 17 and len(protos["xv2_wce_backward"][1]) == 17
    assert len(protos["xv2_border_distances"][1]) == 9 and protos["xv2_border_workspace"][0] is ctypes.c_size_t
    assert _capi.query("xv2_border_workspace", 3, 37, 45) == 4 * 3 * 37 * 45
    assert _capi.query("xv2_border_workspace", 1, 1 << 15, 1 << 15) == 0 and _capi.query("xv2_border_workspace", 0, 4, 4) == 0
    assert _capi.query("xv2_wce_workspace", 2, 2, 64, 64) == 1024 * 2 * 8 and _capi.query("xv2_wce_workspace", 2, 3, 64, 64) == 0


def test_argument_errors_come_back_as_einval_with_a_message():
    from xview2_amd import _capi, _lib
    err = _lib.lib().xv2_last_error
    dist = _capi._func("xv2_border_distances")
    for rad in (0, 33):
        assert dist(None, 1, 8, 8, rad, None, None, None, None) == 1 and b"R=%d" % rad in err()
    assert dist(None, 1, 1 << 15, 1 << 15, 4, None, None, None, None) == 1 and b"2^30" in err()
    assert dist(None, 65536, 8, 8, 4, None, None, None, None) == 1 and b"B=65536" in err()
    assert dist(None, 1, 8, 8, 4, None, None, None, None) == 1 and b"null" in err()
    wmap = _capi._func("xv2_border_weights")
    assert wmap(None, None, 0, 1.0, 1.0, None, None) == 1 and b"n=0" in err()
    assert wmap(None, None, 4, -1.0, 1.0, None, None) == 1 and b"w0" in err()
    assert wmap(None, None, 4, 1.0, 0.0, None, None) == 1 and b"sigma" in err()
    fwd, bwd = _capi._func("xv2_wce_forward"), _capi._func("xv2_wce_backward")
    one = 1 << 20      # any non-null address: the checks below return before a pointer is followed
    assert fwd(None, None, 1, 3, 8, 8, 1, 0, None, None, None, 0.0, 1.0, None, None, None, None) == 1 and b"C=3" in err()
    assert fwd(None, None, 1, 4, 8, 8, 1, 1, None, one, one, 1.0, 1.0, None, None, None, None) == 1 and b"post" in err()
    assert bwd(None, None, 1, 4, 8, 8, 1, 1, None, one, one, 1.0, 1.0, None, None, None, None) == 1 and b"post" in err()
    assert fwd(None, None, 1, 2, 8, 8, 1, 0, None, one, None, 1.0, 1.0, None, None, None, None) == 1 and b"d1 and d2" in err()
    assert fwd(None, None, 1, 2, 8, 8, 1, 0, None, one, one, 1.0, -2.0, None, None, None, None) == 1 and b"sigma" in err()
    assert fwd(None, None, 1, 2, 8, 8, 0, 0, None, None, None, 0.0, 1.0, None, None, None, None) == 1 and b"lstride" in err()
    assert fwd(None, None, 65536, 2, 8, 8, 1, 0, None, None, None, 0.0, 1.0, None, None, None, None) == 1 and b"N=65536" in err()
    assert fwd(None, None, 1, 2, 8, 8, 1, 0, None, None, None, 0.0, 1.0, None, None, None, None) == 1 and b"null" in err()
