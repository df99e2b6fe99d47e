"""The weight average without a GPU: the new ABI symbol and its argument errors, the properties of the float64
restatement (tests/ema_ref.py), and the CLI / Trainer / FlatEMA surface."""
import ctypes

import numpy as np
import torch

from tests import ema_ref


def test_the_symbol_is_declared_exported_and_bound():
    from xview2_amd import _capi, _lib
    lib = ctypes.CDLL(_lib.build())
    P, I, I64, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert "xv2_ema_update_dev" in _lib.declared_symbols() and hasattr(lib, "xv2_ema_update_dev")
    assert _capi._parse_header()["xv2_ema_update_dev"] == (I, [P, P, I64, D, I, P, P, P])


def test_argument_errors_come_back_as_einval_with_a_message():
    from xview2_amd import _capi, _lib
    f = _capi._func("xv2_ema_update_dev")
    err = _lib.lib().xv2_last_error
    buf = ctypes.create_string_buffer(64)            # (never dereferenced: every call below returns before a launch)
    a = ctypes.addressof(buf)
    cases = [((a, a, 8, -0.1, 1, a, None, None), b"decay"),
             ((a, a, 8, 1.0, 1, a, None, None), b"decay"),
             ((a, a, 8, 1.5, 0, a, None, None), b"decay"),
             ((a, a, 8, float("nan"), 1, a, None, None), b"decay"),
             ((a, a, 8, float("inf"), 1, a, None, None), b"decay"),
             ((a, a, -1, 0.9, 1, a, None, None), b"negative"),
             ((None, a, 8, 0.9, 1, a, None, None), b"null"),
             ((a, None, 8, 0.9, 1, a, None, None), b"null"),
             ((a, a, 8, 0.9, 1, None, None, None), b"null")]
    for args, word in cases:
        assert f(*args) == 1 and word in err(), (args, err())
    # nothing to average: OK without a launch, whatever the pointers
    assert f(None, None, 0, 0.9, 1, None, None, None) == 0
    assert f(None, None, 0, 0.0, 0, None, a, None) == 0


def test_equal_average_and_parameter_are_a_fixed_point_bit_for_bit():
    gen = torch.Generator().manual_seed(5)
    e = (0.1 * torch.randn(4099, generator=gen)).float()
    e[:4] = torch.tensor([0.0, -0.0, 1e-38, -3e38])
    for decay, t, warm in ((0.0, 0, False), (0.9, 0, True), (0.9, 500, True), (0.9999, 3, False)):
        om = ema_ref.om32(decay, t, warm)
        new = ema_ref.update(e, e, om)
        assert torch.equal(new, e.double())
        # bit for bit with one exception that IEEE arithmetic makes: an average of -0 comes out as +0 ((-0) - (-0) = +0 and
        # +0 + -0 = +0 under round-to-nearest) - the same value
        bits, was = new.float().view(torch.int32), e.view(torch.int32)
        assert torch.equal(bits[2:], was[2:]) and bits[:2].tolist() == [0, 0] and was[:2].tolist() == [0, -2 ** 31]
        assert float(ema_ref.bound(e, e, new, om).min()) == 0.0                         # (the zeros: nothing but the bits passes)
        assert ema_ref.check(e.clone(), e, e, om) == 0.0


def test_the_warmup_schedule_of_decay_0_9():
    for t in range(0, 200):
        want = (1.0 + t) / (10.0 + t) if t <= 80 else 0.9
        assert ema_ref.decay_at(0.9, t) == want, t
    assert ema_ref.decay_at(0.9, 79) == 80.0 / 89.0 < 0.9 < 82.0 / 91.0       # t = 80: 81 / 90, the two meet
    assert ema_ref.decay_at(0.9, 0) == 0.1 and ema_ref.om32(0.9, 0) == float(np.float32(0.9))
    for decay in (0.0, 0.9, 0.9999):
        for t in (0, 1, 80, 81, 10 ** 6):
            assert ema_ref.decay_at(decay, t, warmup=False) == decay
            assert ema_ref.om32(decay, t, warmup=False) == float(np.float32(1.0 - decay))
    # the complement is formed in double before the one rounding: 1 - float32(0.9999) would be 2.5e-9 away
    assert ema_ref.om32(0.9999, 0, False) == float(np.float32(1e-4)) != 1.0 - float(np.float32(0.9999))
    assert ema_ref.decay_at(0.0, 7) == 0.0                                    # decay 0: the average is the parameters


def test_check_rejects_what_lies_outside_the_bound_or_in_another_class():
    import pytest
    e = torch.tensor([0.5, -0.25, 1.0, 2.0])
    p = torch.tensor([0.25, 0.75, float("inf"), float("nan")])
    om = ema_ref.om32(0.9, 10 ** 3)
    good = ema_ref.update(e, p, om).float()
    assert good[2] == float("inf") and bool(torch.isnan(good[3]))
    assert ema_ref.check(good, e, p, om) <= 1.0
    for i, v in ((0, float(good[0]) * (1 + 2.0 ** -20)), (2, float("-inf")), (2, 1.0), (3, 0.0), (1, float("nan"))):
        bad = good.clone()
        bad[i] = v
        with pytest.raises(AssertionError):
            ema_ref.check(bad, e, p, om)
    # an Inf already in the average meets a finite parameter: Inf - Inf
    assert bool(torch.isnan(ema_ref.update(torch.tensor([float("inf")]), torch.tensor([1.0]), om))[0])


def test_cli_has_both_flags_off_by_default():
    import main as cli
    from argparse import ArgumentParser
    from tests.test_abi_cpu import test_cli_flags_match_reference_defaults
    from xview2_amd.model.plt import Model
    a = cli.build_parser().parse_args(["--type", "pre"])
    assert a.ema_decay == 0.0 and a.eval_ema is False
    b = cli.build_parser().parse_args(["--type", "pre", "--ema_decay", "0.999", "--eval_ema"])
    assert b.ema_decay == 0.999 and b.eval_ema is True
    # launcher flags, not the reference's model flags; every other default is where it was
    m = Model.add_model_specific_args(ArgumentParser()).parse_args([])
    assert not hasattr(m, "ema_decay") and not hasattr(m, "eval_ema")
    test_cli_flags_match_reference_defaults()
    assert (a.exec_mode, a.data, a.results, a.gpus, a.num_workers, a.batch_size, a.val_batch_size, a.precision, a.epochs,
            a.patience, a.ckpt, a.logname, a.ckpt_pre, a.seed, a.gradient_clip_val, a.skip_nonfinite) == (
        "train", "/data", "/results", 1, 8, 16, 13, 16, 250, 100, None, "logs", None, 1, 0.0, False)


def test_trainer_model_and_optim_surface():
    import inspect
    import pytest
    from xview2_amd import optim
    from xview2_amd.lightning import Model
    from xview2_amd.trainer import Trainer
    assert inspect.signature(Trainer.__init__).parameters["ema_decay"].default == 0.0
    assert inspect.signature(Model.load_from_checkpoint).parameters["ema"].default is False
    sig = inspect.signature(optim.FlatEMA.__init__).parameters
    assert list(sig)[1:] == ["optimizer", "decay", "warmup"] and sig["warmup"].default is True
    for name in ("update", "applied", "model_state_dict", "state_dict", "load_state_dict"):
        assert callable(getattr(optim.FlatEMA, name))
    with pytest.raises(TypeError):
        optim.FlatEMA(torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1), 0.9)


def test_load_from_checkpoint_raises_keyerror_naming_a_file_without_an_average(tmp_path):
    import pytest
    from xview2_amd.lightning import Model
    path = str(tmp_path / "plain.ckpt")
    torch.save({"state_dict": {}, "hyper_parameters": {"args": None}}, path)
    with pytest.raises(KeyError, match="plain.ckpt"):
        Model.load_from_checkpoint(path, ema=True)
