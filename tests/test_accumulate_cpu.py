"""Gradient accumulation without a GPU: the new ABI symbol and its argument errors, the properties of the host restatement
(tests/accum_ref.py) that pin the order of the sum, and the CLI / Trainer surface."""
import ctypes
import inspect

import pytest
import torch

from tests import accum_ref


def test_the_symbol_is_declared_exported_and_bound():
    from xview2_amd import _capi, _lib
    lib = ctypes.CDLL(_lib.build())
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert "xv2_grad_accumulate" in _lib.declared_symbols() and hasattr(lib, "xv2_grad_accumulate")
    assert _capi._parse_header()["xv2_grad_accumulate"] == (I, [P, P, I64, I, P])


def test_argument_errors_come_back_as_einval_with_a_message():
    from xview2_amd import _capi, _lib
    f = _capi._func("xv2_grad_accumulate")
    err = _lib.lib().xv2_last_error
    buf = ctypes.create_string_buffer(256)           # (never dereferenced: every call below returns before a launch)
    a = ctypes.addressof(buf)
    b = a + 128
    cases = [((a, b, -1, 0, None), b"negative"),
             ((None, b, 8, 0, None), b"null"),
             ((a, None, 8, 1, None), b"null"),
             ((None, None, 8, 2, None), b"null"),
             ((a, b, 8, -1, None), b"mode"),
             ((a, b, 8, 3, None), b"mode"),
             ((a, a, 8, 1, None), b"overlap"),                # the same array
             ((a, a + 4, 8, 2, None), b"overlap"),            # shifted by one element, either way round
             ((a + 28, a, 8, 0, None), b"overlap"),
             ((a, b, 33, 1, None), b"overlap")]               # 33 floats from a reach one element into b
    for args, word in cases:
        assert f(*args) == 1 and word in err(), (args, err())
    # nothing to add: OK without a launch, whatever the pointers
    for mode in (0, 1, 2):
        assert f(None, None, 0, mode, None) == 0
        assert f(a, a, 0, mode, None) == 0


def test_the_sum_runs_left_to_right():
    one, tiny = torch.tensor([1.0]), torch.tensor([2.0 ** -24])
    # half an ulp of 1 twice: added to 1 one at a time each is rounded away (ties to even), added first they make a whole ulp
    assert float(accum_ref.group_sum([one, tiny, tiny])[0]) == 1.0
    assert float(accum_ref.group_sum([tiny, tiny, one])[0]) == 1.0 + 2.0 ** -23 != 1.0
    assert accum_ref.group_sum([one]) is not one and float(accum_ref.group_sum([one])[0]) == 1.0


def test_the_modes_restate_the_table():
    acc, grad = torch.tensor([1.0, -0.0, 3.0, float("inf")]), torch.tensor([0.5, -0.0, float("nan"), 1.0])
    keep = (acc.clone(), grad.clone())
    a, g = accum_ref.apply(accum_ref.OPEN, acc, grad)
    assert accum_ref.same_bits(a, grad) and accum_ref.same_bits(g, grad)
    a, g = accum_ref.apply(accum_ref.ADD, acc, grad)
    assert accum_ref.same_bits(a, torch.tensor([1.5, -0.0, float("nan"), float("inf")])) and accum_ref.same_bits(g, grad)
    a, g = accum_ref.apply(accum_ref.CLOSE, acc, grad)
    assert accum_ref.same_bits(g, torch.tensor([1.5, -0.0, float("nan"), float("inf")])) and accum_ref.same_bits(a, acc)
    assert accum_ref.same_bits(acc, keep[0]) and accum_ref.same_bits(grad, keep[1])           # the inputs are left alone
    with pytest.raises(ValueError):
        accum_ref.apply(3, acc, grad)


def test_minus_zero_plus_minus_zero_keeps_its_sign_and_same_bits_sees_it():
    nz, pz = torch.tensor([-0.0]), torch.tensor([0.0])
    assert int(accum_ref.group_sum([nz, nz]).view(torch.int32)[0]) == -2 ** 31
    assert int(accum_ref.group_sum([nz, pz]).view(torch.int32)[0]) == 0
    assert torch.equal(nz, pz) and not accum_ref.same_bits(nz, pz) and accum_ref.same_bits(nz, nz)
    nan = torch.tensor([float("nan"), 1.0])
    assert accum_ref.same_bits(nan, nan.clone()) and not accum_ref.same_bits(nan, torch.tensor([1.0, 1.0]))
    assert not accum_ref.same_bits(nan, torch.tensor([float("nan"), 2.0]))


def test_cli_and_trainer_have_the_argument_with_default_1():
    import main as cli
    from argparse import ArgumentParser
    from xview2_amd.model.plt import Model
    from xview2_amd.trainer import Trainer
    a = cli.build_parser().parse_args(["--type", "pre"])
    assert a.accumulate_grad_batches == 1
    assert cli.build_parser().parse_args(["--type", "pre", "--accumulate_grad_batches", "4"]).accumulate_grad_batches == 4
    # a launcher flag, not one of the reference's model flags
    assert not hasattr(Model.add_model_specific_args(ArgumentParser()).parse_args([]), "accumulate_grad_batches")
    assert inspect.signature(Trainer.__init__).parameters["accumulate_grad_batches"].default == 1


@pytest.mark.parametrize("bad", [0, -2, 1.5, "2", None, True])
def test_trainer_refuses_anything_but_an_integer_of_at_least_1(bad):
    from xview2_amd.trainer import Trainer
    with pytest.raises(ValueError, match="accumulate_grad_batches = %s" % repr(bad).replace(".", r"\.")):
        Trainer(accumulate_grad_batches=bad)


def test_the_optimizer_and_reducer_surface():
    from xview2_amd import dist as xdist, optim
    assert callable(optim.FlatOptimizer.accumulate)
    assert inspect.signature(xdist.GradReducer.prepare).parameters["sync"].default is True


def test_mark_last_knows_the_last_batch_with_and_without_len():
    from xview2_amd.trainer import _mark_last

    def gen(n):
        return (x for x in range(n))
    for n in (0, 1, 2, 5):
        want = [(i, i, i == n - 1) for i in range(n)]
        assert list(_mark_last(list(range(n)), True)) == want
        assert list(_mark_last(gen(n), True)) == want                     # no len: one batch of look-ahead
        assert list(_mark_last(gen(n), False)) == [(i, i, False) for i in range(n)]
