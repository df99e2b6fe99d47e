"""The gradient guard without a GPU: its float64 restatement (tests/guard_ref.py) against torch's own clip_grad_norm_,
the three new ABI symbols and their argument errors, and the CLI / Trainer surface."""
import ctypes
import math

import pytest
import torch

from tests import guard_ref

# the ragged shape set of tests/test_optimizers_gpu.py
SHAPES = [(64, 32, 3, 3), (256, 64, 1, 1), (64, 3, 7, 7), (5, 64), (64,), (7,), (16, 16), (2, 70000)]


def _grads(seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen, dtype=torch.float64) * 2.5e-4 * (i + 1) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("max_norm", [0.5, 1.1, 1e9])
def test_restatement_matches_torch_clip_grad_norm_in_float64(max_norm):
    gs = _grads()
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    want = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    norm, coef, skip = guard_ref.guard(gs, 1.0, max_norm)
    assert not skip and abs(norm - want) <= 1e-12 * want, (norm, want)
    assert 0.5 < want < 1.1 or max_norm == 0.5          # 0.5 clips, 1.1 and 1e9 do not
    if max_norm >= 1.1:
        assert coef == 1.0
    else:
        assert coef < 1.0
    for p, c in zip(ps, guard_ref.clipped(gs, coef)):
        d = float((p.grad - c).abs().max())
        assert d <= 1e-12 * float(p.grad.abs().max()), d


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_restatement_propagates_a_non_finite_element_as_torch_does(bad):
    gs = _grads()
    gs[5][3] = bad
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    want = float(torch.nn.utils.clip_grad_norm_(ps, 0.5))
    norm, coef, skip = guard_ref.guard(gs, 1.0, 0.5)
    assert not skip and (math.isnan(norm) if math.isnan(bad) else norm == want == float("inf"))
    assert math.isnan(coef) if math.isnan(bad) else coef == 0.0
    for p, c in zip(ps, guard_ref.clipped(gs, coef)):
        assert torch.equal(torch.isnan(p.grad), torch.isnan(c)) and torch.equal(p.grad.nan_to_num(), c.nan_to_num())
    assert guard_ref.guard(gs, 1.0, 0.5, skip_nonfinite=True)[2]
    assert not guard_ref.guard(_grads(), 1.0, 0.5, skip_nonfinite=True)[2]
    # the reducer's 1 / world scales the norm; max_norm = 0 never clips
    n1, n2 = guard_ref.guard(_grads(), 1.0)[0], guard_ref.guard(_grads(), 0.5)[0]
    assert abs(n2 - 0.5 * n1) <= 1e-15 * n1 and guard_ref.guard(_grads(), 1.0, 0.0)[1] == 1.0


def test_guard_symbols_are_declared_exported_and_bound():
    from xview2_amd import _capi, _lib
    lib = ctypes.CDLL(_lib.build())
    declared = _lib.declared_symbols()
    protos = _capi._parse_header()
    P, I, I64, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    want = {"xv2_grad_guard_workspace": (ctypes.c_size_t, [I64]),
            "xv2_grad_guard": (I, [P, I64, F, F, I, P, P, P]),
            "xv2_optim_guard_ctx": (I, [P])}
    for name, proto in want.items():
        assert name in declared and hasattr(lib, name), name
        assert protos[name] == proto, name
    ws = _capi.query("xv2_grad_guard_workspace", 262147)
    assert ws > 0 and ws % 8 == 0
    # one double per block, and the grid is a function of n alone
    assert _capi.query("xv2_grad_guard_workspace", 262147) == ws and _capi.query("xv2_grad_guard_workspace", 1) == 8
    assert _capi.query("xv2_grad_guard_workspace", 0) == 0


def test_guard_argument_errors_come_back_as_einval_with_a_message():
    from xview2_amd import _capi, _lib
    f = _capi._func("xv2_grad_guard")
    err = _lib.lib().xv2_last_error
    buf = ctypes.create_string_buffer(64)            # (never dereferenced: every call below fails its argument check)
    a = ctypes.addressof(buf)
    cases = [((None, 8, 1.0, 1.0, 0, a, a, None), b"null"),
             ((a, 8, 1.0, 1.0, 0, a, None, None), b"null"),
             ((a, 0, 1.0, 1.0, 0, a, a, None), b"positive"),
             ((a, -3, 1.0, 1.0, 0, a, a, None), b"positive"),
             ((a, 8, 1.0, -1.0, 0, a, a, None), b"max_norm"),
             ((a, 8, 1.0, float("inf"), 0, a, a, None), b"max_norm"),
             ((a, 8, 1.0, float("nan"), 0, a, a, None), b"max_norm"),
             ((a, 8, 1.0, 1.0, 1, None, a, None), b"workspace")]
    for args, word in cases:
        assert f(*args) == 1 and word in err(), (args, err())
    # the host-scalar AdamW entry point cannot honour a skip (its step comes from the host): it refuses a guard, and the
    # context serves that one call only
    ctx = _capi._func("xv2_optim_guard_ctx")
    assert ctx(a) == 0
    step = _capi._func("xv2_adamw_step")
    assert step(a, a, a, a, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == 1 and b"guard" in err()
    assert ctx(None) == 0


def test_cli_has_both_flags_off_by_default():
    import main as cli
    from argparse import ArgumentParser
    from xview2_amd.model.plt import Model
    a = cli.build_parser().parse_args(["--type", "pre"])
    assert a.gradient_clip_val == 0.0 and a.skip_nonfinite is False
    b = cli.build_parser().parse_args(["--type", "pre", "--gradient_clip_val", "0.5", "--skip_nonfinite"])
    assert b.gradient_clip_val == 0.5 and b.skip_nonfinite is True
    # the reference's model flags (test_cli_flags_match_reference_defaults) are untouched: the new ones are launcher flags
    m = Model.add_model_specific_args(ArgumentParser()).parse_args([])
    assert not hasattr(m, "gradient_clip_val") and not hasattr(m, "skip_nonfinite")
    assert (m.optimizer, m.lr, m.weight_decay, m.momentum, m.warmup) == ("adamw", 3e-4, 0, 0.9, 1)


def test_trainer_accepts_the_two_keywords(tmp_path):
    import inspect
    from xview2_amd.optim import FlatOptimizer
    from xview2_amd.trainer import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["gradient_clip_val"].default == 0.0 and sig["skip_nonfinite"].default is False
    for name in ("set_guard", "guard_stats"):
        assert callable(getattr(FlatOptimizer, name))
    if torch.cuda.is_available():
        t = Trainer(gpus=1, precision=32, default_root_dir=str(tmp_path), gradient_clip_val=0.5, skip_nonfinite=True)
        assert t.gradient_clip_val == 0.5 and t.skip_nonfinite is True and t.guard_log == []
