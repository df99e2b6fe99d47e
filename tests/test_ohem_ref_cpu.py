"""The fp64 restatement of ``ohem_hard`` (tests/ohem_ref.py) pinned on the CPU: the integer k, the post-style routing, that
the term is not the mean CE in disguise, the tie weights, and the host layers' handling of the new name."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ohem_ref as R
from tests.golden.cases import ARGS


def test_integer_k_equals_the_float_formula():
    for cn in range(201):
        for cp in range(121):
            assert R.k_int(cn, cp) == R.k_float(cn, cp), (cn, cp)


def test_post_style_rows_give_mean_ce():
    """behind the building mask every pixel is its own row: the one entry is kept whatever its class"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(500, 4, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, 4, (500,), generator=g)
    got = R.ohem_hard(x.reshape(500, 4, 1, 1), y.reshape(500, 1, 1))
    assert abs(float(got) - float(F.cross_entropy(x, y))) < 1e-12


def test_not_the_mean_ce_when_positives_are_few():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 2, 40, 40, generator=g, dtype=torch.float64) * 2
    y = (torch.rand(2, 40, 40, generator=g) < 0.03).to(torch.uint8)
    got = float(R.ohem_hard(x, y))
    ce = float(F.cross_entropy(x, y.long()))
    # the kept negatives are the hardest quarter: their mean loss is far above the mean over all of them
    assert got > 1.5 * ce, (got, ce)
    _, info = R.weights(*R.pixel_ce(x, y))
    for cp, cn, k, *_ in info:
        assert k == max(cn // 4, 5, 2 * cp) and k < cn


def test_tied_weights_sum_to_k_and_match_sort_without_ties():
    g = torch.Generator().manual_seed(5)
    # logits on a coarse grid: many exactly equal losses, the threshold falls inside a tied class
    x = torch.round(torch.randn(3, 2, 20, 20, generator=g, dtype=torch.float64))
    y = (torch.rand(3, 20, 20, generator=g) < 0.1).to(torch.uint8)
    l, yy = R.pixel_ce(x, y)
    w, info = R.weights(l, yy)
    tied = 0
    for i, (cp, cn, k, t, c_gt, c_eq, r) in enumerate(info):
        neg = yy[i] == 0
        assert abs(float(w[i][neg].sum()) - k) < 1e-9 and float(w[i][~neg].sum()) == cp
        assert 1 <= r <= c_eq and c_gt + c_eq >= k
        tied += c_eq > r
    assert tied > 0
    # the loss does not depend on which members of the tied class are taken: it equals the sum of the k largest
    want = sum(float(l[i][yy[i] > 0].sum() + torch.sort(l[i][yy[i] == 0], descending=True).values[:info[i][2]].sum())
               for i in range(3)) / sum(cp + k for cp, _, k, *_ in info)
    assert abs(float(R.ohem_hard(x, y)) - want) < 1e-12
    # without ties the gradient is the one autograd takes through sort
    x = (torch.randn(2, 2, 12, 12, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    y = (torch.rand(2, 12, 12, generator=g) < 0.1).to(torch.uint8)
    R.ohem_hard(x, y).backward()
    x2 = x.detach().clone().requires_grad_(True)
    l, yy = R.pixel_ce(x2, y)
    tot, cnt = 0, 0
    for i in range(2):
        pos, neg = l[i][yy[i] > 0], l[i][yy[i] == 0]
        hard = neg.sort(descending=True).values[:R.k_int(neg.numel(), pos.numel())]
        tot = tot + pos.sum() + hard.sum()
        cnt += pos.numel() + hard.numel()
    (tot / cnt).backward()
    assert float((x.grad - x2.grad).abs().max()) < 1e-15


def test_select_model_on_signed_zero_and_skips():
    bits = np.array([0x80000000, 0, 0x3f800000, 0xbf800000, 0x7f800000, 0xffc00000], dtype=np.uint32)
    assert R.select_record(bits, 1) == [0, 4, 1, 0x7f800000, 0, 1, 1, 0]
    assert R.select_record(bits, 3) == [0, 4, 3, 0, 2, 2, 1, 0]
    assert R.select_record(bits, 9)[:3] == [0, 4, 4] and R.select_record(bits, 0) == [0, 4, 0, 0, 0, 0, 0, 0]


def test_criterion_accepts_ohem_hard_and_keeps_the_unsupported_combinations():
    from xview2_amd import criterion
    for s in ("ohem_hard", "ohem_hard+dice", "focal+ohem_hard+ohem_hard"):
        assert "ohem_hard" in criterion.Loss(ARGS(type="pre", loss_str=s)).names
    with pytest.raises(KeyError):
        criterion.Loss(ARGS(type="pre", loss_str="ohem_soft"))
    for combo in ("coral+ohem_hard", "ohem_hard+mse"):
        loss = criterion.Loss(ARGS(type="post", loss_str=combo))
        with pytest.raises(RuntimeError):
            loss(torch.zeros(1, 4, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))


def test_cli_and_abi_name_the_new_term():
    from argparse import ArgumentParser
    from xview2_amd import _capi, _lib
    from xview2_amd.model.plt import Model
    p = Model.add_model_specific_args(ArgumentParser())
    assert p.parse_args(["--loss_str", "ohem_hard+dice"]).loss_str == "ohem_hard+dice"
    assert "ohem_hard" in p.format_help()
    assert "ohem.hip" in _lib.SOURCES
    protos = _capi._parse_header()
    for name in ("xv2_ohem_workspace", "xv2_ohem_forward", "xv2_ohem_backward", "xv2_topk_select"):
        assert name in protos
    # argument validation is reachable without a GPU
    assert _capi.query("xv2_ohem_workspace", 2, 1024 * 1024) == 2 * 128 * (16 + 2048 * 4)
    rc = _capi._func("xv2_ohem_forward")(None, None, 1, 3, 8, 8, 1, None, None, None, None, None, None)
    assert rc == 1 and b"C=3" in _lib.lib().xv2_last_error()
