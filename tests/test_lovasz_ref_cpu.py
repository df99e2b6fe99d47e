"""The fp64 restatement of ``lovasz`` (tests/lovasz_ref.py) pinned on the CPU: its two forms against each other, the tie rule,
the numpy models of the key encoding and of the sorted-row read-out, and the host layers' handling of the new name."""
import numpy as np
import pytest
import torch

from tests import lovasz_ref as R
from tests.golden.cases import ARGS


def _case(shape, seed, post=False, absent=None, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64) * scale
    if post:
        y = torch.randint(0, C + 1, (N, H, W), generator=g, dtype=torch.uint8)
        if absent is not None:
            y[y == absent + 1] = 0
    else:
        y = torch.randint(0, C, (N, H, W), generator=g, dtype=torch.uint8)
        if absent is not None:
            y[y == absent] = 0
    return x, y


# C = 2 with the building class alone; C = 4, every class, one absent; post with skipped pixels (and one absent class)
TIE_FREE = {"pre_c2": ((3, 2, 13, 17), 1, False, None, None), "c4_absent": ((2, 4, 16, 16), 2, False, 2, 0b1111),
            "post_skipped": ((2, 4, 16, 16), 3, True, None, None), "post_absent": ((2, 4, 12, 12), 4, True, 1, None)}


@pytest.mark.parametrize("name", sorted(TIE_FREE))
def test_sorted_and_ranked_forms_agree_without_ties(name):
    shape, seed, post, absent, mask = TIE_FREE[name]
    x, y = _case(shape, seed, post, absent)
    e, fg, valid, _ = R.errors(x, y, post)
    for c in range(shape[1]):
        assert np.unique(e[c][valid].numpy()).size == int(valid.sum()), "choose another seed: tied errors"
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    la, lb = R.lovasz_sorted(a, y, post, 1, mask), R.lovasz_ranked(b, y, post, 1, mask)
    la.backward()
    lb.backward()
    la, lb = float(la.detach()), float(lb.detach())
    assert la > 0.1
    assert abs(la - lb) <= 1e-12
    assert float((a.grad - b.grad).abs().max()) <= 1e-12
    if post:
        skipped = (y == 0).unsqueeze(1).expand_as(a.grad)
        assert skipped.any() and (a.grad[skipped] == 0).all() and (b.grad[skipped] == 0).all()
    if absent is not None:
        # an absent class is left out of the mean: the present ones are averaged over one class fewer
        present = shape[1] - 1
        e, fg, valid, _ = R.errors(x, y, post)
        tot = sum(float((e[c][valid] * torch.from_numpy(R.rank_weights(e[c][valid].numpy(), fg[c][valid].numpy()))).sum())
                  for c in range(shape[1]) if bool(fg[c].any()))
        assert abs(lb - tot / present) <= 1e-12


def test_deep_supervision_label_stride_and_empty_sets():
    x, y = _case((2, 2, 8, 8), 5)
    big = torch.zeros(2, 16, 16, dtype=torch.uint8)
    big[:, ::2, ::2] = y
    big[:, 1::2, 1::2] = 1 - y
    assert float(R.lovasz_sorted(x, big, label_stride=2)) == float(R.lovasz_sorted(x, y))
    assert float(R.lovasz_ranked(x, big, label_stride=2)) == float(R.lovasz_ranked(x, y))
    # no building pixel: no class is present, loss and gradient are 0
    for post, C in ((False, 2), (True, 4)):
        x = torch.randn(1, C, 4, 4, dtype=torch.float64).requires_grad_(True)
        for fn in (R.lovasz_sorted, R.lovasz_ranked):
            l = fn(x, torch.zeros(1, 4, 4, dtype=torch.uint8), post)
            l.backward()
            assert float(l) == 0.0 and float(x.grad.abs().max()) == 0.0


def test_tied_errors_same_loss_and_group_weights_sum_to_the_jaccard_increment():
    g = torch.Generator().manual_seed(6)
    # logits on a coarse grid: many exactly equal errors, tied groups that mix foreground and background
    x = torch.round(torch.randn(2, 2, 20, 20, generator=g, dtype=torch.float64))
    y = (torch.rand(2, 20, 20, generator=g) < 0.3).to(torch.uint8)
    assert abs(float(R.lovasz_sorted(x, y)) - float(R.lovasz_ranked(x, y))) <= 1e-12
    e, fg, valid, _ = R.errors(x, y)
    ev, f = e[1].numpy(), fg[1].numpy()
    w = R.rank_weights(ev, f)
    G = int(f.sum())
    vals = np.unique(ev)[::-1]
    assert vals.size < ev.size // 4
    prev, mixed = 0.0, 0
    for v in vals:
        F, B = int((ev[f] >= v).sum()), int((ev[~f] >= v).sum())
        jac = 1.0 - (G - F) / (G + B)
        group = ev == v
        assert abs(w[group].sum() - (jac - prev)) <= 1e-12, v
        # inside a group: every tied background weight equal; the foreground's as if it came first
        wb = w[group & ~f]
        assert wb.size == 0 or np.ptp(wb) == 0.0
        mixed += int(wb.size > 1 and (group & f).any())
        prev = jac
    assert mixed > 0 and abs(prev - 1.0) <= 1e-12
    # b = 1 reduces to (G - F_>=) / ((G + B - 1) (G + B)), B the entry's own descending rank among the background
    x, y = _case((1, 2, 9, 9), 7)
    e, fg, valid, _ = R.errors(x, y)
    ev, f = e[1].numpy(), fg[1].numpy()
    w, G = R.rank_weights(ev, f), int(f.sum())
    for i in np.nonzero(~f)[0][:20]:
        B = int((ev[~f] >= ev[i]).sum())
        fge = int((ev[f] >= ev[i]).sum())
        assert abs(w[i] - (G - fge) / ((G + B - 1) * (G + B))) <= 1e-15


def test_key_encoding_model():
    e = np.array([0.25, 0.0, -0.0, -1e-9, 1.0, np.nan, -np.nan, 1e-45, 0.5], dtype=np.float32)
    fg = np.array([0, 0, 1, 1, 1, 0, 1, 0, 1], dtype=bool)
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0], dtype=bool)
    keys = R.encode_keys(e, fg, valid)
    assert keys.tolist() == [0x3E800000, 0, 0x80000000, 0x80000000, 0xBF800000, 0x7FC00000, 0xFFC00000, 1, 0xFFFFFFFF]
    d, f, v = R.decode_keys(keys)
    assert np.array_equal(f, fg & valid) and np.array_equal(v, valid) and d[0] == 0.25 and d[4] == 1.0 and np.isnan(d[5])
    # ascending: background ascending (NaN above 1.0), foreground ascending, skipped
    s = np.sort(keys)
    bg, fgk, skipped = R.segments(s)
    assert bg.tolist() == [0, 1, 0x3E800000, 0x7FC00000] and fgk.tolist() == [0, 0, 0x3F800000, 0x7FC00000] and skipped == 1
    assert R.records(np.stack([keys, keys]), 0b01).tolist() == [[4, 4, 1, 1], [4, 4, 1, 0]]


@pytest.mark.parametrize("ties", [False, True])
def test_sorted_row_model_matches_the_ranked_form(ties):
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, 14, 14, generator=g) * 3
    if ties:
        x = torch.round(x)
    y = torch.randint(0, 5, (2, 14, 14), generator=g, dtype=torch.uint8)
    p32 = torch.softmax(x.reshape(2, 4, -1), 1).permute(1, 0, 2).reshape(4, -1).numpy()
    _, fg, valid, _ = R.errors(x, y, True)
    fg, valid = fg.numpy(), valid.numpy()
    for c in range(4):
        e32 = np.where(fg[c], np.float32(1) - p32[c], p32[c]).astype(np.float32)
        keys = R.encode_keys(e32, fg[c], valid)
        s = np.sort(keys)
        w = R.key_weights(keys, s)
        assert (w[~valid] == 0).all() and (w[fg[c]] < 0).all() and (w[valid & ~fg[c]] >= 0).all()
        e64 = e32.astype(np.float64)[valid]
        want = R.rank_weights(e64, fg[c][valid])
        assert np.abs(np.abs(w[valid]) - want).max() <= 1e-15
        assert abs(R.sorted_loss(s) - float(np.sum(e64 * want))) <= 1e-12
    # a class without foreground: no weight, no loss
    keys = R.encode_keys(np.float32([0.1, 0.2, 0.3]), np.zeros(3, bool), np.ones(3, bool))
    assert not R.key_weights(keys, np.sort(keys)).any() and R.sorted_loss(np.sort(keys)) == 0.0


def test_lattice_inputs_keep_foreground_and_background_apart():
    x, y = R.lattice_inputs((1, 2, 22, 24), 9)
    assert R.min_fg_bg_gap(x, y) >= 1e-5
    e, fg, valid, _ = R.errors(x, y)
    e32 = np.where(fg[1].numpy(), np.float32(1) - torch.softmax(x, 1)[:, 1].reshape(-1).numpy(),
                   torch.softmax(x, 1)[:, 1].reshape(-1).numpy())
    assert np.array_equal(np.argsort(e32, kind="stable"), np.argsort(e[1].numpy(), kind="stable"))


def test_criterion_accepts_lovasz_and_keeps_the_unsupported_combinations():
    from xview2_amd import criterion
    for s in ("lovasz", "lovasz+ce", "focal+lovasz", "lovasz+dice+lovasz"):
        for t in ("pre", "post"):
            assert "lovasz" in criterion.Loss(ARGS(type=t, loss_str=s)).names
    assert criterion.Loss(ARGS(type="pre", loss_str="lovasz+lovasz")).names == ["lovasz", "lovasz"]
    with pytest.raises(KeyError):
        criterion.Loss(ARGS(type="pre", loss_str="lovasz_hinge"))
    for combo in ("coral+lovasz", "lovasz+mse"):
        loss = criterion.Loss(ARGS(type="post", loss_str=combo))
        with pytest.raises(RuntimeError):
            loss(torch.zeros(1, 4, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))
    # no CPU fallback: the term needs the device
    with pytest.raises(RuntimeError):
        criterion.Loss(ARGS(type="pre", loss_str="lovasz"))(torch.zeros(1, 2, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8))


def test_cli_and_abi_name_the_new_term():
    from argparse import ArgumentParser
    from xview2_amd import _capi, _lib, ops
    from xview2_amd.model.plt import Model
    p = Model.add_model_specific_args(ArgumentParser())
    assert p.parse_args(["--loss_str", "lovasz+ce"]).loss_str == "lovasz+ce"
    assert "lovasz" in p.format_help()
    assert "sort.hip" in _lib.SOURCES and "lovasz.hip" in _lib.SOURCES
    protos = _capi._parse_header()
    for name in ("xv2_sort_workspace", "xv2_sort_u32", "xv2_lovasz_workspace", "xv2_lovasz_forward", "xv2_lovasz_backward"):
        assert name in protos
    assert len(protos["xv2_lovasz_forward"][1]) == 16
    assert ops.lovasz_class_mask(2, False) == 0b10 and ops.lovasz_class_mask(4, True) == 0b1111
    assert R.class_mask(2, False) == 0b10 and R.class_mask(4, True) == 0b1111
    # sizes and argument validation are reachable without a GPU
    M = 3 * 2048 + 17
    assert _capi.query("xv2_sort_workspace", 3, M) == 4 * (3 * M + 3 * 256 * 4 + 3 * 256)
    assert _capi.query("xv2_sort_workspace", 1, 1 << 30) == 0 and _capi.query("xv2_sort_workspace", 0, 5) == 0
    assert _capi.query("xv2_lovasz_workspace", 2, 2, 64, 64) > _capi.query("xv2_sort_workspace", 2, 2 * 64 * 64)
    err = _lib.lib().xv2_last_error
    rc = _capi._func("xv2_lovasz_forward")(None, None, 1, 3, 8, 8, 1, 0, 1, None, None, None, None, None, None, None)
    assert rc == 1 and b"C=3" in err()
    rc = _capi._func("xv2_lovasz_forward")(None, None, 1, 2, 8, 8, 1, 0, 4, None, None, None, None, None, None, None)
    assert rc == 1 and b"class_mask" in err()
    rc = _capi._func("xv2_lovasz_backward")(None, 1, 3, 8, 8, None, None, None, None, None, None, None)
    assert rc == 1 and b"C=3" in err()
    rc = _capi._func("xv2_sort_u32")(None, None, 1, 1 << 30, None, None)
    assert rc == 1 and b"2^30" in err()
