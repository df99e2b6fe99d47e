"""``ops.sort_u32`` (csrc/sort.hip) against ``np.sort``, row by row, bit for bit.

Sizes: around one wave, one 256-key step and one 2048-key tile, several tiles with a ragged end, and one row long enough
(more than 1024 tiles) that a block walks several tiles.  Patterns: random full-range keys, all equal, sorted, reversed, keys
that differ in one digit only (each of the four), keys equal in the low digits and different above (wrong unless every pass
is stable), and the extreme keys."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 2048
MAX_BLOCKS = 1024
SIZES = [1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
WALK = 2 * MAX_BLOCKS * TILE + 3 * TILE + 5          # 3 tiles per block, the last block short
POISON = 0x5A5A5A5A


def dev():
    return torch.device("cuda:0")


def patterns(R, M, seed):
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 1 << 32, (R, M), dtype=np.uint64).astype(np.uint32)
    out = {"random": full, "equal": np.full((R, M), 0xDEADBEEF, dtype=np.uint32)}
    out["sorted"] = np.sort(full, axis=1)
    out["reversed"] = out["sorted"][:, ::-1].copy()
    for d in range(4):
        digit = rng.integers(0, 256, (R, M), dtype=np.uint64).astype(np.uint32) << np.uint32(8 * d)
        out["digit%d" % d] = (np.uint32(0x9C3A65F1) & ~(np.uint32(0xFF) << np.uint32(8 * d))) | digit
    # few distinct low halves under random high halves: a pass that reorders equal digits breaks the low halves' order
    low = rng.choice(np.array([0, 1, 0x100, 0xFFFF], dtype=np.uint32), (R, M))
    out["stability"] = (rng.integers(0, 7, (R, M), dtype=np.uint64).astype(np.uint32) << np.uint32(16 + 8 * (seed % 2))) | low
    ext = full.copy()
    ext[:, ::3] = 0
    ext[:, 1::3] = 0xFFFFFFFF
    out["extremes"] = ext
    return out


def gpu_sort(keys):
    from xview2_amd import ops
    t = torch.from_numpy(keys.view(np.int32).copy()).to(dev())
    out = ops.sort_u32(t)
    assert out.shape == t.shape and out.dtype == t.dtype
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("M", SIZES)
def test_every_pattern_equals_numpy(M, R):
    for name, keys in patterns(R, M, 31 * M + R).items():
        got = gpu_sort(keys)
        assert np.array_equal(got, np.sort(keys, axis=1)), (name, M, R)


@pytest.mark.parametrize("R", [1, 3])
def test_a_block_walks_several_tiles(R):
    rng = np.random.default_rng(5 + R)
    keys = rng.integers(0, 1 << 32, (R, WALK), dtype=np.uint64).astype(np.uint32)
    keys[:, ::5] &= np.uint32(0xFFFF0003)          # long runs of equal low digits across tile and block borders
    got = gpu_sort(keys)
    assert np.array_equal(got, np.sort(keys, axis=1))


def test_one_dimensional_and_uint32_inputs():
    from xview2_amd import ops
    keys = np.random.default_rng(6).integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(gpu_sort(keys), np.sort(keys))
    t = torch.from_numpy(keys.view(np.int32).copy()).to(dev()).view(torch.uint32)
    out = ops.sort_u32(t)
    assert out.dtype == torch.uint32 and np.array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), np.sort(keys))
    with pytest.raises(TypeError):
        ops.sort_u32(torch.zeros(4, device=dev()))


@pytest.mark.parametrize("R,M", [(1, 257), (3, TILE + 1), (2, 3 * TILE + 17)])
def test_guard_bands_input_and_repeat(R, M):
    """poisoned bands around the output and the workspace stay untouched, the input is left alone, a second call and an
    in-place call give the same bits"""
    from xview2_amd import _capi
    from xview2_amd._capi import Ptr
    G = 1024
    keys = np.random.default_rng(7 + M).integers(0, 1 << 32, (R, M), dtype=np.uint64).astype(np.uint32)
    want = np.sort(keys, axis=1).reshape(-1)
    src = torch.from_numpy(keys.view(np.int32).copy()).to(dev())
    nws = (_capi.query("xv2_sort_workspace", R, M) + 3) // 4
    runs = []
    for _ in range(2):
        out = torch.full((R * M + 2 * G,), POISON, dtype=torch.int32, device=dev())
        ws = torch.full((nws + 2 * G,), POISON, dtype=torch.int32, device=dev())
        _capi.call("xv2_sort_u32", src, Ptr(out, G), R, M, Ptr(ws, G))
        torch.cuda.synchronize()
        o, w = out.cpu().numpy(), ws.cpu().numpy()
        assert (o[:G] == POISON).all() and (o[G + R * M:] == POISON).all(), "output guard bands"
        assert (w[:G] == POISON).all() and (w[G + nws:] == POISON).all(), "workspace guard bands"
        assert np.array_equal(o[G:G + R * M].view(np.uint32), want)
        runs.append(o)
    assert np.array_equal(runs[0], runs[1])
    assert np.array_equal(src.cpu().numpy().view(np.uint32), keys)
    ws = torch.empty((nws,), dtype=torch.int32, device=dev())
    _capi.call("xv2_sort_u32", src, src, R, M, ws)
    assert np.array_equal(src.cpu().numpy().view(np.uint32).reshape(-1), want)
