"""Self-checks of tests/weights_ref.py, the bit-level restatement the weight-refresh GPU tests compare against: the properties
include/xv2.h promises of the splits and the layouts, checked on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import weights_ref as W


def _random_f32(n, seed):
    """fp32 values over the whole finite range below 0x7f7f8000 (random bit patterns) mixed with ordinary magnitudes"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    b = np.where((b & 0x7fffffff) >= 0x7f7f8000, b & np.uint32(0xbfffffff), b)
    x = W.from_bits32(b).copy()
    x[::2] = rng.standard_normal(x[::2].size).astype(np.float32)
    return x


def test_bf16_rounding_is_torchs_round_to_nearest_even():
    x = np.concatenate([W.edge_values(), _random_f32(100000, 1)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(W.bf16_bits(x), want)


def test_split3_is_exact_on_the_edge_list_and_on_random_values():
    x = np.concatenate([W.edge_values(), _random_f32(100000, 2)])
    h, m, l = W.split3(x)
    assert np.isfinite(W.bf16_value(h)).all()
    # every level is the rounding of what the previous one left
    assert np.array_equal(h, W.bf16_bits(x))
    r1 = x - W.bf16_value(h)
    assert np.array_equal(m, W.bf16_bits(r1))
    assert np.array_equal(l, W.bf16_bits(r1 - W.bf16_value(m)))
    # Three bf16 terms hold 24 significant bits, but none of them a bit below 2^-133, the smallest bf16 denormal: the split is
    # exact for every fp32 that is a multiple of 2^-133 - all of them from 2^-110 upwards, and below that those whose low bits
    # are zero - and off by at most half of 2^-133 for the rest (denormals and the smallest normals with low bits set).
    fits = np.mod(np.abs(x.astype(np.float64)) * 2.0 ** 133, 1.0) == 0
    assert fits[np.abs(x) >= 2.0 ** -110].all() and fits.sum() > 0.9 * x.size and (~fits).sum() >= 8
    assert _equal_up_to_the_sign_of_zero(W.join3(h, m, l)[fits], x[fits])
    assert not np.any(((r1 - W.bf16_value(m)) - W.bf16_value(l))[fits])          # nothing is left after the third term
    left = np.abs(W.join3(h, m, l)[~fits].astype(np.float64) - x[~fits].astype(np.float64))
    assert left.max() <= 2.0 ** -134


def _equal_up_to_the_sign_of_zero(a, b):
    """a == b as fp32 values everywhere, and bit for bit wherever the value is not zero (-0.0 splits into h = -0.0 and
    m = l = +0.0, whose fp32 sum is +0.0)"""
    a, b = W.f32(a), W.f32(b)
    nz = b != 0
    return bool((a == b).all() and np.array_equal(W.bits32(a)[nz], W.bits32(b)[nz]))


def test_split3_ties_round_to_even_at_both_levels():
    # first level: 1 + 2^-8 lies halfway between the bf16 neighbours 1 (even) and 1 + 2^-7 (odd): down; 1 + 3 * 2^-8: up
    h, m, l = W.split3(W.from_bits32(np.array([0x3f808000, 0x3f818000], dtype=np.uint32)))
    assert h.tolist() == [0x3f80, 0x3f82]
    assert W.bf16_value(m).tolist() == [2.0 ** -8, -2.0 ** -8] and not W.bf16_value(l).any()
    # second level: residuals 0x4040 and 0x40c0 (in units of 2^-23) have nine significant bits: 0x4000 (even) and 0x4100
    h, m, l = W.split3(W.from_bits32(np.array([0x3f804040, 0x3f8040c0], dtype=np.uint32)))
    assert h.tolist() == [0x3f80, 0x3f80]
    assert W.bf16_value(m).tolist() == [0x4000 * 2.0 ** -23, 0x4100 * 2.0 ** -23]
    assert W.bf16_value(l).tolist() == [0x40 * 2.0 ** -23, -0x40 * 2.0 ** -23]


@pytest.mark.parametrize("k", [-126, -100, -14, -1, 0, 1, 13, 40, 98])
def test_f16_scale_brings_the_maximum_into_2_14_to_2_15(k):
    for amax in (np.float32(2.0 ** k), np.nextafter(np.float32(2.0 ** k), np.float32(0))):
        if amax < 2.0 ** -110 or amax >= 2.0 ** 114:      # (outside the clamp: next test)
            continue
        s = W.f16_scale(W.amax_bits(amax))
        assert 2.0 ** 14 <= float(amax) * float(s) < 2.0 ** 15, (k, float(amax))


def test_f16_scale_clamps_the_exponent_at_both_ends():
    # biased exponent 16 is 2^-111, 240 is 2^113: the last maxima whose scale still follows them
    lo, hi = np.float32(2.0 ** -111), np.float32(2.0 ** 113)
    assert W.f16_scale(W.amax_bits(lo)) == np.float32(2.0 ** 125) and float(lo) * 2.0 ** 125 == 2.0 ** 14
    assert W.f16_scale(W.amax_bits(hi)) == np.float32(2.0 ** -99) and float(hi) * 2.0 ** -99 == 2.0 ** 14
    # across the clamp the scale stays: a smaller maximum lands below 2^14, a larger one above 2^15 (and past 65504: Inf planes)
    for amax in (np.nextafter(lo, np.float32(0)), np.float32(1e-36) * np.float32(1e-2), np.float32(0.0)):
        assert W.f16_scale(W.amax_bits(amax)) == np.float32(2.0 ** 125) and float(amax) * 2.0 ** 125 < 2.0 ** 14
    for amax in (np.float32(2.0 ** 114), np.float32(2.0 ** 120), np.float32(np.inf)):
        assert W.f16_scale(W.amax_bits(amax)) == np.float32(2.0 ** -99) and float(amax) * 2.0 ** -99 >= 2.0 ** 15
    h, m = W.split2h(np.float32(2.0 ** 120), W.f16_scale(W.amax_bits(np.float32(2.0 ** 120))))
    assert h.item() == 0x7c00 and m.item() == 0xfc00          # +Inf and -Inf: loud


@pytest.mark.parametrize("amax", [1.0, float(np.nextafter(np.float32(1.0), np.float32(0))), 0.7, 3.1e-5, 2.0 ** 40, 2.0 ** 113,
                                  1e-30])
def test_split2h_holds_every_element_to_2_minus_21_of_the_maximum(amax):
    rng = np.random.default_rng(3)
    x = (rng.uniform(-1, 1, 100000) * amax).astype(np.float32)
    x[:64] = (amax * 2.0 ** -np.arange(64)).astype(np.float32)          # down through the range where m runs out of bits
    x[64] = -np.float32(amax)
    x = np.clip(x, -np.float32(amax), np.float32(amax))
    s = W.f16_scale(W.amax_bits(x))
    assert 2.0 ** 14 <= float(np.float32(amax)) * float(s) < 2.0 ** 15
    h, m = W.split2h(x, s)
    err = np.abs(W.join2h(h, m, s) - x.astype(np.float64)).max()
    assert err <= 2.0 ** -21 * float(np.float32(amax)), err


def test_amax_bits_orders_like_the_values_and_ignores_the_sign():
    assert W.amax_bits(np.array([-0.0], np.float32)) == 0 and W.amax_bits(np.zeros(8, np.float32)) == 0
    assert W.amax_bits(np.array([0.5, -3.0, 2.0], np.float32)) == 0x40400000
    assert W.amax_bits(np.array([1e38, -np.inf], np.float32)) == 0x7f800000
    assert W.amax_bits(np.array([np.inf, np.nan], np.float32)) > 0x7f800000
    x = _random_f32(10000, 4)
    assert W.from_bits32(np.array([W.amax_bits(x)], np.uint32))[0] == np.abs(x).max()


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("rows,T,ctot", [(64, 9, 32), (192, 9, 96), (128, 1, 48), (64, 1, 16)])
def test_plane_image_round_trip_is_the_identity(rows, T, ctot, P):
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 1 << 16, size=(rows, T, ctot), dtype=np.uint32).astype(np.uint16) for _ in range(P)]
    img = W.plane_image(planes)
    assert img.shape == (rows * T * ctot * P,)
    back = W.plane_image_inverse(img, rows, T, ctot, P)
    assert all(np.array_equal(a, b) for a, b in zip(planes, back))
    # the image is a permutation: each plane's elements exactly once
    assert np.array_equal(np.sort(img), np.sort(np.concatenate([p.reshape(-1) for p in planes])))


def test_plane_image_places_elements_where_the_header_says():
    rows, T, ctot = 128, 9, 64
    tag = np.arange(rows * T * ctot, dtype=np.uint32).reshape(rows, T, ctot)
    img = W.plane_image([tag, tag + 10 ** 6, tag + 2 * 10 ** 6]).reshape(rows // 64, T, ctot // 16, 3, 64, 16)
    for (r, t, c, p) in [(0, 0, 0, 0), (7, 3, 5, 1), (8, 0, 0, 0), (8, 0, 8, 2), (15, 8, 63, 1), (16, 4, 17, 0), (72, 2, 40, 2),
                         (127, 8, 63, 2)]:
        rl, cl = r % 64, c % 16
        if (rl >> 3) & 1:
            cl ^= 8           # the two 8-element halves change places
        assert img[r // 64, t, c // 16, p, rl, cl] == tag[r, t, c] + p * 10 ** 6, (r, t, c, p)


@pytest.mark.parametrize("Cout,Cin,KH,KW,cin_pad", [(5, 3, 7, 7, 4), (33, 65, 3, 3, 96), (40, 24, 2, 2, 32), (8, 16, 1, 1, 16)])
def test_packed_is_permute_plus_pad(Cout, Cin, KH, KW, cin_pad):
    w = torch.randn(Cout, Cin, KH, KW, generator=torch.Generator().manual_seed(6))
    ohwi = F.pad(w.permute(0, 2, 3, 1).reshape(Cout, KH * KW, Cin), (0, cin_pad - Cin))
    ihwo = ohwi.permute(2, 1, 0).contiguous()
    for which, want in (("ohwi", ohwi), ("ihwo", ihwo)):
        got = W.packed(w.numpy(), cin_pad, which)
        assert got.shape == tuple(want.shape) and np.array_equal(W.bits32(got), W.bits32(want.numpy()))
        gotb = W.packed(w.numpy(), cin_pad, which, bf16=True)
        assert np.array_equal(gotb, want.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    pad = W.packed(w.numpy(), cin_pad, "ohwi")[:, :, Cin:]
    assert not W.bits32(pad).any()            # exactly +0.0


def test_pad_band_and_stem_band_against_torch():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 5, 7, 4, generator=g)
    want = F.pad(x, (0, 0, 3, 6, 3, 5))            # W: 3 left, 16 - 7 - 3 right; H: 3 top, 13 - 5 - 3 bottom
    got = W.pad_band(x.numpy(), 3, 3, 13, 16)
    assert np.array_equal(W.bits32(got), W.bits32(want.numpy()))
    for Cin, KH, KW in ((3, 7, 7), (4, 5, 5), (3, 7, 8)):
        w = torch.randn(5, Cin, KH, KW, generator=g)
        want = F.pad(w.permute(0, 2, 3, 1), (0, 4 - Cin, 0, 8 - KW))
        assert np.array_equal(W.bits32(W.stem_band(w.numpy())), W.bits32(want.contiguous().numpy()))
        assert np.array_equal(W.stem_band(w.numpy(), bf16=True), W.bf16_bits(want.contiguous().numpy()))


def test_every_shape_of_the_gpu_tables_is_one_the_library_supports():
    for rows, T, ctot in W.PRESPLIT_SHAPES:
        assert T == 9 and rows % 64 == 0 and ctot % 32 == 0 and W.presplit_supported(rows, T, ctot)
    for rows, T, ctot in W.PRESPLIT_F16_SHAPES:
        if T == 9:
            assert rows % 64 == 0 and ctot % 32 == 0
        else:
            assert T == 1 and rows % 64 == 0 and ctot % 16 == 0
        assert W.presplit_f16_supported(rows, T, ctot)
    # tail chunks of the table-driven pack (9 taps per tile): 1, 4, 9 and other counts, at t0 != 0 too
    chunks = {(t0, min(9, T - t0)) for T in W.PACK_TAPS for t0 in range(0, T, 9)}          # (first tap, taps) of every chunk
    assert {1, 4, 9} <= {tc for t0, tc in chunks if t0} and any(t0 and tc not in (1, 4, 9) for t0, tc in chunks)
    assert {1, 2, 4, 9} <= {tc for t0, tc in chunks if not t0}
    assert all(cp >= ci for _, ci, cp in W.PACK_GEOMS)
    assert all(not W.presplit_supported(r, T, c) for r, T, c in [(64, 1, 32), (32, 9, 32), (64, 9, 16), (64, 4, 32)])
    assert not W.presplit_f16_supported(64, 1, 8) and not W.presplit_f16_supported(64, 4, 32)


def test_the_refresh_names_its_tables_the_arena_and_every_buffer_of_every_entry():
    """ops.refresh_named_tensors() - what a captured step keeps alive - returns the very objects the cache holds (plain CPU
    tensors stand in for device memory: the function only walks the module's bookkeeping)"""
    from xview2_amd import ops
    saved = (dict(ops._packs), ops._pack_table, dict(ops._wamax))
    try:
        ops._packs.clear()
        ops._wamax.clear()
        t = lambda: torch.zeros(4)
        e = ops._PackEntry()
        e.w, e.ohwi, e.ihwo = t(), t(), None
        e.x3, e.x2 = {1: t()}, {2: (t(), 0), 3: (t(), 0)}
        bare = ops._PackEntry()
        bare.w, bare.ohwi, bare.ihwo, bare.x3, bare.x2 = t(), None, t(), None, None
        ops._packs["a"], ops._packs["b"] = e, bare
        ops._wamax[0] = [t(), 1, []]
        ops._pack_table = (t(), 2, 5, (t(), 1, 2), None, (t(), 2, 3))
        want = [ops._pack_table[0], ops._pack_table[3][0], ops._pack_table[5][0], ops._wamax[0][0], e.w, e.ohwi, e.x3[1], e.x2[2][0],
                e.x2[3][0], bare.w, bare.ihwo]
        got = ops.refresh_named_tensors()
        assert sorted(map(id, got)) == sorted(map(id, want))
        ops._pack_table = None                 # tables dropped: the entries and the arena are still named
        assert sorted(map(id, ops.refresh_named_tensors())) == sorted(map(id, want[3:]))
    finally:
        ops._packs.clear()
        ops._packs.update(saved[0])
        ops._pack_table = saved[1]
        ops._wamax.clear()
        ops._wamax.update(saved[2])
