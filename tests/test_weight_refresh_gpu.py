"""The weight refresh that ends every optimizer step (ops.repack_all: xv2_pack_weights_table, xv2_presplit_table,
xv2_weight_amax_table, xv2_presplit_f16_table) and the host-side cache that drives it (ops._packs), against the bit-level
restatement tests/weights_ref.py.  Every comparison is on bit patterns: no tolerance anywhere.

A. each entry point (single-weight and table form) against the restatement, outputs as views inside poisoned allocations;
B. the cache through real optimizer steps: after every step every buffer of every entry restates the CURRENT weights, through
   table rebuilds, evictions, a deleted parameter and a second tensor over the same storage;
C. the cache is invisible: a model's loss, gradient and eval output do not change when the cache is cleared and rebuilt;
D. a captured step keeps what its recorded refresh launches name."""
import gc

import numpy as np
import pytest
import torch

from tests import weights_ref as W
from tests.test_f16x2_gpu import _prof

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (float("nan"), 2.0 ** 100)          # (2^100 is Inf in an fp16 buffer: as good a poison)
STALE = (0x7fc00000, 0x71800000)              # the same two as bit patterns, for the integer slots: above every maximum used here
SLOT_INTS = 2048                              # one tensor's maximum: 64 slots, one 128-byte line each


def _bits(t):
    """the bit patterns of a tensor as a numpy array (uint16 / uint32)"""
    t = t.detach().contiguous().cpu()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.view(torch.int32).numpy().view(np.uint32).copy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """n elements as a view inside a larger allocation (64 elements before, 192 after) that is filled with `poison` - the view
    too: what the kernel leaves unwritten shows, and so does what it writes outside"""
    PRE, POST = 64, 192

    def __init__(self, n, dtype, poison):
        self.n = n
        if dtype == torch.float16 and abs(poison) > 65504:
            poison = float("inf")                # (what 2^100 is in fp16)
        self.flat = torch.empty(self.PRE + n + self.POST, dtype=dtype, device=DEV)
        self.flat.fill_(poison)
        self.view = self.flat[self.PRE:self.PRE + n]
        self.poison = _bits(torch.full((1,), poison, dtype=dtype))[0]
        assert self.view.data_ptr() % 16 == 0

    def guards_hold(self):
        b = _bits(self.flat)
        return bool((b[:self.PRE] == self.poison).all() and (b[self.PRE + self.n:] == self.poison).all())

    def bits(self):
        return _bits(self.view)


def _both_poisons(run, poisons=POISONS):
    """run(poison) -> list of bit arrays; twice, and the two results are identical"""
    first, second = run(poisons[0]), run(poisons[1])
    assert len(first) == len(second) and all(np.array_equal(a, b) for a, b in zip(first, second))


# ================================================================================================================================
# A. entry points against the restatement

KHKW = {1: (1, 1), 2: (1, 2), 4: (2, 2), 9: (3, 3), 10: (2, 5), 13: (13, 1), 25: (5, 5), 49: (7, 7)}


def _pack_cases():
    """(Cout, Cin, T, cin_pad, bf16, which) over every tap count x geometry x element type, the wanted layouts cycling through
    both / OHWI only / IHWO only; ordered so that one-tile entries stand first, last and between many-tile ones"""
    cases, i = [], 0
    for T in W.PACK_TAPS:
        for co, ci, cp in W.PACK_GEOMS:
            for bf in (False, True):
                cases.append((co, ci, T, cp, bf, ("both", "ohwi", "ihwo")[i % 3]))
                i += 1
    tiles = lambda c: -(-c[0] // 32) * -(-c[3] // 32) * -(-c[2] // 9)
    ones, many = [c for c in cases if tiles(c) == 1], [c for c in cases if tiles(c) > 1]
    assert len(ones) >= 4 and {(c[4], c[5]) for c in cases} == {(b, w) for b in (False, True) for w in ("both", "ohwi", "ihwo")}
    order, step = [ones.pop(0)], len(many) // len(ones) + 1
    for j, c in enumerate(many):
        order.append(c)
        if j % step == step - 1 and len(ones) > 1:
            order.append(ones.pop(0))
    return order + ones


def _pack_weights(cases):
    gen = np.random.default_rng(21)
    return [gen.standard_normal((co, ci) + KHKW[T]).astype(np.float32) for co, ci, T, cp, bf, which in cases]


def _pack_outputs(cases, poison):
    outs = []
    for co, ci, T, cp, bf, which in cases:
        dt = torch.bfloat16 if bf else torch.float32
        outs.append({k: Guarded(co * T * cp, dt, poison) for k in ("ohwi", "ihwo") if which in ("both", k)})
    return outs


def _check_packs(cases, ws, outs, what):
    torch.cuda.synchronize()
    res = []
    for c, w, o in zip(cases, ws, outs):
        co, ci, T, cp, bf, which = c
        for k, g in o.items():
            want = W.packed(w, cp, k, bf)
            got = g.bits()
            assert np.array_equal(got, want.reshape(-1) if bf else W.bits32(want).reshape(-1)), (what, c, k)
            pad = got.reshape(want.shape)[:, :, ci:] if k == "ohwi" else got.reshape(want.shape)[ci:]
            assert not pad.any(), (what, c, k, "padded channels are not +0.0")
            assert g.guards_hold(), (what, c, k)
            res.append(got)
    return res


def _table_of(cases, wd, outs):
    from xview2_amd._capi import query
    rows, start = [], 0
    for (co, ci, T, cp, bf, which), w, o in zip(cases, wd, outs):
        rows.append([w.data_ptr(), o["ohwi"].view.data_ptr() if "ohwi" in o else 0, o["ihwo"].view.data_ptr() if "ihwo" in o else 0,
                     co, ci, T | ((1 if bf else 0) << 16), cp, start])
        start += query("xv2_pack_weights_tiles", co, KHKW[T][0], KHKW[T][1], cp)
    return torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), start


def test_pack_weight_single_launches_match_the_restatement():
    from xview2_amd._capi import call
    cases = _pack_cases()
    ws = _pack_weights(cases)
    wd = [_gpu(w) for w in ws]

    def run(poison):
        outs = _pack_outputs(cases, poison)
        for (co, ci, T, cp, bf, which), w, o in zip(cases, wd, outs):
            call("xv2_pack_weight", w, co, ci, KHKW[T][0], KHKW[T][1], cp, o["ohwi"].view if "ohwi" in o else None,
                 o["ihwo"].view if "ihwo" in o else None, 1 if bf else 0)
        return _check_packs(cases, ws, outs, "single")
    _both_poisons(run)


def test_pack_weights_table_one_launch_over_every_case_matches_the_restatement():
    from xview2_amd._capi import call, query
    cases = _pack_cases()
    ws = _pack_weights(cases)
    wd = [_gpu(w) for w in ws]
    ntiles = [query("xv2_pack_weights_tiles", co, KHKW[T][0], KHKW[T][1], cp) for co, ci, T, cp, bf, which in cases]
    assert ntiles[0] == 1 and ntiles[-1] == 1          # the search's first and last boundary are one-tile entries
    assert sum(1 for j in range(1, len(cases) - 1) if ntiles[j] == 1 and ntiles[j - 1] > 1 and ntiles[j + 1] > 1) >= 3

    def run(poison):
        outs = _pack_outputs(cases, poison)
        table, n, total = _table_of(cases, wd, outs)
        assert total == sum(ntiles)
        call("xv2_pack_weights_table", table, n, total)
        return _check_packs(cases, ws, outs, "table")
    _both_poisons(run)


def test_pack_weights_table_of_one_entry():
    from xview2_amd._capi import call
    cases = [(33, 65, 13, 96, False, "both")]
    ws = _pack_weights(cases)
    wd = [_gpu(w) for w in ws]

    def run(poison):
        outs = _pack_outputs(cases, poison)
        table, n, total = _table_of(cases, wd, outs)
        assert n == 1 and total == 2 * 3 * 2
        call("xv2_pack_weights_table", table, n, total)
        return _check_packs(cases, ws, outs, "n = 1")
    _both_poisons(run)


# ---- three bf16 planes ----------------------------------------------------------------------------------------------------------

# (rows, T, ctot) ordered so that 64-row entries (one block per 16-channel slice) stand on both sides of larger ones
PRESPLIT_ORDER = [(64, 9, 32), (128, 9, 32), (64, 9, 64), (192, 9, 64), (64, 9, 96), (128, 9, 96), (192, 9, 32), (128, 9, 64),
                  (192, 9, 96)]


def _presplit_sources():
    assert sorted(PRESPLIT_ORDER) == sorted(W.PRESPLIT_SHAPES)
    rng = np.random.default_rng(22)
    edges = W.edge_values()
    srcs = []
    for rows, T, ctot in PRESPLIT_ORDER:
        x = (rng.standard_normal((rows, T, ctot)) * 0.05).astype(np.float32)
        srcs.append(W.sprinkle(x, np.concatenate([edges, -edges]), rng))
    return srcs


def _check_planes(shape, g, P, want, what):
    rows, T, ctot = shape
    got = g.bits().reshape(rows // 64, T, ctot // 16, P, 64, 16)
    want = want.reshape(got.shape)
    for p in range(P):
        assert np.array_equal(got[:, :, :, p], want[:, :, :, p]), (what, shape, "plane %d" % p)
    assert g.guards_hold(), (what, shape)
    return got


def test_presplit_weights_and_table_write_the_three_planes_of_the_restatement():
    from xview2_amd._capi import call, query
    srcs = _presplit_sources()
    wants = [W.plane_image(W.split3(x)) for x in srcs]
    sd = [_gpu(x) for x in srcs]
    for table_form in (False, True):
        def run(poison):
            outs = [Guarded(r * T * c * 3, torch.bfloat16, poison) for r, T, c in PRESPLIT_ORDER]
            assert all(query("xv2_presplit_bytes", r, T, c) == 2 * g.n for (r, T, c), g in zip(PRESPLIT_ORDER, outs))
            try:
                if table_form:
                    rows, start = [], 0
                    for (r, T, c), s, g in zip(PRESPLIT_ORDER, sd, outs):
                        rows.append([s.data_ptr(), g.view.data_ptr(), r, T, c, start])
                        start += query("xv2_presplit_blocks", r, T, c)
                    call("xv2_presplit_table", torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), start)
                else:
                    for (r, T, c), s, g in zip(PRESPLIT_ORDER, sd, outs):
                        call("xv2_presplit_weights", s, r, T, c, g.view)
                torch.cuda.synchronize()
            finally:
                for s in sd:
                    query("xv2_presplit_forget", s.data_ptr())      # (xv2_presplit_weights remembers the pair)
            return [_check_planes(sh, g, 3, w, "table" if table_form else "single") for sh, g, w in zip(PRESPLIT_ORDER, outs, wants)]
        _both_poisons(run)


# ---- maxima ---------------------------------------------------------------------------------------------------------------------

def _check_slots(ints, want, what):
    """`ints`: the 2048 uint32 of one tensor's slots"""
    heads = ints.reshape(64, 32)[:, 0]
    assert int(heads.max()) == want, (what, hex(int(heads.max())), hex(want))
    assert int(ints.max()) <= want, (what, "a slot holds more than the maximum")


@pytest.mark.parametrize("n4", W.AMAX_COUNTS)
def test_tensor_amax_records_the_largest_bit_pattern(n4):
    from xview2_amd._capi import call
    n = 4 * n4
    rng = np.random.default_rng(23)
    base = (rng.random(n, dtype=np.float32) - np.float32(0.5))
    variants = {"first": (0, 3.0), "last": (n - 1, 3.0), "negative": (n // 2, -3.0), "zeros": None, "negative zeros": None}
    for name, put in variants.items():
        if put is None:
            x = np.full(n, -0.0 if name == "negative zeros" else 0.0, dtype=np.float32)
        else:
            x = base.copy()
            x[put[0]] = put[1]
        want = W.amax_bits(x)
        assert want == (0x40400000 if put else 0)
        xd = _gpu(x)

        def run(stale):
            g = Guarded(SLOT_INTS, torch.int32, stale)          # a larger stale maximum in every slot: the call lowers it
            call("xv2_tensor_amax", xd, n, g.view)
            torch.cuda.synchronize()
            _check_slots(g.bits(), want, (n4, name))
            assert g.guards_hold(), (n4, name)
            return [g.bits().reshape(64, 32)[:, 0].max(keepdims=True)]
        _both_poisons(run, STALE)


def test_weight_amax_table_keeps_every_entry_to_its_own_elements_and_slots():
    """Entries of 1, 1024 and 1025 float4 (one block, one full block, one block and one element) between neighbours with LARGER
    maxima at their first and last element, all in one allocation back to back: a block that reads past its entry, or records
    into a neighbour's slots, shows.  Slots beyond amax_bytes keep their stale content."""
    from xview2_amd._capi import call
    rng = np.random.default_rng(24)
    sizes = [300, 1, 700, 1024, 2049, 1025, 5]                    # float4 counts; odd positions are the entries under test
    peaks = [64.0, 0.5, 32.0, 0.25, 16.0, 0.125, 128.0]
    slot_of = [3, 0, 6, 1, 5, 2, 4]                               # (slots in another order than the entries)
    flat = (rng.random(4 * sum(sizes), dtype=np.float32) - np.float32(0.5)) * np.float32(0.02)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]) * 4
    for j, (o, s, p) in enumerate(zip(offs, sizes, peaks)):
        if j % 2:
            flat[o + 4 * s - 3] = -p                              # inside the last float4 of the entry's last block
        else:
            flat[o] = p
            flat[o + 4 * s - 1] = -p
    wants = [W.amax_bits(flat[o:o + 4 * s]) for o, s in zip(offs, sizes)]
    assert wants == [W.amax_bits(np.float32(p)) for p in peaks]
    xd = _gpu(flat)

    def run(stale):
        arena = Guarded(8 * SLOT_INTS, torch.int32, stale)
        rows, start = [], 0
        for o, s, k in zip(offs, sizes, slot_of):
            rows.append([xd.data_ptr() + 4 * int(o), s, arena.view.data_ptr() + 4 * SLOT_INTS * k, start])
            start += (s + 1023) // 1024
        call("xv2_weight_amax_table", torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), start, arena.view, 7 * 4 * SLOT_INTS)
        torch.cuda.synchronize()
        got = arena.bits().reshape(8, SLOT_INTS)
        for j, k in enumerate(slot_of):
            _check_slots(got[k], wants[j], ("entry", j))
        assert (got[7] == arena.poison).all(), "slots beyond amax_bytes were touched"
        assert arena.guards_hold()
        return [got[:7]]
    _both_poisons(run, STALE)


# ---- two scaled fp16 planes -----------------------------------------------------------------------------------------------------

F16_AMAX = {"2^k": 2.0 ** -3, "below 2^k": float(np.nextafter(np.float32(2.0 ** -3), np.float32(0))), "zeros": 0.0,
            "1e-36": float(np.float32(1e-36)), "2^113": 2.0 ** 113, "2^120": 2.0 ** 120}


def _f16_source(shape, amax, rng):
    x = (rng.uniform(-1, 1, shape) * amax).astype(np.float32)
    x = np.clip(x, -np.float32(amax), np.float32(amax))
    x.reshape(-1)[rng.integers(x.size)] = -amax if rng.integers(2) else amax
    return x


def _f16_want(x, kind):
    bits = W.amax_bits(x)
    assert bits == W.amax_bits(np.float32(F16_AMAX[kind]))
    img = W.plane_image(W.split2h(x, W.f16_scale(bits)))
    finite = (img & 0x7c00) != 0x7c00
    assert finite.all() if kind != "2^120" else not finite.all()      # past the clamp the planes overflow: loud, as xv2.h promises
    return bits, img


def _slots_holding(bits, where, poison):
    g = Guarded(SLOT_INTS, torch.int32, poison)
    g.view.zero_()
    g.view[32 * where] = bits                # one of the 64 slots holds the maximum: the kernels take the largest of them
    return g


def test_presplit_weights_f16_writes_the_two_scaled_planes_of_the_restatement():
    from xview2_amd._capi import call, query
    rng = np.random.default_rng(25)
    cases = [(sh, kind) for sh in W.PRESPLIT_F16_SHAPES for kind in F16_AMAX]
    srcs = [_f16_source(sh, F16_AMAX[kind], rng) for sh, kind in cases]
    wants = [_f16_want(x, kind) for x, (sh, kind) in zip(srcs, cases)]
    sd = [_gpu(x) for x in srcs]

    def run(poison):
        res = []
        for j, ((sh, kind), s, (bits, img)) in enumerate(zip(cases, sd, wants)):
            rows, T, ctot = sh
            assert query("xv2_presplit_f16_supported", rows, T, ctot) == 1
            out = Guarded(rows * T * ctot * 2, torch.float16, poison)
            assert query("xv2_presplit_f16_bytes", rows, T, ctot) == 2 * out.n
            slots = _slots_holding(bits, (7 * j + 5) % 64, STALE[0])
            before = slots.bits()
            try:
                call("xv2_presplit_weights_f16", s, rows, T, ctot, out.view, slots.view)
                torch.cuda.synchronize()
            finally:
                query("xv2_presplit_forget", s.data_ptr())
            res.append(_check_planes(sh, out, 2, img, kind))
            assert np.array_equal(slots.bits(), before) and slots.guards_hold(), (sh, kind, "the slots are read only")
        return res
    _both_poisons(run)


def test_presplit_f16_table_scales_every_entry_by_its_own_maximum():
    from xview2_amd._capi import call, query
    rng = np.random.default_rng(26)
    cases = [((64, 9, 32), "zeros"), ((128, 9, 64), "2^113"), ((64, 1, 16), "2^120"), ((128, 1, 48), "1e-36"), ((64, 9, 32), "below 2^k"),
             ((128, 9, 64), "2^k"), ((64, 1, 16), "2^k"), ((128, 1, 48), "below 2^k")]
    srcs = [_f16_source(sh, F16_AMAX[kind], rng) for sh, kind in cases]
    wants = [_f16_want(x, kind) for x, (sh, kind) in zip(srcs, cases)]
    sd = [_gpu(x) for x in srcs]

    def run(poison):
        outs = [Guarded(r * T * c * 2, torch.float16, poison) for (r, T, c), _ in cases]
        slots = [_slots_holding(bits, (11 * j + 3) % 64, STALE[1]) for j, (bits, _) in enumerate(wants)]
        rows, start = [], 0
        for ((r, T, c), _), s, g, sl in zip(cases, sd, outs, slots):
            rows.append([s.data_ptr(), g.view.data_ptr(), r, T, c, start, sl.view.data_ptr()])
            start += query("xv2_presplit_blocks", r, T, c)
        call("xv2_presplit_f16_table", torch.tensor(rows, dtype=torch.int64).to(DEV), len(rows), start)
        torch.cuda.synchronize()
        assert all(sl.guards_hold() for sl in slots)
        return [_check_planes(sh, g, 2, img, kind) for (sh, kind), g, (_, img) in zip(cases, outs, wants)]
    _both_poisons(run)


# ---- the RGB stem's band form ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True])
def test_pad_band_is_the_image_in_a_zero_frame(bf16):
    from xview2_amd._capi import call
    N, H, Wd, pad, IHp, IWp = 2, 5, 7, 3, 13, 16          # (two slack rows and three slack columns beyond the padding)
    x = np.random.default_rng(27).standard_normal((N, H, Wd, 4)).astype(np.float32)
    want = W.pad_band(x, pad, pad, IHp, IWp, bf16)
    want = want.reshape(-1) if bf16 else W.bits32(want).reshape(-1)
    xd = _gpu(x)

    def run(poison):
        g = Guarded(N * IHp * IWp * 4, torch.bfloat16 if bf16 else torch.float32, poison)
        call("xv2_pad_band", xd, N, H, Wd, pad, pad, IHp, IWp, g.view, 1 if bf16 else 0)
        torch.cuda.synchronize()
        assert np.array_equal(g.bits(), want) and g.guards_hold()
        return [g.bits()]
    _both_poisons(run)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("Cin,KH,KW", [(3, 7, 7), (4, 5, 5), (3, 7, 8)])
def test_pack_stem_band_lays_eight_pixels_of_four_channels_per_tap_row(Cin, KH, KW, bf16):
    from xview2_amd._capi import call
    Cout = 5                                              # 5 * KH * 32 elements: more than one block, the last one partial
    w = np.random.default_rng(28).standard_normal((Cout, Cin, KH, KW)).astype(np.float32)
    want = W.stem_band(w, bf16)
    want = want.reshape(-1) if bf16 else W.bits32(want).reshape(-1)
    wd = _gpu(w)

    def run(poison):
        g = Guarded(Cout * KH * 32, torch.bfloat16 if bf16 else torch.float32, poison)
        call("xv2_pack_stem_band", wd, Cout, Cin, KH, KW, g.view, 1 if bf16 else 0)
        torch.cuda.synchronize()
        assert np.array_equal(g.bits(), want) and g.guards_hold()
        return [g.bits()]
    _both_poisons(run)


# ================================================================================================================================
# B. the cache through real optimizer steps

def _need_f32x3():
    from xview2_amd import ops
    if ops.MATH_MODE != ops.MATH_F32X3:
        pytest.skip("planes and maxima are made under XV2_MATH_F32X3 only")


def _entry_matches_current_weights(key, e):
    """every buffer of one cache entry against the restatement of the fp32 weights as they are NOW; returns what the entry has"""
    from xview2_amd import ops
    _, Cout, Cin, KH, KW, cp, code = key
    w = e.w.detach().cpu().numpy().reshape(Cout, Cin, KH, KW)
    bf = code == ops.XV2_BF16
    layouts = {}
    for which, buf in (("ohwi", e.ohwi), ("ihwo", e.ihwo)):
        if buf is None:
            continue
        assert buf.dtype == (torch.bfloat16 if bf else torch.float32)
        want = W.packed(w, cp, which, bf)
        assert tuple(buf.shape) == want.shape
        assert np.array_equal(_bits(buf), want if bf else W.bits32(want)), (key, which, "packed layout is not the current weights'")
        layouts[buf.data_ptr()] = which
    amax = W.amax_bits(w)
    for ptr, planes in (e.x3 or {}).items():
        src = W.packed(w, cp, layouts[ptr])
        assert np.array_equal(_bits(planes), W.plane_image(W.split3(src))), (key, layouts[ptr], "three bf16 planes are stale")
    for ptr, (planes, slots) in (e.x2 or {}).items():
        assert slots == e.amax
        src = W.packed(w, cp, layouts[ptr])
        want = W.plane_image(W.split2h(src, W.f16_scale(amax)))
        assert np.array_equal(_bits(planes), want), (key, layouts[ptr], "two fp16 planes are stale")
    if e.amax is not None:
        arena = ops._wamax[e.w.device.index][0]
        assert (e.amax - arena.data_ptr()) % ops.AMAX_BYTES == 0
        _check_slots(_bits(arena[(e.amax - arena.data_ptr()) // ops.AMAX_BYTES]), amax, (key, "recorded maximum"))
    return (len(e.x3 or ()), len(e.x2 or ()), e.amax is not None)


def _all_entries_match():
    from xview2_amd import ops
    torch.cuda.synchronize()
    return {key: _entry_matches_current_weights(key, e) for key, e in ops._packs.items()}


#        name: (shape OIHW, cin_pad, groups)
ZOO = {"stem": ((64, 3, 7, 7), 4, 1), "c64": ((64, 64, 3, 3), 64, 1), "c128": ((192, 128, 3, 3), 128, 1), "p1x1": ((256, 64, 1, 1), 64, 1),
       "t2x2": ((64, 128, 2, 2), 128, 1), "odd": ((40, 24, 3, 3), 32, 1), "grp": ((128, 32, 3, 3), 32, 2), "late": ((128, 64, 3, 3), 64, 1)}
# (three-plane copies, two-plane copies, recorded maximum) of each layer's entries; a group's IHWO layout has 32 rows: no planes
HAS = {"f16x2": {"stem": (0, 0, False), "c64": (0, 2, True), "c128": (0, 2, True), "p1x1": (0, 2, True), "t2x2": (0, 0, True),
                 "odd": (0, 0, True), "grp": (0, 1, True), "late": (0, 2, True)},
       "x3": {n: ((2, 0, False) if n in ("c64", "c128", "late") else (1, 0, False) if n == "grp" else (0, 0, False)) for n in ZOO},
       "bf16": {n: (0, 0, False) for n in ZOO}}


@pytest.mark.parametrize("mode", ["f16x2", "x3", "bf16"])
def test_every_cached_copy_restates_the_current_weights_after_every_step(mode):
    from xview2_amd import ops
    from xview2_amd.optim import make_flat_optimizer
    _need_f32x3()
    half = mode == "bf16"
    old = ops.F16X2
    ops.clear_pack_cache()
    ops.F16X2 = mode != "x3"
    try:
        gen = torch.Generator().manual_seed(31)
        params = {n: torch.nn.Parameter((torch.randn(*shape, generator=gen) * 0.05).to(DEV)) for n, (shape, cp, G) in ZOO.items()}
        opt = make_flat_optimizer("sgd", list(params.values()), lr=1.0, weight_decay=0.0, momentum=0.0)
        code = lambda n: ops.XV2_BF16 if (half and ZOO[n][1] != 4) else ops.XV2_F32

        def views(n, t=None):
            t = params[n] if t is None else t
            G = ZOO[n][2]
            return [t] if G == 1 else [t[g * (t.shape[0] // G):(g + 1) * (t.shape[0] // G)] for g in range(G)]

        def keys(n):
            return [(v.data_ptr(),) + tuple(v.shape) + (ZOO[n][1], code(n)) for v in views(n)]

        def use(names):
            for n in names:
                for v in views(n):          # (a grouped layer is packed as the views of its groups, as _conv_forward does it)
                    ops._pack(v, ZOO[n][1], True, True, half)

        def check(present):
            got = _all_entries_match()
            assert set(got) == {k for n in present for k in keys(n)} | extra_keys, (mode, sorted(present))
            for n in present:
                assert all(got[k] == HAS[mode][n] for k in keys(n)), (mode, n, [got[k] for k in keys(n)])

        exps = {n: [] for n in params}

        def step(c):
            """SGD with lr 1 on the gradient c * w: w <- (1 - c) * w, 2.5 w or 0.4 w - each weight's maximum crosses a power of two"""
            opt.zero_grad()
            opt.flat_g.copy_(opt.flat_p * c)
            opt.step()
            torch.cuda.synchronize()
            for n, p in params.items():
                exps[n].append(int(torch.floor(torch.log2(p.detach().abs().max())).item()))

        extra_keys = set()
        base = [n for n in ZOO if n != "late"]
        step(0.0)                                         # (records the starting exponents; nothing is cached yet)
        use(base)
        check(base)                                       # first packs: the single-weight launches
        step(-1.5)
        check(base)
        use(base)
        step(0.6)
        check(base)
        use(base + ["late"])                              # a layer packed for the first time: the tables are rebuilt
        assert ops._pack_table is None
        check(base + ["late"])
        step(0.6)
        assert ops._pack_table is not None
        check(base + ["late"])
        use([n for n in ZOO if n != "p1x1"])              # one layer sits out a whole step ...
        step(-1.5)
        assert not any(k in ops._packs for k in keys("p1x1")), "a layer not touched since the last refresh is evicted"
        check([n for n in ZOO if n != "p1x1"])
        use(list(ZOO))                                    # ... and is fresh when it is used again
        check(list(ZOO))
        gone = torch.nn.Parameter((torch.randn(64, 64, 3, 3, generator=gen) * 0.05).to(DEV))      # a parameter that goes away
        ops._pack(gone, 64, True, True, half)
        gone_key = (gone.data_ptr(), 64, 64, 3, 3, 64, ops.XV2_BF16 if half else ops.XV2_F32)
        extra_keys = {gone_key}
        check(list(ZOO))
        del gone
        gc.collect()
        assert gone_key in ops._packs                     # (touched since the last refresh: only the dead owner removes it)
        step(0.6)
        extra_keys = set()
        assert gone_key not in ops._packs
        check(list(ZOO))
        use(list(ZOO))
        # a second tensor object over the same storage and shape, other values written through it: its own pack, never the cached one
        p = params["c64"]
        cached = ops._packs[keys("c64")[0]]
        cached_ohwi = cached.ohwi
        alias = torch.empty(0, device=DEV).set_(p.untyped_storage(), p.storage_offset(), p.shape, p.stride())
        alias.copy_((torch.randn(*p.shape, generator=gen) * 0.07).to(DEV))
        assert alias.data_ptr() == p.data_ptr() and cached.version == p._version       # (the parameter's own counter saw nothing)
        ohwi, ihwo = ops._pack(alias, 64, True, True, half)
        mine = ops._packs[keys("c64")[0]]
        assert mine is not cached and ohwi is not cached_ohwi and mine.owner() is alias
        want = W.packed(alias.cpu().numpy(), 64, "ohwi", half)
        assert np.array_equal(_bits(ohwi), want if half else W.bits32(want))
        check(list(ZOO))
        use(list(ZOO))                                    # the parameter again: again a pack of its own
        assert ops._packs[keys("c64")[0]].owner() is p
        check(list(ZOO))
        step(-1.5)
        check(list(ZOO))
        for n in base:                                    # every step moved every maximum across a power of two, both ways
            d = np.diff(exps[n])
            assert (d != 0).all() and (d > 0).any() and (d < 0).any(), (n, exps[n])
    finally:
        ops.clear_pack_cache()
        ops.F16X2 = old


def test_two_refreshes_without_a_forward_between_them_empty_the_cache():
    """Pinned, not a defect: 'not touched since the last refresh' also holds for every entry at a second refresh that follows the
    first directly - an optimizer step followed by FlatEMA's swap.  The cache is then empty and the next forward packs every
    layer afresh, from the weights as they are."""
    from xview2_amd import ops
    ops.clear_pack_cache()
    try:
        gen = torch.Generator().manual_seed(32)
        ws = [(torch.randn(64, 64, 3, 3, generator=gen) * 0.05).to(DEV), (torch.randn(256, 64, 1, 1, generator=gen) * 0.05).to(DEV)]
        for w in ws:
            ops._pack(w, 64, True, True, False)
        ops.weights_changed()
        ops.repack_all()
        assert len(ops._packs) == 2 and ops._pack_table is not None          # touched before the first refresh: kept
        for w in ws:
            w.mul_(3.0)
        ops.weights_changed()
        ops.repack_all()
        assert not ops._packs and ops._pack_table is None                    # not touched since: evicted, all of them
        for w in ws:
            ops._pack(w, 64, True, True, False)
        assert len(_all_entries_match()) == 2
    finally:
        ops.clear_pack_cache()


# ================================================================================================================================
# C. the cache must be invisible to the kernels

def _unet(encoder, **kw):
    from tests.golden.cases import ARGS, labels, model_input
    from xview2_amd import criterion, networks
    from xview2_amd.optim import make_flat_optimizer
    from xview2_amd.weights import deterministic_init_
    a = ARGS(encoder=encoder, **kw)
    torch.manual_seed(0)
    m = networks.UNetLoc(a)
    deterministic_init_(m, 1)
    m.cuda().train()
    opt = make_flat_optimizer("adamw", m.parameters(), lr=1e-3, weight_decay=1e-2)
    return a, m, opt, criterion.Loss(a), model_input(a).cuda(), labels(a).cuda()


def _three_passes(a, m, opt, lf, x, y):
    """training forward + backward, then an eval forward: (loss, flat_g, eval output, kernel names)"""
    from xview2_amd import criterion, ops
    with _prof() as pr:
        m.train()
        opt.zero_grad()
        loss = criterion.compute_loss(lf, m(x), y, a.deep_supervision)
        loss.backward()
        ops.join_wgrad_stream()
        opt._gather_foreign_grads()
        m.eval()
        with torch.no_grad():
            out = m(x)
        m.train()
        names = pr.names()
    out = out[0] if isinstance(out, (tuple, list)) else out
    return loss.detach().clone(), opt.flat_g.clone(), out.detach().clone(), names


def _same_with_and_without_the_cache(a, m, opt, lf, x, y):
    from xview2_amd import ops
    saved = {k: v.detach().clone() for k, v in m.named_buffers()}
    first = _three_passes(a, m, opt, lf, x, y)
    assert ops._packs
    ops.clear_pack_cache()
    assert not ops._packs
    with torch.no_grad():
        for k, v in m.named_buffers():
            v.copy_(saved[k])
    ops.bn_stats_changed()
    second = _three_passes(a, m, opt, lf, x, y)
    for names in (first[3], second[3]):      # both plane-reading forms ran (else the equality below says nothing about planes)
        assert any("f16x2,halo,wx2>" in n for n in names), sorted(set(names))
        assert any(n.startswith("sg_conv_kernel<") and "f16x2" in n for n in names), sorted(set(names))
    assert first[3] == second[3]
    assert torch.isfinite(first[0]) and torch.equal(first[0], second[0]), "loss"
    assert torch.equal(first[1], second[1]), "gradient"
    assert torch.equal(first[2], second[2]), "eval output"


def _need_f16x2():
    from xview2_amd import ops
    if ops.MATH_MODE != ops.MATH_F32X3 or not ops.F16X2:
        pytest.skip("the plane-reading kernels run under XV2_MATH_F32X3 with F16X2 on")


@pytest.mark.parametrize("encoder", ["resnet50", "resnest50"])
def test_refreshed_copies_and_copies_built_from_scratch_give_the_same_passes(encoder):
    _need_f16x2()
    a, m, opt, lf, x, y = _unet(encoder, loss_str="ce")
    for _ in range(3):
        opt.zero_grad()
        lf(m(x), y).backward()
        opt.step()
    _same_with_and_without_the_cache(a, m, opt, lf, x, y)


def _graphed(a, m, opt, lf, x, y):
    from xview2_amd import criterion
    from xview2_amd.graph import GraphedStep

    def step():
        opt.zero_grad()
        loss = criterion.compute_loss(lf, m(x), y, True)
        loss.backward()
        opt.step()
        return loss
    return step, GraphedStep(step, opt, [], warmup=2)


def test_after_graph_replays_the_eager_passes_do_not_depend_on_the_cache():
    _need_f16x2()
    a, m, opt, lf, x, y = _unet("resnet50", deep_supervision=True)
    step, g = _graphed(a, m, opt, lf, x, y)
    for _ in range(3):
        g()
    torch.cuda.synchronize()
    _same_with_and_without_the_cache(a, m, opt, lf, x, y)          # (the graph is not replayed again: it keeps what it names anyway)
    del g


# ================================================================================================================================
# D. a captured refresh names tables, arena and buffers by address: the graph keeps them

def _named_by_the_refresh():
    from xview2_amd import ops
    table, _, _, xt, at, ht = ops._pack_table
    named = [table] + [t[0] for t in (xt, at, ht) if t is not None] + [a[0] for a in ops._wamax.values()]
    for e in ops._packs.values():
        named += [t for t in (e.ohwi, e.ihwo) if t is not None] + list((e.x3 or {}).values()) + [v[0] for v in (e.x2 or {}).values()]
    return named


def test_a_captured_step_owns_what_its_refresh_launches_name():
    from xview2_amd import ops
    _need_f16x2()
    a, m, opt, lf, x, y = _unet("resnet50", deep_supervision=True)
    step, g = _graphed(a, m, opt, lf, x, y)
    assert ops._pack_table is not None and ops._pack_table[4] is not None and ops._pack_table[5] is not None
    named = _named_by_the_refresh()
    assert len(named) > 4 + len(ops._packs)
    ops._invalidate_pack_table()
    assert ops._pack_table is None
    kept = {id(t) for t in g._refresh_keep}
    assert all(id(t) in kept for t in named), "the graph does not hold every tensor its refresh launches name"
    ptrs = {t.data_ptr() for t in g._refresh_keep}
    assert all(t.data_ptr() in ptrs for t in named)
    del g


def test_replays_after_a_table_rebuild_equal_the_eager_steps():
    """An unrelated weight packed after the capture drops the module's tables (and the next eager refresh builds new ones); the
    graph still owns the ones its launches name, so two more replays give the eager run's parameters bit for bit."""
    from xview2_amd import ops
    _need_f16x2()
    res = {}
    for mode in ("eager", "graph"):
        a, m, opt, lf, x, y = _unet("resnet50", deep_supervision=True)
        step, g = _graphed(a, m, opt, lf, x, y) if mode == "graph" else (None, None)
        if mode == "eager":
            from xview2_amd import criterion
            for _ in range(4):
                opt.zero_grad()
                criterion.compute_loss(lf, m(x), y, True).backward()
                opt.step()
        else:
            assert ops._pack_table is not None
            other = (torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(41)) * 0.05).to(DEV)
            ops._pack(other, 64, True, True, False)
            assert ops._pack_table is None
            g()
            g()
        torch.cuda.synchronize()
        res[mode] = opt.flat_p.clone()
        del g
    assert torch.isfinite(res["eager"]).all() and torch.equal(res["eager"], res["graph"])
