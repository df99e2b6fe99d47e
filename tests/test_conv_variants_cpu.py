"""CPU side of the convolution variant matrix (tests/test_conv_variants_gpu.py) and of its gates (tests/conv_ref.py):
- the gates have teeth: torch's fp32 convolution passes both, and each of three plausible kernel faults fails one;
- the variant table is complete: it lists exactly the kernel instantiations of the convolution sources (the rows of the
  weight-gradient kernel table among them), under the names the library registers, and the cases name every entry that is not
  ablation-only."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xview2_amd", "csrc")
CONV_SOURCES = ("igemm_conv.hip", "wgrad_conv.hip", "sg_conv.hip", "thin_conv.hip", "direct_conv.hip", "stem_conv.hip")


# ---- the gates have teeth ---------------------------------------------------------------------------------------------

SHAPES = [  # N, H, W, Cin, Cout, k, stride, pad, dil
    (2, 12, 10, 64, 64, 3, 1, 1, 1),
    (2, 17, 15, 96, 128, 3, 2, 1, 1),
    (2, 9, 13, 128, 64, 1, 1, 0, 1),
    (1, 14, 14, 64, 96, 3, 1, 2, 2),
]


def _problem(shape):
    N, H, W, Ci, Co, k, s, p, d = shape
    gen = torch.Generator().manual_seed(Ci * 1000 + Co + k)
    x = R.lognormal((N, H, W, Ci), gen)
    w = (torch.randn((Co, Ci, k, k), generator=gen) / math.sqrt(Ci * k * k)).float()
    f = lambda A, B: R.conv_fwd(A, B, s, p, d)
    y64 = f(x, w)
    a, sc = R.scales(f, x, w)
    return x, w, f, y64, a, sc, Ci * k * k


def _fp32(x, w, shape):
    """torch's own fp32 convolution: a correct fp32-class result"""
    _, _, _, _, _, _, s, p, d = shape
    return R.nhwc(F.conv2d(R.nchw(x), w, None, s, p, d)).double()


def _gates(y, y64, a, sc, K, mode, w, x):
    return R.check(y, y64, a, sc, K, mode, amax=(float(x.abs().max()), float(w.abs().max())))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_correct_fp32_convolution_passes_both_gates(shape):
    x, w, f, y64, a, sc, K = _problem(shape)
    y = _fp32(x, w, shape)
    for mode in ("f32", "f32x3", "f16x2"):
        r = _gates(y, y64, a, sc, K, mode, w, x)
        assert r["ok"], (mode, r)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_operands_truncated_to_16_significant_bits_fail(shape):
    """a three-plane kernel that lost its third plane: 16 significant bits per operand"""
    x, w, f, y64, a, sc, K = _problem(shape)
    trunc = lambda t: (t.contiguous().view(torch.int32) & ~0xff).view(torch.float32)
    y = _fp32(trunc(x), trunc(w), shape)
    for mode in ("f32", "f32x3", "f16x2"):
        r = _gates(y, y64, a, sc, K, mode, w, x)
        assert not r["ok"], (mode, r)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_32_channel_k_slice_missing_from_one_64_row_tile_fails(shape):
    x, w, f, y64, a, sc, K = _problem(shape)
    y = _fp32(x, w, shape)
    k = w.shape[2]
    ws = torch.zeros_like(w)
    ws[:, 32:64, k // 2, k // 2] = w[:, 32:64, k // 2, k // 2]         # one K tile: 32 channels of one tap
    part = f(x, ws)
    M, Co = y.numel() // y.shape[-1], y.shape[-1]
    assert M > 128
    yf = y.reshape(M, Co).clone()
    yf[64:128] -= part.reshape(M, Co)[64:128]
    for mode in ("f32", "f32x3", "f16x2"):
        r = _gates(yf.reshape(y.shape), y64, a, sc, K, mode, w, x)
        assert not r["ok"] and r["el"] > 1.0, (mode, r)
        assert 64 <= r["where"] // Co < 128


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_tap_missing_on_the_image_border_only_fails(shape):
    x, w, f, y64, a, sc, K = _problem(shape)
    y = _fp32(x, w, shape)
    k = w.shape[2]
    wt = torch.zeros_like(w)
    wt[:, :, k // 2, k // 2] = w[:, :, k // 2, k // 2]
    part = f(x, wt)
    OH, OW = y.shape[1], y.shape[2]
    border = torch.zeros((OH, OW), dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    yf = torch.where(border[None, :, :, None], y - part, y)
    for mode in ("f32", "f32x3", "f16x2"):
        r = _gates(yf, y64, a, sc, K, mode, w, x)
        assert not r["ok"] and r["el"] > 1.0, (mode, r)


def test_bf16_storage_gate_takes_the_output_rounding_and_nothing_more():
    """bf16 storage: operands rounded by the test, so the correctly rounded result passes and a result rounded more
    coarsely (7 significant bits) fails"""
    x, w, f, _, _, _, K = _problem(SHAPES[0])
    xb, wb = x.bfloat16().float(), w.bfloat16().float()
    y64 = f(xb, wb)
    a, sc = R.scales(f, xb, wb)
    good = R.bf16_round(_fp32(xb, wb, SHAPES[0]))
    assert R.check(good, y64, a, sc, K, "bf16", bf16_out=True)["ok"]
    coarse = (good.float().contiguous().view(torch.int32) & ~0x1ffff).view(torch.float32)
    assert not R.check(coarse, y64, a, sc, K, "bf16", bf16_out=True)["ok"]


# ---- the variant table is complete ------------------------------------------------------------------------------------

_MACROS = ("XV2_IGEMM_TILES", "XV2_THIN_CASE", "XV2_SG_CASE")      # macros whose expansions launch kernels (igemm_conv.hip, thin_conv.hip, sg_conv.hip)
# enum Form of igemm_kernel.h -> the form's part of the registered name (restating FORM_TRAITS there)
_IGEMM_FORMS = {"RGB": "rgb", "RGB_BF16OUT": "rgb,bf16out", "C32": "c32", "BF16": "c32,bf16", "BF16HBM": "c32,bf16hbm",
                "BF16HBM_HALO": "c32,bf16hbm,halo", "F32X3": "c32,f32x3", "F32X3_HALO": "c32,f32x3,halo",
                "F32X3_HALO_WX3": "c32,f32x3,halo,wx3", "F16X2": "c32,f16x2", "F16X2_HALO": "c32,f16x2,halo,wx2"}


def expand_launch_macros(t):
    """the text with the definitions of _MACROS replaced by nothing and their invocations by their expansions (parameters
    substituted, #param stringified, adjacent string literals joined)"""
    t = t.replace("\\\n", " ")
    for name in _MACROS:
        m = re.search(r"#define\s+%s\(([^)]*)\)([^\n]*)\n" % name, t)
        if not m:
            continue
        params = [p.strip() for p in m.group(1).split(",")]
        body = m.group(2)
        t = t[:m.start()] + "\n" + t[m.end():]

        def expand(inv, params=params, body=body):
            args = [a.strip() for a in inv.group(1).split(",")]
            out = body
            for p, v in zip(params, args):
                out = re.sub(r"#\s*%s\b" % p, '"%s"' % v, out)
                out = re.sub(r"\b%s\b" % p, v, out)
            return re.sub(r'"\s+"', "", out)
        t = re.sub(r"\b%s\(([^()]*)\)" % name, expand, t)
    return t


def _top_level_args(s):
    """s split at the commas outside ( ) and < >"""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "(<"
        depth -= ch in ")>"
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def source_variants(texts):
    """keys of VARIANTS found in the given source texts -> the profiler name each registers (None: derived from the template
    arguments, registered_name())"""
    keys = {}
    for t in texts:
        t = expand_launch_macros(t)
        for m in re.finditer(r"\b(launch_one|sg_launch_one)<([^<>]*)>\s*\(", t):
            keys["%s<%s>" % (m.group(1), ",".join(a.strip() for a in m.group(2).split(",")))] = None
        for m in re.finditer(r'^\s*XV2_WGRAD_ROW\(\s*"([^"]*)"\s*,(.*)\)\s*$', t, flags=re.M):      # (NAME, ..., kernel): a table row
            keys["XV2_WGRAD_ROW(%s)" % _top_level_args(m.group(2))[-1].replace(" ", "")] = m.group(1)
        for m in re.finditer(r'\bthin_launch_one<([^<>]*)>\s*\(\s*q\s*,\s*"([^"]*)"', t):
            keys["thin_launch_one<%s>" % ",".join(a.strip() for a in m.group(1).split(","))] = m.group(2)
        for m in re.finditer(r'\bprof_register\("([^"]*)"\)', t):
            keys['prof_register("%s")' % m.group(1)] = m.group(1)
    return keys


def _texts():
    return [open(os.path.join(CSRC, f)).read() for f in CONV_SOURCES]


def registered_name(key):
    """the profiler name the library registers for a VARIANTS key whose name is built from its template arguments
    (restating launch_one / sg_launch_one of igemm_conv.hip / sg_conv.hip)"""
    m = re.match(r"(launch_one|sg_launch_one)<(.*)>$", key)
    a = m.group(2).split(",")
    t = lambda i, dflt: (a[i] == "true") if i < len(a) else dflt
    if m.group(1) == "launch_one":
        form, BM, BN = a
        WGM, WGN = ("4", "1") if BN == "32" else ("2", "2")      # waves of a block along M x N: a function of the tile
        return "igemm_kernel<%s,%s,%s,%s,%s>" % (BM, BN, WGM, WGN, _IGEMM_FORMS[form[len("Form::"):]])
    WM, G, NB = (int(v) for v in a[:3])
    return "sg_conv_kernel<%d,%d,g%d,%s%s>" % (32 * WM, 32 * NB, G, "1x1," if t(3, False) else "", "bf16hbm" if t(4, False) else "f16x2")


def test_variant_table_lists_exactly_the_instantiations_of_the_conv_sources():
    from tests.test_conv_variants_gpu import VARIANTS
    src = set(source_variants(_texts()))
    assert len(src) >= 112
    assert set(VARIANTS) == src, ("in the sources, not in VARIANTS: %s" % sorted(src - set(VARIANTS)),
                                  "in VARIANTS, not in the sources: %s" % sorted(set(VARIANTS) - src))


def test_an_added_instantiation_is_caught():
    from tests.test_conv_variants_gpu import VARIANTS
    texts = _texts()
    texts[0] += "\n    return launch_one<Form::F32X3, 64, 32>(p, stream);\n"
    texts[3] = texts[3].replace("    XV2_THIN_CASE(64, 64)\n", "    XV2_THIN_CASE(64, 64)\n    XV2_THIN_CASE(32, 64)\n")
    texts[2] = texts[2].replace("        XV2_SG_CASE(242, 2, 4, 2)\n", "        XV2_SG_CASE(242, 2, 4, 2)\n        XV2_SG_CASE(222, 2, 2, 2)\n")
    texts[1] = texts[1].replace("#undef XV2_WGRAD_ROW\n", '    XV2_WGRAD_ROW("wgrad_kernel<64,32,2,1,2,c32,bf16hbm>", C32_BF16HBM, 64, 32, '
                                "tiled_lds(64, 32), 2, 2, X_IN, wgrad_kernel<WForm::C32_BF16HBM, 64, 32>)\n#undef XV2_WGRAD_ROW\n")
    added = set(source_variants(texts)) - set(VARIANTS)
    assert added == {"launch_one<Form::F32X3,64,32>", "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32_BF16HBM,64,32>)", "thin_launch_one<32,64,true,2,2>",
                     "thin_launch_one<32,64,false,4,4,0,2>", "thin_launch_one<32,64,false,4,4>",
                     "sg_launch_one<2,2,2,true,true>", "sg_launch_one<2,2,2,false,true>", "sg_launch_one<2,2,2,true,false>",
                     "sg_launch_one<2,2,2,false,false>"}, sorted(added)


def test_variant_names_are_the_ones_the_library_registers():
    from tests.test_conv_variants_gpu import VARIANTS
    texts = "\n".join(_texts())
    src = source_variants(_texts())
    for key, name in VARIANTS.items():
        if name.startswith("ablation-only: "):
            switch = name.split(": ", 1)[1]
            assert switch.startswith("XV2_") and ('getenv("%s")' % switch) in texts, (key, name)
        else:
            assert name == (src[key] if src[key] is not None else registered_name(key)), (key, name)
    # one name per reachable instantiation: the table can tell which of them ran
    reachable = [v for v in VARIANTS.values() if not v.startswith("ablation-only: ")]
    assert len(reachable) == len(set(reachable))


def test_every_variant_is_reached_by_a_case():
    from tests.test_conv_variants_gpu import CASES, EXPECT, VARIANTS
    ids = [c.cid for c in CASES]
    assert len(ids) == len(set(ids))
    assert set(EXPECT) == set(ids), (sorted(set(ids) - set(EXPECT)), sorted(set(EXPECT) - set(ids)))
    reached = {n for names in EXPECT.values() for n in names}
    missing = [k for k, v in VARIANTS.items() if not v.startswith("ablation-only: ") and v not in reached]
    assert not missing, missing
