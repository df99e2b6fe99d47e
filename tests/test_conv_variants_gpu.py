"""Every convolution kernel variant against a float64 reference, at the shapes, math modes and edges where kernels go wrong.

VARIANTS names the kernel instantiations of the convolution sources that carry a profiler name of their own - each distinct
launch_one<...> / sg_launch_one<...> / thin_launch_one<...> template argument list (the XV2_IGEMM_TILES, XV2_SG_CASE and
XV2_THIN_CASE macros expanded), each XV2_WGRAD_ROW(...) row of the weight-gradient kernel table (keyed by its kernel) and each
prof_register("...") literal - with that name.  An instantiation that only an A/B switch reaches reads
"ablation-only: XV2_<switch>".  tests/test_conv_variants_cpu.py keeps the table equal to the sources and checks that the cases
below reach every other entry.

A case calls the C ABI directly (xview2_amd._capi.call with an ops._desc descriptor, weights packed by xv2_pack_weight) and
asserts the exact profiler names of its launches (EXPECT).  Every output, workspace, statistics buffer, packed weight operand
and strided input is a view inside a larger allocation whose remainder is a sentinel: guard rows after the last pixel, guard
columns where ld > C.  Overwrite outputs, workspaces and statistics partials start as the sentinel; accumulated outputs start
as a random base.  The case runs twice, sentinel NaN and then 2^100: the results must be bit-identical and every guard
unchanged.  Results are held to the two gates of tests/conv_ref.py against float64.

XV2_VARIANTS_RECORD=<file.json>: a calibration run - nothing is asserted; every case's launches, gate ratios and failures go
to the file (EXPECT and the constants of tests/conv_ref.py come from such a run)."""
import contextlib
import ctypes
import json
import math
import os
import zlib

import pytest
import torch

from tests import conv_ref as R
from tests.test_f16x2_gpu import _prof

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POISONS = (float("nan"), 2.0 ** 100)
RECORD = os.environ.get("XV2_VARIANTS_RECORD")

VARIANTS = {
    # igemm_conv.hip igemm_launch: halo form (3x3 / stride 1 / same size), split-K, RGB, per-tap tiles per math mode
    "launch_one<Form::BF16HBM_HALO,128,128>": "igemm_kernel<128,128,2,2,c32,bf16hbm,halo>",
    "launch_one<Form::BF16HBM_HALO,128,64>": "igemm_kernel<128,64,2,2,c32,bf16hbm,halo>",
    "launch_one<Form::F16X2_HALO,128,128>": "igemm_kernel<128,128,2,2,c32,f16x2,halo,wx2>",
    "launch_one<Form::F16X2_HALO,128,64>": "igemm_kernel<128,64,2,2,c32,f16x2,halo,wx2>",
    "launch_one<Form::F32X3_HALO_WX3,128,128>": "igemm_kernel<128,128,2,2,c32,f32x3,halo,wx3>",
    "launch_one<Form::F32X3_HALO_WX3,128,64>": "igemm_kernel<128,64,2,2,c32,f32x3,halo,wx3>",
    "launch_one<Form::F32X3_HALO,128,128>": "igemm_kernel<128,128,2,2,c32,f32x3,halo>",
    "launch_one<Form::F32X3_HALO,128,64>": "igemm_kernel<128,64,2,2,c32,f32x3,halo>",
    "launch_one<Form::BF16HBM,128,128>": "igemm_kernel<128,128,2,2,c32,bf16hbm>",
    "launch_one<Form::F16X2,128,128>": "igemm_kernel<128,128,2,2,c32,f16x2>",
    "launch_one<Form::F32X3,128,128>": "igemm_kernel<128,128,2,2,c32,f32x3>",
    "launch_one<Form::BF16,128,128>": "igemm_kernel<128,128,2,2,c32,bf16>",
    "launch_one<Form::C32,128,128>": "igemm_kernel<128,128,2,2,c32>",
    "launch_one<Form::RGB_BF16OUT,128,128>": "igemm_kernel<128,128,2,2,rgb,bf16out>",
    "launch_one<Form::RGB_BF16OUT,128,64>": "igemm_kernel<128,64,2,2,rgb,bf16out>",
    "launch_one<Form::RGB_BF16OUT,128,32>": "igemm_kernel<128,32,4,1,rgb,bf16out>",
    "launch_one<Form::RGB,128,128>": "igemm_kernel<128,128,2,2,rgb>",
    "launch_one<Form::RGB,128,64>": "igemm_kernel<128,64,2,2,rgb>",
    "launch_one<Form::RGB,128,32>": "igemm_kernel<128,32,4,1,rgb>",
    "launch_one<Form::BF16HBM,64,128>": "igemm_kernel<64,128,2,2,c32,bf16hbm>",
    "launch_one<Form::BF16HBM,128,64>": "igemm_kernel<128,64,2,2,c32,bf16hbm>",
    "launch_one<Form::BF16HBM,64,64>": "igemm_kernel<64,64,2,2,c32,bf16hbm>",
    "launch_one<Form::BF16HBM,128,32>": "igemm_kernel<128,32,4,1,c32,bf16hbm>",
    "launch_one<Form::F16X2,64,128>": "igemm_kernel<64,128,2,2,c32,f16x2>",
    "launch_one<Form::F16X2,128,64>": "igemm_kernel<128,64,2,2,c32,f16x2>",
    "launch_one<Form::F16X2,64,64>": "igemm_kernel<64,64,2,2,c32,f16x2>",
    "launch_one<Form::F16X2,128,32>": "igemm_kernel<128,32,4,1,c32,f16x2>",
    "launch_one<Form::F32X3,64,128>": "igemm_kernel<64,128,2,2,c32,f32x3>",
    "launch_one<Form::F32X3,128,64>": "igemm_kernel<128,64,2,2,c32,f32x3>",
    "launch_one<Form::F32X3,64,64>": "igemm_kernel<64,64,2,2,c32,f32x3>",
    "launch_one<Form::F32X3,128,32>": "igemm_kernel<128,32,4,1,c32,f32x3>",
    "launch_one<Form::BF16,64,128>": "igemm_kernel<64,128,2,2,c32,bf16>",
    "launch_one<Form::BF16,128,64>": "igemm_kernel<128,64,2,2,c32,bf16>",
    "launch_one<Form::BF16,64,64>": "igemm_kernel<64,64,2,2,c32,bf16>",
    "launch_one<Form::BF16,128,32>": "igemm_kernel<128,32,4,1,c32,bf16>",
    "launch_one<Form::C32,64,128>": "igemm_kernel<64,128,2,2,c32>",
    "launch_one<Form::C32,128,64>": "igemm_kernel<128,64,2,2,c32>",
    "launch_one<Form::C32,64,64>": "igemm_kernel<64,64,2,2,c32>",
    "launch_one<Form::C32,128,32>": "igemm_kernel<128,32,4,1,c32>",
    # wgrad_conv.hip WGRAD_ROWS: one row per weight-gradient device kernel (tiled, transpose-read, all-taps 32 x 32 and 64 x 64)
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::RGB_BF16HBM,64,64>)": "wgrad_kernel<64,64,2,2,1,rgb,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::RGB_BF16HBM,32,64>)": "wgrad_kernel<32,64,1,2,2,rgb,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::RGB,64,64>)": "wgrad_kernel<64,64,2,2,1,rgb>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::RGB,32,64>)": "wgrad_kernel<32,64,1,2,2,rgb>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16_BF16HBM,128,128>)": "wgrad_kernel<128,128,2,2,1,c32,bf16,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16_BF16HBM,64,64>)": "wgrad_kernel<64,64,2,2,1,c32,bf16,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16_BF16HBM,64,32>)": "wgrad_kernel<64,32,2,1,2,c32,bf16,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16_BF16HBM,32,64>)": "wgrad_kernel<32,64,1,2,2,c32,bf16,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32_BF16HBM,32,32>)": "wgrad_kernel<32,32,1,1,4,c32,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16,128,128>)": "wgrad_kernel<128,128,2,2,1,c32,bf16>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16,64,64>)": "wgrad_kernel<64,64,2,2,1,c32,bf16>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16,64,32>)": "wgrad_kernel<64,32,2,1,2,c32,bf16>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::BF16,32,64>)": "wgrad_kernel<32,64,1,2,2,c32,bf16>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32,128,128>)": "wgrad_kernel<128,128,2,2,1,c32>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32,64,64>)": "wgrad_kernel<64,64,2,2,1,c32>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32,64,32>)": "wgrad_kernel<64,32,2,1,2,c32>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32,32,64>)": "wgrad_kernel<32,64,1,2,2,c32>",
    "XV2_WGRAD_ROW(wgrad_kernel<WForm::C32,32,32>)": "wgrad_kernel<32,32,1,1,4,c32>",
    "XV2_WGRAD_ROW(wgrad_tr_x3_kernel<128,128,3>)": "wgrad_tr_kernel<128,128,f32x3>",
    "XV2_WGRAD_ROW(wgrad_tr_x3_kernel<64,64,3>)": "wgrad_tr_kernel<64,64,f32x3>",
    "XV2_WGRAD_ROW(wgrad_tr_x3_kernel<128,128,2>)": "wgrad_tr_kernel<128,128,f16x2>",
    "XV2_WGRAD_ROW(wgrad_tr_x3_kernel<64,64,2>)": "wgrad_tr_kernel<64,64,f16x2>",
    "XV2_WGRAD_ROW(wgrad_tr_kernel<128,128>)": "wgrad_tr_kernel<128,128,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_tr_kernel<64,64>)": "wgrad_tr_kernel<64,64,bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_alltaps_kernel<false>)": "wgrad_alltaps_kernel",
    "XV2_WGRAD_ROW(wgrad_alltaps_kernel<true>)": "wgrad_alltaps_kernel<bf16>",
    "XV2_WGRAD_ROW(wgrad_alltaps_tr_kernel)": "wgrad_alltaps_kernel<bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_alltaps_x3_kernel<3>)": "wgrad_alltaps_kernel<f32x3>",
    "XV2_WGRAD_ROW(wgrad_alltaps_x3_kernel<2>)": "wgrad_alltaps_kernel<f16x2>",
    "XV2_WGRAD_ROW(wgrad_alltaps64_tr_kernel)": "wgrad_alltaps64_kernel<bf16hbm>",
    "XV2_WGRAD_ROW(wgrad_alltaps64_x3_kernel<3>)": "wgrad_alltaps64_kernel<f32x3>",
    "XV2_WGRAD_ROW(wgrad_alltaps64_x3_kernel<2>)": "wgrad_alltaps64_kernel<f16x2>",
    # direct_conv.hip, stem_conv.hip
    'prof_register("direct3x3_n32_kernel")': "direct3x3_n32_kernel",
    'prof_register("direct3x3_n32_kernel<bf16>")': "direct3x3_n32_kernel<bf16>",
    'prof_register("direct3x3_n32_kernel<bf16hbm>")': "direct3x3_n32_kernel<bf16hbm>",
    'prof_register("direct3x3_n32_kernel<f32x3>")': "direct3x3_n32_kernel<f32x3>",
    'prof_register("direct3x3_n32_kernel<f16x2>")': "direct3x3_n32_kernel<f16x2>",
    'prof_register("stem7x7_kernel<rgb>")': "stem7x7_kernel<rgb>",
    'prof_register("stem7x7_wgrad_kernel<rgb>")': "stem7x7_wgrad_kernel<rgb>",
    # thin_conv.hip (XV2_THIN_CASE and the transposed-convolution forms): the streaming 1x1 kernel and its 2x2 / 2 twins
    "thin_launch_one<64,64,true,2,2>": "thin1x1_kernel<64,64,bf16hbm>",
    "thin_launch_one<64,64,false,4,4,0,2>": "thin1x1_kernel<64,64,f16x2>",
    "thin_launch_one<64,64,false,4,4>": "thin1x1_kernel<64,64,f32x3>",
    "thin_launch_one<64,128,true,2,2>": "thin1x1_kernel<64,128,bf16hbm>",
    "thin_launch_one<64,128,false,4,4,0,2>": "thin1x1_kernel<64,128,f16x2>",
    "thin_launch_one<64,128,false,4,4>": "thin1x1_kernel<64,128,f32x3>",
    "thin_launch_one<64,256,true,2,2>": "thin1x1_kernel<64,256,bf16hbm>",
    "thin_launch_one<64,256,false,4,4,0,2>": "thin1x1_kernel<64,256,f16x2>",
    "thin_launch_one<64,256,false,4,4>": "thin1x1_kernel<64,256,f32x3>",
    "thin_launch_one<128,64,true,2,2>": "thin1x1_kernel<128,64,bf16hbm>",
    "thin_launch_one<128,64,false,4,4,0,2>": "thin1x1_kernel<128,64,f16x2>",
    "thin_launch_one<128,64,false,4,4>": "thin1x1_kernel<128,64,f32x3>",
    "thin_launch_one<256,64,true,2,2>": "thin1x1_kernel<256,64,bf16hbm>",
    "thin_launch_one<256,64,false,4,4,0,2>": "thin1x1_kernel<256,64,f16x2>",
    "thin_launch_one<256,64,false,4,4>": "thin1x1_kernel<256,64,f32x3>",
    "thin_launch_one<64,128,true,2,2,1>": "thin_convT_fwd<64,32,bf16hbm>",
    "thin_launch_one<64,128,false,4,4,1>": "thin_convT_fwd<64,32,f32x3>",
    "thin_launch_one<128,64,true,2,2,2>": "thin_convT_bwd<32,64,bf16hbm>",
    # sg_conv.hip (XV2_SG_CASE): the small-grid kernel per configuration (rows, columns, wave groups), 1x1 / per-tap form and
    # storage; the 128-row configuration serves only statistics plans of 128-row tiles, which no default plan asks for
    "sg_launch_one<2,2,4,true,true>": "sg_conv_kernel<64,128,g2,1x1,bf16hbm>",
    "sg_launch_one<2,2,4,true,false>": "sg_conv_kernel<64,128,g2,1x1,f16x2>",
    "sg_launch_one<2,2,4,false,true>": "sg_conv_kernel<64,128,g2,bf16hbm>",
    "sg_launch_one<2,2,4,false,false>": "sg_conv_kernel<64,128,g2,f16x2>",
    "sg_launch_one<2,4,4,true,true>": "sg_conv_kernel<64,128,g4,1x1,bf16hbm>",
    "sg_launch_one<2,4,4,true,false>": "sg_conv_kernel<64,128,g4,1x1,f16x2>",
    "sg_launch_one<2,4,4,false,true>": "sg_conv_kernel<64,128,g4,bf16hbm>",
    "sg_launch_one<2,4,4,false,false>": "sg_conv_kernel<64,128,g4,f16x2>",
    "sg_launch_one<2,4,2,true,true>": "sg_conv_kernel<64,64,g4,1x1,bf16hbm>",
    "sg_launch_one<2,4,2,true,false>": "sg_conv_kernel<64,64,g4,1x1,f16x2>",
    "sg_launch_one<2,4,2,false,true>": "sg_conv_kernel<64,64,g4,bf16hbm>",
    "sg_launch_one<2,4,2,false,false>": "sg_conv_kernel<64,64,g4,f16x2>",
    "sg_launch_one<4,2,4,true,true>": "ablation-only: XV2_SG_CFG",
    "sg_launch_one<4,2,4,true,false>": "ablation-only: XV2_SG_CFG",
    "sg_launch_one<4,2,4,false,true>": "ablation-only: XV2_SG_CFG",
    "sg_launch_one<4,2,4,false,false>": "ablation-only: XV2_SG_CFG",
}

# math mode of the descriptor; the bound family of tests/conv_ref.py
MATH = {"f32": 0, "bf16m": 1, "bf16s": 2, "x3": 3, "wx3": 3, "h2": 3, "h2pt": 3}
FAMILY = {"f32": "f32", "x3": "f32x3", "wx3": "f32x3", "h2": "f16x2", "h2pt": "f16x2", "bf16s": "bf16", "bf16m": "bf16"}


class Case:
    """op: fwd | fused | bwd | wgrad | tfwd | tbwd | twgrad | gbwd.  The geometry is always that of the convolution the
    descriptor describes: for the transposed ops the equivalent 2x2 / stride-2 convolution (N, H, W = the large grid, C0 = the
    ConvTranspose2d's output channels, Cout = its input channels), for gbwd one of the two groups.
    mode: f32 (XV2_MATH_F32), x3 (XV2_MATH_F32X3, no operand maxima, no weight planes), wx3 (x3 with the three-plane weights
    registered), h2 (x3 with every operand maximum, the weight maximum and the fp16 weight planes: F16X2), h2pt (maxima without
    planes: the per-tap F16X2 form), bf16s (XV2_MATH_BF16_STORE), bf16m (XV2_MATH_BF16 on fp32 tensors).
    tile: XV2_FORCE_TILE for the call; ldx / ldy: extra elements per row of the input / output views; acc: accumulate bits;
    split: the planner must pick a split-K plan by itself (a forced factor > 1 implies one)."""

    def __init__(self, cid, op, mode, N, H, W, C0, Cout, k=1, s=1, pad=None, dil=1, C1=0, tile=None, ldx=0, ldy=0, acc=0,
                 bias=False, stats=False, cin_real=None, split=False):
        self.cid, self.op, self.mode = cid, op, mode
        self.N, self.H, self.W, self.C0, self.C1, self.Cout = N, H, W, C0, C1, Cout
        self.k, self.s, self.dil = k, s, dil
        self.pad = dil * (k // 2) if pad is None else pad
        self.tile, self.ldx, self.ldy, self.acc = tile, ldx, ldy, acc
        self.bias, self.stats, self.cin_real = bias, stats, cin_real
        # split-K plan expected: the factor XV2_FORCE_TILE asks for, or True for one the planner picks by itself
        ks = int(tile.split(",")[2]) if tile else 1
        self.split = ks if ks > 1 else split
        self.OH = (H + 2 * self.pad - dil * (k - 1) - 1) // s + 1
        self.OW = (W + 2 * self.pad - dil * (k - 1) - 1) // s + 1

    def __repr__(self):
        return self.cid


def _cases():
    L = []

    def add(*a, **k):
        L.append(Case(*a, **k))

    # per-tap implicit GEMM: each tile shape (XV2_FORCE_TILE picks the rows; Cout the columns: 96 / 160 -> 32-column tiles) in
    # each math mode, over entry points and geometries the halo form cannot take.  bf16 storage: two sources (the small-grid
    # kernel takes single-source problems)
    acc_of = {"f32": 1, "x3": 2, "h2pt": 3, "bf16m": 0, "bf16s": 3}
    for m in ("f32", "x3", "h2pt", "bf16m", "bf16s"):
        two = m == "bf16s"
        add(m + "-fwd-1x1-M480-128x128", "fwd", m, 1, 24, 20, 32 if two else 64, 128, C1=32 if two else 0, tile="128,128,1")
        add(m + "-bwd-3x3s2-odd15-64x128", "bwd", m, 2, 15, 15, 64 if two else 128, 64, k=3, s=2, C1=64 if two else 0,
            tile="64,128,1")
        add(m + "-fused-3x3d2-128x64", "fused", m, 1, 12, 20, 64, 64, k=3, dil=2, C1=32 if two else 0, tile="128,64,1")
        add(m + "-fwd-bias-3x3s2-dual-64x64", "fwd", m, 2, 17, 13, 64, 64, k=3, s=2, C1=32, tile="64,64,1", bias=True)
        add(m + "-bwd-acc%d-1x1-160-128x32" % acc_of[m], "bwd", m, 1, 9, 11, 96, 64, C1=64, acc=acc_of[m])
    # halo form (3x3 / stride 1 / same size, OH % 4 == 0, OW % 32 == 0), 128-row tiles, 128 and 64 columns, every weight form
    add("x3-halo-fwd-128", "fwd", "x3", 1, 8, 64, 96, 128, k=3, tile="128,128,1")
    add("x3-halo-bwd-64", "bwd", "x3", 1, 8, 64, 64, 96, k=3, tile="128,64,1")
    add("wx3-halo-fwd-128-strided", "fwd", "wx3", 1, 8, 64, 96, 128, k=3, tile="128,128,1", ldx=32, ldy=64)
    add("wx3-halo-fused-64", "fused", "wx3", 2, 4, 32, 64, 192, k=3, tile="128,64,1")
    add("h2-halo-fwd-128-dual", "fwd", "h2", 1, 8, 64, 64, 128, k=3, C1=32, tile="128,128,1")
    add("h2-halo-bwd-64-dual", "bwd", "h2", 1, 8, 32, 32, 64, k=3, C1=32, tile="128,64,1")
    add("bf16s-halo-fwd-128", "fwd", "bf16s", 1, 8, 64, 64, 128, k=3, C1=64, tile="128,128,1")
    add("bf16s-halo-bwd-64", "bwd", "bf16s", 1, 8, 32, 32, 64, k=3, C1=32, tile="128,64,1")
    # where the halo form falls back; grids of one row / column; dilation 4; stride 2 with parity classes of unequal size
    add("x3-fwd-3x3-ow40", "fwd", "x3", 1, 12, 40, 64, 128, k=3, tile="128,128,1")
    add("x3-bwd-3x3-oh6", "bwd", "x3", 1, 6, 32, 128, 64, k=3, tile="128,128,1")
    add("f32-fwd-3x3-h1", "fwd", "f32", 3, 1, 37, 64, 64, k=3)
    add("x3-bwd-3x3-w1", "bwd", "x3", 2, 29, 1, 64, 96, k=3)
    add("x3-fwd-3x3-d4", "fwd", "x3", 1, 20, 20, 64, 64, k=3, dil=4)
    add("x3-bwd-3x3s2-15x13", "bwd", "x3", 1, 15, 13, 64, 64, k=3, s=2)
    # 1x1 / stride 2 backward-data: three of the four parity classes have no tap (zeroed, or kept when accumulating)
    add("x3-bwd-1x1s2-empty", "bwd", "x3", 2, 9, 7, 64, 128, s=2)
    add("x3-bwd-acc1-1x1s2-empty", "bwd", "x3", 2, 9, 7, 64, 128, s=2, acc=1)
    add("f32-bwd-acc3-1x1s2-empty-dual", "bwd", "f32", 1, 11, 10, 32, 64, s=2, C1=64, acc=3)
    add("bf16s-bwd-acc2-1x1s2-empty-dual", "bwd", "bf16s", 1, 9, 9, 64, 64, s=2, C1=32, acc=2)
    # split-K, per-tap form: 1x1 over 736 channels = 23 K tiles (uneven ranges), M = 35 (one partial tile)
    for ks, m in ((2, "x3"), (3, "f32"), (4, "bf16m"), (5, "h2pt"), (6, "bf16s"), (8, "x3")):
        add("%s-fwd-1x1-736-ks%d" % (m, ks), "fwd", m, 1, 5, 7, 384, 128, C1=352, tile="128,128,%d" % ks,
            stats=ks in (3, 6), bias=ks == 2)
    add("f32-fwd-3x3s2-96-ks7", "fwd", "f32", 2, 9, 9, 96, 128, k=3, s=2, tile="128,128,7")   # 27 K tiles: 6 x 4 + 3
    add("f32-bwd-1x1-736-ks4", "bwd", "f32", 1, 6, 6, 128, 736, tile="128,128,4")
    # split-K, halo form: K ranges of whole 32-channel chunks; 15 / 17 / 19 chunks leave uneven and odd last ranges
    for C, ks, m in ((480, 2, "x3"), (480, 3, "wx3"), (480, 4, "h2"), (480, 5, "bf16s"), (544, 6, "x3"), (608, 7, "wx3"),
                     (480, 8, "h2"), (480, 2, "bf16s"), (544, 4, "bf16s")):
        two = m in ("h2", "bf16s")
        add("%s-halo-fwd-%d-ks%d" % (m, C, ks), "fwd", m, 1, 4, 32, C - 96 if two else C, 128, k=3, C1=96 if two else 0,
            tile="128,128,%d" % ks)
    add("x3-halo-bwd-480-ks3", "bwd", "x3", 1, 4, 32, 128, 480, k=3, tile="128,128,3")
    # split-K plans the planner picks by itself (no XV2_FORCE_TILE): one source, and two sources with statistics (a single
    # source with statistics is planned for the small-grid kernel and its 64-row tiles instead)
    add("x3-fwd-3x3-512-natural-split", "fwd", "x3", 2, 8, 8, 512, 512, k=3, split=True)
    add("x3-fwd-3x3-dual-natural-split-stats", "fwd", "x3", 2, 8, 8, 256, 512, k=3, C1=256, stats=True, split=True)
    add("x3-fwd-3x3-512-stats-sg-plan", "fwd", "x3", 2, 8, 8, 512, 512, k=3, stats=True)
    # statistics partials of the tiled, small-grid and streaming plans
    add("x3-fwd-stats-207rows", "fwd", "x3", 1, 9, 23, 64, 128, stats=True)
    add("bf16s-fwd-stats-dual", "fwd", "bf16s", 2, 7, 9, 64, 64, k=3, C1=32, stats=True)
    add("h2-sg-fwd-stats", "fwd", "h2", 2, 16, 16, 128, 128, k=3, stats=True)
    # small-grid kernel (sg_conv.hip): F16X2 with weight planes, bf16 storage; its pixel limit (40000) from both sides
    add("h2-sg-fwd-3x3", "fwd", "h2", 2, 16, 16, 128, 256, k=3)
    add("h2-sg-fwd-1x1s2", "fwd", "h2", 2, 32, 32, 256, 512, s=2)
    add("h2-sg-bwd-3x3", "bwd", "h2", 2, 8, 8, 256, 256, k=3)
    add("bf16s-sg-fwd-1x1-M40000", "fwd", "bf16s", 1, 200, 200, 128, 128)
    add("bf16s-fwd-1x1-M40200", "fwd", "bf16s", 1, 200, 201, 128, 128)
    add("h2-fwd-3x3-ldx-unaligned", "fwd", "h2", 2, 16, 16, 128, 128, k=3, ldx=2)
    # each small-grid configuration (sg_pick: 64 x 64 / g4 up to 160 tiles, 64 x 128 / g4 up to 384, 64 x 128 / g2 beyond, or
    # where the K steps do not split four ways) in its 1x1 and per-tap forms, both storage types
    add("h2-sg242-fwd-1x1", "fwd", "h2", 2, 16, 16, 64, 64)
    add("bf16s-sg242-fwd-1x1", "fwd", "bf16s", 2, 16, 16, 128, 64)
    add("bf16s-sg242-fwd-3x3", "fwd", "bf16s", 2, 16, 16, 128, 64, k=3)
    add("h2-sg244-fwd-1x1", "fwd", "h2", 2, 80, 80, 64, 128)
    add("h2-sg244-bwd-3x3", "bwd", "h2", 2, 80, 80, 128, 64, k=3)
    add("bf16s-sg244-fwd-1x1", "fwd", "bf16s", 2, 80, 80, 128, 128)
    add("bf16s-sg244-fwd-3x3", "fwd", "bf16s", 2, 80, 80, 128, 128, k=3)
    add("h2-sg224-fwd-1x1", "fwd", "h2", 2, 16, 16, 32, 128)
    add("h2-sg224-fwd-3x3", "fwd", "h2", 2, 16, 16, 32, 128, k=3)
    add("h2-sg-grouped-bwd", "gbwd", "h2", 2, 16, 16, 64, 64, k=3)
    add("bf16s-sg-grouped-bwd-acc", "gbwd", "bf16s", 2, 16, 16, 128, 64, k=3, acc=1)
    add("bf16s-grouped-bwd-tiled", "gbwd", "bf16s", 2, 16, 16, 64, 64, k=3)
    # streaming 1x1 kernel (thin_conv.hip): >= 65536 pixels, 16-byte aligned rows
    add("x3-thin-fwd-M65536", "fwd", "x3", 1, 256, 256, 64, 128)
    add("x3-fwd-1x1-M65280", "fwd", "x3", 1, 255, 256, 64, 128)
    add("h2-thin-fwd-stats", "fwd", "h2", 1, 256, 256, 128, 64, stats=True)
    add("bf16s-thin-fwd", "fwd", "bf16s", 2, 128, 256, 256, 64)
    add("x3-fwd-1x1-M65536-ldx-unaligned", "fwd", "x3", 1, 256, 256, 64, 64, ldx=2)
    for K, N in ((64, 64), (64, 128), (64, 256), (128, 64), (256, 64)):      # every shape of the streaming kernel, every form
        for m in ("x3", "h2", "bf16s"):
            if (K, N, m) not in ((64, 128, "x3"), (128, 64, "h2"), (256, 64, "bf16s")):      # (above)
                add("%s-thin-fwd-%dx%d" % (m, K, N), "fwd", m, 1, 256, 256, K, N)
    # transposed convolution 2x2 / 2 (the streaming form at 64 -> 32 channels over >= 65536 small-grid pixels)
    add("x3-thinT-fwd", "tfwd", "x3", 1, 512, 512, 32, 64, k=2, s=2, pad=0)
    add("x3-convT-bwd-M65536", "tbwd", "x3", 1, 512, 512, 32, 64, k=2, s=2, pad=0)      # (fp32: the tiled kernel)
    add("bf16s-thinT-fwd", "tfwd", "bf16s", 1, 512, 512, 32, 64, k=2, s=2, pad=0)
    add("bf16s-thinT-bwd-acc", "tbwd", "bf16s", 1, 512, 512, 32, 64, k=2, s=2, pad=0, acc=1)
    add("x3-convT-fwd", "tfwd", "x3", 2, 32, 24, 64, 128, k=2, s=2, pad=0)
    add("h2-convT-fwd", "tfwd", "h2", 2, 32, 32, 64, 128, k=2, s=2, pad=0)
    add("bf16s-convT-fwd", "tfwd", "bf16s", 1, 16, 48, 128, 256, k=2, s=2, pad=0)
    add("x3-convT-bwd", "tbwd", "x3", 2, 32, 24, 64, 128, k=2, s=2, pad=0)
    add("h2-convT-bwd-acc", "tbwd", "h2", 2, 32, 32, 64, 128, k=2, s=2, pad=0, acc=1)
    add("x3-convT-wgrad", "twgrad", "x3", 2, 32, 32, 64, 128, k=2, s=2, pad=0)
    add("h2-convT-wgrad", "twgrad", "h2", 2, 32, 64, 128, 64, k=2, s=2, pad=0)
    add("bf16s-convT-wgrad", "twgrad", "bf16s", 1, 20, 20, 64, 64, k=2, s=2, pad=0)
    # direct 3x3 kernel (32 -> 32 channels, LDS-resident halo and weights)
    for m in ("f32", "bf16m", "bf16s", "x3", "h2"):
        add(m + "-direct-fwd", "fwd", m, 2, 16, 32, 32, 32, k=3)
    add("x3-direct-bwd", "bwd", "x3", 1, 16, 64, 32, 32, k=3)
    # RGB stems: the 7x7 / 2 kernels and the 4-channel gather kernel of the tiled form
    add("x3-stem-fwd", "fwd", "x3", 1, 32, 64, 4, 64, k=7, s=2)
    add("bf16s-stem-fwd-stats", "fwd", "bf16s", 1, 32, 64, 4, 64, k=7, s=2, stats=True)
    add("x3-stem-wgrad", "wgrad", "x3", 2, 32, 64, 4, 64, k=7, s=2)
    add("f32-stem-fwd-30x50", "fwd", "f32", 1, 30, 50, 4, 64, k=7, s=2)
    for m in ("f32", "bf16s"):
        add(m + "-rgb-fwd-128", "fwd", m, 1, 20, 30, 4, 128, k=3)
        add(m + "-rgb-fwd-64-ldy", "fwd", m, 1, 20, 30, 4, 64, k=3, ldy=8)
        add(m + "-rgb-fwd-96", "fwd", m, 2, 9, 31, 4, 96, k=3)
        add(m + "-rgb-wgrad-64", "wgrad", m, 1, 20, 30, 4, 64, k=3)
        add(m + "-rgb-wgrad-96", "wgrad", m, 1, 20, 30, 4, 96, k=3)
    # weight gradient: all-taps 3x3 form, transpose-read form (OW % 32 == 0), tiled kernel (every tile of its plan)
    for m in ("f32", "bf16m", "bf16s", "x3", "h2"):
        add(m + "-wgrad-alltaps", "wgrad", m, 2, 8, 32, 64, 128, k=3)
    # (Cout 96 rules out the 64 x 64 tile; two row chunks: the chunk-boundary halo rows, the second source)
    for m in ("x3", "h2", "bf16s"):
        add(m + "-wgrad-alltaps-96-dual", "wgrad", m, 1, 16, 32, 64, 96, k=3, C1=32)
    # (64 x 64 tile, the second source selected by cn0 >= C0, three row chunks)
    for m in ("x3", "h2", "bf16s"):
        add(m + "-wgrad-alltaps64-dual", "wgrad", m, 1, 24, 32, 64, 128, k=3, C1=64)
    for m in ("x3", "h2", "bf16s"):
        add(m + "-wgrad-tr-128", "wgrad", m, 1, 4, 64, 128, 128)
        add(m + "-wgrad-tr-64", "wgrad", m, 1, 4, 64, 64, 192, k=3, s=2)
    geos = (dict(k=1), dict(k=3, s=2), dict(k=3), dict(k=3, dil=2), dict(k=1, s=2))
    for m in ("f32", "bf16m", "bf16s"):
        for (co, ci), geo in zip(((128, 128), (64, 64), (64, 96), (96, 64), (96, 96)), geos):
            add("%s-wgrad-%dx%d-k%ds%dd%d" % (m, co, ci, geo["k"], geo.get("s", 1), geo.get("dil", 1)), "wgrad", m, 1, 7, 20,
                ci, co, **geo)
    add("f32-wgrad-cin-real-50", "wgrad", "f32", 2, 6, 10, 64, 64, k=3, cin_real=50)
    add("x3-wgrad-3x3s2-dual", "wgrad", "x3", 1, 9, 20, 64, 96, k=3, s=2, C1=32, ldx=32, ldy=4)
    return L


CASES = _cases()

# the profiler names of each case's launches, in order (from a calibration run, checked against the planner by hand)
EXPECT = {
    'f32-fwd-1x1-M480-128x128': ('igemm_kernel<128,128,2,2,c32>',),
    'f32-bwd-3x3s2-odd15-64x128': ('igemm_kernel<64,128,2,2,c32>',),
    'f32-fused-3x3d2-128x64': ('igemm_kernel<128,64,2,2,c32>',),
    'f32-fwd-bias-3x3s2-dual-64x64': ('igemm_kernel<64,64,2,2,c32>',),
    'f32-bwd-acc1-1x1-160-128x32': ('igemm_kernel<128,32,4,1,c32>',),
    'x3-fwd-1x1-M480-128x128': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'x3-bwd-3x3s2-odd15-64x128': ('igemm_kernel<64,128,2,2,c32,f32x3>',),
    'x3-fused-3x3d2-128x64': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-fwd-bias-3x3s2-dual-64x64': ('igemm_kernel<64,64,2,2,c32,f32x3>',),
    'x3-bwd-acc2-1x1-160-128x32': ('igemm_kernel<128,32,4,1,c32,f32x3>',),
    'h2pt-fwd-1x1-M480-128x128': ('igemm_kernel<128,128,2,2,c32,f16x2>',),
    'h2pt-bwd-3x3s2-odd15-64x128': ('igemm_kernel<64,128,2,2,c32,f16x2>',),
    'h2pt-fused-3x3d2-128x64': ('igemm_kernel<128,64,2,2,c32,f16x2>',),
    'h2pt-fwd-bias-3x3s2-dual-64x64': ('igemm_kernel<64,64,2,2,c32,f16x2>',),
    'h2pt-bwd-acc3-1x1-160-128x32': ('igemm_kernel<128,32,4,1,c32,f16x2>',),
    'bf16m-fwd-1x1-M480-128x128': ('igemm_kernel<128,128,2,2,c32,bf16>',),
    'bf16m-bwd-3x3s2-odd15-64x128': ('igemm_kernel<64,128,2,2,c32,bf16>',),
    'bf16m-fused-3x3d2-128x64': ('igemm_kernel<128,64,2,2,c32,bf16>',),
    'bf16m-fwd-bias-3x3s2-dual-64x64': ('igemm_kernel<64,64,2,2,c32,bf16>',),
    'bf16m-bwd-acc0-1x1-160-128x32': ('igemm_kernel<128,32,4,1,c32,bf16>',),
    'bf16s-fwd-1x1-M480-128x128': ('igemm_kernel<128,128,2,2,c32,bf16hbm>',),
    'bf16s-bwd-3x3s2-odd15-64x128': ('igemm_kernel<64,128,2,2,c32,bf16hbm>',),
    'bf16s-fused-3x3d2-128x64': ('igemm_kernel<128,64,2,2,c32,bf16hbm>',),
    'bf16s-fwd-bias-3x3s2-dual-64x64': ('igemm_kernel<64,64,2,2,c32,bf16hbm>',),
    'bf16s-bwd-acc3-1x1-160-128x32': ('igemm_kernel<128,32,4,1,c32,bf16hbm>',),
    'x3-halo-fwd-128': ('igemm_kernel<128,128,2,2,c32,f32x3,halo>',),
    'x3-halo-bwd-64': ('igemm_kernel<128,64,2,2,c32,f32x3,halo>',),
    'wx3-halo-fwd-128-strided': ('igemm_kernel<128,128,2,2,c32,f32x3,halo,wx3>',),
    'wx3-halo-fused-64': ('igemm_kernel<128,64,2,2,c32,f32x3,halo,wx3>',),
    'h2-halo-fwd-128-dual': ('igemm_kernel<128,128,2,2,c32,f16x2,halo,wx2>',),
    'h2-halo-bwd-64-dual': ('igemm_kernel<128,64,2,2,c32,f16x2,halo,wx2>',),
    'bf16s-halo-fwd-128': ('igemm_kernel<128,128,2,2,c32,bf16hbm,halo>',),
    'bf16s-halo-bwd-64': ('igemm_kernel<128,64,2,2,c32,bf16hbm,halo>',),
    'x3-fwd-3x3-ow40': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'x3-bwd-3x3-oh6': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'f32-fwd-3x3-h1': ('igemm_kernel<64,64,2,2,c32>',),
    'x3-bwd-3x3-w1': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-fwd-3x3-d4': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-bwd-3x3s2-15x13': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-bwd-1x1s2-empty': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-bwd-acc1-1x1s2-empty': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'f32-bwd-acc3-1x1s2-empty-dual': ('igemm_kernel<128,32,4,1,c32>',),
    'bf16s-bwd-acc2-1x1s2-empty-dual': ('igemm_kernel<128,32,4,1,c32,bf16hbm>',),
    'x3-fwd-1x1-736-ks2': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'f32-fwd-1x1-736-ks3': ('igemm_kernel<128,128,2,2,c32>',),
    'bf16m-fwd-1x1-736-ks4': ('igemm_kernel<128,128,2,2,c32,bf16>',),
    'h2pt-fwd-1x1-736-ks5': ('igemm_kernel<128,128,2,2,c32,f16x2>',),
    'bf16s-fwd-1x1-736-ks6': ('igemm_kernel<128,128,2,2,c32,bf16hbm>',),
    'x3-fwd-1x1-736-ks8': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'f32-fwd-3x3s2-96-ks7': ('igemm_kernel<128,128,2,2,c32>',),
    'f32-bwd-1x1-736-ks4': ('igemm_kernel<128,128,2,2,c32>',),
    'x3-halo-fwd-480-ks2': ('igemm_kernel<128,128,2,2,c32,f32x3,halo>',),
    'wx3-halo-fwd-480-ks3': ('igemm_kernel<128,128,2,2,c32,f32x3,halo,wx3>',),
    'h2-halo-fwd-480-ks4': ('igemm_kernel<128,128,2,2,c32,f16x2,halo,wx2>',),
    'bf16s-halo-fwd-480-ks5': ('igemm_kernel<128,128,2,2,c32,bf16hbm,halo>',),
    'x3-halo-fwd-544-ks6': ('igemm_kernel<128,128,2,2,c32,f32x3,halo>',),
    'wx3-halo-fwd-608-ks7': ('igemm_kernel<128,128,2,2,c32,f32x3,halo,wx3>',),
    'h2-halo-fwd-480-ks8': ('igemm_kernel<128,128,2,2,c32,f16x2,halo,wx2>',),
    'bf16s-halo-fwd-480-ks2': ('igemm_kernel<128,128,2,2,c32,bf16hbm,halo>',),
    'bf16s-halo-fwd-544-ks4': ('igemm_kernel<128,128,2,2,c32,bf16hbm,halo>',),
    'x3-halo-bwd-480-ks3': ('igemm_kernel<128,128,2,2,c32,f32x3,halo>',),
    'x3-fwd-3x3-512-natural-split': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'x3-fwd-3x3-dual-natural-split-stats': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'x3-fwd-3x3-512-stats-sg-plan': ('igemm_kernel<64,128,2,2,c32,f32x3>',),
    'x3-fwd-stats-207rows': ('igemm_kernel<64,128,2,2,c32,f32x3>',),
    'bf16s-fwd-stats-dual': ('igemm_kernel<64,64,2,2,c32,bf16hbm>',),
    'h2-sg-fwd-stats': ('sg_conv_kernel<64,64,g4,f16x2>',),
    'h2-sg-fwd-3x3': ('sg_conv_kernel<64,64,g4,f16x2>',),
    'h2-sg-fwd-1x1s2': ('sg_conv_kernel<64,64,g4,f16x2>',),
    'h2-sg-bwd-3x3': ('sg_conv_kernel<64,64,g4,f16x2>',),
    'bf16s-sg-fwd-1x1-M40000': ('sg_conv_kernel<64,128,g2,1x1,bf16hbm>',),
    'bf16s-fwd-1x1-M40200': ('igemm_kernel<64,128,2,2,c32,bf16hbm>',),
    'h2-fwd-3x3-ldx-unaligned': ('igemm_kernel<128,128,2,2,c32,f16x2>',),
    'h2-sg242-fwd-1x1': ('sg_conv_kernel<64,64,g4,1x1,f16x2>',),
    'bf16s-sg242-fwd-1x1': ('sg_conv_kernel<64,64,g4,1x1,bf16hbm>',),
    'bf16s-sg242-fwd-3x3': ('sg_conv_kernel<64,64,g4,bf16hbm>',),
    'h2-sg244-fwd-1x1': ('sg_conv_kernel<64,128,g4,1x1,f16x2>',),
    'h2-sg244-bwd-3x3': ('sg_conv_kernel<64,128,g4,f16x2>',),
    'bf16s-sg244-fwd-1x1': ('sg_conv_kernel<64,128,g4,1x1,bf16hbm>',),
    'bf16s-sg244-fwd-3x3': ('sg_conv_kernel<64,128,g4,bf16hbm>',),
    'h2-sg224-fwd-1x1': ('sg_conv_kernel<64,128,g2,1x1,f16x2>',),
    'h2-sg224-fwd-3x3': ('sg_conv_kernel<64,128,g2,f16x2>',),
    'h2-sg-grouped-bwd': ('sg_conv_kernel<64,64,g4,f16x2>',),
    'bf16s-sg-grouped-bwd-acc': ('sg_conv_kernel<64,128,g2,bf16hbm>',),
    'bf16s-grouped-bwd-tiled': ('igemm_kernel<64,64,2,2,c32,bf16hbm>', 'igemm_kernel<64,64,2,2,c32,bf16hbm>'),
    'x3-thin-fwd-M65536': ('thin1x1_kernel<64,128,f32x3>',),
    'x3-fwd-1x1-M65280': ('igemm_kernel<128,128,2,2,c32,f32x3>',),
    'h2-thin-fwd-stats': ('thin1x1_kernel<128,64,f16x2>',),
    'bf16s-thin-fwd': ('thin1x1_kernel<256,64,bf16hbm>',),
    'x3-fwd-1x1-M65536-ldx-unaligned': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'x3-thin-fwd-64x64': ('thin1x1_kernel<64,64,f32x3>',),
    'h2-thin-fwd-64x64': ('thin1x1_kernel<64,64,f16x2>',),
    'bf16s-thin-fwd-64x64': ('thin1x1_kernel<64,64,bf16hbm>',),
    'h2-thin-fwd-64x128': ('thin1x1_kernel<64,128,f16x2>',),
    'bf16s-thin-fwd-64x128': ('thin1x1_kernel<64,128,bf16hbm>',),
    'x3-thin-fwd-64x256': ('thin1x1_kernel<64,256,f32x3>',),
    'h2-thin-fwd-64x256': ('thin1x1_kernel<64,256,f16x2>',),
    'bf16s-thin-fwd-64x256': ('thin1x1_kernel<64,256,bf16hbm>',),
    'x3-thin-fwd-128x64': ('thin1x1_kernel<128,64,f32x3>',),
    'bf16s-thin-fwd-128x64': ('thin1x1_kernel<128,64,bf16hbm>',),
    'x3-thin-fwd-256x64': ('thin1x1_kernel<256,64,f32x3>',),
    'h2-thin-fwd-256x64': ('thin1x1_kernel<256,64,f16x2>',),
    'x3-thinT-fwd': ('thin_convT_fwd<64,32,f32x3>',),
    'x3-convT-bwd-M65536': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'bf16s-thinT-fwd': ('thin_convT_fwd<64,32,bf16hbm>',),
    'bf16s-thinT-bwd-acc': ('thin_convT_bwd<32,64,bf16hbm>',),
    'x3-convT-fwd': ('igemm_kernel<128,64,2,2,c32,f32x3>',),
    'h2-convT-fwd': ('igemm_kernel<128,64,2,2,c32,f16x2>',),
    'bf16s-convT-fwd': ('igemm_kernel<64,128,2,2,c32,bf16hbm>',),
    'x3-convT-bwd': ('igemm_kernel<64,128,2,2,c32,f32x3>',),
    'h2-convT-bwd-acc': ('igemm_kernel<64,128,2,2,c32,f16x2>',),
    'x3-convT-wgrad': ('wgrad_kernel<64,64,2,2,1,c32>',),
    'h2-convT-wgrad': ('wgrad_tr_kernel<64,64,f16x2>',),
    'bf16s-convT-wgrad': ('wgrad_kernel<64,64,2,2,1,c32,bf16,bf16hbm>',),
    'f32-direct-fwd': ('direct3x3_n32_kernel',),
    'bf16m-direct-fwd': ('direct3x3_n32_kernel<bf16>',),
    'bf16s-direct-fwd': ('direct3x3_n32_kernel<bf16hbm>',),
    'x3-direct-fwd': ('direct3x3_n32_kernel<f32x3>',),
    'h2-direct-fwd': ('direct3x3_n32_kernel<f16x2>',),
    'x3-direct-bwd': ('direct3x3_n32_kernel<f32x3>',),
    'x3-stem-fwd': ('stem7x7_kernel<rgb>',),
    'bf16s-stem-fwd-stats': ('stem7x7_kernel<rgb>',),
    'x3-stem-wgrad': ('stem7x7_wgrad_kernel<rgb>',),
    'f32-stem-fwd-30x50': ('igemm_kernel<128,64,2,2,rgb>',),
    'f32-rgb-fwd-128': ('igemm_kernel<128,128,2,2,rgb>',),
    'f32-rgb-fwd-64-ldy': ('igemm_kernel<128,64,2,2,rgb>',),
    'f32-rgb-fwd-96': ('igemm_kernel<128,32,4,1,rgb>',),
    'f32-rgb-wgrad-64': ('wgrad_kernel<64,64,2,2,1,rgb>',),
    'f32-rgb-wgrad-96': ('wgrad_kernel<32,64,1,2,2,rgb>',),
    'bf16s-rgb-fwd-128': ('igemm_kernel<128,128,2,2,rgb,bf16out>',),
    'bf16s-rgb-fwd-64-ldy': ('igemm_kernel<128,64,2,2,rgb,bf16out>',),
    'bf16s-rgb-fwd-96': ('igemm_kernel<128,32,4,1,rgb,bf16out>',),
    'bf16s-rgb-wgrad-64': ('wgrad_kernel<64,64,2,2,1,rgb,bf16hbm>',),
    'bf16s-rgb-wgrad-96': ('wgrad_kernel<32,64,1,2,2,rgb,bf16hbm>',),
    'f32-wgrad-alltaps': ('wgrad_alltaps_kernel',),
    'bf16m-wgrad-alltaps': ('wgrad_alltaps_kernel<bf16>',),
    'bf16s-wgrad-alltaps': ('wgrad_alltaps64_kernel<bf16hbm>',),
    'x3-wgrad-alltaps': ('wgrad_alltaps64_kernel<f32x3>',),
    'h2-wgrad-alltaps': ('wgrad_alltaps64_kernel<f16x2>',),
    'x3-wgrad-alltaps-96-dual': ('wgrad_alltaps_kernel<f32x3>',),
    'h2-wgrad-alltaps-96-dual': ('wgrad_alltaps_kernel<f16x2>',),
    'bf16s-wgrad-alltaps-96-dual': ('wgrad_alltaps_kernel<bf16hbm>',),
    'x3-wgrad-alltaps64-dual': ('wgrad_alltaps64_kernel<f32x3>',),
    'h2-wgrad-alltaps64-dual': ('wgrad_alltaps64_kernel<f16x2>',),
    'bf16s-wgrad-alltaps64-dual': ('wgrad_alltaps64_kernel<bf16hbm>',),
    'x3-wgrad-tr-128': ('wgrad_tr_kernel<128,128,f32x3>',),
    'x3-wgrad-tr-64': ('wgrad_tr_kernel<64,64,f32x3>',),
    'h2-wgrad-tr-128': ('wgrad_tr_kernel<128,128,f16x2>',),
    'h2-wgrad-tr-64': ('wgrad_tr_kernel<64,64,f16x2>',),
    'bf16s-wgrad-tr-128': ('wgrad_tr_kernel<128,128,bf16hbm>',),
    'bf16s-wgrad-tr-64': ('wgrad_tr_kernel<64,64,bf16hbm>',),
    'f32-wgrad-128x128-k1s1d1': ('wgrad_kernel<128,128,2,2,1,c32>',),
    'f32-wgrad-64x64-k3s2d1': ('wgrad_kernel<64,64,2,2,1,c32>',),
    'f32-wgrad-64x96-k3s1d1': ('wgrad_kernel<64,32,2,1,2,c32>',),
    'f32-wgrad-96x64-k3s1d2': ('wgrad_kernel<32,64,1,2,2,c32>',),
    'f32-wgrad-96x96-k1s2d1': ('wgrad_kernel<32,32,1,1,4,c32>',),
    'bf16m-wgrad-128x128-k1s1d1': ('wgrad_kernel<128,128,2,2,1,c32,bf16>',),
    'bf16m-wgrad-64x64-k3s2d1': ('wgrad_kernel<64,64,2,2,1,c32,bf16>',),
    'bf16m-wgrad-64x96-k3s1d1': ('wgrad_kernel<64,32,2,1,2,c32,bf16>',),
    'bf16m-wgrad-96x64-k3s1d2': ('wgrad_kernel<32,64,1,2,2,c32,bf16>',),
    'bf16m-wgrad-96x96-k1s2d1': ('wgrad_kernel<32,32,1,1,4,c32>',),
    'bf16s-wgrad-128x128-k1s1d1': ('wgrad_kernel<128,128,2,2,1,c32,bf16,bf16hbm>',),
    'bf16s-wgrad-64x64-k3s2d1': ('wgrad_kernel<64,64,2,2,1,c32,bf16,bf16hbm>',),
    'bf16s-wgrad-64x96-k3s1d1': ('wgrad_kernel<64,32,2,1,2,c32,bf16,bf16hbm>',),
    'bf16s-wgrad-96x64-k3s1d2': ('wgrad_kernel<32,64,1,2,2,c32,bf16,bf16hbm>',),
    'bf16s-wgrad-96x96-k1s2d1': ('wgrad_kernel<32,32,1,1,4,c32,bf16hbm>',),
    'f32-wgrad-cin-real-50': ('wgrad_kernel<64,64,2,2,1,c32>',),
    'x3-wgrad-3x3s2-dual': ('wgrad_kernel<32,32,1,1,4,c32>',),
}


# ---- buffers ----------------------------------------------------------------------------------------------------------

class Buf:
    """rows x cols elements with row stride ld, inside an allocation whose remainder (64 elements before, two rows and 64
    elements after, columns cols..ld) is the guard"""
    PRE = 64

    def __init__(self, rows, cols, ld=None, dtype=torch.float32):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld or cols, dtype
        body = rows * self.ld
        self.flat = torch.empty(self.PRE + body + 2 * self.ld + 64, dtype=dtype, device=DEV)
        self.view = self.flat[self.PRE:self.PRE + body].view(rows, self.ld)[:, :cols]
        self.guard = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        self.guard[self.PRE:self.PRE + body].view(rows, self.ld)[:, :cols] = False

    def fill(self, poison, content=None):
        self.flat.fill_(poison)
        if content is not None:
            self.view.copy_(content.reshape(self.rows, self.cols))
        return self

    @property
    def ptr(self):
        return self.view.data_ptr()

    @staticmethod
    def _bits(t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def guards_hold(self, poison):
        ref = self._bits(torch.full((1,), poison, dtype=self.dtype, device=DEV))
        return bool((self._bits(self.flat)[self.guard] == ref).all())

    def bits(self):
        return self._bits(self.view.contiguous()).clone()


def _ws(nbytes, poison, bufs):
    if not nbytes:
        return None
    b = Buf(1, (int(nbytes) + 3) // 4).fill(poison)
    bufs.append(b)
    return b


def _slots_of(t):
    from xview2_amd._capi import call
    s = torch.zeros(2048, dtype=torch.int32, device=DEV)
    t = t.contiguous()
    call("xv2_tensor_amax", t, t.numel(), s)
    return s


@contextlib.contextmanager
def _forced_tile(spec):
    """XV2_FORCE_TILE for the span (the planner re-reads it at every call; memoised workspace sizes are dropped on both sides)"""
    from xview2_amd import _capi
    old = os.environ.get("XV2_FORCE_TILE")
    try:
        if spec:
            os.environ["XV2_FORCE_TILE"] = spec
        else:
            os.environ.pop("XV2_FORCE_TILE", None)
        _capi.query_cache_clear()
        yield
    finally:
        if old is None:
            os.environ.pop("XV2_FORCE_TILE", None)
        else:
            os.environ["XV2_FORCE_TILE"] = old
        _capi.query_cache_clear()


# ---- one case -------------------------------------------------------------------------------------------------------

def _data(c):
    """operands of the case (CPU fp32; values a bf16 tensor holds in the bf16 modes): x [N,H,W,C0+C1], w [Cout,Cin,k,k],
    dy [N,OH,OW,Cout] (gbwd: both groups), bias, fused-epilogue operands, accumulation bases"""
    gen = torch.Generator().manual_seed(zlib.crc32(c.cid.encode()))
    bf = c.mode in ("bf16s", "bf16m")
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    G = 2 if c.op == "gbwd" else 1
    Ctot = c.C0 + c.C1
    cin = 3 if c.C0 == 4 else Ctot
    D = {}
    x = R.lognormal((c.N, c.H, c.W, Ctot), gen)
    if c.C0 == 4:
        x[..., 3] = 0.0
    D["x"] = rnd(x)
    w = torch.randn((G * c.Cout, cin, c.k, c.k), generator=gen, dtype=torch.float64)
    w = w * torch.exp(0.5 * torch.randn((G * c.Cout, 1, 1, 1), generator=gen, dtype=torch.float64)) / math.sqrt(cin * c.k * c.k)
    D["w"] = rnd(w.float())
    D["dy"] = rnd(R.lognormal((c.N, c.OH, c.OW, G * c.Cout), gen))
    D["bias"] = rnd(torch.randn(c.Cout, generator=gen)) if c.bias else None
    if c.op == "fused":
        D["scale"] = rnd(1.0 + 0.5 * torch.rand(c.Cout, generator=gen))
        D["shift"] = rnd(torch.randn(c.Cout, generator=gen))
        D["res"] = rnd(torch.randn((c.N, c.OH, c.OW, c.Cout), generator=gen))
    D["base_in"] = rnd(torch.randn((c.N, c.H, c.W, G * Ctot), generator=gen))       # accumulation bases (large-grid side)
    D["base_out"] = rnd(torch.randn((c.N, c.OH, c.OW, c.Cout), generator=gen))     # (small-grid side: convT backward-data)
    return D


def _packed(w, Cout, Cin, k, cin_pad, which, wdt, poison, bufs):
    """xv2_pack_weight into a guarded view: which = "ohwi" ([Cout][T][cin_pad]) or "ihwo" ([cin_pad][T][Cout])"""
    from xview2_amd._capi import call
    T = k * k
    b = Buf(Cout, T * cin_pad, None, wdt) if which == "ohwi" else Buf(cin_pad, T * Cout, None, wdt)
    b.fill(poison)
    bufs.append(b)
    wd = w.to(DEV).contiguous()
    call("xv2_pack_weight", wd, Cout, Cin, k, k, cin_pad, b.ptr if which == "ohwi" else None, b.ptr if which == "ihwo" else None,
         1 if wdt == torch.bfloat16 else 0)
    return b


def _register(mode, packs, keep):
    """what the mode needs beside each packed weight operand (the library keys it by the operand's address)"""
    from xview2_amd._capi import call, query
    for b, rows, T, ct in packs:
        if mode == "wx3":
            assert query("xv2_presplit_supported", rows, T, ct) == 1
            x3 = torch.empty((query("xv2_presplit_bytes", rows, T, ct) // 2,), dtype=torch.bfloat16, device=DEV)
            call("xv2_presplit_weights", b.ptr, rows, T, ct, x3)
            keep.append(x3)
        elif mode in ("h2", "h2pt"):
            s = torch.zeros(2048, dtype=torch.int32, device=DEV)
            call("xv2_tensor_amax", b.ptr, rows * T * ct, s)
            query("xv2_weight_amax_register", b.ptr, s)
            keep.append(s)
            if mode == "h2" and query("xv2_presplit_f16_supported", rows, T, ct) == 1:
                x2 = torch.empty((query("xv2_presplit_f16_bytes", rows, T, ct) // 2,), dtype=torch.float16, device=DEV)
                call("xv2_presplit_weights_f16", b.ptr, rows, T, ct, x2, s)
                keep.append(x2)


def _launch(c, D, poison):
    """one run: -> (profiler names, {result: Buf}, [every Buf], statistics (Buf, tile rows) or None, split-K workspace bytes of
    a forward / backward-data plan)"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query, set_amax
    hs = c.mode == "bf16s"
    h2 = c.mode in ("h2", "h2pt")
    adt = torch.bfloat16 if hs else torch.float32
    rgb = c.C0 == 4
    xdt = torch.float32 if rgb else adt          # the RGB image of a stem stays fp32 (include/xv2.h)
    wdt = torch.float32 if rgb else adt
    Ctot = c.C0 + c.C1
    cin = 3 if rgb else Ctot
    T = c.k * c.k
    Mi, Mo = c.N * c.H * c.W, c.N * c.OH * c.OW
    g = ops.conv_cfg(c.k, c.k, c.s, c.pad, c.dil, math=MATH[c.mode])
    d = ops._desc(c.N, c.H, c.W, c.C0, c.C1, c.Cout, g, c.OH, c.OW, hs)
    bufs, keep, packs, outs, stats, wsb = [], [], [], {}, None, None

    def hold(t):
        """the maximum slots of t, kept alive until the call has run (set_amax hands the library their address only)"""
        keep.append(_slots_of(t))
        return keep[-1]

    def src(t, rows, cols, extra, dt):
        b = Buf(rows, cols, cols + extra, dt).fill(poison, t.to(DEV))
        bufs.append(b)
        return b

    def dst(rows, cols, extra, base=None):
        b = Buf(rows, cols, cols + extra, adt).fill(poison, None if base is None else base.to(DEV))
        bufs.append(b)
        return b

    x, w, dy = D["x"], D["w"], D["dy"]
    with _forced_tile(c.tile):
        try:
            if c.op in ("fwd", "fused", "wgrad"):
                x0 = src(x[..., :c.C0], Mi, c.C0, c.ldx, xdt)
                x1 = src(x[..., c.C0:], Mi, c.C1, c.ldx, xdt) if c.C1 else None
                ax = (hold(x[..., :c.C0].to(DEV)), hold(x[..., c.C0:].to(DEV)) if c.C1 else None) if h2 else None
            if c.op in ("fwd", "fused"):
                ohwi = _packed(w, c.Cout, cin, c.k, 4 if rgb else Ctot, "ohwi", wdt, poison, bufs)
                packs.append((ohwi, c.Cout, T, 4 if rgb else Ctot))
                _register(c.mode, packs, keep)
                wsb = query("xv2_conv2d_forward_workspace", d)
                ws = _ws(wsb, poison, bufs)
                y = outs["y"] = dst(Mo, c.Cout, c.ldy)
                if c.op == "fused":
                    sc, sh = D["scale"].to(DEV), D["shift"].to(DEV)
                    res = src(D["res"], Mo, c.Cout, 0, adt)
                    if h2:
                        set_amax(*ax)
                    with _prof() as pr:
                        call("xv2_conv2d_forward_fused", d, x0.ptr, x0.ld, x1.ptr if x1 else None, x1.ld if x1 else 0, ohwi.ptr,
                             sc, sh, res.ptr, res.ld, ops.ACTS["relu"], y.ptr, y.ld, ws.ptr if ws else None)
                        names = pr.names()
                else:
                    if c.stats:
                        tiles = query("xv2_conv2d_forward_stats_tiles", d)
                        stats = (Buf(tiles, 2 * c.Cout).fill(poison), query("xv2_conv2d_forward_stats_tile_rows", d))
                        bufs.append(stats[0])
                    bias = D["bias"].to(DEV) if c.bias else None
                    if h2:
                        set_amax(*ax)
                    with _prof() as pr:
                        call("xv2_conv2d_forward", d, x0.ptr, x0.ld, x1.ptr if x1 else None, x1.ld if x1 else 0, ohwi.ptr, bias,
                             y.ptr, y.ld, stats[0].ptr if stats else None, ws.ptr if ws else None)
                        names = pr.names()
            elif c.op == "wgrad":
                dyb = src(dy, Mo, c.Cout, c.ldy, adt)
                cr = c.cin_real or cin
                dw = outs["dw"] = Buf(c.Cout, cr * T).fill(poison)
                bufs.append(dw)
                ws = _ws(query("xv2_conv2d_backward_weight_workspace", d), poison, bufs)
                if h2:
                    set_amax(ax[0], ax[1], hold(dy.to(DEV)))
                with _prof() as pr:
                    call("xv2_conv2d_backward_weight", d, x0.ptr, x0.ld, x1.ptr if x1 else None, x1.ld if x1 else 0, dyb.ptr,
                         dyb.ld, dw.ptr, cr, ws.ptr if ws else None)
                    names = pr.names()
            elif c.op == "bwd":
                dyb = src(dy, Mo, c.Cout, c.ldx, adt)
                ihwo = _packed(w, c.Cout, Ctot, c.k, Ctot, "ihwo", wdt, poison, bufs)
                packs.append((ihwo, Ctot, T, c.Cout))
                _register(c.mode, packs, keep)
                base = D["base_in"]
                dx0 = outs["dx0"] = dst(Mi, c.C0, c.ldy, base[..., :c.C0] if c.acc & 1 else None)
                dx1 = outs["dx1"] = dst(Mi, c.C1, c.ldy, base[..., c.C0:Ctot] if c.acc & 2 else None) if c.C1 else None
                if dx1 is None:
                    del outs["dx1"]
                wsb = query("xv2_conv2d_backward_data_workspace", d)
                ws = _ws(wsb, poison, bufs)
                if h2:
                    set_amax(None, None, hold(dy.to(DEV)))
                with _prof() as pr:
                    if c.acc:
                        call("xv2_conv2d_backward_data_acc", d, dyb.ptr, dyb.ld, ihwo.ptr, dx0.ptr, dx0.ld,
                             dx1.ptr if dx1 else None, dx1.ld if dx1 else 0, c.acc, ws.ptr if ws else None)
                    else:
                        call("xv2_conv2d_backward_data", d, dyb.ptr, dyb.ld, ihwo.ptr, dx0.ptr, dx0.ld,
                             dx1.ptr if dx1 else None, dx1.ld if dx1 else 0, ws.ptr if ws else None)
                    names = pr.names()
            elif c.op == "gbwd":
                G = 2
                dyb = src(dy, Mo, G * c.Cout, c.ldx, adt)
                gp = [_packed(w[i * c.Cout:(i + 1) * c.Cout], c.Cout, c.C0, c.k, c.C0, "ihwo", wdt, poison, bufs) for i in range(G)]
                packs.extend((b, c.C0, T, c.Cout) for b in gp)
                _register(c.mode, packs, keep)
                dx = outs["dx"] = dst(Mi, G * c.C0, c.ldy, D["base_in"][..., :G * c.C0] if c.acc else None)
                ws = _ws(query("xv2_conv2d_backward_data_workspace", d), poison, bufs)
                warr = (ctypes.c_void_p * G)(*[b.ptr for b in gp])
                if h2:
                    set_amax(None, None, hold(dy.to(DEV)))
                with _prof() as pr:
                    call("xv2_conv2d_backward_data_grouped", d, G, dyb.ptr, dyb.ld, ctypes.addressof(warr), dx.ptr, dx.ld,
                         1 if c.acc else 0, ws.ptr if ws else None, 1 if hs else 0)
                    names = pr.names()
            elif c.op == "tfwd":      # ConvTranspose2d forward = backward-data of the equivalent convolution
                xs = src(dy, Mo, c.Cout, c.ldx, adt)
                ihwo = _packed(w, c.Cout, c.C0, c.k, c.C0, "ihwo", wdt, poison, bufs)
                packs.append((ihwo, c.C0, T, c.Cout))
                _register(c.mode, packs, keep)
                y = outs["y"] = dst(Mi, c.C0, c.ldy)
                if h2:
                    set_amax(None, None, hold(dy.to(DEV)))
                with _prof() as pr:
                    call("xv2_conv_transpose2d_forward", d, xs.ptr, xs.ld, ihwo.ptr, y.ptr, y.ld)
                    names = pr.names()
            elif c.op == "tbwd":      # its backward-data = forward of the equivalent convolution
                dyb = src(x, Mi, c.C0, c.ldx, adt)
                ohwi = _packed(w, c.Cout, c.C0, c.k, c.C0, "ohwi", wdt, poison, bufs)
                packs.append((ohwi, c.Cout, T, c.C0))
                _register(c.mode, packs, keep)
                dx = outs["dx"] = dst(Mo, c.Cout, c.ldy, D["base_out"] if c.acc else None)
                ws = _ws(query("xv2_conv2d_forward_workspace", d), poison, bufs) if c.acc else None
                if h2:
                    set_amax(hold(x.to(DEV)))
                with _prof() as pr:
                    if c.acc:
                        call("xv2_conv_transpose2d_backward_data_acc", d, dyb.ptr, dyb.ld, ohwi.ptr, dx.ptr, dx.ld, 1,
                             ws.ptr if ws else None)
                    else:
                        call("xv2_conv_transpose2d_backward_data", d, dyb.ptr, dyb.ld, ohwi.ptr, dx.ptr, dx.ld)
                    names = pr.names()
            elif c.op == "twgrad":    # its weight gradient = that of the equivalent convolution (X = dy, dY = x)
                xs = src(dy, Mo, c.Cout, c.ldx, adt)
                dyb = src(x, Mi, c.C0, c.ldx, adt)
                dw = outs["dw"] = Buf(c.Cout, c.C0 * T).fill(poison)
                bufs.append(dw)
                ws = _ws(query("xv2_conv2d_backward_weight_workspace", d), poison, bufs)
                if h2:
                    set_amax(hold(x.to(DEV)), None, hold(dy.to(DEV)))
                with _prof() as pr:
                    call("xv2_conv_transpose2d_backward_weight", d, xs.ptr, xs.ld, dyb.ptr, dyb.ld, dw.ptr, ws.ptr if ws else None)
                    names = pr.names()
            else:
                raise ValueError(c.op)
            torch.cuda.synchronize()
        finally:
            set_amax()
            for b, _, _, _ in packs:
                query("xv2_presplit_forget", b.ptr)
    return tuple(names), outs, bufs, stats, wsb


def _reference(c, D):
    """{result: (y64, a, s, K, amax)} on the device, float64"""
    x, w, dy = (D[k].to(DEV).double() for k in ("x", "w", "dy"))
    rgb = c.C0 == 4
    cin = 3 if rgb else c.C0 + c.C1
    out = {}
    if c.op in ("fwd", "fused"):
        f = lambda A, B: R.conv_fwd(A, B, c.s, c.pad, c.dil)
        X = x[..., :cin]
        y64 = f(X, w)
        a, s = R.scales(f, X, w)
        amax = (float(X.abs().max()), float(w.abs().max()))
        if c.bias:
            b = D["bias"].to(DEV).double()
            y64, a, s = y64 + b, a + b.abs(), (s * s + b * b).sqrt()
        if c.op == "fused":
            sc, sh, res = (D[k].to(DEV).double() for k in ("scale", "shift", "res"))
            y64 = torch.relu(y64 * sc + sh + res)
            a = a * sc.abs() + sh.abs() + res.abs()
            s = (s * s * sc * sc + sh * sh + res * res).sqrt()
        out["y"] = (y64, a, s, cin * c.k * c.k, amax)
    elif c.op in ("bwd", "gbwd"):
        G = 2 if c.op == "gbwd" else 1
        f = lambda A, B: R.conv_bwd_data(A, B, (c.H, c.W), c.s, c.pad, c.dil, G)
        y64 = f(dy, w)
        a, s = R.scales(f, dy, w)
        if c.op == "gbwd":
            if c.acc:
                base = D["base_in"][..., :G * c.C0].to(DEV).double()
                y64, a, s = y64 + base, a + base.abs(), (s * s + base * base).sqrt()
            out["dx"] = (y64, a, s, c.Cout * c.k * c.k, (float(dy.abs().max()), float(w.abs().max())))
        else:
            base = D["base_in"][..., :c.C0 + c.C1].to(DEV).double()
            for name, lo, hi, bit in (("dx0", 0, c.C0, 1), ("dx1", c.C0, c.C0 + c.C1, 2)):
                if hi == lo:
                    continue
                yy, aa, ss = y64[..., lo:hi], a[..., lo:hi], s[..., lo:hi]
                if c.acc & bit:
                    bb = base[..., lo:hi]
                    yy, aa, ss = yy + bb, aa + bb.abs(), (ss * ss + bb * bb).sqrt()
                out[name] = (yy, aa, ss, c.Cout * c.k * c.k, (float(dy.abs().max()), float(w.abs().max())))
    elif c.op == "wgrad":
        cr = c.cin_real or cin
        f = lambda A, B: R.conv_bwd_weight(A, B, (c.Cout, cin, c.k, c.k), c.s, c.pad, c.dil)
        X = x[..., :cin]
        y64 = f(X, dy)[:, :cr]
        a, s = R.scales(f, X, dy)
        out["dw"] = (y64, a[:, :cr], s[:, :cr], c.N * c.OH * c.OW, (float(X.abs().max()), float(dy.abs().max())))
    elif c.op == "tfwd":
        f = R.convT_fwd
        a, s = R.scales(f, dy, w)
        out["y"] = (f(dy, w), a, s, c.Cout, (float(dy.abs().max()), float(w.abs().max())))
    elif c.op == "tbwd":
        f = R.convT_bwd_data
        y64 = f(x, w)
        a, s = R.scales(f, x, w)
        if c.acc:
            b = D["base_out"].to(DEV).double()
            y64, a, s = y64 + b, a + b.abs(), (s * s + b * b).sqrt()
        out["dx"] = (y64, a, s, c.C0 * 4, (float(x.abs().max()), float(w.abs().max())))
    elif c.op == "twgrad":
        f = R.convT_bwd_weight
        a, s = R.scales(f, dy, x)
        out["dw"] = (f(dy, x), a, s, c.N * c.OH * c.OW, (float(dy.abs().max()), float(x.abs().max())))
    return out


def _stats_error(c, y, stats):
    """largest error of the statistics partials [tile][Cout][2] against sums (float64) of what the kernel stored, relative to
    a bound of 4 x rows x u x sum |term| (an fp32 sum of `rows` terms)"""
    buf, rows = stats
    yk = y.view.double()
    M = yk.shape[0]
    tiles = buf.rows
    pad = torch.zeros((tiles * rows - M, yk.shape[1]), dtype=torch.float64, device=DEV)
    yt = torch.cat([yk, pad]).view(tiles, rows, -1)
    p = buf.view.double().view(tiles, -1, 2)
    worst = 0.0
    for j, v in ((0, yt), (1, yt * yt)):
        ref, mag = v.sum(1), v.abs().sum(1)
        err = (p[..., j] - ref).abs()
        b = 4.0 * rows * R.U * mag + 1e-30
        worst = max(worst, float((err / b).nan_to_num(math.inf).max()))
    return worst


def _evaluate(c):
    """both runs of a case, compared: -> record dict"""
    rec = {"case": c.cid, "mode": c.mode, "names": None, "outs": {}, "identical": None, "guards": None, "stats": None,
           "ws_bytes": None, "error": None}
    try:
        D = _data(c)
        runs = []
        for poison in POISONS:
            names, outs, bufs, stats, wsb = _launch(c, D, poison)
            bad = [i for i, b in enumerate(bufs) if not b.guards_hold(poison)]
            runs.append((names, {k: b.bits() for k, b in outs.items()}, stats[0].bits() if stats else None, bad, outs, stats))
        rec["names"] = list(runs[0][0])
        rec["ws_bytes"] = wsb
        rec["identical"] = (runs[0][0] == runs[1][0] and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
                            and (runs[0][2] is None or torch.equal(runs[0][2], runs[1][2])))
        rec["guards"] = not runs[0][3] and not runs[1][3]
        outs, stats = runs[1][4], runs[1][5]
        ref = _reference(c, D)
        fam = FAMILY[c.mode]
        for k, (y64, a, s, K, amax) in ref.items():
            bf16_out = c.mode == "bf16s" and k != "dw"
            y = outs[k].view.reshape(y64.shape)
            r = R.check(y, y64, a, s, K, fam, bf16_out=bf16_out, amax=amax)
            rec["outs"][k] = {"el": r["el"], "rms": r["rms"], "ok": r["ok"], "where": r["where"], "K": K}
        if stats:
            rec["stats"] = _stats_error(c, outs["y"], stats)
    except Exception as e:      # (a call the library refuses; reported by the case)
        rec["error"] = "%s: %s" % (type(e).__name__, e)
    return rec


_SEEN = {}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.cid)
def test_variant_case_against_float64(case):
    rec = _SEEN[case.cid] = _evaluate(case)
    if RECORD:
        return
    assert rec["error"] is None, rec["error"]
    assert tuple(rec["names"]) == tuple(EXPECT[case.cid]), (rec["names"], EXPECT[case.cid])
    assert rec["guards"], "a guard around an operand, output or workspace changed"
    assert rec["identical"], "the NaN-poisoned and the 2^100-poisoned runs differ"
    for k, o in rec["outs"].items():
        assert o["ok"], (k, o)
    if rec["stats"] is not None:
        assert rec["stats"] <= 1.0, rec["stats"]
    if case.split is True:          # a split-K plan of the planner's own: it asks for slabs
        assert rec["ws_bytes"], rec["ws_bytes"]
    elif case.split:                # the forced factor: ks slabs of M x Nout fp32 partial sums (igemm_splitk_bytes)
        M, Nout = ((case.N * case.OH * case.OW, case.Cout) if case.op in ("fwd", "fused") else
                   (case.N * case.H * case.W, case.C0 + case.C1))
        assert rec["ws_bytes"] == case.split * M * Nout * 4, (rec["ws_bytes"], case.split, M, Nout)


def test_every_variant_is_reached_within_its_bounds():
    """the table the suite prints: per VARIANTS entry the case that reached it and the worst ratio to its bounds; every entry
    that is not ablation-only must be reached (cases not run in this session run here)"""
    for c in CASES:
        if c.cid not in _SEEN:
            _SEEN[c.cid] = _evaluate(c)
    best = {}
    for c in CASES:
        r = _SEEN[c.cid]
        worst = max([max(o["el"], o["rms"]) for o in r["outs"].values()] or [math.inf])
        for n in r["names"] or ():
            if n not in best or worst > best[n][1]:
                best[n] = (c.cid, worst)
    print("\n%-62s %-44s %s" % ("variant", "case", "worst error / bound"))
    for key, name in VARIANTS.items():
        cid, worst = best.get(name, ("-", math.nan))
        print("%-62s %-44s %.3f" % (name, cid, worst))
    others = sorted(set(best) - set(VARIANTS.values()))
    for name in others:
        print("%-62s %-44s %.3f" % (name, best[name][0], best[name][1]))
    if RECORD:
        fam = {}
        for c in CASES:
            r = _SEEN[c.cid]
            for o in r["outs"].values():
                f = fam.setdefault(FAMILY[c.mode], [0.0, 0.0])
                f[0], f[1] = max(f[0], o["el"] * R.EL[FAMILY[c.mode]]), max(f[1], o["rms"] * R.TAU_RMS[FAMILY[c.mode]])
        with open(RECORD, "w") as fh:
            json.dump({"cases": [_SEEN[c.cid] for c in CASES], "family_raw_max": fam}, fh, indent=1, default=str)
        return
    missing = [k for k, v in VARIANTS.items() if not v.startswith("ablation-only") and v not in best]
    assert not missing, missing


# ---- operands near the 2 GiB guard of the 32-bit buffer offsets (igemm_conv.hip conv_forward_impl / dgrad_impl) --------

GIB2 = 1 << 31


def _per_image_check(y, y64, a, s, K, fam, tag):
    r = R.check(y, y64, a, s, K, fam)
    assert r["ok"], (tag, r)


def test_forward_with_an_input_one_image_row_below_2_GiB():
    """x0 = 255 x 257 x 128 pixels x 64 fp32 channels = 2^31 bytes minus one image row: runs; images 0 and N-1 match float64"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query
    N, H, W, C, Co = 255, 257, 128, 64, 64
    assert N * H * W * C * 4 == GIB2 - W * C * 4
    g = ops.conv_cfg(3, 3, 1, 1, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, C, 0, Co, g, H, W)
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((N, H, W, C), generator=gen, device=DEV)
    w = torch.randn((Co, C, 3, 3), generator=gen, device=DEV) / 24.0
    ohwi = torch.empty((Co, 9, C), device=DEV)
    call("xv2_pack_weight", w, Co, C, 3, 3, C, ohwi, None, 0)
    y = torch.full((N, H, W, Co), float("nan"), device=DEV)
    assert query("xv2_conv2d_forward_workspace", d) == 0
    with _prof() as pr:
        call("xv2_conv2d_forward", d, x, C, None, 0, ohwi, None, y, Co, None, None)
        assert pr.names() == ["igemm_kernel<128,64,2,2,c32,f32x3>"]      # (OH % 4 != 0: the per-tap form)
    f = lambda A, B: R.conv_fwd(A, B, 1, 1, 1)
    for i in (0, N - 1):
        xi = x[i:i + 1].double()
        a, s = R.scales(f, xi, w)
        _per_image_check(y[i:i + 1], f(xi, w), a, s, C * 9, "f32x3", i)


def test_forward_one_image_past_2_GiB_is_refused_before_any_launch():
    """one image more than the guard allows: the documented error, and the output is untouched"""
    from xview2_amd import ops
    from xview2_amd._capi import call
    N, H, W, C, Co = 256, 257, 128, 64, 64
    g = ops.conv_cfg(3, 3, 1, 1, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, C, 0, Co, g, H, W)
    x = torch.zeros((N, H, W, C), device=DEV)
    ohwi = torch.zeros((Co, 9, C), device=DEV)
    y = torch.full((N, 1, 1, Co), 7.0, device=DEV)       # (never written: the call must fail before it launches)
    with _prof() as pr:
        with pytest.raises(RuntimeError, match="2 GiB"):
            call("xv2_conv2d_forward", d, x, C, None, 0, ohwi, None, y, Co, None, None)
        assert pr.names() == []
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_backward_data_with_dy_one_image_row_below_2_GiB():
    """dy = 255 x 257 x 128 pixels x 64 fp32 channels = 2^31 bytes minus one image row (the guard of dgrad_impl): runs;
    images 0 and N-1 match float64"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query
    N, H, W, Ci, Co = 255, 257, 128, 64, 64
    assert N * H * W * Co * 4 == GIB2 - W * Co * 4
    g = ops.conv_cfg(3, 3, 1, 1, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, Ci, 0, Co, g, H, W)
    gen = torch.Generator(device=DEV).manual_seed(14)
    dy = torch.randn((N, H, W, Co), generator=gen, device=DEV)
    w = torch.randn((Co, Ci, 3, 3), generator=gen, device=DEV) / 24.0
    ihwo = torch.empty((Ci, 9, Co), device=DEV)
    call("xv2_pack_weight", w, Co, Ci, 3, 3, Ci, None, ihwo, 0)
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    assert query("xv2_conv2d_backward_data_workspace", d) == 0
    with _prof() as pr:
        call("xv2_conv2d_backward_data", d, dy, Co, ihwo, dx, Ci, None, 0, None)
        assert pr.names() == ["igemm_kernel<128,64,2,2,c32,f32x3>"]
    f = lambda A, B: R.conv_bwd_data(A, B, (H, W), 1, 1, 1)
    for i in (0, N - 1):
        di = dy[i:i + 1].double()
        a, s = R.scales(f, di, w)
        _per_image_check(dx[i:i + 1], f(di, w), a, s, Co * 9, "f32x3", i)
    del dx, dy


def test_backward_data_with_dy_past_2_GiB_is_refused_before_any_launch():
    from xview2_amd import ops
    from xview2_amd._capi import call
    N, H, W, Ci, Co = 256, 257, 128, 64, 64
    g = ops.conv_cfg(3, 3, 1, 1, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, Ci, 0, Co, g, H, W)
    dy = torch.zeros((N, H, W, Co), device=DEV)
    ihwo = torch.zeros((Ci, 9, Co), device=DEV)
    dx = torch.full((N, 1, 1, Ci), 7.0, device=DEV)
    with _prof() as pr:
        with pytest.raises(RuntimeError, match="2 GiB"):
            call("xv2_conv2d_backward_data", d, dy, Co, ihwo, dx, Ci, None, 0, None)
        assert pr.names() == []
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all())


def test_stride2_backward_data_with_dx_above_2_GiB_and_dy_below():
    """3x3 / stride 2 backward-data: dy = 151 MB, dx = 9 x 512^2 x 256 fp32 = 2.25 GiB (no guard checks dx: the epilogue
    addresses it with size_t); images 0 and N-1 match float64"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query
    N, H, W, Ci, Co = 9, 512, 512, 256, 64
    assert N * H * W * Ci * 4 > GIB2 and N * (H // 2) * (W // 2) * Co * 4 < GIB2
    g = ops.conv_cfg(3, 3, 2, 1, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, Ci, 0, Co, g, H // 2, W // 2)
    gen = torch.Generator(device=DEV).manual_seed(12)
    dy = torch.randn((N, H // 2, W // 2, Co), generator=gen, device=DEV)
    w = torch.randn((Co, Ci, 3, 3), generator=gen, device=DEV) / 24.0
    ihwo = torch.empty((Ci, 9, Co), device=DEV)
    call("xv2_pack_weight", w, Co, Ci, 3, 3, Ci, None, ihwo, 0)
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    assert query("xv2_conv2d_backward_data_workspace", d) == 0
    with _prof() as pr:
        call("xv2_conv2d_backward_data", d, dy, Co, ihwo, dx, Ci, None, 0, None)
        assert pr.names() == ["igemm_kernel<128,128,2,2,c32,f32x3>"]
    f = lambda A, B: R.conv_bwd_data(A, B, (H, W), 2, 1, 1)
    for i in (0, N - 1):
        di = dy[i:i + 1].double()
        a, s = R.scales(f, di, w)
        _per_image_check(dx[i:i + 1], f(di, w), a, s, Co * 9, "f32x3", i)
    del dx


def test_weight_gradient_with_an_input_one_image_row_below_2_GiB():
    """x0 one image row below 2^31 bytes: the transpose-read form still runs (its 32-bit offsets); dy is zero except on images
    0 and N-1, so the float64 weight gradient of those two images is the whole one"""
    from xview2_amd import ops
    from xview2_amd._capi import call, query
    N, H, W, C, Co = 255, 257, 128, 64, 64
    g = ops.conv_cfg(1, 1, 1, 0, 1, math=ops.MATH_F32X3)
    d = ops._desc(N, H, W, C, 0, Co, g, H, W)
    gen = torch.Generator(device=DEV).manual_seed(13)
    x = torch.randn((N, H, W, C), generator=gen, device=DEV)
    dy = torch.zeros((N, H, W, Co), device=DEV)
    dy[0].normal_(generator=gen)
    dy[N - 1].normal_(generator=gen)
    dw = torch.full((Co, C, 1, 1), float("nan"), device=DEV)
    ws = torch.full((query("xv2_conv2d_backward_weight_workspace", d) // 4 + 4,), float("nan"), device=DEV)
    with _prof() as pr:
        call("xv2_conv2d_backward_weight", d, x, C, None, 0, dy, Co, dw, C, ws)
        assert pr.names() == ["wgrad_tr_kernel<64,64,f32x3>"]
    idx = torch.tensor([0, N - 1], device=DEV)
    xs, ds = x[idx].double(), dy[idx].double()
    f = lambda A, B: R.conv_bwd_weight(A, B, (Co, C, 1, 1))
    a, s = R.scales(f, xs, ds)
    _per_image_check(dw, f(xs, ds), a, s, 2 * H * W, "f32x3", "dw")      # (zero rows of dy add nothing to the fp32 sums)
