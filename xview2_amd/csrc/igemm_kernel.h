// Implicit-GEMM convolution on the matrix cores of gfx950: the device side of igemm_conv.hip (planner, dispatch, operand
// preparation and the ABI entry points are there).
//
// One kernel template serves every "gather-GEMM" of the U-Net hot path - conv2d forward, conv2d backward-data (stride 1
// directly, stride s as s*s output-parity classes), conv_transpose2d forward (the backward-data of a 2x2/s2 conv) and its
// backward-data (the forward of that conv):
//
//   Out[m][n] = sum_{tap t} sum_{c} A[pix(m, t)][c] * B[n][slot(t)][c]
//
// m runs over the logical output grid (N, OHl, OWl); pix(m,t) = (n, a*s_in + dh[t], b*s_in + dw[t]) (zero outside the
// input); A is NHWC and may be the virtual concatenation of two tensors (channel split C0|C1, K-tiles never straddle the
// split because C0 % 32 == 0).  256 threads = 4 waves, block tile BM x BN x 32, an XCD-aware block order; the epilogue stages
// the tile through LDS: optional bias / inference epilogue, scattered NHWC store through a per-row pixel-offset table, and
// (training) per-channel partial sums and sums of squares for the following BatchNorm.
//
// What differs between the arithmetic modes is the operand path, i.e. the K loop.  The kernel exists in eleven FORMS (enum Form
// below; the flags the body reads are derived from the form in one table):
//   RGB, RGB_BF16OUT   4-channel image source (SMALLC): every float4 is one tap; fp32 image, fp32 weights, exact-fp32 MFMA
//                      (v_mfma_f32_32x32x2_f32); _BF16OUT rounds the output tile to bf16 (bf16 storage)
//   C32                fp32: global -> registers -> LDS (rows padded to 36 floats: conflict-free ds_read_b128), double-buffered,
//                      one barrier per K-tile; a lane reads 4 consecutive k and feeds 4 MFMAs (k order permuted inside a tile,
//                      identically for A and B)
//   BF16               "--precision 16": operands stay fp32 in HBM, are rounded to bf16 (RNE) while being staged into LDS and
//                      multiplied with v_mfma_f32_32x32x16_bf16 (fp32 accumulate)
//   BF16HBM            XV2_MATH_BF16_STORE (HS): activations and packed weights are bf16 IN HBM.  A K-tile row (32 channels) is
//                      64 bytes = 4 lanes x 16 bytes, so a pass of the 256 threads covers 64 rows and the loaded registers go
//                      to the bf16 LDS image as they are; the output tile is rounded to bf16 in the epilogue and the BatchNorm
//                      statistics are taken on the ROUNDED values (what the next kernel will read)
//   F32X3              XV2_MATH_F32X3 (X3): fp32 tensors, each operand element split into three bf16 terms on its way into LDS
//                      (three bf16 planes per operand), six bf16 MFMAs per fp32-grade product
//   F16X2              the same with TWO fp16 planes (NPL = 2) of operands scaled by their recorded maxima, three fp16 MFMAs
//   ..._HALO           3x3 / stride 1 / pad 1 forward and backward-data: the M tile is a 4 x 32 pixel PATCH of one image and
//                      the K loop runs slice-major: the 6 x 34 halo of a channel slice reaches LDS ONCE and serves all nine
//                      taps (shifted fragment addresses) - global loads, operand splits and LDS stores of the activation
//                      operand drop 6.4x; the weight operand streams per tap.  BF16HBM_HALO: both operands by direct-to-LDS
//                      loads; F32X3_HALO: weights split in the kernel
//   F32X3_HALO_WX3,    (BX3) the weight operand arrives PRE-SPLIT (three bf16 / two fp16 planes, xv2_presplit_weights: once per
//   F16X2_HALO         optimizer step) and goes global -> LDS with direct-to-LDS buffer loads: no registers, no split, no
//                      ds_write for it.  PMC had shown the plane stores as the most expensive producer step in clock;
//                      emulated first (garbage data): -12 %
#pragma once
#include "igemm_params.h"
#include <type_traits>

#ifndef XV2_ABL
#define XV2_ABL 0   // debug ablations (scripts/ablate.sh): 1 no global loads, 2 no LDS stores, 4 no MFMA, 8 no epilogue
#endif

#ifndef XV2_HABL
#define XV2_HABL 0      // halo-form ablations (debug): 1 no halo stores, 2 unshifted fragment rows, 4 no weight stores and 8 conflict-free weight reads
                        // (three planes, weights split in the kernel), 16 no MFMA; F16X2 form: 32 no DMA inside the K loop, 64 every second barrier dropped
#endif

namespace xv2 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int N> struct IC { static constexpr int value = N; };
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// The forms of igemm_kernel (the map at the top of this file).  `suffix` is the form's part of the name the launcher registers
// with the profiler: tests, scripts and the committed profiles key on it.
enum class Form { RGB, RGB_BF16OUT, C32, BF16, BF16HBM, BF16HBM_HALO, F32X3, F32X3_HALO, F32X3_HALO_WX3, F16X2, F16X2_HALO };
struct FormTraits {
    const char* suffix;
    bool SMALLC, BF16, HS, X3, HALO, BX3;
    int NPL;
};
constexpr FormTraits FORM_TRAITS[] = {
    // suffix                 SMALLC BF16   HS     X3     HALO   BX3    NPL
    {"rgb",                   true,  false, false, false, false, false, 3},
    {"rgb,bf16out",           true,  false, true,  false, false, false, 3},
    {"c32",                   false, false, false, false, false, false, 3},
    {"c32,bf16",              false, true,  false, false, false, false, 3},
    {"c32,bf16hbm",           false, true,  true,  false, false, false, 3},
    {"c32,bf16hbm,halo",      false, true,  true,  false, true,  false, 3},
    {"c32,f32x3",             false, true,  false, true,  false, false, 3},
    {"c32,f32x3,halo",        false, true,  false, true,  true,  false, 3},
    {"c32,f32x3,halo,wx3",    false, true,  false, true,  true,  true,  3},
    {"c32,f16x2",             false, true,  false, true,  false, false, 2},
    {"c32,f16x2,halo,wx2",    false, true,  false, true,  true,  true,  2},
};
constexpr FormTraits form_traits(Form f) { return FORM_TRAITS[(int)f]; }
// waves of a block along M: 128 x 32 tiles 4 x 1, every other tile 2 x 2
constexpr int tile_wgm(int BN) { return BN == 32 ? 4 : 2; }

constexpr int LDS_LD = BK + 4;
constexpr int LDS_LD_H = BK + 8;   // bf16 row stride in elements (80 bytes: conflict-free 16-byte fragment reads)
// floats of LDS shared by the main-loop operand buffers and the epilogue staging tile
template <Form F, int BM, int BN>
constexpr int igemm_main_floats() {
    constexpr bool HIN = form_traits(F).HS && !form_traits(F).SMALLC, HALO = form_traits(F).HALO;
    constexpr int NPL = form_traits(F).NPL, NH = (HIN && tile_wgm(BN) >= 2) ? 2 : 1;      // NH: epilogue staging passes
    if (NPL == 2 && !HALO && !HIN) {      // F16X2, per-tap form: two stage buffers of two fp16 planes [BM + BN][24], or the epilogue tile
        const int loop = 2 * 2 * (BM + BN) * 24 / 2, epi = BM * (BN + 4);      // (64 x 128: 37 KB instead of 55 - three blocks per CU)
        return loop > epi ? loop : epi;
    }
    if (HALO && HIN) {      // bf16 storage: two halo buffers (17 KB each: 208 rows of 80 bytes in 1 KB DMA pieces) + three weight stages [BN][32] bf16, or half the tile
        const int loop = (2 * 17 * 1024 + 3 * BN * 64) / 4, epi = (BM / NH) * (BN + 4);
        return loop > epi ? loop : epi;
    }
    if (HALO) {      // three halo planes [208][24] bf16 + two weight stages of three planes [BN][24] bf16, or the epilogue tile
        const int loop = (3 * 208 * 24 + 2 * 3 * BN * 24) / 2, epi = BM * (BN + 4);
        return loop > epi ? loop : epi;
    }
    if (!HIN) return 2 * (BM + BN) * LDS_LD;
    const int loop = 2 * (BM + BN) * LDS_LD_H / 2, epi = (BM / NH) * (BN + 4);
    return loop > epi ? loop : epi;
}

// Halo form, 64-column tiles, two fp16 planes (F16X2): three blocks per CU.  The launches of this instantiation (64-channel 3x3
// layers: resnet50 layer1, ResNeSt's radix convolutions of layer1, the 512^2 decoder level, the ResNeSt stem) are latency-bound -
// 4 to 18 K slices per block, each behind a global-load round trip - and the kernel needed 171 VGPRs, three over the 168 that admit
// a third block.  With the bound the compiler fits 168 without scratch (the three-plane instantiations spill: they keep two).
// Same box: cfg2 step 20.75 -> 20.68 ms, resnest50 encoder forward 4.82 -> 4.80 ms (profiles/r06_*_ab6_halo_3blocks.txt).
template <Form F, int BM, int BN>
__global__ void __launch_bounds__(256, (F == Form::F16X2_HALO && BN == 64) ? 3 : form_traits(F).X3 ? 2 : 1) igemm_kernel(const IgemmParams p) {
    constexpr FormTraits FT = form_traits(F);      // the form's flags, under the names the body reads
    constexpr bool SMALLC = FT.SMALLC, BF16 = FT.BF16, HS = FT.HS, X3 = FT.X3, HALO = FT.HALO, BX3 = FT.BX3;
    constexpr int NPL = FT.NPL, WGM = tile_wgm(BN), WGN = 4 / WGM;
    static_assert(!HALO || BM == 128, "halo form: 128-pixel patches");
    constexpr int WTM = BM / WGM, WTN = BN / WGN;
    constexpr int MR = WTM / 32, NR = WTN / 32;
    constexpr bool HIN = HS && !SMALLC;                 // bf16 operands in HBM
    constexpr int LPR = (HIN || X3) ? 4 : 8;            // lanes per row of a load pass (16-byte loads); X3 loads 16-channel
    constexpr int RPP = 256 / LPR;                      // half K-tiles: 4 lanes x 4 floats.  Rows per pass of the block
    constexpr int EPL = X3 ? 4 : 32 / LPR;              // elements per lane per row
    constexpr int ESH = HIN ? 1 : 2;                    // log2(bytes per element)
    constexpr int AROWS = (BM + RPP - 1) / RPP, BROWS = (BN + RPP - 1) / RPP;
    static_assert(MR >= 1 && NR >= 1, "wave tile");
    static_assert(!HIN || BF16, "bf16 operands imply the bf16 MFMA");
    typedef typename std::conditional<HS, bf16_t, float>::type OT;   // output / residual element type

    // bf16 operands: the LDS image is half as large, and with the epilogue staged in two row halves a block needs
    // ~45 KB instead of 74 KB - three blocks per CU instead of two hide more of the global-load latency
    constexpr int NH = (HIN && WGM >= 2) ? 2 : 1;       // epilogue staging passes
    constexpr int MAIN_FLOATS = igemm_main_floats<F, BM, BN>();
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][BM][LDS_LD]
    float* Bs = smem + 2 * BM * LDS_LD;     // [2][BN][LDS_LD]
    int* rowoff = reinterpret_cast<int*>(smem + MAIN_FLOATS);             // [BM]
    float* red = reinterpret_cast<float*>(rowoff + BM);                   // [WGM][BN][2]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;

    // XCD-aware block remap: consecutive tiles (sharing A rows / B columns) stay on one XCD's L2
    const int nwg = gridDim.x;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const ClassInfo ci = p.cls[blockIdx.y];
    const int ntn = p.Nout / BN;
    const int tn = bid % ntn, tm = bid / ntn;
    if (tm >= ci.mtiles) return;   // classes of one launch may differ by a tile (uniform per block)
    const int m0 = tm * BM, n0 = tn * BN;
    const Tap* taps = p.taps + ci.tap0;
    const int kt_begin = blockIdx.z * p.kt_per_split;
    const int kt_end = min(kt_begin + p.kt_per_split, ci.nkt);

    // row of the pass this thread loads / stores.  The bf16 LDS images have 80-byte rows and LDS stores are banked mod 32
    // dwords per group of contiguous lanes (two rows per group): rows r and r+1 overlap on 4 banks, rows r and r+4 do not,
    // so consecutive row slots of a wave are mapped to rows 0,4,8,12, 1,5,9,13, ... (a permutation inside 16 rows).
    const int c4 = tid % LPR, q0 = tid / LPR;
    // (X3: 48-byte rows, four rows per store lane group: rows 0,2,4,6 / 1,3,5,7 partition the 32 banks)
    const int r0 = X3 ? ((q0 & ~7) | ((q0 & 3) << 1) | ((q0 >> 2) & 1))
                      : HIN ? (((q0 & 3) << 2) | ((q0 >> 2) & 3) | (q0 & ~15)) : q0;
    const int ohw = ci.OHl * ci.OWl;

    int a_n[AROWS], a_h[AROWS], a_w[AROWS];
#pragma unroll
    for (int j = 0; j < AROWS; ++j) {
        const int m = m0 + r0 + RPP * j;
        if (m < ci.M && r0 + RPP * j < BM) {
            const int n = m / ohw;
            const int rem = m - n * ohw;
            const int a = rem / ci.OWl;
            const int b = rem - a * ci.OWl;
            a_n[j] = n * p.IH;
            a_h[j] = a * p.s_in;
            a_w[j] = b * p.s_in;
        } else {
            a_n[j] = 0;
            a_h[j] = -(1 << 28);
            a_w[j] = 0;
        }
    }
    // fast loader state (32-channel path): per-row pixel index + per-tap validity bits, buffer descriptors.
    // A K-tile load is then  offset = (pix + dpix(tap)) * ld + channel  ->  one buffer_load_dwordx4 whose
    // out-of-image rows are redirected past num_records (the hardware returns zeros: conv padding for free).
    int a_pix[AROWS];
    unsigned a_msk[AROWS];
    int b_off[BROWS];
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    __amdgpu_buffer_rsrc_t rsA0, rsA1, rsB;
    if constexpr (!SMALLC) {
#pragma unroll
        for (int j = 0; j < AROWS; ++j) {
            a_pix[j] = (a_n[j] + a_h[j]) * p.IW + a_w[j];
            unsigned mk = 0;
            for (int t = 0; t < ci.ntaps; ++t) {
                const int ih = a_h[j] + taps[t].dh, iw = a_w[j] + taps[t].dw;
                if ((unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW) mk |= 1u << t;
            }
            a_msk[j] = mk;
        }
#pragma unroll
        for (int j = 0; j < BROWS; ++j) b_off[j] = (n0 + r0 + RPP * j) * (p.T * p.Ctot) + c4 * EPL;
        rsA0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A0), 0, p.bytesA0, 0x00020000);
        rsA1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A1 ? p.A1 : p.A0), 0, p.A1 ? p.bytesA1 : p.bytesA0, 0x00020000);
        rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.B), 0, p.bytesB, 0x00020000);
    }
    constexpr int PW = 32, PH = BM / PW;        // HALO: patch width / height (one MFMA row tile = 32 pixels of ONE patch row)
    int h_n = 0, h_oh0 = 0, h_ow0 = 0;         // HALO: image and patch origin of this tile
    if constexpr (HALO) {
        const int tiles_w = ci.OWl / PW, tiles_h = ci.OHl / PH;
        const int tw = tm % tiles_w, q = tm / tiles_w;
        h_n = q / tiles_h;
        h_oh0 = (q - h_n * tiles_h) * PH;
        h_ow0 = tw * PW;
        if (tid < BM) {
            const int oh = h_oh0 + tid / PW, ow = h_ow0 + tid % PW;
            rowoff[tid] = p.ksplit > 1 ? (h_n * ci.OHl + oh) * ci.OWl + ow      // slab row = GEMM row
                                                          : h_n * p.osN + oh * p.osH + ow * p.osW + ci.os0;
        }
    } else
    if (tid < BM) {
        const int m = m0 + tid;
        int off = -1;
        if (m < ci.M) {
            if (p.ksplit > 1) {
                off = m;   // slab rows are plain GEMM rows (summed by splitk_reduce_kernel)
            } else {
                const int n = m / ohw;
                const int rem = m - n * ohw;
                const int a = rem / ci.OWl;
                const int b = rem - a * ci.OWl;
                off = n * p.osN + a * p.osH + b * p.osW + ci.os0;
            }
        }
        rowoff[tid] = off;
    }

    float4 ra[AROWS], rb[BROWS];

    auto gload_into = [&](int kt, float4 (&ra)[AROWS], float4 (&rb)[BROWS], int koff = 0) {
#if XV2_ABL & 1
        return;
#endif
        if constexpr (!SMALLC) {
            // K order = (32-channel chunk, tap): consecutive K-tiles re-read the same channel slice of
            // neighbouring pixels, which the per-CU L1 can serve (tap-major order re-streamed it from L2)
            const int chunk = kt / ci.ntaps;
            const int tap = kt - chunk * ci.ntaps;
            const int cc = chunk * BK;
            const Tap t = taps[tap];
            const int dpix = t.dh * p.IW + t.dw;
            const bool first = cc < p.C0;
            const int ld = first ? p.ldA0 : p.ldA1;
            const int ch = (first ? cc : cc - p.C0) + c4 * EPL + koff;
#pragma unroll
            for (int j = 0; j < AROWS; ++j) {
                const bool ok = (a_msk[j] >> tap) & 1u;
                const int off = ok ? (((a_pix[j] + dpix) * ld + ch) << ESH) : (int)0x80000000;
                const i32x4 v = first ? __builtin_amdgcn_raw_buffer_load_b128(rsA0, off, 0, 0)
                                      : __builtin_amdgcn_raw_buffer_load_b128(rsA1, off, 0, 0);
                ra[j] = __builtin_bit_cast(float4, v);
            }
            const int kb = t.slot * p.Ctot + cc + koff;
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsB, (b_off[j] + kb) << ESH, 0, 0);
                rb[j] = __builtin_bit_cast(float4, v);
            }
        } else {
            // 4-channel source: every float4 is one tap
            const int tap = kt * 8 + c4;
            const bool tok = tap < ci.ntaps;
            const Tap t = taps[tok ? tap : 0];
#pragma unroll
            for (int j = 0; j < AROWS; ++j) {
                const int ih = a_h[j] + t.dh, iw = a_w[j] + t.dw;
                const bool ok = tok && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) {
                    const size_t pix = (size_t)(a_n[j] + ih) * p.IW + iw;
                    v = *reinterpret_cast<const float4*>(p.A0 + pix * p.ldA0);
                }
                ra[j] = v;
            }
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (tok) v = *reinterpret_cast<const float4*>(p.B + ((size_t)(n0 + r0 + RPP * j) * p.T + t.slot) * 4);
                rb[j] = v;
            }
        }
    };
    auto gload = [&](int kt) { gload_into(kt, ra, rb); };
    auto lstore = [&](int buf) {
#if XV2_ABL & 2
        return;
#endif
        if constexpr (HIN) {
            // bf16 in HBM: the 16 loaded bytes ARE 8 consecutive channels of the LDS image
            __bf16* a = reinterpret_cast<__bf16*>(smem) + buf * (BM + BN) * LDS_LD_H;
            __bf16* b = a + BM * LDS_LD_H;
#pragma unroll
            for (int j = 0; j < AROWS; ++j)
                if (BM % RPP == 0 || r0 + RPP * j < BM)
                    *reinterpret_cast<float4*>(a + (r0 + RPP * j) * LDS_LD_H + c4 * 8) = ra[j];
#pragma unroll
            for (int j = 0; j < BROWS; ++j)
                if (BN % RPP == 0 || r0 + RPP * j < BN)
                    *reinterpret_cast<float4*>(b + (r0 + RPP * j) * LDS_LD_H + c4 * 8) = rb[j];
            return;
        }
        if constexpr (BF16) {
            __bf16* a = reinterpret_cast<__bf16*>(smem) + buf * (BM + BN) * LDS_LD_H;
            __bf16* b = a + BM * LDS_LD_H;
#pragma unroll
            for (int j = 0; j < AROWS; ++j) {
                bf16x4 v = {(__bf16)ra[j].x, (__bf16)ra[j].y, (__bf16)ra[j].z, (__bf16)ra[j].w};
                *reinterpret_cast<bf16x4*>(a + (r0 + 32 * j) * LDS_LD_H + c4 * 4) = v;
            }
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                bf16x4 v = {(__bf16)rb[j].x, (__bf16)rb[j].y, (__bf16)rb[j].z, (__bf16)rb[j].w};
                *reinterpret_cast<bf16x4*>(b + (r0 + 32 * j) * LDS_LD_H + c4 * 4) = v;
            }
            return;
        }
        float* a = As + buf * BM * LDS_LD;
        float* b = Bs + buf * BN * LDS_LD;
#pragma unroll
        for (int j = 0; j < AROWS; ++j)
            *reinterpret_cast<float4*>(a + (r0 + 32 * j) * LDS_LD + c4 * 4) = ra[j];
#pragma unroll
        for (int j = 0; j < BROWS; ++j)
            *reinterpret_cast<float4*>(b + (r0 + 32 * j) * LDS_LD + c4 * 4) = rb[j];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if constexpr (HS && HALO) {
        // bf16 storage, halo form: NO register path for the operands at all.  Per 32-channel slice the 6 x 34 halo of the 4 x 32
        // patch (204 pixels x 64 B) and, per tap, the [BN][32] weight tile go global -> LDS with direct-to-LDS loads (16 B per
        // lane, each lane its own global address: the gather and the LDS swizzle are one address computation); the nine taps
        // read shifted rows of the same halo.
        constexpr int HWD = PW + 2;
        const int ntp = ci.ntaps;
        const int sl_begin = kt_begin / ntp, sl_end = kt_end / ntp;              // 32-channel slices
        const int sgn = __builtin_amdgcn_readfirstlane(taps[0].dh < 0 ? 1 : -1);
        // ---- the K loop as straight-line code (the F16X2_HALO form below, without its split): two 32-channel slices = 18 stages per
        // trip, ring slot / halo buffer / fragment set / fragment offsets as immediates, spatial tap order (weight tap u or 8 - u),
        // waves 0, 1 gather the weight stages (16 rows x 64 B per 1 KB piece, the LDS swizzle is the lane's choice of chunk),
        // waves 2, 3 fetch the next slice's halo straight into the other halo buffer at tap 0 and confirm it at tap 7, fragments
        // of stage j + 1 are read between the MFMAs of stage j, bare barriers.  Halo rows are 80 bytes (64 + a pad chunk the DMA
        // fills with zeros): no row-dependent swizzle, so the nine taps are nine immediates, and consecutive rows are
        // conflict-free for ds_read_b128's lane groups; weight rows are 64 bytes with chunk c of row r at c ^ ((r >> 3) & 3).
        constexpr int HPC = 17, HBB = HPC * 1024, WBB = BN * 64;                 // halo buffer: 17 pieces of 1 KB (1040 of 1088 granules are rows)
        constexpr int NWP = BN / 16 / 2;                                         // weight pieces per weight wave and stage: 4 / 2
        constexpr int NHW = (HPC + 1) / 2;                                       // halo pieces per halo wave: 9 (the second one's last is idle)
        static_assert((size_t)2 * HBB + 3 * WBB <= (size_t)MAIN_FLOATS * 4, "halo buffers + weight ring fit");
        char* lds = reinterpret_cast<char*>(smem);
        const bool wwave = __builtin_amdgcn_readfirstlane(wave) < 2;
        const int nsl = p.Ctot / BK;
        // weight waves: lane -> (row, chunk) of its pieces; voff[j] carries MINUS the piece's immediate (the immediate applies to
        // the global AND the LDS address; the range check sees their sum)
        // (four scalars, not an array: a captured int[] in these lambdas makes this clang drop the HOST stub of the instantiation)
        auto w_off = [&](int j) {
            const int row = ((wave & 1) * NWP + j) * 16 + (lane >> 2), pos = lane & 3;
            return (((n0 + row) * p.T * p.Ctot) << 1) + ((pos ^ ((row >> 3) & 3)) << 4) - j * 1024;
        };
        const int w_voff0 = w_off(0), w_voff1 = w_off(1), w_voff2 = w_off(NWP == 4 ? 2 : 0), w_voff3 = w_off(NWP == 4 ? 3 : 0);
        const int w_lds = 2 * HBB + (wave & 1) * NWP * 1024;
        const int tstep = sgn * (p.Ctot << 1), t0 = sgn > 0 ? 0 : 8 * (p.Ctot << 1);
        auto dma_w = [&](auto SLOT, auto U, int sl, bool live = true) {
            constexpr int slot = decltype(SLOT)::value, u = decltype(U)::value;
            const int so = __builtin_amdgcn_readfirstlane(t0 + u * tstep + sl * (BK * 2));
            auto dst = (__attribute__((address_space(3))) void*)(lds + w_lds + slot * WBB);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, live ? w_voff0 : (int)0x80000000, so, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, live ? w_voff1 : (int)0x80000000, so, 1024, 0);
            if constexpr (NWP == 4) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, live ? w_voff2 : (int)0x80000000, so, 2048, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, dst, 16, live ? w_voff3 : (int)0x80000000, so, 3072, 0);
            }
        };
        // halo waves: granule g = (hw * 9 + i) * 64 + lane = (row g / 5, position g % 5); position 4 is the pad
        int hpx[NHW];
#pragma unroll
        for (int i = 0; i < NHW; ++i) {
            const int g = ((wave & 1) * NHW + i) * 64 + lane, row = g / 5, pos = g - row * 5;
            const int hr = row / HWD, hc = row - hr * HWD;
            const int ih = h_oh0 - 1 + hr, iw = h_ow0 - 1 + hc;
            const bool ok = pos < 4 && row < (PH + 2) * HWD && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
            hpx[i] = ok ? (((h_n * p.IH + ih) * p.IW + iw) << 2) + pos : -1;     // pixel * 4 + chunk
        }
        auto dma_h = [&](int sl, auto HBUF) {
            constexpr int hbuf = decltype(HBUF)::value;
            const int cc = sl * BK;
            const bool first = cc < p.C0;
            const int ld = first ? p.ldA0 : p.ldA1;
            const int so = __builtin_amdgcn_readfirstlane((first ? cc : cc - p.C0) << 1);
#pragma unroll
            for (int i = 0; i < NHW; ++i) {
                if ((wave & 1) * NHW + i < HPC) {                                 // wave-uniform
                    const int vo = hpx[i] >= 0 ? (((hpx[i] >> 2) * ld) << 1) + ((hpx[i] & 3) << 4) : (int)0x80000000;
                    auto dst = (__attribute__((address_space(3))) void*)(lds + hbuf * HBB + ((wave & 1) * NHW + i) * 1024);
                    if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA0, dst, 16, vo, so, 0, 0);
                    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA1, dst, 16, vo, so, 0, 0);
                }
            }
        };
        // fragment addresses: A = halo row of (pixel, tap (-1, -1)), 8 channels at 16 * (2 ks + h); B = the lane's row of a stage
        const char* a_ptr[MR];
#pragma unroll
        for (int i = 0; i < MR; ++i) a_ptr[i] = lds + (((wm * WTM + i * 32) / PW) * HWD + l31) * 80 + h * 16;
        const char* b_ptr[NR][2];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int row = wn * WTN + j * 32 + l31;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) b_ptr[j][ks] = lds + 2 * HBB + row * 64 + (((ks * 2 + h) ^ ((row >> 3) & 3)) << 4);
        }
        bf16x8 fa[2][2][MR], fb[2][2][NR];
        auto rd_a = [&](auto U, auto HBUF, bf16x8 (&f)[2][MR]) {
            constexpr int off = decltype(HBUF)::value * HBB + ((decltype(U)::value / 3) * HWD + (decltype(U)::value % 3)) * 80;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < MR; ++i) f[ks][i] = *reinterpret_cast<const bf16x8*>(a_ptr[i] + off + ks * 32);
        };
        auto rd_b = [&](auto SLOT, bf16x8 (&f)[2][NR]) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int j = 0; j < NR; ++j) f[ks][j] = *reinterpret_cast<const bf16x8*>(b_ptr[j][ks] + decltype(SLOT)::value * WBB);
        };
        auto stage = [&](auto JJ, int sl) {
            constexpr int J = decltype(JJ)::value, u = J % 9, shf = J / 9, slot = J % 3, par = J & 1;
            constexpr int J3 = J + 3, u3 = J3 % 9, sh3 = J3 / 9;
            if (wwave) {
                if constexpr (sh3 == 0) dma_w(IC<slot>{}, IC<u3>{}, sl + sh3);
                else dma_w(IC<slot>{}, IC<u3>{}, sl + sh3, sl + sh3 < nsl);
            } else if (u == 0) {
                if (sl + shf + 1 < sl_end) dma_h(sl + shf + 1, IC<(shf ^ 1)>{});
            }
            rd_b(IC<(J + 1) % 3>{}, fb[par ^ 1]);
            if constexpr (u != 8) rd_a(IC<u + 1>{}, IC<shf>{}, fa[par ^ 1]);
            else rd_a(IC<0>{}, IC<(shf ^ 1)>{}, fa[par ^ 1]);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[par][ks][i], fb[par][ks][j], acc[i][j], 0, 0, 0);
            {
                constexpr int NMF = 2 * MR * NR, NRD = 2 * (MR + NR);
#pragma unroll
                for (int g = 0; g < NMF; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, (NRD + NMF - 1) / NMF, 0);
                }
            }
            if (wwave) {
                if constexpr (NWP == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            } else if (u == 7) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        };
        if (wwave) {
            dma_w(IC<0>{}, IC<0>{}, sl_begin);
            dma_w(IC<1>{}, IC<1>{}, sl_begin);
            dma_w(IC<2>{}, IC<2>{}, sl_begin);
            if constexpr (NWP == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            dma_h(sl_begin, IC<0>{});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        rd_a(IC<0>{}, IC<0>{}, fa[0]);
        rd_b(IC<0>{}, fb[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();      // (every wave holds its first fragments before slot 0 is re-filled)
        int sl = sl_begin;
        for (; sl + 1 < sl_end; sl += 2) {
            stage(IC<0>{}, sl); stage(IC<1>{}, sl); stage(IC<2>{}, sl); stage(IC<3>{}, sl); stage(IC<4>{}, sl); stage(IC<5>{}, sl);
            stage(IC<6>{}, sl); stage(IC<7>{}, sl); stage(IC<8>{}, sl); stage(IC<9>{}, sl); stage(IC<10>{}, sl); stage(IC<11>{}, sl);
            stage(IC<12>{}, sl); stage(IC<13>{}, sl); stage(IC<14>{}, sl); stage(IC<15>{}, sl); stage(IC<16>{}, sl); stage(IC<17>{}, sl);
        }
        if (sl < sl_end) {      // an odd number of slices: the first half of a trip
            stage(IC<0>{}, sl); stage(IC<1>{}, sl); stage(IC<2>{}, sl); stage(IC<3>{}, sl); stage(IC<4>{}, sl); stage(IC<5>{}, sl);
            stage(IC<6>{}, sl); stage(IC<7>{}, sl); stage(IC<8>{}, sl);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the DMA issued past the end: before the epilogue re-uses LDS)
        __syncthreads();
    } else if constexpr (X3 && HALO) {
        // 6 x 34 halo pixels.  The patch is 4 x 32 so that the 32 lanes of an MFMA row tile read 32 CONSECUTIVE LDS rows
        // whatever the tap: with 8 x 16 patches (two patch rows per tile, a jump of 18 or 24 LDS rows between lanes 15 and
        // 16) SQ_LDS_BANK_CONFLICT counted 2.1e7 cycles per launch, 8 % of the kernel; consecutive rows: 0.
        constexpr int LDK = 24, HWD = PW + 2, HUSE = PW + 2, NHP = ((PH + 2) * HWD + 7) / 8 * 8;      // 204 -> 208 LDS rows
        constexpr int PLA = NHP * LDK;                                   // halo plane [240][24] bf16
        constexpr int PLB = BN * LDK, STB = NPL * PLB;                   // weight stage: NPL planes [BN][24]
        constexpr int HL = (NHP * 4 + 255) / 256;                        // 16-byte halo loads per thread (4, a quarter idle)
        static_assert((size_t)(NPL * PLA + 2 * STB) * 2 <= (size_t)MAIN_FLOATS * 4, "halo + weight stages fit the operand buffers");
        __bf16* sa = reinterpret_cast<__bf16*>(smem);                    // [NPL][NHPP][LDK]
        __bf16* sbw = sa + NPL * PLA;                                    // [2][NPL][BN][LDK]
        // BX3: ring of three weight stages, each [BN / 64 units][3 planes][64 rows][16] bf16 with the two 16-byte halves of a
        // row swapped on rows 8..15 mod 16 (conflict-free 16-byte fragment reads without padding - for the lane groups ds_read_b128
        // is really served in, MI355X_MICROARCH "LDS": rows r and r + 8 share a 256-byte bank window and meet in one group; the
        // round-3 choice, bit 2 of the row, left every B read 2-way conflicted: SQ_LDS_BANK_CONFLICT 28 % of the LDS cycles), 1 KB per DMA instruction
        constexpr int STBX = NPL * BN * 16;                              // elements per pre-split weight stage
        static_assert(!BX3 || (size_t)(NPL * PLA + 3 * STBX) * 2 <= (size_t)MAIN_FLOATS * 4, "halo + three weight stages fit");
        // F16X2: scale of the activation operand (a power of two from the producer's recorded maximum)
        float sA = 1.f;
        if constexpr (NPL == 2) sA = amax_scale(amax_exponent(p.amaxA0, p.amaxA1));
        const int ntp = ci.ntaps;                                        // 9
        // split-K ranges are whole 32-channel chunks (kt_per_split % ntaps == 0, igemm_launch)
        const int cs_begin = 2 * (kt_begin / ntp), cs_end = 2 * (kt_end / ntp);      // 16-channel slices
        const int s_begin = cs_begin * ntp, s_end = cs_end * ntp;        // stage = (slice, tap)
        // this thread's halo elements: pixel (permuted inside groups of 8 rows: conflict-free 8-byte LDS stores) x 4 channels
        int hpix[HL], hrow[HL];
#pragma unroll
        for (int j = 0; j < HL; ++j) {
            const int e = tid + j * 256, hq = e >> 2;
            const int hp = (hq & ~7) | ((hq & 3) << 1) | ((hq >> 2) & 1);      // LDS row (NHP is a multiple of 8)
            const int hr = hp / HWD, hc = hp - hr * HWD;
            const int ih = h_oh0 - 1 + hr, iw = h_ow0 - 1 + hc;
            const bool used = hq < NHP && hr < PH + 2 && hc < HUSE;
            const bool ok = used && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
            hpix[j] = ok ? (h_n * p.IH + ih) * p.IW + iw : -1;
            hrow[j] = used ? hp : -1;
        }
        // fragment rows: A tile i of this wave = one patch row of 32 pixels; halo row of (pixel, tap (0,0))
        int abase[MR];
#pragma unroll
        for (int i = 0; i < MR; ++i) abase[i] = ((wm * WTM + i * 32) / PW + 1) * HWD + l31 + 1;
        float4 hraw[HL], rbb[BROWS], rbb1[BROWS];
        uint2 pkb[BROWS][NPL], pkh[HL][NPL];
        bf16x8 fa0[MR][NPL], fb0[NR][NPL], fa1[MR][NPL], fb1[NR][NPL];
        auto hload = [&](int cs) {
            const int cc = (cs >> 1) * BK + (cs & 1) * 16;
            const bool first = cc < p.C0;
            const int ld = first ? p.ldA0 : p.ldA1;
            const int ch = (first ? cc : cc - p.C0) + (tid & 3) * 4;
#pragma unroll
            for (int j = 0; j < HL; ++j) {
                const int off = hpix[j] >= 0 ? ((hpix[j] * ld + ch) << 2) : (int)0x80000000;
                const i32x4 v = first ? __builtin_amdgcn_raw_buffer_load_b128(rsA0, off, 0, 0)
                                      : __builtin_amdgcn_raw_buffer_load_b128(rsA1, off, 0, 0);
                hraw[j] = __builtin_bit_cast(float4, v);
            }
        };
        auto hsplit = [&]() {
#pragma unroll
            for (int j = 0; j < HL; ++j) {
                const float4 v = hraw[j];
                if constexpr (NPL == 2) split2hx4(v, sA, pkh[j][0], pkh[j][1]);
                else split3x4(v, pkh[j][0], pkh[j][1], pkh[j][NPL - 1]);
            }
        };
        auto hstore = [&]() {
#if XV2_HABL & 1
            return;
#endif
#pragma unroll
            for (int j = 0; j < HL; ++j)
                if (hrow[j] >= 0) {
                    __bf16* d = sa + hrow[j] * LDK + (tid & 3) * 4;
#pragma unroll
                    for (int q = 0; q < NPL; ++q) *reinterpret_cast<uint2*>(d + q * PLA) = pkh[j][q];
                }
        };
        // taps are the 3 x 3 neighbourhood in slot order, (dh, dw) = sgn * (t / 3 - 1, t % 3 - 1) with sgn = +1 (forward) or
        // -1 (backward-data) - checked by halo_eligible(): scalar arithmetic instead of a dynamically indexed table load
        const int sgn = __builtin_amdgcn_readfirstlane(taps[0].dh < 0 ? 1 : -1);
        auto bload = [&](int st, float4 (&xb)[BROWS]) {      // weights of stage st = (slice st / ntp, tap st % ntp)
            const int cs = st / ntp, tp = st - cs * ntp;
            const int kb = tp * p.Ctot + (cs >> 1) * BK + (cs & 1) * 16;
#pragma unroll
            for (int j = 0; j < BROWS; ++j)
                xb[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsB, (b_off[j] + kb) << 2, 0, 0));
        };
        auto bsplit = [&](const float4 (&xb)[BROWS]) {
#pragma unroll
            for (int j = 0; j < BROWS; ++j) split3x4(xb[j], pkb[j][0], pkb[j][1], pkb[j][NPL - 1]);
        };
        auto bstore = [&](int buf) {
#if XV2_HABL & 4
            return;
#endif
#pragma unroll
            for (int j = 0; j < BROWS; ++j) {
                const int rr = r0 + RPP * j;
                if (BN % RPP == 0 || rr < BN) {
                    __bf16* d = sbw + buf * STB + rr * LDK + c4 * 4;
#pragma unroll
                    for (int q = 0; q < NPL; ++q) *reinterpret_cast<uint2*>(d + q * PLB) = pkb[j][q];
                }
            }
        };
        auto read_a = [&](int tp, bf16x8 (&fa)[MR][NPL]) {
            const int th = tp / 3;
#if XV2_HABL & 2
            const int toff = 0;
#else
            const int toff = sgn * ((th - 1) * HWD + (tp - th * 3 - 1));
#endif
#pragma unroll
            for (int q = 0; q < NPL; ++q)
#pragma unroll
                for (int i = 0; i < MR; ++i)
                    fa[i][q] = *reinterpret_cast<const bf16x8*>(sa + q * PLA + (abase[i] + toff) * LDK + 8 * h);
        };
        auto read_b = [&](int buf, bf16x8 (&fb)[NR][NPL]) {
#if XV2_HABL & 8
            const __bf16* b = sbw + buf * STB + l31 * 8 + 256 * h;      // conflict-free by construction (wrong data)
#else
            const __bf16* b = sbw + buf * STB + (wn * WTN + l31) * LDK + 8 * h;
#endif
#pragma unroll
            for (int q = 0; q < NPL; ++q)
#pragma unroll
                for (int j = 0; j < NR; ++j) fb[j][q] = *reinterpret_cast<const bf16x8*>(b + q * PLB + j * 32 * LDK);
        };
        auto mfma_stage = [&](const bf16x8 (&fa)[MR][NPL], const bf16x8 (&fb)[NR][NPL]) {
#if XV2_HABL & 16
            return;
#endif
            if constexpr (NPL == 2) {        // fp16 planes: m*h, h*m, h*h
                typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int i = 0; i < MR; ++i)
#pragma unroll
                        for (int j = 0; j < NR; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[i][t == 0 ? 1 : 0]),
                                                                               __builtin_bit_cast(f16x8, fb[j][t == 1 ? 1 : 0]),
                                                                               acc[i][j], 0, 0, 0);
                return;
            }
#pragma unroll
            for (int t = XV2_T0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        const int qa = t == 0 ? NPL - 1 : (t == 2 || t == 3) ? 1 : 0;
                        const int qb = t == 1 ? NPL - 1 : (t == 2 || t == 4) ? 1 : 0;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][qa], fb[j][qb], acc[i][j], 0, 0, 0);
                    }
        };
        // iteration st: fragments of st in (fa, fb); (na, nb) receive st+1; xb holds the raw weights of st+2 (split here);
        // yb is free and receives st+3.  At the last tap of a slice the next slice's halo (in flight since the slice began)
        // is split and replaces the halo in LDS - nobody reads it any more: the A fragments of the last tap were fetched one
        // iteration earlier - and the first tap's A fragments are read behind the barrier.
        // (tp, cs = tap and slice of stage st, by value: as captured loop state they ended up in scratch memory)
        auto iter = [&](int st, const int tp, const int cs, const bf16x8 (&fa)[MR][NPL], const bf16x8 (&fb)[NR][NPL],
                        bf16x8 (&na)[MR][NPL], bf16x8 (&nb)[NR][NPL], float4 (&xb)[BROWS], float4 (&yb)[BROWS]) {
            const bool last = tp == ntp - 1;
            const bool more = st + 1 < s_end;
            if (more) {
                read_b((st + 1) & 1, nb);
                if (!last) read_a(tp + 1, na);
            }
            if (st + 3 < s_end) bload(st + 3, yb);
            bsplit(xb);
            mfma_stage(fa, fb);
#pragma unroll
            for (int j = 0; j < BROWS; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) asm volatile("" : "+v"(pkb[j][q].x), "+v"(pkb[j][q].y));
            constexpr int NMFMA = (6 - XV2_T0) * MR * NR, NRD = NPL * (MR + NR);
#pragma unroll
            for (int g = 0; g < NMFMA; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (g < NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, BROWS * 20 / NMFMA + 1, 0);
            }
            if (st + 2 < s_end) bstore(st & 1);
            const bool swap = last && more;
            if (swap) {
                hsplit();
                hstore();
            }
            __syncthreads();
            if (swap) {
                read_a(0, na);
                if (cs + 2 < cs_end) hload(cs + 2);
            }
        };
        if constexpr (BX3 && NPL == 2) {
            // ---- F16X2: the K loop as straight-line code.  Two 16-channel slices = 18 stages (slice half, spatial tap u) per trip:
            // ring slot, fragment set, fragment offsets and LDS destinations are instruction immediates; per stage a wave issues
            // its MFMAs, the fragment reads of the next stage between them, and two to four DMA instructions whose only
            // run-time input is one scalar offset.  (The loop it replaces carried tap / slice / ring state at run time: ~170
            // instructions per stage around 12 MFMAs, the matrix pipe waiting for both waves of a SIMD to get through them.)
            //   * spatial order: stage tap u multiplies the halo shifted by (u / 3 - 1, u % 3 - 1) with weight tap u (forward)
            //     or 8 - u (backward-data: the flipped kernel) - the fragment offsets do not depend on the direction;
            //   * BOTH operands arrive by DMA and the two kinds have their own waves, because vmcnt counts in order: waves 0, 1
            //     stream the weight stages (confirmed two stages after issue), waves 2, 3 fetch the fp32 halo of the NEXT slice
            //     into a staging area at tap 0 and confirm it at tap 7 - seven stages of cover instead of the one a shared
            //     queue leaves; at tap 8 every thread takes its four 16-byte pieces from staging, splits, stores the planes;
            //   * every DMA is unconditional: past the end of the K range it lands in a slot nobody reads (or past the buffer:
            //     the hardware writes zeros); bare s_barrier + explicit counts (__syncthreads() is vmcnt(0) with LDS-DMA in flight).
            constexpr int NCHW = STBX * 2 / 1024 / 2;                // 1 KB weight pieces per weight wave and stage: 4 / 2
            constexpr int HCH = 7;                                   // 1 KB halo pieces per halo wave and slice (13 of 14 carry rows)
            constexpr int STG_B = (NPL * PLA + 3 * STBX) * 2;        // byte offset of the staging area
            static_assert((size_t)STG_B + 2 * HCH * 1024 <= (size_t)MAIN_FLOATS * 4, "planes + weight ring + halo staging fit");
            static_assert(NCHW == 4 || NCHW == 2, "weight pieces per wave");
            char* lds = reinterpret_cast<char*>(smem);
            const int nsl = p.Ctot / 16;
            __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Bx3), 0, p.bytesBx3, 0x00020000);
            const bool wwave = __builtin_amdgcn_readfirstlane(wave) < 2;
            // weight waves: unit / first piece of this wave inside a stage image (BN = 128: one 64-row unit each; 64: half a unit)
            const int w_unit = BN == 128 ? (wave & 1) : 0, w_cq0 = BN == 128 ? 0 : (wave & 1) * 2;
            const int w_voff = ((tn * (BN / 64) + w_unit) * p.T * nsl) * (2048 * NPL) + w_cq0 * 1024 + lane * 16;
            const int w_lds = NPL * PLA * 2 + w_unit * 4096 + w_cq0 * 1024;      // + slot * STBX * 2
            // weight tap of spatial tap u, as a byte offset: u * tstep + t0 (forward: u, backward-data: 8 - u)
            const int tstep = sgn * nsl * (2048 * NPL), t0 = sgn > 0 ? 0 : 8 * nsl * (2048 * NPL);
            // (the scalar offset takes no part in the buffer's range check: a stage past the END of the weight tensor is sent out
            //  of range through the lane offset - zeros into a slot nobody reads, no memory access)
            auto dma_w = [&](auto SLOT, auto U, int cs, bool live = true) {
                constexpr int slot = decltype(SLOT)::value, u = decltype(U)::value;
                const int so = __builtin_amdgcn_readfirstlane(t0 + u * tstep + cs * (2048 * NPL));
                const int vo = live ? w_voff : (int)0x80000000;
                auto dst = (__attribute__((address_space(3))) void*)(lds + w_lds + slot * STBX * 2);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, dst, 16, vo, so, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, dst, 16, vo, so, 1024, 0);
                if constexpr (NCHW == 4) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, dst, 16, vo, so, 2048, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsX, dst, 16, vo, so, 3072, 0);
                }
            };
            // halo waves: pixel of this lane's 16-byte piece e = (hw * 7 + i) * 64 + lane  (row slot e >> 2, channel quad e & 3)
            int hvp[HCH];
            {
                const int hw = wave & 1;
#pragma unroll
                for (int i = 0; i < HCH; ++i) {
                    const int e = (hw * HCH + i) * 64 + lane, hq = e >> 2;
                    const int hp = (hq & ~7) | ((hq & 3) << 1) | ((hq >> 2) & 1);
                    const int hr = hp / HWD, hc = hp - hr * HWD;
                    const int ih = h_oh0 - 1 + hr, iw = h_ow0 - 1 + hc;
                    const bool ok = hq < NHP && hr < PH + 2 && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
                    hvp[i] = ok ? (h_n * p.IH + ih) * p.IW + iw : -1;
                }
            }
            auto dma_h = [&](int cs) {
                const int cc = (cs >> 1) * BK + (cs & 1) * 16;
                const bool first = cc < p.C0;
                const int ld = first ? p.ldA0 : p.ldA1;
                const int so = __builtin_amdgcn_readfirstlane((first ? cc : cc - p.C0) * 4);
                const int hw = wave & 1;
#pragma unroll
                for (int i = 0; i < HCH; ++i) {
                    const int vo = hvp[i] >= 0 ? ((hvp[i] * ld + (lane & 3) * 4) << 2) : (int)0x80000000;
                    auto dst = (__attribute__((address_space(3))) void*)(lds + STG_B + (hw * HCH + i) * 1024);
                    if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA0, dst, 16, vo, so, 0, 0);
                    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA1, dst, 16, vo, so, 0, 0);
                }
            };
            // staging -> planes: this thread's pieces e = tid + 256 j (the mapping of hpix / hrow above)
            unsigned stg_a[HL];
#pragma unroll
            for (int j = 0; j < HL; ++j) {
                const int e = tid + j * 256;
                stg_a[j] = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)(lds + STG_B) + (e < NHP * 4 ? e : 0) * 16;
            }
            auto stage_to_planes = [&]() {
#pragma unroll
                for (int j = 0; j < HL; j += 2) {
                    i32x4 r0_, r1_;
                    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(r0_), "=&v"(r1_) : "v"(stg_a[j]), "v"(stg_a[j + 1]) : "memory");
                    hraw[j] = __builtin_bit_cast(float4, r0_);
                    hraw[j + 1] = __builtin_bit_cast(float4, r1_);
                }
                hsplit();
                hstore();
            };
            // fragment addresses: A = halo row of (pixel, tap (-1, -1)) of this lane, B = its row of a weight stage image
            const __bf16* a_ptr[MR];
#pragma unroll
            for (int i = 0; i < MR; ++i) a_ptr[i] = sa + (abase[i] - HWD - 1) * LDK + 8 * h;
            const __bf16* b_ptr[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int row = wn * WTN + j * 32 + l31, unit = row >> 6, r = row & 63;
                b_ptr[j] = sbw + unit * (1024 * NPL) + r * 16 + ((h ^ ((r >> 3) & 1)) * 8);
            }
            bf16x8 fa[2][MR][NPL], fb[2][NR][NPL];
            auto rd_a = [&](auto U, bf16x8 (&f)[MR][NPL]) {
                constexpr int u = decltype(U)::value, off = ((u / 3) * HWD + (u % 3)) * LDK;
#pragma unroll
                for (int q = 0; q < NPL; ++q)
#pragma unroll
                    for (int i = 0; i < MR; ++i) f[i][q] = *reinterpret_cast<const bf16x8*>(a_ptr[i] + q * PLA + off);
            };
            auto rd_b = [&](auto SLOT, bf16x8 (&f)[NR][NPL]) {
                constexpr int slot = decltype(SLOT)::value;
#pragma unroll
                for (int j = 0; j < NR; ++j)
#pragma unroll
                    for (int q = 0; q < NPL; ++q) f[j][q] = *reinterpret_cast<const bf16x8*>(b_ptr[j] + slot * STBX + q * 1024);
            };
            // stage J of a trip (slices cs, cs + 1): see above
            auto stage = [&](auto JJ, int cs) {
                constexpr int J = decltype(JJ)::value, u = J % 9, shf = J / 9, slot = J % 3, par = J & 1;
                constexpr int J3 = J + 3, u3 = J3 % 9, sh3 = J3 / 9;               // the stage whose weights are issued here
#if !(XV2_HABL & 32)
                if (wwave) {
                    if constexpr (sh3 == 2) dma_w(IC<slot>{}, IC<u3>{}, cs + sh3, cs + sh3 < nsl);
                    else dma_w(IC<slot>{}, IC<u3>{}, cs + sh3);
                } else if (u == 0) {
                    if (shf == 0 || cs + 2 < cs_end) dma_h(cs + shf + 1);
                }
#endif
                rd_b(IC<(J + 1) % 3>{}, fb[par ^ 1]);
                if constexpr (u != 8) rd_a(IC<(u + 1) % 9>{}, fa[par ^ 1]);
                mfma_stage(fa[par], fb[par]);
                {
                    constexpr int NMF = 3 * MR * NR, NRD = NPL * NR + (u != 8 ? NPL * MR : 0);
#pragma unroll
                    for (int g = 0; g < NMF; ++g) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        if (g < NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                }
                if constexpr (u == 8) stage_to_planes();
                if (wwave) {
                    if constexpr (NCHW == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                } else if (u == 7) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if XV2_HABL & 64
                if constexpr ((J & 1) == 0 || u >= 7)      // (timing only: every second barrier dropped - wrong results)
#endif
                __builtin_amdgcn_s_barrier();
                if constexpr (u == 8) rd_a(IC<0>{}, fa[par ^ 1]);
            };
            // prologue: halo of the first slice (staging -> planes), weight stages 0, 1, 2
            if (wwave) {
                dma_w(IC<0>{}, IC<0>{}, cs_begin);
                dma_w(IC<1>{}, IC<1>{}, cs_begin);
                dma_w(IC<2>{}, IC<2>{}, cs_begin);
                if constexpr (NCHW == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            } else {
                dma_h(cs_begin);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            stage_to_planes();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            rd_a(IC<0>{}, fa[0]);
            rd_b(IC<0>{}, fb[0]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();      // (every wave holds its first fragments before slot 0 is re-filled: r05_race_halo_prologue.md)
            for (int cs = cs_begin; cs < cs_end; cs += 2) {
                stage(IC<0>{}, cs); stage(IC<1>{}, cs); stage(IC<2>{}, cs); stage(IC<3>{}, cs); stage(IC<4>{}, cs); stage(IC<5>{}, cs);
                stage(IC<6>{}, cs); stage(IC<7>{}, cs); stage(IC<8>{}, cs); stage(IC<9>{}, cs); stage(IC<10>{}, cs); stage(IC<11>{}, cs);
                stage(IC<12>{}, cs); stage(IC<13>{}, cs); stage(IC<14>{}, cs); stage(IC<15>{}, cs); stage(IC<16>{}, cs); stage(IC<17>{}, cs);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the DMA issued past the end: before the epilogue re-uses LDS)
            __syncthreads();
        } else if constexpr (BX3) {
            // ---- three bf16 planes, pre-split weights: tap, slice and ring slot are run-time loop state
            constexpr int NCH = STBX * 2 / 1024;                 // 1 KB DMA chunks per stage: 12 (BN = 128) / 6 (BN = 64)
            constexpr int CPW = (NCH + 3) / 4;                   // per wave: 3 / 2 (BN = 64: two chunks are fetched twice)
            const int nsl = p.Ctot / 16;
            __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Bx3), 0, p.bytesBx3, 0x00020000);
            auto dma = [&](int st, int buf) {                    // weights of stage st -> ring slot buf
                const int cs = st / ntp, tp = st - cs * ntp;
#pragma unroll
                for (int u = 0; u < CPW; ++u) {
                    const int chunk = (wave * CPW + u) % NCH;
                    const int unit = chunk / (2 * NPL), cq = chunk - unit * (2 * NPL);
                    const int goff = (((tn * (BN / 64) + unit) * p.T + tp) * nsl + cs) * (2048 * NPL) + cq * 1024 + lane * 16;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        rsX, (__attribute__((address_space(3))) void*)(sbw + buf * STBX + unit * (1024 * NPL) + cq * 512), 16, goff, 0, 0, 0);
                }
            };
            auto read_bx = [&](int buf, bf16x8 (&fb)[NR][NPL]) {
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const int row = wn * WTN + j * 32 + l31, unit = row >> 6, r = row & 63;
                    const __bf16* b = sbw + buf * STBX + unit * (1024 * NPL) + r * 16 + ((h ^ ((r >> 3) & 1)) * 8);
#pragma unroll
                    for (int q = 0; q < NPL; ++q) fb[j][q] = *reinterpret_cast<const bf16x8*>(b + q * 1024);
                }
            };
            // iteration st (ring slot bc = st % 3): fragments of st in (fa, fb); (na, nb) receive st+1; the DMA of st+2 (issued
            // one iteration ago) must have landed by the barrier, the DMA of st+3 is issued here into the slot of st
            auto iterx = [&](int st, const int tp, const int cs, const int bc, const bf16x8 (&fa)[MR][NPL], const bf16x8 (&fb)[NR][NPL],
                             bf16x8 (&na)[MR][NPL], bf16x8 (&nb)[NR][NPL]) {
                const bool last = tp == ntp - 1;
                const bool more = st + 1 < s_end;
                if (more) {
                    read_bx(bc == 2 ? 0 : bc + 1, nb);
                    if (!last) read_a(tp + 1, na);
                }
                const bool pf = st + 3 < s_end;
                if (pf) dma(st + 3, bc);
                mfma_stage(fa, fb);
                const bool swap = last && more;
                if (swap) {
                    hsplit();
                    hstore();
                }
                if (pf) {
                    if constexpr (CPW == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                // a bare barrier: __syncthreads() carries a workgroup fence, and with LDS-DMA in flight the fence is
                // `s_waitcnt vmcnt(0)` - the DMA of st+3 issued in THIS iteration had to land before its barrier
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (swap) {
                    read_a(0, na);
                    if (cs + 2 < cs_end) hload(cs + 2);
                }
            };
            hload(cs_begin);
            dma(s_begin, 0);
            dma(s_begin + 1, 1);
            hsplit();
            hstore();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (s_begin + 2 < s_end) dma(s_begin + 2, 2);
            if (cs_begin + 1 < cs_end) hload(cs_begin + 1);
            __syncthreads();
            read_a(0, fa0);
            read_bx(0, fb0);
            __builtin_amdgcn_s_waitcnt(0xc07f);
            // EVERY wave holds its first fragments before any wave's first iteration re-fills ring slot 0 (the DMA of stage 3):
            // in the loop that ordering comes from the barrier that ends the previous iteration, here it needs its own.  Without
            // it a wave delayed between the barrier above and its reads (another process's waves on the same CU) picked up
            // stage 3's weights as stage 0's - profiles/r05_race_halo_prologue.md
            __syncthreads();
            int tp = 0, cs = cs_begin, bc = 0;
            for (int st = s_begin; st < s_end; st += 2) {
                iterx(st, tp, cs, bc, fa0, fb0, fa1, fb1);
                if (++tp == ntp) {
                    tp = 0;
                    ++cs;
                }
                bc = bc == 2 ? 0 : bc + 1;
                iterx(st + 1, tp, cs, bc, fa1, fb1, fa0, fb0);
                if (++tp == ntp) {
                    tp = 0;
                    ++cs;
                }
                bc = bc == 2 ? 0 : bc + 1;
            }
        } else {
        hload(cs_begin);
        bload(s_begin, rbb);
        bload(s_begin + 1, rbb1);
        hsplit();
        hstore();
        bsplit(rbb);
        bstore(0);
        if (s_begin + 2 < s_end) bload(s_begin + 2, rbb);
        bsplit(rbb1);
        bstore(1);
        if (cs_begin + 1 < cs_end) hload(cs_begin + 1);
        __syncthreads();
        read_a(0, fa0);
        read_b(0, fb0);
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __syncthreads();      // (see the pre-split form above: the first iteration stores stage 2 into the buffer of stage 0)
        int tp = 0, cs = cs_begin;
        for (int st = s_begin; st < s_end; st += 2) {        // the stage count is even (two slices per 32-channel chunk)
            iter(st, tp, cs, fa0, fb0, fa1, fb1, rbb, rbb1);
            if (++tp == ntp) {
                tp = 0;
                ++cs;
            }
            iter(st + 1, tp, cs, fa1, fb1, fa0, fb0, rbb1, rbb);
            if (++tp == ntp) {
                tp = 0;
                ++cs;
            }
        }
        }      // !BX3
    } else if constexpr (X3) {
        // K advances in STAGES of 16 channels (half a K-tile).  LDS: two stage buffers, each three bf16 planes
        // [hi | mid | lo] x ([A rows | B rows] x 24 bf16: 16 + 8 pad, 48-byte rows) - 73.7 KB for 128x128, the size of the
        // fp32 double buffer.  Registers: two raw load sets and two fragment sets.  Iteration s multiplies stage s out of
        // the fragment registers filled during iteration s-1, while (a) the fragments of stage s+1 are read from LDS,
        // (b) the raw registers of stage s+2 are split on the VALU in the shadow of the MFMAs and stored into the LDS buffer
        // stage s occupied, (c) stage s+3 is fetched from memory.  One barrier per stage, no LDS latency on the MFMA path.
        constexpr int LDK = 24;
        // prefetch depth: stages between a global load and its split.  Three planes: 3 (two raw register sets; 4 measured identical
        // on every cfg2 layer and on the step, and the 128 x 128 tile spills: the chip is power-limited there).
        // Two planes (F16X2): 4 (three raw sets) - a stage holds half the MFMA work and the load latency shows: -0.2 ms per cfg2
        // step (22.88 -> 22.67 ms, two same-box pairs; isolated layers unchanged), 219 VGPRs for the 128 x 128 tile
        constexpr int PF = NPL == 2 ? 4 : 3;
        constexpr int PL = (BM + BN) * LDK, STG = NPL * PL;
        static_assert((size_t)2 * STG * 2 <= (size_t)MAIN_FLOATS * 4, "stage buffers fit the fp32 operand buffers");
        __bf16* sb = reinterpret_cast<__bf16*>(smem);
        const int s_begin = 2 * kt_begin, s_end = 2 * kt_end;       // stage s = K-tile s / 2, channel half s & 1
        uint2 pk[AROWS + BROWS][NPL];
        float4 ra1[AROWS], rb1[BROWS];
        bf16x8 fa0[MR][NPL], fb0[NR][NPL], fa1[MR][NPL], fb1[NR][NPL];
        float sA = 1.f, sB = 1.f;      // F16X2 operand scales
        if constexpr (NPL == 2) {
            sA = amax_scale(amax_exponent(p.amaxA0, p.amaxA1));
            sB = amax_scale(amax_exponent(p.amaxB));
        }
        auto gstage = [&](int st, float4 (&xa)[AROWS], float4 (&xb)[BROWS]) { gload_into(st >> 1, xa, xb, (st & 1) * 16); };
        auto split_regs = [&](const float4 (&xa)[AROWS], const float4 (&xb)[BROWS]) {
#pragma unroll
            for (int j = 0; j < AROWS + BROWS; ++j) {
                const float4 v = j < AROWS ? xa[j < AROWS ? j : 0] : xb[j >= AROWS ? j - AROWS : 0];
#if XV2_ABL & 16
                pk[j][0] = make_uint2(__float_as_uint(v.x), __float_as_uint(v.y));
                pk[j][1] = make_uint2(__float_as_uint(v.z), __float_as_uint(v.w));
                pk[j][NPL - 1] = pk[j][0];
#else
                if constexpr (NPL == 2) split2hx4(v, j < AROWS ? sA : sB, pk[j][0], pk[j][1]);
                else split3x4(v, pk[j][0], pk[j][1], pk[j][NPL - 1]);
#endif
            }
        };
        auto store_planes = [&](int buf) {
#if XV2_ABL & 2
            return;
#endif
#pragma unroll
            for (int j = 0; j < AROWS + BROWS; ++j) {
                const int rr = r0 + RPP * (j < AROWS ? j : j - AROWS);
                if (j < AROWS ? (BM % RPP == 0 || rr < BM) : (BN % RPP == 0 || rr < BN)) {
                    __bf16* d = sb + buf * STG + ((j < AROWS ? 0 : BM) + rr) * LDK + c4 * 4;
#pragma unroll
                    for (int q = 0; q < NPL; ++q) *reinterpret_cast<uint2*>(d + q * PL) = pk[j][q];
                }
            }
        };
        auto read_frags = [&](int buf, bf16x8 (&fa)[MR][NPL], bf16x8 (&fb)[NR][NPL]) {
            const __bf16* a = sb + buf * STG + (wm * WTM + l31) * LDK + 8 * h;
            const __bf16* b = sb + buf * STG + (BM + wn * WTN + l31) * LDK + 8 * h;
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
#pragma unroll
                for (int i = 0; i < MR; ++i) fa[i][q] = *reinterpret_cast<const bf16x8*>(a + q * PL + i * 32 * LDK);
#pragma unroll
                for (int j = 0; j < NR; ++j) fb[j][q] = *reinterpret_cast<const bf16x8*>(b + q * PL + j * 32 * LDK);
            }
        };
        auto mfma_stage = [&](const bf16x8 (&fa)[MR][NPL], const bf16x8 (&fb)[NR][NPL]) {
            if constexpr (NPL == 2) {        // fp16 planes: m*h, h*m, h*h
                typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int i = 0; i < MR; ++i)
#pragma unroll
                        for (int j = 0; j < NR; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[i][t == 0 ? 1 : 0]),
                                                                               __builtin_bit_cast(f16x8, fb[j][t == 1 ? 1 : 0]),
                                                                               acc[i][j], 0, 0, 0);
                return;
            }
            // smallest terms first (l*h, h*l, m*m, m*h, h*m, h*h); the accumulator tiles interleave, so dependent MFMAs
            // are MR*NR issues apart
#pragma unroll
            for (int t = XV2_T0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        const int qa = t == 0 ? NPL - 1 : (t == 2 || t == 3) ? 1 : 0;
                        const int qb = t == 1 ? NPL - 1 : (t == 2 || t == 4) ? 1 : 0;
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][qa], fb[j][qb], acc[i][j], 0, 0, 0);
                    }
        };
        // iteration st: fragments of st in (fa, fb); (na, nb) receive st+1; (xa, xb) hold the raw stage st+2 (split here);
        // (za, zb) are free and receive stage st+PF (PF == 4: stage st+3 is in flight in a third register set)
        auto iter = [&](int st, const bf16x8 (&fa)[MR][NPL], const bf16x8 (&fb)[NR][NPL], bf16x8 (&na)[MR][NPL],
                        bf16x8 (&nb)[NR][NPL], float4 (&xa)[AROWS], float4 (&xb)[BROWS], float4 (&za)[AROWS],
                        float4 (&zb)[BROWS]) {
            if (st + 1 < s_end) read_frags((st + 1) & 1, na, nb);
            if (st + PF < s_end) gstage(st + PF, za, zb);
            split_regs(xa, xb);
            mfma_stage(fa, fb);
            // pin the split results here: the instruction selector otherwise sinks the whole split below its consumer
            // (the LDS stores), out of reach of the scheduling groups that follow
#pragma unroll
            for (int j = 0; j < AROWS + BROWS; ++j)
#pragma unroll
                for (int q = 0; q < NPL; ++q) asm volatile("" : "+v"(pk[j][q].x), "+v"(pk[j][q].y));
            // per MFMA slot (32 cycles): one fragment read of the next stage while there are any, ~4 split VALU
            constexpr int NMFMA = (NPL == 2 ? 3 : 6 - XV2_T0) * MR * NR, NRD = NPL * (MR + NR);
#pragma unroll
            for (int g = 0; g < NMFMA; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (g < NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, (AROWS + BROWS) * 20 / NMFMA + 1, 0);
            }
            if (st + 2 < s_end) store_planes(st & 1);      // the buffer of stage st: every wave read it before the last barrier
            __syncthreads();
        };
        gstage(s_begin, ra, rb);
        gstage(s_begin + 1, ra1, rb1);
        split_regs(ra, rb);
        store_planes(0);
        if (s_begin + 2 < s_end) gstage(s_begin + 2, ra, rb);
        split_regs(ra1, rb1);
        store_planes(1);
        float4 ra2[PF == 4 ? AROWS : 1], rb2[PF == 4 ? BROWS : 1];
        if constexpr (PF == 4) {
            if (s_begin + 3 < s_end) gstage(s_begin + 3, ra1, rb1);
        }
        __syncthreads();
        read_frags(0, fa0, fb0);
        // the first fragments land before the loop is entered: otherwise the loop header, reached from here and from the
        // back edge, waits for lgkmcnt(0) in EVERY iteration - on the next stage's reads it has just issued
        __builtin_amdgcn_s_waitcnt(0xc07f);
        // ... and in EVERY wave before the first iteration stores stage 2 into the buffer of stage 0 ("every wave read it before
        // the last barrier" holds from the second iteration on; profiles/r05_race_halo_prologue.md)
        __syncthreads();
        if constexpr (PF == 4) {
        // raw sets rotate with period 3, fragment sets with period 2: six iterations per trip (the stage count is even;
        // iterations past s_end are skipped as a whole)
        auto& r2a = reinterpret_cast<float4(&)[AROWS]>(ra2);
        auto& r2b = reinterpret_cast<float4(&)[BROWS]>(rb2);
        for (int st = s_begin; st < s_end; st += 6) {
            iter(st, fa0, fb0, fa1, fb1, ra, rb, r2a, r2b);
            iter(st + 1, fa1, fb1, fa0, fb0, ra1, rb1, ra, rb);
            if (st + 2 >= s_end) break;
            iter(st + 2, fa0, fb0, fa1, fb1, r2a, r2b, ra1, rb1);
            iter(st + 3, fa1, fb1, fa0, fb0, ra, rb, r2a, r2b);
            if (st + 4 >= s_end) break;
            iter(st + 4, fa0, fb0, fa1, fb1, ra1, rb1, ra, rb);
            iter(st + 5, fa1, fb1, fa0, fb0, r2a, r2b, ra1, rb1);
        }
        } else {
        for (int st = s_begin; st < s_end; st += 2) {        // the stage count is even
            iter(st, fa0, fb0, fa1, fb1, ra, rb, ra1, rb1);
            iter(st + 1, fa1, fb1, fa0, fb0, ra1, rb1, ra, rb);
        }
        }
    } else {
    // 3-stage pipeline: registers <- global (tile kt+2), LDS[buf^1] <- registers (tile kt+1), MFMA on LDS[buf]
    // (tile kt).  The LDS store of the next tile sits at the START of an iteration, so nothing but the MFMA
    // tail stands between the last fragment read and the barrier.
    gload(kt_begin);
    lstore(0);
    if (kt_begin + 1 < kt_end) gload(kt_begin + 1);
    __syncthreads();

    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int buf = (kt - kt_begin) & 1;
        if (kt + 1 < kt_end) {
            lstore(buf ^ 1);
            if (kt + 2 < kt_end) gload(kt + 2);
        }
        if constexpr (BF16) {
            const __bf16* ha = reinterpret_cast<const __bf16*>(smem) + buf * (BM + BN) * LDS_LD_H;
            const __bf16* a = ha + (wm * WTM + l31) * LDS_LD_H + 8 * h;
            const __bf16* b = ha + BM * LDS_LD_H + (wn * WTN + l31) * LDS_LD_H + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 af[MR], bf[NR];
#pragma unroll
                for (int i = 0; i < MR; ++i) af[i] = *reinterpret_cast<const bf16x8*>(a + i * 32 * LDS_LD_H + ks * 16);
#pragma unroll
                for (int j = 0; j < NR; ++j) bf[j] = *reinterpret_cast<const bf16x8*>(b + j * 32 * LDS_LD_H + ks * 16);
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            continue;
        }
        const float* a = As + buf * BM * LDS_LD + (wm * WTM + l31) * LDS_LD + 4 * h;
        const float* b = Bs + buf * BN * LDS_LD + (wn * WTN + l31) * LDS_LD + 4 * h;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float4 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i)
                af[i] = *reinterpret_cast<const float4*>(a + i * 32 * LDS_LD + kk * 8);
#pragma unroll
            for (int j = 0; j < NR; ++j)
                bf[j] = *reinterpret_cast<const float4*>(b + j * 32 * LDS_LD + kk * 8);
#if XV2_ABL & 4
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j) acc[i][j][0] += af[i].x * bf[j].x + af[i].y * bf[j].y + af[i].z * bf[j].z + af[i].w * bf[j].w;
#else
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
#endif
        }
        __syncthreads();
    }

    }      // !X3
#if XV2_ABL & 8
    {      // (every accumulator stays live: a test of acc[0][0][0] alone let the compiler drop three quarters of the MFMAs)
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) t += acc[i][j][r];
        if (t == 123.456f) p.Out0[0] = t;
        return;
    }
#endif
    if constexpr (NPL == 2) {      // F16X2: undo the operand scales (powers of two: exact)
        const float ia = amax_inv(amax_exponent(p.amaxA0, p.amaxA1)), ib = amax_inv(amax_exponent(p.amaxB));
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = acc[i][j][r] * ia * ib;
    }
    // ---- epilogue.  C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
    // The tile is staged through LDS (the A/B buffers are free now) so that global stores are 16 bytes per lane
    // and cover whole 128..512-byte output rows: for the K<=256 1x1 convolutions the dword-store epilogue was
    // two thirds of the kernel.  BatchNorm partial sums are taken from the registers on the way.
    constexpr int CLD = BN + 4;
    constexpr int HROWS = BM / NH;          // rows staged per pass
    float* Cs = smem;
    float omax = 0.f;                                     // F16X2: max |value stored to Out0| (IgemmParams::amax_out)
    const bool do_stats = p.stats && p.ksplit == 1;
    if (do_stats) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int cl = wn * WTN + j * 32 + l31;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < MR; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = HS ? bf16_round(acc[i][j][r]) : acc[i][j][r];
                    s1 += sv;
                    s2 += sv * sv;
                }
            }
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (h == 0) {
                red[(wm * BN + cl) * 2 + 0] = s1;
                red[(wm * BN + cl) * 2 + 1] = s2;
            }
        }
    }
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) {
    if (NH == 1 || (wm * WTM) / HROWS == hh) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int cl = wn * WTN + j * 32 + l31;
#pragma unroll
            for (int i = 0; i < MR; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h - hh * HROWS;
                    Cs[row * CLD + cl] = acc[i][j][r];
                }
            }
        }
    }
    __syncthreads();
    if (hh == 0 && do_stats && tid < BN) {
        // this tile's row of statistics partials (red[] is complete behind the barrier above)
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int w = 0; w < WGM; ++w) {
            s1 += red[(w * BN + tid) * 2 + 0];
            s2 += red[(w * BN + tid) * 2 + 1];
        }
        float* st = p.stats + ((size_t)tm * p.Nout + n0 + tid) * 2;
        st[0] = s1;
        st[1] = s2;
    }
    {
        constexpr int F4R = BN / 4;
        float* slab = p.ksplit > 1 ? p.part + (size_t)blockIdx.z * ci.M * p.Nout : nullptr;
        // the training step's launch (one output, no bias, no inference epilogue, no accumulation, unsplit): the loop without
        // the general one's six kernel-uniform tests per row (every instruction of a power-limited kernel is paid in clock)
        if (!slab && !p.bias && !p.ep_scale && !p.accum && p.N0 == p.Nout) {
            OT* const o0 = reinterpret_cast<OT*>(p.Out0) + n0;
            const bool rec = p.amax_out != nullptr;
#pragma unroll 4
            for (int e = tid; e < HROWS * F4R; e += 256) {
                const int row = hh * HROWS + e / F4R, c = (e % F4R) * 4;
                const int off = rowoff[row];
                if (off < 0) continue;
                const float4 v = *reinterpret_cast<const float4*>(Cs + (row - hh * HROWS) * CLD + c);
                st4(o0 + (size_t)off * p.ldo0 + c, v);
                if (rec) omax = amax_acc(omax, v);
            }
        } else
#pragma unroll 4
        for (int e = tid; e < HROWS * F4R; e += 256) {
            const int row = hh * HROWS + e / F4R, c = (e % F4R) * 4;
            const int off = rowoff[row];
            if (off < 0) continue;
            float4 v = *reinterpret_cast<const float4*>(Cs + (row - hh * HROWS) * CLD + c);
            const int col = n0 + c;
            if (slab) {      // split-K: this block's partial tile goes to its slab (summed by splitk_reduce_kernel)
                *reinterpret_cast<float4*>(slab + (size_t)off * p.Nout + col) = v;
                continue;
            }
            if (p.bias) {
                const float4 bv = *reinterpret_cast<const float4*>(p.bias + col);
                v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            }
            if (p.ep_scale) {     // same arithmetic as bn_act_fwd_kernel on the materialised conv output
                const float4 sc = *reinterpret_cast<const float4*>(p.ep_scale + col);
                const float4 sf = *reinterpret_cast<const float4*>(p.ep_shift + col);
                v.x = __fmaf_rn(v.x, sc.x, sf.x); v.y = __fmaf_rn(v.y, sc.y, sf.y);
                v.z = __fmaf_rn(v.z, sc.z, sf.z); v.w = __fmaf_rn(v.w, sc.w, sf.w);
                if (p.ep_res) {
                    const float4 r = ld4(reinterpret_cast<const OT*>(p.ep_res) + (size_t)off * p.ep_ldres + col);
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                v.x = apply_act(v.x, p.ep_act); v.y = apply_act(v.y, p.ep_act);
                v.z = apply_act(v.z, p.ep_act); v.w = apply_act(v.w, p.ep_act);
            }
            OT* o = col < p.N0 ? reinterpret_cast<OT*>(p.Out0) + (size_t)off * p.ldo0 + col
                               : reinterpret_cast<OT*>(p.Out1) + (size_t)off * p.ldo1 + (col - p.N0);
            if (p.accum & (col < p.N0 ? 1 : 2)) {
                const float4 old = ld4(o);
                v.x += old.x; v.y += old.y; v.z += old.z; v.w += old.w;
            }
            st4(o, v);
            if (p.amax_out && col < p.N0) omax = amax_acc(omax, v);
        }
    }
    if (NH > 1 && hh + 1 < NH) __syncthreads();      // the staging tile is rewritten by the next pass
  }
    // (blocks that stored FINAL values: unsplit launches; slab writers leave it to the slab sum)
    if (!HS && p.amax_out && p.ksplit == 1) amax_record(p.amax_out, omax, red, blockIdx.x + 13 * blockIdx.y);
}

// Sum the split-K slabs, add the bias, scatter to the NHWC output(s) and emit the BatchNorm partial sums
// for 32-row tiles: stats[tile][Nout][2].  256 threads = 64 column lanes (float4) x 4 row lanes.  (32 rows, all slabs
// of a row in flight: 64-row tiles left a 128-block grid latency-bound - cfg3 bf16 20.5 -> 19.2 ms; 16 rows: slower)
constexpr int SPLITK_ROWS = 32;
template <typename OT>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ part, int ksplit, int M,
                                                             int Nout, const float* __restrict__ bias,
                                                             OT* __restrict__ out0, int ldo0, int N0,
                                                             OT* __restrict__ out1, int ldo1,
                                                             float* __restrict__ stats, int accum,
                                                             const float* __restrict__ ep_scale,
                                                             const float* __restrict__ ep_shift,
                                                             const OT* __restrict__ ep_res, int ep_ldres, int ep_act,
                                                             unsigned* __restrict__ amax_out) {
    __shared__ float sh[256 * 8];
    float omax = 0.f;      // F16X2: max |value stored to out0| (IgemmParams::amax_out)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int r0 = blockIdx.x * SPLITK_ROWS;
    const size_t slab = (size_t)M * Nout;
    for (int cb = blockIdx.y * 256; cb < Nout; cb += gridDim.y * 256) {
        const int c = cb + tx * 4;
        float4 s1 = make_float4(0, 0, 0, 0), s2 = make_float4(0, 0, 0, 0);
        if (c < Nout) {
            float4 bv = make_float4(0, 0, 0, 0);
            if (bias) bv = *reinterpret_cast<const float4*>(bias + c);
            float4 sc = make_float4(1, 1, 1, 1), sf = make_float4(0, 0, 0, 0);      // inference epilogue coefficients: once per thread
            if (ep_scale) {
                sc = *reinterpret_cast<const float4*>(ep_scale + c);
                sf = *reinterpret_cast<const float4*>(ep_shift + c);
            }
            // the row's tail: statistics, bias / inference epilogue, (accumulating) store of the summed row `a`
            auto finish_row = [&](int r, float4 a, bool have_old, float4 old_v) {
                {      // statistics on the values as they will be stored
                    const float4 q = make_float4(Elem<OT>::round(a.x), Elem<OT>::round(a.y), Elem<OT>::round(a.z), Elem<OT>::round(a.w));
                    s1.x += q.x; s1.y += q.y; s1.z += q.z; s1.w += q.w;
                    s2.x += q.x * q.x; s2.y += q.y * q.y; s2.z += q.z * q.z; s2.w += q.w * q.w;
                }
                a.x += bv.x; a.y += bv.y; a.z += bv.z; a.w += bv.w;
                if (ep_scale) {
                    a.x = __fmaf_rn(a.x, sc.x, sf.x); a.y = __fmaf_rn(a.y, sc.y, sf.y);
                    a.z = __fmaf_rn(a.z, sc.z, sf.z); a.w = __fmaf_rn(a.w, sc.w, sf.w);
                    if (ep_res) {
                        const float4 rr = ld4(ep_res + (size_t)r * ep_ldres + c);
                        a.x += rr.x; a.y += rr.y; a.z += rr.z; a.w += rr.w;
                    }
                    a.x = apply_act(a.x, ep_act); a.y = apply_act(a.y, ep_act);
                    a.z = apply_act(a.z, ep_act); a.w = apply_act(a.w, ep_act);
                }
                OT* o = c < N0 ? out0 + (size_t)r * ldo0 + c : out1 + (size_t)r * ldo1 + (c - N0);
                if (accum & (c < N0 ? 1 : 2)) {
                    const float4 old = have_old ? old_v : ld4(o);
                    a.x += old.x; a.y += old.y; a.z += old.z; a.w += old.w;
                }
                st4(o, a);
                if (amax_out && c < N0) omax = amax_acc(omax, a);
            };
            // ksplit <= 8: ALL eight rows of this thread (5 - 8 slabs: four at a time) and all their slabs in flight at once (up to 32 loads of 16 bytes,
            // slab count as a compile-time constant: no branch between the loads), then the sums in the fixed slab order -
            // one memory round trip per block instead of one per pair of rows.  These grids are a block or two per CU,
            // i.e. latency-bound (ISA of the rolled loop: every pair of rows ended in s_waitcnt vmcnt(0))
            auto all_rows = [&](auto ksc) {
                constexpr int KS = decltype(ksc)::value;
                constexpr int NR = KS <= 4 ? SPLITK_ROWS / 4 : SPLITK_ROWS / 8;      // 5 - 8 slabs: two batches of four rows
                const bool acc = (accum & (c < N0 ? 1 : 2)) != 0;
#pragma unroll 1
              for (int rb = r0 + ty; rb < r0 + SPLITK_ROWS; rb += 4 * NR) {
                float4 t[NR][KS], olds[NR];
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int rr = min(rb + 4 * i, M - 1);
#pragma unroll
                    for (int z = 0; z < KS; ++z) t[i][z] = *reinterpret_cast<const float4*>(part + z * slab + (size_t)rr * Nout + c);
                }
                if (acc) {        // what an accumulating store adds to: in flight with the slabs
#pragma unroll
                    for (int i = 0; i < NR; ++i) {
                        const int rr = min(rb + 4 * i, M - 1);
                        olds[i] = ld4(c < N0 ? out0 + (size_t)rr * ldo0 + c : out1 + (size_t)rr * ldo1 + (c - N0));
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < NR; ++i) olds[i] = make_float4(0, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int r = rb + 4 * i;
                    if (r < M) {
                        float4 a = make_float4(0, 0, 0, 0);
#pragma unroll
                        for (int z = 0; z < KS; ++z) {
                            a.x += t[i][z].x; a.y += t[i][z].y; a.z += t[i][z].z; a.w += t[i][z].w;
                        }
                        finish_row(r, a, true, olds[i]);
                    }
                }
              }
            };
            // bit 0x100 of `accum` selects the rolled loop for every slab count.  No launch sets it; the test stays because without it
            // the register allocation of this kernel comes out differently (294 -> 296 VGPRs), and its code is the code that was measured.
            // More than 8 slabs - only XV2_FORCE_TILE asks for them - take the rolled loop.
            const bool rolled = (accum & 0x100) != 0;
            if (ksplit == 2 && !rolled) {
                all_rows(std::integral_constant<int, 2>{});
            } else if (ksplit == 3 && !rolled) {
                all_rows(std::integral_constant<int, 3>{});
            } else if (ksplit == 4 && !rolled) {
                all_rows(std::integral_constant<int, 4>{});
            } else if (ksplit == 5 && !rolled) {
                all_rows(std::integral_constant<int, 5>{});
            } else if (ksplit == 6 && !rolled) {
                all_rows(std::integral_constant<int, 6>{});
            } else if (ksplit == 7 && !rolled) {
                all_rows(std::integral_constant<int, 7>{});
            } else if (ksplit == 8 && !rolled) {
                all_rows(std::integral_constant<int, 8>{});
            } else {
#pragma unroll 2
            for (int r = r0 + ty; r < min(r0 + SPLITK_ROWS, M); r += 4) {
                // all slabs of the row in flight at once (ksplit <= 8), then the fixed-order sum
                float4 t[8];
#pragma unroll
                for (int z = 0; z < 8; ++z)
                    t[z] = z < ksplit ? *reinterpret_cast<const float4*>(part + z * slab + (size_t)r * Nout + c)
                                      : make_float4(0, 0, 0, 0);
                float4 a = make_float4(0, 0, 0, 0);
#pragma unroll
                for (int z = 0; z < 8; ++z)
                    if (z < ksplit) {
                        a.x += t[z].x; a.y += t[z].y; a.z += t[z].z; a.w += t[z].w;
                    }
                for (int z = 8; z < ksplit; ++z) {
                    const float4 v = *reinterpret_cast<const float4*>(part + z * slab + (size_t)r * Nout + c);
                    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
                }
                finish_row(r, a, false, make_float4(0, 0, 0, 0));
            }
            }
        }
        if (stats) {
            float* q = sh + threadIdx.x * 8;
            q[0] = s1.x; q[1] = s1.y; q[2] = s1.z; q[3] = s1.w; q[4] = s2.x; q[5] = s2.y; q[6] = s2.z; q[7] = s2.w;
            __syncthreads();
            if (ty == 0 && c < Nout) {
                for (int k = 0; k < 4; ++k) {
                    float a1 = 0.f, a2 = 0.f;
                    for (int w = 0; w < 4; ++w) {
                        a1 += sh[(w * 64 + tx) * 8 + k];
                        a2 += sh[(w * 64 + tx) * 8 + 4 + k];
                    }
                    float* st = stats + ((size_t)blockIdx.x * Nout + c + k) * 2;
                    st[0] = a1;
                    st[1] = a2;
                }
            }
            __syncthreads();
        }
    }    if (amax_out) amax_record(amax_out, omax, sh, blockIdx.x + 13 * blockIdx.y);
}

}  // namespace xv2
