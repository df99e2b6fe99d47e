// Weight gradient of a convolution on the matrix cores of gfx950: the device side of wgrad_conv.hip (planners, kernel table,
// dispatch, the slab sum and the ABI entry points are there).
//
//   dW[co][t][c] = sum_{m} dY[m][co] * X[pix(m, t)][c]        (m over N*OH*OW output pixels)
//
// Both operands are NHWC, i.e. contiguous along the NON-reduced dimension.  The reduction over pixels is split across
// gridDim.y (and, for narrow tiles, across the waves of a block); every split writes its own slab part[split][Cout][T][Ctot]
// and wgrad_conv.hip sums the slabs in a fixed order (deterministic, no atomics).  256 threads = 4 waves, an XCD-aware block
// order (wgrad_block).  The kernel families, and the operand paths (enum WForm) each exists in:
//   wgrad_kernel<F, BM, BN>      the general per-tap kernel: fp32 LDS tiles [32 pixels][channels] kept as loaded, fragments
//                                gathered with conflict-free ds_read_b32 (lane = channel).  RGB / RGB_BF16HBM: 4-channel image
//                                source (every float4 is one tap); C32: exact fp32 MFMA; BF16: operands rounded to bf16 on
//                                their way out of LDS; BF16_BF16HBM / C32_BF16HBM: dY and X are bf16 in HBM
//   wgrad_tr_kernel<BM, BN>      TR_BF16HBM, OW % 32 == 0: bf16 tiles all the way, fragments by ds_read_b64_tr_b16
//   wgrad_tr_x3_kernel<BM,BN,NPL> TR_F32X3 / TR_F16X2: fp32 tiles split into three bf16 / two scaled fp16 planes into LDS
//   wgrad_alltaps_kernel<BF16>   3x3 / stride 1 / pad 1: a block owns a 32 co x 32 ci tile for ALL nine taps and walks down a
//                                32-pixel-wide column strip through a 4-row LDS ring.  ALLTAPS_C32 / ALLTAPS_BF16
//   wgrad_alltaps_tr_kernel      ALLTAPS_BF16HBM, 32 x 32: the ring in bf16 as loaded, transpose reads
//   wgrad_alltaps_x3_kernel<NPL> ALLTAPS_F32X3 / ALLTAPS_F16X2, 32 x 32: three / two planes of the ring
//   wgrad_alltaps64_x3_kernel<NPL>, wgrad_alltaps64_tr_kernel   the same three paths with a 64 co x 64 ci tile per block
// Shared helpers, value-in / value-out: the transposed fragment read and its lane addressing (tr_frag, tr_row / tr_col), the
// operand splits and their scales (split_planes, put_planes, plane_scales), the all-taps strip decode (alltaps_strip) and the
// prologue of their ring walk (ring_prologue: it only calls the kernel's own staging lambdas).  Operand staging, the MFMA
// body, the row loop of the ring walk and the epilogue are each kernel's own: the all-taps kernels run at the edge of their
// register budgets, and a helper that takes the accumulators by reference, holds the MFMA body as a callable or folds through
// LDS changed their instruction streams (so did tr_frag / tr_row in wgrad_alltaps64_x3_kernel, which keeps its own).
#pragma once
#include "xv2_common.h"
#include "amax_ctx.h"
#include <type_traits>

namespace xv2 {

struct WTap {
    short dh, dw;
};

struct WgradParams {
    const float* X0;
    const float* X1;
    const float* DY;
    float* part;
    int C0, C1, Ctot, ldX0, ldX1, ldDY, Cout;
    int IH, IW, OH, OW, stride;
    int M;
    int T;
    int ktiles, kt_per_split;
    int tiles_n;  // column tiles per tap (Ctot / BN), or column tiles overall for SMALLC
    int fast;     // OW % 32 == 0 and operands < 2 GiB: scalar pixel decode + buffer loads
    unsigned bytesX0, bytesX1, bytesDY;
    // F16X2 (xv2_common.h): the maxima of the X sources and of dY, all three known -> the NPL = 2 kernels (two scaled fp16 planes)
    const unsigned* amaxX0;
    const unsigned* amaxX1;
    const unsigned* amaxDY;
    int xcd_order;      // 1: XCD-aware block order (wgrad_block); always 1 - kept as a field so that the kernels' code stays as measured
    WTap taps[52];
};

// The operand paths of the weight-gradient kernels (the map at the top of this file).  The first six are the forms of
// wgrad_kernel.
enum class WForm { RGB, RGB_BF16HBM, C32, BF16, BF16_BF16HBM, C32_BF16HBM,
                   TR_BF16HBM, TR_F32X3, TR_F16X2, ALLTAPS_C32, ALLTAPS_BF16, ALLTAPS_BF16HBM, ALLTAPS_F32X3, ALLTAPS_F16X2 };
struct WFormTraits {
    bool SMALLC, BF16, HS;
};
constexpr WFormTraits WFORM_TRAITS[] = {
    // SMALLC BF16 HS
    {true,  false, false},      // RGB
    {true,  true,  true},       // RGB_BF16HBM
    {false, false, false},      // C32
    {false, true,  false},      // BF16
    {false, true,  true},       // BF16_BF16HBM
    {false, false, true},       // C32_BF16HBM: fp32 MFMA on bf16 storage, the 32 x 32 tile only (WK = 4)
};
constexpr WFormTraits wform_traits(WForm f) { return WFORM_TRAITS[(int)f]; }
constexpr bool wform_rgb(WForm f) { return f == WForm::RGB || f == WForm::RGB_BF16HBM; }
// waves of a block along co x ci x pixels: at most 2 x 2 over the tile, what is left of the four splits the 32-pixel K tile
constexpr int tile_wgm(int BM) { return BM >= 64 ? 2 : 1; }
constexpr int tile_wk(int BM, int BN) { return 4 / (tile_wgm(BM) * tile_wgm(BN)); }

// Block order of the weight-gradient grids (x = (co, ci[, tap]) tile, y = pixel range).  The hardware hands linear block L to XCD L % 8,
// so the tiles of ONE pixel range - which all read the same dY rows and X rows - land on eight different L2s and each operand row is
// fetched from HBM once per XCD it meets (rocprofv3 FETCH_SIZE of wgrad_alltaps<f16x2>: 360 MB per launch against 128 MB algorithmic).
// Re-numbered so that XCD k works through a CONTIGUOUS range of (pixel range, tile) pairs: the tiles of a pixel range follow each other on
// one XCD and its L2 serves the re-reads.  (bx, by) is a bijection of the grid: every slab is written exactly once, as before.
__device__ __forceinline__ void wgrad_block(int on, int& bx, int& by) {
    bx = blockIdx.x;
    by = blockIdx.y;
    if (!on) return;
    const int gx = gridDim.x, nwg = gx * gridDim.y;
    const int l = by * gx + bx;
    const int q = nwg >> 3, r = nwg & 7, xcd = l & 7, loc = l >> 3;
    const int bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    bx = bid % gx;
    by = bid / gx;
}
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[N]) {
#pragma unroll
    for (int t = 0; t < N; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// ds_read_b64_tr_b16 - the gfx950 transpose read: a 16-lane group fetches a [4 pixels][16 channels] block (each lane 4
// consecutive channels of one pixel) and every lane receives the 4 pixels of ITS channel.  Two reads (pixel rows `lo` and, four
// rows on, `hi`) make one 32 x 16 MFMA operand: no VALU.
__device__ __forceinline__ bf16x8 tr_frag(const bf16_t* lo_p, const bf16_t* hi_p) {
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(lo_p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(hi_p));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// four fp32 values -> NPL bf16x4 / fp16x4 terms: three bf16 (F32X3) or two fp16 of the value scaled by s (F16X2)
template <int NPL>
__device__ __forceinline__ void split_planes(const float4 v, float s, uint2 (&pl)[NPL]) {
    if constexpr (NPL == 2) split2hx4(v, s, pl[0], pl[1]);
    else split3x4(v, pl[0], pl[1], pl[NPL - 1]);
}
// transpose-read addressing: 16-lane group g = lane >> 4 serves channels 16 * (g & 1) .. + 15 of the 32-wide operand and
// pixels 8 * (g >> 1) .. + 7 of the 16-pixel k-step; lane i of the group fetches pixel (i >> 2), channels 4 * (i & 3) .. + 3 of
// the 4 x 16 block and receives the 4 pixels of channel i
__device__ __forceinline__ int tr_row(int lane) { return 8 * (lane >> 5) + ((lane & 15) >> 2); }
__device__ __forceinline__ int tr_col(int lane) { return 16 * ((lane >> 4) & 1) + 4 * (lane & 3); }
// the F16X2 operand scales (INV: their inverses, for the epilogue) of the X source in use and of dY; 1 for the three-plane kernels
template <int NPL, bool INV>
__device__ __forceinline__ void plane_scales(const WgradParams& p, bool first, float& sX, float& sD) {
    sX = 1.f, sD = 1.f;
    if constexpr (NPL == 2) {
        const int eX = amax_exponent(first ? p.amaxX0 : p.amaxX1), eD = amax_exponent(p.amaxDY);
        sX = INV ? amax_inv(eX) : amax_scale(eX);
        sD = INV ? amax_inv(eD) : amax_scale(eD);
    }
}

// BF16 = true: XV2_MATH_BF16 - the fp32 LDS tiles are kept, each lane gathers 8 consecutive pixels of its channel,
// rounds them to bf16 and issues v_mfma_f32_32x32x16_bf16 (8x fewer matrix instructions, fp32 accumulate).
// HS = true (XV2_MATH_BF16_STORE): dY and X are bf16 in HBM (the RGB image of the stem stays fp32); a 4-channel element is
// one 8-byte load widened to fp32 on its way into the unchanged fp32 LDS tiles.
template <WForm F, int BM, int BN>
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradParams p) {
    static_assert((int)F <= (int)WForm::C32_BF16HBM, "a form of the tiled kernel");
    constexpr bool SMALLC = wform_traits(F).SMALLC, BF16 = wform_traits(F).BF16, HS = wform_traits(F).HS;
    constexpr int WGM = tile_wgm(BM), WGN = tile_wgm(BN), WK = tile_wk(BM, BN);
    typedef typename std::conditional<HS, bf16_t, float>::type DT;                 // dY element
    typedef typename std::conditional<HS && !SMALLC, bf16_t, float>::type XT;      // X element
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    constexpr int MR = BM / WGM / 32, NR = BN / WGN / 32;
    static_assert(WGM * WGN * WK == 4, "4 waves");
    constexpr int AF4 = BM / 4, ARPP = 256 / AF4, APASS = 32 / ARPP;  // float4 per row, rows per pass
    constexpr int BF4 = BN / 4, BRPP = 256 / BF4, BPASS = 32 / BRPP;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                 // [2][32][BM]   dY tile
    float* Bs = smem + 2 * 32 * BM;   // [2][32][BN]   X tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int l31 = lane & 31, h = lane >> 5;
    const int wk = wave % WK;
    const int wmn = wave / WK;
    const int wm = wmn / WGN, wn = wmn % WGN;

    // block -> (row tile, tap, column tile)
    int b = bx;
    const int tn = b % p.tiles_n;
    b /= p.tiles_n;
    int tap = 0;
    if constexpr (!SMALLC) {
        tap = b % p.T;
        b /= p.T;
    }
    const int tmr = b;
    const int co0 = tmr * BM;
    const int cn0 = tn * BN;  // column offset (channel within tap, or tap*4+c for SMALLC)

    const float* xsrc;
    int ldx, xch;
    if (cn0 < p.C0) {
        xsrc = p.X0; ldx = p.ldX0; xch = cn0;
    } else {
        xsrc = p.X1; ldx = p.ldX1; xch = cn0 - p.C0;
    }

    const int a_c4 = tid % AF4, a_r = tid / AF4;
    const int b_c4 = tid % BF4, b_r = tid / BF4;
    int dh = 0, dw = 0;
    bool tapok = true;
    if constexpr (SMALLC) {
        const int t = (cn0 >> 2) + b_c4;
        tapok = t < p.T;
        dh = p.taps[tapok ? t : 0].dh;
        dw = p.taps[tapok ? t : 0].dw;
    } else {
        dh = p.taps[tap].dh;
        dw = p.taps[tap].dw;
    }
    const int ohw = p.OH * p.OW;

    const int kt0 = by * p.kt_per_split;
    const int kt1 = min(kt0 + p.kt_per_split, p.ktiles);

    float4 ra[APASS], rb[BPASS];
    // fast path: a 32-pixel reduction tile never crosses an output row (OW % 32 == 0), so its (n, oh, ow0) is
    // wave-uniform and each lane only adds a constant: one VALU add + one select per 16-byte buffer load.
    __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(cn0 < p.C0 || SMALLC ? p.X0 : p.X1), 0, (cn0 < p.C0 || SMALLC) ? p.bytesX0 : p.bytesX1, 0x00020000);
    __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.DY), 0, p.bytesDY, 0x00020000);
    int a_const[APASS], b_const[BPASS], b_k[BPASS];
#pragma unroll
    for (int j = 0; j < APASS; ++j) a_const[j] = (a_r + j * ARPP) * p.ldDY + co0 + a_c4 * 4;
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
        b_k[j] = (b_r + j * BRPP) * p.stride + dw;
        b_const[j] = b_k[j] * ldx + xch + b_c4 * 4;
    }
    auto gload_fast = [&](int kt) {
        const int mb = kt * 32;             // uniform
        const int n = mb / ohw;
        const int rem = mb - n * ohw;
        const int oh = rem / p.OW;
        const int ow0 = rem - oh * p.OW;
        const int ih = oh * p.stride + dh;
        const bool rowok = (unsigned)ih < (unsigned)p.IH;
        const int ubase = ((n * p.IH + ih) * p.IW + ow0 * p.stride) * ldx;
        const int iw0 = ow0 * p.stride;
        const int dbase = mb * p.ldDY;
#pragma unroll
        for (int j = 0; j < APASS; ++j) {
            if constexpr (HS) {
                const i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsD, (dbase + a_const[j]) << 1, 0, 0);
                ra[j] = bf16x4_to_f32((unsigned)v.x, (unsigned)v.y);
            } else {
                ra[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsD, (dbase + a_const[j]) << 2, 0, 0));
            }
        }
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const bool ok = rowok && (unsigned)(iw0 + b_k[j]) < (unsigned)p.IW;
            if constexpr (HS) {
                const int off = ok ? ((ubase + b_const[j]) << 1) : (int)0x80000000;
                const i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsX, off, 0, 0);
                rb[j] = bf16x4_to_f32((unsigned)v.x, (unsigned)v.y);
            } else {
                const int off = ok ? ((ubase + b_const[j]) << 2) : (int)0x80000000;
                rb[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsX, off, 0, 0));
            }
        }
    };
    auto gload = [&](int kt) {
        if constexpr (!SMALLC) {
            if (p.fast) {
                gload_fast(kt);
                return;
            }
        }
        const int mb = kt * 32;
#pragma unroll
        for (int j = 0; j < APASS; ++j) {
            const int m = mb + a_r + j * ARPP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < p.M) v = ld4(reinterpret_cast<const DT*>(p.DY) + (size_t)m * p.ldDY + co0 + a_c4 * 4);
            ra[j] = v;
        }
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const int m = mb + b_r + j * BRPP;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < p.M && tapok) {
                const int n = m / ohw;
                const int rem = m - n * ohw;
                const int oh = rem / p.OW;
                const int ow = rem - oh * p.OW;
                const int ih = oh * p.stride + dh, iw = ow * p.stride + dw;
                if ((unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW) {
                    const size_t pix = ((size_t)n * p.IH + ih) * p.IW + iw;
                    if constexpr (SMALLC)
                        v = *reinterpret_cast<const float4*>(p.X0 + pix * p.ldX0);
                    else
                        v = ld4(reinterpret_cast<const XT*>(xsrc) + pix * ldx + xch + b_c4 * 4);
                }
            }
            rb[j] = v;
        }
    };
    auto lstore = [&](int buf) {
        float* a = As + buf * 32 * BM;
        float* bb = Bs + buf * 32 * BN;
#pragma unroll
        for (int j = 0; j < APASS; ++j)
            *reinterpret_cast<float4*>(a + (a_r + j * ARPP) * BM + a_c4 * 4) = ra[j];
#pragma unroll
        for (int j = 0; j < BPASS; ++j)
            *reinterpret_cast<float4*>(bb + (b_r + j * BRPP) * BN + b_c4 * 4) = rb[j];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i) zero_acc(acc[i]);

    if (kt0 < kt1) {
        gload(kt0);
        lstore(0);
        if (kt0 + 1 < kt1) gload(kt0 + 1);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        if (kt + 1 < kt1) {
            lstore(buf ^ 1);
            if (kt + 2 < kt1) gload(kt + 2);
        }
        const float* a = As + buf * 32 * BM + wm * (MR * 32) + l31;
        const float* bb = Bs + buf * 32 * BN + wn * (NR * 32) + l31;
        if constexpr (BF16) {
            static_assert(!BF16 || WK <= 2, "bf16 wgrad splits at most 2 ways over a 32-pixel tile");
#pragma unroll
            for (int ks0 = 0; ks0 < 2 / WK; ++ks0) {
                const int ks = ks0 * WK + wk;
                bf16x8 af[MR], bf[NR];
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int q = 0; q < 8; ++q) af[i][q] = (__bf16)a[(16 * ks + 8 * h + q) * BM + i * 32];
#pragma unroll
                for (int j = 0; j < NR; ++j)
#pragma unroll
                    for (int q = 0; q < 8; ++q) bf[j][q] = (__bf16)bb[(16 * ks + 8 * h + q) * BN + j * 32];
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int s0 = 0; s0 < 16 / WK; ++s0) {
            const int s = s0 * WK + wk;
            float af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) af[i] = a[(2 * s + h) * BM + i * 32];
#pragma unroll
            for (int j = 0; j < NR; ++j) bf[j] = bb[(2 * s + h) * BN + j * 32];
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // store the slab: part[split*WK + wk][co][T][Ctot]   (SMALLC: [co][T*4])
    const size_t rowlen = (size_t)p.T * p.Ctot;
    float* slab = p.part + (size_t)(by * WK + wk) * p.Cout * rowlen;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int col = cn0 + wn * (NR * 32) + j * 32 + l31;
        size_t coloff;
        bool cok = true;
        if constexpr (SMALLC) {
            cok = col < p.T * 4;
            coloff = col;
        } else {
            coloff = (size_t)tap * p.Ctot + col;
        }
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = co0 + wm * (MR * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (cok) slab[(size_t)row * rowlen + coloff] = acc[i][j][r];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// bf16-native weight gradient (XV2_MATH_BF16_STORE, shapes with OW % 32 == 0): the tiles stay bf16 all the way.
// dY and X arrive pixel-major / channel-minor, and the MFMA wants, per lane, 8 consecutive PIXELS of one channel; the
// fp32-LDS variant above gathers them with 8 ds_read_b32 + 8 conversions per fragment.  Here the 16-byte global loads
// (8 channels of a pixel) are stored to LDS as they are and the fragments come out of ds_read_b64_tr_b16 - the gfx950
// transpose read: a 16-lane group fetches a [4 pixels][16 channels] block (each lane 4 consecutive channels of one
// pixel) and every lane receives the 4 pixels of ITS channel - two reads per 32x16 operand, no VALU.
// Row stride = tile width + 32 elements (64 bytes: BM = 128 -> 320 B, BM = 64 -> 192 B), i.e. 64 or 192 mod 256:
// the 4 pixel rows x 2 channel groups a 32-lane half touches fall into 8 different 32-byte bank groups.
template <int BM, int BN>
__global__ void __launch_bounds__(256) wgrad_tr_kernel(const WgradParams p) {
    constexpr int MR = BM / 64, NR = BN / 64;              // 4 waves as 2 x 2, wave tile (BM/2) x (BN/2)
    constexpr int SA = BM + 32, SB = BN + 32;              // LDS row strides in bf16 elements
    constexpr int ALPR = BM / 8, ARPP = 256 / ALPR, APASS = 32 / ARPP;   // 16-byte lanes per row, rows per pass
    constexpr int BLPR = BN / 8, BRPP = 256 / BLPR, BPASS = 32 / BRPP;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bf16_t* As = reinterpret_cast<bf16_t*>(smem);          // [2][32 px][SA]   dY tile
    bf16_t* Bs = As + 2 * 32 * SA;                         // [2][32 px][SB]   X tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    int b = bx;
    const int tn = b % p.tiles_n;
    b /= p.tiles_n;
    const int tap = b % p.T;
    const int co0 = (b / p.T) * BM, cn0 = tn * BN;
    const bool first = cn0 < p.C0;
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;
    const int dh = p.taps[tap].dh, dw = p.taps[tap].dw;
    const int ohw = p.OH * p.OW;
    const int kt0 = by * p.kt_per_split, kt1 = min(kt0 + p.kt_per_split, p.ktiles);

    __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(first ? p.X0 : p.X1), 0,
                                                                   first ? p.bytesX0 : p.bytesX1, 0x00020000);
    __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.DY), 0, p.bytesDY, 0x00020000);
    const int a_c8 = tid % ALPR, a_r = tid / ALPR, b_c8 = tid % BLPR, b_r = tid / BLPR;
    int a_const[APASS], b_const[BPASS], b_k[BPASS];
#pragma unroll
    for (int j = 0; j < APASS; ++j) a_const[j] = (a_r + j * ARPP) * p.ldDY + co0 + a_c8 * 8;
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
        b_k[j] = (b_r + j * BRPP) * p.stride + dw;
        b_const[j] = b_k[j] * ldx + xch + b_c8 * 8;
    }
    i32x4 ra[APASS], rb[BPASS];
    // (image, output row, first column) of the NEXT tile to fetch - the tiles are fetched in order: no division per tile
    int t_n = (kt0 * 32) / ohw, t_oh = ((kt0 * 32) - t_n * ohw) / p.OW, t_ow0 = (kt0 * 32) - t_n * ohw - t_oh * p.OW;
    auto gload = [&](int kt) {      // a 32-pixel reduction tile lies inside one output row (OW % 32 == 0)
        const int mb = kt * 32;
        const int n = t_n, oh = t_oh, ow0 = t_ow0;
        t_ow0 += 32;
        if (t_ow0 >= p.OW) {
            t_ow0 = 0;
            if (++t_oh == p.OH) {
                t_oh = 0;
                ++t_n;
            }
        }
        const int ih = oh * p.stride + dh;
        const bool rowok = (unsigned)ih < (unsigned)p.IH;
        const int iw0 = ow0 * p.stride;
        const int ubase = ((n * p.IH + ih) * p.IW + iw0) * ldx;
        const int dbase = mb * p.ldDY;
#pragma unroll
        for (int j = 0; j < APASS; ++j) ra[j] = __builtin_amdgcn_raw_buffer_load_b128(rsD, (dbase + a_const[j]) << 1, 0, 0);
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const bool ok = rowok && (unsigned)(iw0 + b_k[j]) < (unsigned)p.IW;
            rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? ((ubase + b_const[j]) << 1) : (int)0x80000000, 0, 0);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < APASS; ++j)
            *reinterpret_cast<i32x4*>(As + (buf * 32 + a_r + j * ARPP) * SA + a_c8 * 8) = ra[j];
#pragma unroll
        for (int j = 0; j < BPASS; ++j)
            *reinterpret_cast<i32x4*>(Bs + (buf * 32 + b_r + j * BRPP) * SB + b_c8 * 8) = rb[j];
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i) zero_acc(acc[i]);

    const int frow = tr_row(lane), fcol = tr_col(lane);
    if (kt0 < kt1) {
        gload(kt0);
        lstore(0);
        if (kt0 + 1 < kt1) gload(kt0 + 1);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        if (kt + 1 < kt1) {
            lstore(buf ^ 1);
            if (kt + 2 < kt1) gload(kt + 2);
        }
        const bf16_t* a = As + (buf * 32 + frow) * SA + wm * (BM / 2) + fcol;
        const bf16_t* bb = Bs + (buf * 32 + frow) * SB + wn * (BN / 2) + fcol;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[MR], bf[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) {
                af[i] = tr_frag(a + (16 * ks) * SA + i * 32, a + (16 * ks + 4) * SA + i * 32);
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                bf[j] = tr_frag(bb + (16 * ks) * SB + j * 32, bb + (16 * ks + 4) * SB + j * 32);
            }
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // slab: part[split][co][T][Ctot]
    const size_t rowlen = (size_t)p.T * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const size_t coloff = (size_t)tap * p.Ctot + cn0 + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = co0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                slab[(size_t)row * rowlen + coloff] = acc[i][j][r];
            }
    }
}

// XV2_MATH_F32X3 variant of wgrad_tr_kernel: fp32 dY / X tiles split into three bf16 planes on their way into LDS
// (single-buffered, 60 KB for 128 x 128), six bf16 MFMAs per product.  Two raw register sets as in the implicit-GEMM
// kernel: tile kt+1 is split on the VALU in the shadow of tile kt's MFMAs while tile kt+2 is in flight.
template <int BM, int BN, int NPL = 3>
__global__ void __launch_bounds__(256) wgrad_tr_x3_kernel(const WgradParams p) {
    constexpr int MR = BM / 64, NR = BN / 64;
    constexpr int SA = BM + 32, SB = BN + 32;              // LDS row strides in bf16 elements
    constexpr int PL = 32 * (SA + SB);                     // elements per plane
    constexpr int ALPR = BM / 4, ARPP = 256 / ALPR, APASS = 32 / ARPP;   // 16-byte (4 float) lanes per row
    constexpr int BLPR = BN / 4, BRPP = 256 / BLPR, BPASS = 32 / BRPP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bf16_t* As = reinterpret_cast<bf16_t*>(smem);          // [32 px][SA]   dY tile, plane 0 (planes PL apart)
    bf16_t* Bs = As + 32 * SA;                             // [32 px][SB]   X tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int l31 = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    int b = bx;
    const int tn = b % p.tiles_n;
    b /= p.tiles_n;
    const int tap = b % p.T;
    const int co0 = (b / p.T) * BM, cn0 = tn * BN;
    const bool first = cn0 < p.C0;
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;
    const int dh = p.taps[tap].dh, dw = p.taps[tap].dw;
    const int ohw = p.OH * p.OW;
    const int kt0 = by * p.kt_per_split, kt1 = min(kt0 + p.kt_per_split, p.ktiles);
    float sX = 1.f, sD = 1.f;      // F16X2 operand scales
    if constexpr (NPL == 2) {
        sX = amax_scale(amax_exponent(first ? p.amaxX0 : p.amaxX1));
        sD = amax_scale(amax_exponent(p.amaxDY));
    }

    __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(first ? p.X0 : p.X1), 0,
                                                                   first ? p.bytesX0 : p.bytesX1, 0x00020000);
    __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.DY), 0, p.bytesDY, 0x00020000);
    const int a_c4 = tid % ALPR, a_r = tid / ALPR, b_c4 = tid % BLPR, b_r = tid / BLPR;
    int a_const[APASS], b_const[BPASS], b_k[BPASS];
#pragma unroll
    for (int j = 0; j < APASS; ++j) a_const[j] = (a_r + j * ARPP) * p.ldDY + co0 + a_c4 * 4;
#pragma unroll
    for (int j = 0; j < BPASS; ++j) {
        b_k[j] = (b_r + j * BRPP) * p.stride + dw;
        b_const[j] = b_k[j] * ldx + xch + b_c4 * 4;
    }
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    // (image, output row, first column) of the NEXT tile to fetch: the tiles are fetched in order kt0, kt0 + 1, ..., so the two
    // integer divisions per tile of the first version (~40 scalar instructions each) happen once per block
    int t_n = (kt0 * 32) / ohw, t_oh = ((kt0 * 32) - t_n * ohw) / p.OW, t_ow0 = (kt0 * 32) - t_n * ohw - t_oh * p.OW;
    auto gload_into = [&](int kt, i32x4 (&ra)[APASS], i32x4 (&rb)[BPASS]) {   // a 32-pixel tile lies inside one output row
        const int mb = kt * 32;
        const int n = t_n, oh = t_oh, ow0 = t_ow0;
        t_ow0 += 32;
        if (t_ow0 >= p.OW) {
            t_ow0 = 0;
            if (++t_oh == p.OH) {
                t_oh = 0;
                ++t_n;
            }
        }
        const int ih = oh * p.stride + dh;
        const bool rowok = (unsigned)ih < (unsigned)p.IH;
        const int iw0 = ow0 * p.stride;
        const int ubase = ((n * p.IH + ih) * p.IW + iw0) * ldx;
        const int dbase = mb * p.ldDY;
#pragma unroll
        for (int j = 0; j < APASS; ++j) ra[j] = __builtin_amdgcn_raw_buffer_load_b128(rsD, (dbase + a_const[j]) << 2, 0, 0);
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            const bool ok = rowok && (unsigned)(iw0 + b_k[j]) < (unsigned)p.IW;
            rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? ((ubase + b_const[j]) << 2) : (int)0x80000000, 0, 0);
        }
    };
    uint2 pk[APASS + BPASS][NPL];
    auto split_regs = [&](const i32x4 (&xa)[APASS], const i32x4 (&xb)[BPASS]) {
#pragma unroll
        for (int j = 0; j < APASS + BPASS; ++j) {
            const i32x4 v = j < APASS ? xa[j < APASS ? j : 0] : xb[j >= APASS ? j - APASS : 0];
            const float4 f = make_float4(__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]));
            split_planes<NPL>(f, j < APASS ? sD : sX, pk[j]);
        }
    };
    auto store_planes = [&]() {
#pragma unroll
        for (int j = 0; j < APASS + BPASS; ++j) {
            bf16_t* d = j < APASS ? As + (a_r + j * ARPP) * SA + a_c4 * 4 : Bs + (b_r + (j - APASS) * BRPP) * SB + b_c4 * 4;
#pragma unroll
            for (int q = 0; q < NPL; ++q) *reinterpret_cast<uint2*>(d + q * PL) = pk[j][q];
        }
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int i = 0; i < MR; ++i) zero_acc(acc[i]);

    const int frow = tr_row(lane), fcol = tr_col(lane);
    auto frag = [&](const bf16_t* base, int stride) {
        return tr_frag(base, base + 4 * stride);
    };
    auto mfma_tile = [&]() {
        const bf16_t* a = As + frow * SA + wm * (BM / 2) + fcol;
        const bf16_t* bb = Bs + frow * SB + wn * (BN / 2) + fcol;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 ah[MR], am[MR], al[MR], bh[NR], bm_[NR], bl[NR];
#pragma unroll
            for (int i = 0; i < MR; ++i) {
                ah[i] = frag(a + (16 * ks) * SA + i * 32, SA);
                am[i] = frag(a + PL + (16 * ks) * SA + i * 32, SA);
                if constexpr (NPL == 3) al[i] = frag(a + 2 * PL + (16 * ks) * SA + i * 32, SA);
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                bh[j] = frag(bb + (16 * ks) * SB + j * 32, SB);
                bm_[j] = frag(bb + PL + (16 * ks) * SB + j * 32, SB);
                if constexpr (NPL == 3) bl[j] = frag(bb + 2 * PL + (16 * ks) * SB + j * 32, SB);
            }
            if constexpr (NPL == 2) {
#pragma unroll
                for (int t = 0; t < 3; ++t)
#pragma unroll
                    for (int i = 0; i < MR; ++i)
#pragma unroll
                        for (int j = 0; j < NR; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, t == 0 ? am[i] : ah[i]),
                                                                               __builtin_bit_cast(f16x8, t == 1 ? bm_[j] : bh[j]),
                                                                               acc[i][j], 0, 0, 0);
            } else
#pragma unroll
            for (int t = XV2_T0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < MR; ++i)
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        const bf16x8 x = t == 0 ? al[i] : t == 1 ? ah[i] : t == 2 ? am[i] : t == 3 ? am[i] : ah[i];
                        const bf16x8 y = t == 0 ? bh[j] : t == 1 ? bl[j] : t == 2 ? bm_[j] : t == 3 ? bh[j] : t == 4 ? bm_[j] : bh[j];
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc[i][j], 0, 0, 0);
                    }
        }
#pragma unroll
        for (int j = 0; j < APASS + BPASS; ++j)
#pragma unroll
            for (int q = 0; q < NPL; ++q) asm volatile("" : "+v"(pk[j][q].x), "+v"(pk[j][q].y));
        constexpr int NMFMA = 2 * (NPL == 2 ? 3 : 6 - XV2_T0) * MR * NR;
#pragma unroll
        for (int g = 0; g < NMFMA; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, (APASS + BPASS) * 18 / NMFMA + 1, 0);
        }
    };
    i32x4 ra0[APASS], rb0[BPASS], ra1[APASS], rb1[BPASS];
    auto step = [&](int kt, i32x4 (&xa)[APASS], i32x4 (&xb)[BPASS]) {
        split_regs(xa, xb);
        mfma_tile();
        __syncthreads();
        if (kt + 1 < kt1) {
            store_planes();
            if (kt + 3 < kt1) gload_into(kt + 3, xa, xb);
        }
        __syncthreads();
    };
    if (kt0 < kt1) {
        gload_into(kt0, ra0, rb0);
        split_regs(ra0, rb0);
        store_planes();
        if (kt0 + 1 < kt1) gload_into(kt0 + 1, ra1, rb1);
        if (kt0 + 2 < kt1) gload_into(kt0 + 2, ra0, rb0);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; kt += 2) {
        step(kt, ra1, rb1);
        if (kt + 1 < kt1) step(kt + 1, ra0, rb0);
    }
    // slab: part[split][co][T][Ctot]
    const size_t rowlen = (size_t)p.T * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
    float iX = 1.f, iD = 1.f;
    if constexpr (NPL == 2) {
        iX = amax_inv(amax_exponent(first ? p.amaxX0 : p.amaxX1));
        iD = amax_inv(amax_exponent(p.amaxDY));
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const size_t coloff = (size_t)tap * p.Ctot + cn0 + wn * (BN / 2) + j * 32 + l31;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = co0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                slab[(size_t)row * rowlen + coloff] = NPL == 2 ? acc[i][j][r] * iX * iD : acc[i][j][r];
            }
    }
}
// ---------------------------------------------------------------------------------------------------------------
// What the five all-taps kernels share (the row loop of their ring walk and their epilogues are written out in each: as
// helpers they changed the kernels' instruction streams).
// Strip decode: block (bx, by) -> (co, ci) tile of width TILE, sample n, 32-pixel column strip at ow0 and the output rows
// r0 .. r1 - 1 of the strip's row chunk (`chunks` chunks of `rows_per` rows)
struct Strip {
    int co0, cn0, n, ow0, r0, r1;
};
template <int TILE>
__device__ __forceinline__ Strip alltaps_strip(int bx, int by, int tiles_n, int chunks, int rows_per, int OW, int OH) {
    Strip s;
    const int tn = bx % tiles_n, tm = bx / tiles_n;
    s.co0 = tm * TILE, s.cn0 = tn * TILE;
    const int strip = by / chunks, chunk = by % chunks;
    const int tilesW = OW / 32;
    s.n = strip / tilesW, s.ow0 = (strip % tilesW) * 32;
    s.r0 = chunk * rows_per, s.r1 = min(s.r0 + rows_per, OH);
    return s;
}
// Split-plane put: four fp32 values as NPL planes (PL elements apart) at element offset `off` of a plane
template <int NPL, int PL>
__device__ __forceinline__ void put_planes(bf16_t* planes, int off, const float4 v, float s) {
    uint2 h, m, l;
    if constexpr (NPL == 2) {
        split2hx4(v, s, h, m);
    } else {
        split3x4(v, h, m, l);
        *reinterpret_cast<uint2*>(planes + (NPL - 1) * PL + off) = l;
    }
    *reinterpret_cast<uint2*>(planes + off) = h;
    *reinterpret_cast<uint2*>(planes + PL + off) = m;
}
// Ring walk, prologue: input rows r0-1, r0, r0+1 into their ring slots and dY(r0) into buffer 0.  (Row step r then prefetches
// dY(r+1) and input row r+2 into registers in front of its MFMAs and stores them behind, where step r-1 read last - all waves
// are past its barrier: dY buffer buf ^ 1 and the ring slot of row r-2.)
template <class LDY, class LX, class SDY, class SX>
__device__ __forceinline__ void ring_prologue(int r0, const LDY& load_dy, const LX& load_x, const SDY& store_dy, const SX& store_x) {
    load_x(r0 - 1);
    store_x(r0 - 1);
    load_x(r0);
    store_x(r0);
    load_x(r0 + 1);
    store_x(r0 + 1);
    load_dy(r0);
    store_dy(0);
    __syncthreads();
}

// All-taps variant for 3x3 / stride 1 / pad 1 layers with few channels (the 1024x1024 decoder level, 32 -> 32).
// The per-tap kernel above re-reads the dY tile and a shifted X tile for every tap: 8 KB of L2->LDS traffic per
// 16 MFMAs per wave set, which is what bounds it at ~58 TFLOP/s for a 32x32 tile.  Here one block owns a
// (32 co x 32 ci) tile for ALL 9 taps (9 accumulators = 144 VGPRs per lane) and walks DOWN a 32-pixel-wide column
// strip: per output row it pulls ONE new input row (34 pixels incl. halo) into a 4-row LDS ring and one dY row -
// 8.4 KB per 36 MFMAs per wave.  The 4 waves split the 16 k-steps of a row (WK = 4) and are summed through LDS at
// the end, so a block emits one slab.  model/layers.py:92 (ConvLayer 3x3) weight gradient.
// BF16 = true (XV2_MATH_BF16): same data movement; a wave takes one 16-pixel k-group of the row and every other tap
// (5 or 4 accumulators), gathers 8 pixels of its channel per lane out of the fp32 LDS rows, rounds them to bf16 and
// issues v_mfma_f32_32x32x16_bf16.  Pixel rows are padded to 36 floats so the two lane halves (8 pixels apart) fall
// into different banks.
template <bool BF16>
__global__ void __launch_bounds__(256, 2) wgrad_alltaps_kernel(const WgradParams p) {
    constexpr int LDP = BF16 ? 36 : 32;
    __shared__ __attribute__((aligned(16))) float smem[(2 * 32 + 4 * 34) * LDP < 4096 ? 4096 : (2 * 32 + 4 * 34) * LDP];
    float* dYs = smem;                  // [2][32 px][LDP]
    float* Xs = smem + 2 * 32 * LDP;    // [4 ring rows][34 px][LDP]

    const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int l31 = lane & 31, h = lane >> 5;
    const Strip s = alltaps_strip<32>(bx, by, p.tiles_n, p.ktiles, p.kt_per_split, p.OW, p.OH);
    const int co0 = s.co0, cn0 = s.cn0, n = s.n, ow0 = s.ow0, r0 = s.r0, r1 = s.r1;

    const float* xsrc;
    int ldx, xch;
    if (cn0 < p.C0) {
        xsrc = p.X0; ldx = p.ldX0; xch = cn0;
    } else {
        xsrc = p.X1; ldx = p.ldX1; xch = cn0 - p.C0;
    }
    const int px = tid >> 3, c4 = tid & 7;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 rd, rx0, rx1;
    // per-thread element pointers at image row 0 of sample n; a row step is ONE uniform pitch away (the 64-bit
    // index arithmetic of three loads per row was a third of this kernel's vector instructions)
    const float* dy0 = p.DY + ((size_t)n * p.OH * p.OW + ow0 + px) * p.ldDY + co0 + c4 * 4;
    const size_t dy_pitch = (size_t)p.OW * p.ldDY;
    const int iw = ow0 - 1 + px;
    const float* xa0 = xsrc + ((size_t)n * p.IH * p.IW + iw) * ldx + xch + c4 * 4;   // halo pixel px
    const size_t x_pitch = (size_t)p.IW * ldx;
    const bool xa_ok = iw >= 0, xb_ok = tid < 16 && iw + 32 < p.IW;                        // halo pixels 32, 33
    auto load_dy = [&](int r) { rd = ld4(dy0 + (size_t)r * dy_pitch); };
    auto load_x = [&](int ih) {      // input row ih, pixels ow0-1 .. ow0+32
        rx0 = zero4;
        rx1 = zero4;
        if ((unsigned)ih < (unsigned)p.IH) {
            const float* row = xa0 + (size_t)ih * x_pitch;
            if (xa_ok) rx0 = ld4(row);
            if (xb_ok) rx1 = ld4(row + (size_t)32 * ldx);
        }
    };
    auto store_dy = [&](int buf) { *reinterpret_cast<float4*>(dYs + buf * (32 * LDP) + px * LDP + c4 * 4) = rd; };
    auto store_x = [&](int ih) {
        float* ring = Xs + ((ih + 4) & 3) * (34 * LDP);
        *reinterpret_cast<float4*>(ring + px * LDP + c4 * 4) = rx0;
        if (tid < 16) *reinterpret_cast<float4*>(ring + (px + 32) * LDP + c4 * 4) = rx1;
    };

    constexpr int NACC = BF16 ? 5 : 9;
    f32x16 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // prologue: rows r0-1, r0, r0+1 and dY(r0)
    ring_prologue(r0, load_dy, load_x, store_dy, store_x);
    for (int r = r0; r < r1; ++r) {
        const int buf = (r - r0) & 1;
        const bool more = r + 1 < r1;
        if (more) {
            load_dy(r + 1);
            load_x(r + 2);
        }
        const float* a = dYs + buf * (32 * LDP) + l31;
        const float* x0 = Xs + ((r + 3) & 3) * (34 * LDP) + l31;   // row r-1
        const float* x1 = Xs + (r & 3) * (34 * LDP) + l31;         // row r
        const float* x2 = Xs + ((r + 1) & 3) * (34 * LDP) + l31;   // row r+1
        if constexpr (BF16) {
            const int q0 = 16 * (wk & 1) + 8 * h;      // this lane's 8 pixels of the wave's k-group
            const int odd = wk >> 1;                   // taps 0,2,4,6,8 (odd == 0) or 1,3,5,7
            bf16x8 af;
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (__bf16)a[(q0 + j) * LDP];
            const float* rows[3] = {x0, x1, x2};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                float v[10];           // pixels q0 .. q0+9 of input row r-1+kh (the three horizontal taps overlap)
#pragma unroll
                for (int j = 0; j < 10; ++j) v[j] = rows[kh][(q0 + j) * LDP];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int t = kh * 3 + kw;
                    if ((t & 1) != odd) continue;      // wave-uniform
                    bf16x8 bf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) bf[j] = (__bf16)v[j + kw];
                    acc[t >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t >> 1], 0, 0, 0);
                }
            }
        } else
#pragma unroll
        for (int s0 = 0; s0 < 4; ++s0) {
            const int q = 2 * (s0 * 4 + wk) + h;
            const float af = a[q * 32];
            float bf[9];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                bf[kw] = x0[(q + kw) * 32];
                bf[3 + kw] = x1[(q + kw) * 32];
                bf[6 + kw] = x2[(q + kw) * 32];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf[t], acc[t], 0, 0, 0);
        }
        if (more) {
            store_dy(buf ^ 1);    // last read in step r-1 (all waves are past its barrier)
            store_x(r + 2);       // ring slot of row r-2, idem
        }
        __syncthreads();
    }

    // sum the 4 waves' k-partials through LDS (16 KB per tap) and write the block's slab part[y][co][T][Ctot]
    const size_t rowlen = (size_t)9 * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        if constexpr (BF16) {
            // the two waves that own tap t (k-groups 0 and 1) deposit it; the other two slots stay zero
            const bool mine = (wk >> 1) == (t & 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) smem[wk * 1024 + r * 64 + lane] = mine ? acc[(t >> 1) < NACC ? (t >> 1) : 0][r] : 0.f;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) smem[wk * 1024 + r * 64 + lane] = acc[t < NACC ? t : 0][r];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j;
            const float v = (smem[e] + smem[1024 + e]) + (smem[2048 + e] + smem[3072 + e]);
            const int r = e >> 6, ln = e & 63;
            const int row = co0 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
            slab[(size_t)row * rowlen + (size_t)t * p.Ctot + cn0 + (ln & 31)] = v;
        }
        __syncthreads();
    }
}

// bf16-native all-taps variant (XV2_MATH_BF16_STORE): same block / strip / ring organisation as above, but the dY row and
// the 4-row X ring live in LDS as bf16 exactly as loaded (16-byte loads, [pixel][32 channels], 64-byte rows: four
// consecutive pixel rows fill one 256-byte bank row) and every MFMA operand is two ds_read_b64_tr_b16 transpose reads
// instead of 8-10 ds_read_b32 + as many conversions - the fp32-LDS bf16 variant spent twice the MFMA time in the LDS.
// Wave wk takes the 16-pixel k-group (wk & 1) and the taps of parity (wk >> 1), as in the BF16 branch above.
__global__ void __launch_bounds__(256, 4) wgrad_alltaps_tr_kernel(const WgradParams p) {
    __shared__ __attribute__((aligned(16))) float smem[4096];     // 16 KB: operand image (12.9 KB) / epilogue fold
    bf16_t* dYs = reinterpret_cast<bf16_t*>(smem);                // [2][32 px][32 co]
    bf16_t* Xs = dYs + 2 * 32 * 32;                               // [4 ring rows][34 px][32 ci]
    typedef int i32x4 __attribute__((ext_vector_type(4)));

    const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const Strip s = alltaps_strip<32>(bx, by, p.tiles_n, p.ktiles, p.kt_per_split, p.OW, p.OH);
    const int co0 = s.co0, cn0 = s.cn0, n = s.n, ow0 = s.ow0, r0 = s.r0, r1 = s.r1;
    const bool first = cn0 < p.C0;
    const bf16_t* xsrc = reinterpret_cast<const bf16_t*>(first ? p.X0 : p.X1);
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;

    // loads: 4 lanes x 16 bytes per pixel; threads 0..127 the dY row (32 px), threads 0..135 the X row (34 px)
    const int px = tid >> 2, c8 = tid & 3;
    const bf16_t* dy0 = reinterpret_cast<const bf16_t*>(p.DY) + ((size_t)n * p.OH * p.OW + ow0 + (px & 31)) * p.ldDY + co0 + c8 * 8;
    const size_t dy_pitch = (size_t)p.OW * p.ldDY;
    const int iw = ow0 - 1 + px;
    const bf16_t* xa0 = xsrc + ((size_t)n * p.IH * p.IW + iw) * ldx + xch + c8 * 8;
    const size_t x_pitch = (size_t)p.IW * ldx;
    const bool do_dy = tid < 128, do_x = tid < 136 && iw >= 0 && iw < p.IW;
    const i32x4 zero = {0, 0, 0, 0};
    i32x4 rd = zero, rx = zero;
    auto load_dy = [&](int r) { if (do_dy) rd = *reinterpret_cast<const i32x4*>(dy0 + (size_t)r * dy_pitch); };
    auto load_x = [&](int ih) {
        rx = zero;
        if (do_x && (unsigned)ih < (unsigned)p.IH) rx = *reinterpret_cast<const i32x4*>(xa0 + (size_t)ih * x_pitch);
    };
    auto store_dy = [&](int buf) { if (do_dy) *reinterpret_cast<i32x4*>(dYs + (buf * 32 + px) * 32 + c8 * 8) = rd; };
    auto store_x = [&](int ih) { if (tid < 136) *reinterpret_cast<i32x4*>(Xs + (((ih + 4) & 3) * 34 + px) * 32 + c8 * 8) = rx; };

    f32x16 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int q0 = 16 * (wk & 1), odd = wk >> 1;
    const int frow = q0 + tr_row(lane), fcol = tr_col(lane);
    auto frag = [&](const bf16_t* base) {       // base -> pixel row `frow` of the operand, channel fcol
        return tr_frag(base, base + 4 * 32);
    };

    ring_prologue(r0, load_dy, load_x, store_dy, store_x);
    for (int r = r0; r < r1; ++r) {
        const int buf = (r - r0) & 1;
        const bool more = r + 1 < r1;
        if (more) {
            load_dy(r + 1);
            load_x(r + 2);
        }
        const bf16x8 af = frag(dYs + (buf * 32 + frow) * 32 + fcol);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const bf16_t* row = Xs + (((r - 1 + kh + 4) & 3) * 34 + frow) * 32 + fcol;     // input row r-1+kh
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int t = kh * 3 + kw;
                if ((t & 1) != odd) continue;          // wave-uniform
                const bf16x8 bf = frag(row + kw * 32);  // halo pixel = output pixel + kw
                acc[t >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t >> 1], 0, 0, 0);
            }
        }
        if (more) {
            store_dy(buf ^ 1);    // last read in step r-1 (all waves are past its barrier)
            store_x(r + 2);       // ring slot of row r-2, idem
        }
        __syncthreads();
    }

    // fold the two k-groups of every tap through LDS and write the block's slab part[y][co][T][Ctot]
    const size_t rowlen = (size_t)9 * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const bool mine = (wk >> 1) == (t & 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[wk * 1024 + r * 64 + lane] = mine ? acc[t >> 1][r] : 0.f;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j;
            const float v = (smem[e] + smem[1024 + e]) + (smem[2048 + e] + smem[3072 + e]);
            const int r = e >> 6, ln = e & 63;
            const int row = co0 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
            slab[(size_t)row * rowlen + (size_t)t * p.Ctot + cn0 + (ln & 31)] = v;
        }
        __syncthreads();
    }
}

// XV2_MATH_F32X3 all-taps variant: fp32 dY / X in HBM, every element split into three bf16 terms (split3x4) on its way
// into LDS - three bf16 planes of the operand image the kernel above uses, 38 KB - and every tap product issued as the
// six significant bf16 cross products (hh, hm, mh, mm, hl, lh; the dropped ml, lm, ll terms are below 2^-23 of |x||dy|).
// 24-30 MFMAs per wave per row step instead of 4-5: the kernel is MFMA-bound where the bf16 one is latency-bound.
// Wave wk takes the 16-pixel k-group (wk & 1) and the taps of one parity; which parity gets the 5-tap share alternates
// pseudo-randomly between blocks so that the SIMDs of a CU are loaded evenly.
template <int NPL>
__global__ void __launch_bounds__(256, 3) wgrad_alltaps_x3_kernel(const WgradParams p) {
    constexpr int PL = 2 * 32 * 32 + 4 * 34 * 32;                 // bf16 elements per plane (dY double buffer + X ring)
    __shared__ __attribute__((aligned(16))) bf16_t planes[NPL * PL];   // 38.4 KB (two planes: 25.6); the epilogue fold reuses the first 16 KB
    float* smem = reinterpret_cast<float*>(planes);

    const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const Strip s = alltaps_strip<32>(bx, by, p.tiles_n, p.ktiles, p.kt_per_split, p.OW, p.OH);
    const int co0 = s.co0, cn0 = s.cn0, n = s.n, ow0 = s.ow0, r0 = s.r0, r1 = s.r1;
    const bool first = cn0 < p.C0;
    const float* xsrc = first ? p.X0 : p.X1;
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;

    // loads: 8 lanes x 16 bytes per pixel; all threads the dY row and X pixels 0..31, threads 0..15 X pixels 32, 33
    const int px = tid >> 3, c4 = tid & 7;
    const float* dy0 = p.DY + ((size_t)n * p.OH * p.OW + ow0 + px) * p.ldDY + co0 + c4 * 4;
    const size_t dy_pitch = (size_t)p.OW * p.ldDY;
    const int iw = ow0 - 1 + px, iw2 = iw + 32;
    const float* xa0 = xsrc + ((size_t)n * p.IH * p.IW + iw) * ldx + xch + c4 * 4;
    const size_t x_pitch = (size_t)p.IW * ldx;
    const bool x_ok = iw >= 0, x2 = tid < 16, x2_ok = x2 && iw2 < p.IW;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rd = zero, rx = zero, rx2 = zero;
    auto load_dy = [&](int r) { rd = *reinterpret_cast<const float4*>(dy0 + (size_t)r * dy_pitch); };
    auto load_x = [&](int ih) {
        rx = zero;
        rx2 = zero;
        if ((unsigned)ih < (unsigned)p.IH) {
            if (x_ok) rx = *reinterpret_cast<const float4*>(xa0 + (size_t)ih * x_pitch);
            if (x2_ok) rx2 = *reinterpret_cast<const float4*>(xa0 + (size_t)ih * x_pitch + (size_t)32 * ldx);
        }
    };
    float sX, sD;      // F16X2 operand scales
    plane_scales<NPL, false>(p, first, sX, sD);
    auto put = [&](int off, const float4 v, float sc) { put_planes<NPL, PL>(planes, off, v, sc); };       // off: element offset inside a plane
    auto store_dy = [&](int buf) { put((buf * 32 + px) * 32 + c4 * 4, rd, sD); };
    auto store_x = [&](int ih) {
        const int ring = 2 * 32 * 32 + ((ih + 4) & 3) * 34 * 32;
        put(ring + px * 32 + c4 * 4, rx, sX);
        if (x2) put(ring + (32 + px) * 32 + c4 * 4, rx2, sX);
    };

    f32x16 acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int q0 = 16 * (wk & 1);
    const int flip = (bx ^ (bx >> 3) ^ by ^ (by >> 3)) & 1;
    const int odd = (wk >> 1) ^ flip;
    const int frow = q0 + tr_row(lane), fcol = tr_col(lane);
    auto frag = [&](const bf16_t* base) {
        return tr_frag(base, base + 4 * 32);
    };

    ring_prologue(r0, load_dy, load_x, store_dy, store_x);
    for (int r = r0; r < r1; ++r) {
        const int buf = (r - r0) & 1;
        const bool more = r + 1 < r1;
        if (more) {
            load_dy(r + 1);
            load_x(r + 2);
        }
        const bf16_t* ab = planes + (buf * 32 + frow) * 32 + fcol;
        const bf16x8 ah = frag(ab), am = frag(ab + PL), al = NPL == 3 ? frag(ab + (NPL - 1) * PL) : ah;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const bf16_t* row = planes + 2 * 32 * 32 + (((r - 1 + kh + 4) & 3) * 34 + frow) * 32 + fcol;   // input row r-1+kh
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int t = kh * 3 + kw;
                if ((t & 1) != odd) continue;          // wave-uniform
                const bf16x8 bh = frag(row + kw * 32), bm = frag(row + kw * 32 + PL);
                f32x16 c = acc[t >> 1];
                if constexpr (NPL == 2) {
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, am), __builtin_bit_cast(f16x8, bh), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bm), c, 0, 0, 0);
                    acc[t >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bh), c, 0, 0, 0);
                    continue;
                }
                const bf16x8 bl = frag(row + kw * 32 + (NPL - 1) * PL);
#if XV2_T0 == 0
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
#endif
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
                acc[t >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
            }
        }
        if (more) {
            store_dy(buf ^ 1);    // last read in step r-1 (all waves are past its barrier)
            store_x(r + 2);       // ring slot of row r-2, idem
        }
        __syncthreads();
    }

    // fold the two k-groups of every tap through LDS and write the block's slab part[y][co][T][Ctot]
    const size_t rowlen = (size_t)9 * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
    float iX, iD;
    plane_scales<NPL, true>(p, first, iX, iD);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const bool mine = odd == (t & 1);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            smem[wk * 1024 + r * 64 + lane] = mine ? (NPL == 2 ? acc[t >> 1][r] * iX * iD : acc[t >> 1][r]) : 0.f;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + 256 * j;
            const float v = (smem[e] + smem[1024 + e]) + (smem[2048 + e] + smem[3072 + e]);
            const int r = e >> 6, ln = e & 63;
            const int row = co0 + (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
            slab[(size_t)row * rowlen + (size_t)t * p.Ctot + cn0 + (ln & 31)] = v;
        }
        __syncthreads();
    }
}

// wgrad_alltaps_x3_kernel with a 64 co x 64 ci tile per block.  Why: that kernel's producer (load, three-way split, plane
// stores of one dY row and one input row per row step) costs 30 % of its time (ablation) and it is redone by every
// (co tile, ci tile) block of a strip - the dY row Ctot / 32 times, the input row Cout / 32 times.  With 64 x 64 tiles
// the same row step feeds four times the MFMAs for twice the producer work: emulated (every second row step's producer
// skipped) the 116-GFLOP decoder layers ran 16 - 20 % faster.  Each of the four waves owns a 32 x 32 quadrant for all nine
// taps and both 16-pixel k-steps (144 accumulator VGPRs, no cross-wave fold in the epilogue); LDS rows are 64 channels =
// 128 B with the 32-byte chunks of pixel column p stored at chunk ^ (p & 3) (conflict-free transpose reads and stores).
constexpr int W64_PL = 2 * 32 * 64 + 4 * 34 * 64;                 // bf16 elements per plane: dY double buffer + X ring
__device__ __forceinline__ int w64_off(int px, int c) { return px * 64 + ((((c >> 4) ^ (px & 3)) << 4) | (c & 15)); }
template <int NPL>
__global__ void __launch_bounds__(256, 2) wgrad_alltaps64_x3_kernel(const WgradParams p) {
    extern __shared__ __attribute__((aligned(16))) bf16_t planes64[];      // [NPL][W64_PL]: 76.8 KB (51.2)
    bf16_t* planes = planes64;
    constexpr int PL = W64_PL;
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int wa = wave >> 1, wb = wave & 1;                            // co half / ci half of this wave's quadrant
    const Strip s = alltaps_strip<64>(bx, by, p.tiles_n, p.ktiles, p.kt_per_split, p.OW, p.OH);
    const int co0 = s.co0, cn0 = s.cn0, n = s.n, ow0 = s.ow0, r0 = s.r0, r1 = s.r1;
    const bool first = cn0 < p.C0;
    const float* xsrc = first ? p.X0 : p.X1;
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;
    // loads: 16 lanes x 16 bytes per pixel (64 channels); slot s = tid + 256 j: pixel s >> 4, channel quad s & 15
    const int c4 = tid & 15, pxa = tid >> 4;                            // pixels pxa and pxa + 16; threads < 32 also 32 + (tid >> 4)
    const float* dy0 = p.DY + ((size_t)n * p.OH * p.OW + ow0 + pxa) * p.ldDY + co0 + c4 * 4;
    const size_t dy_pitch = (size_t)p.OW * p.ldDY;
    const int iw = ow0 - 1 + pxa;
    const float* xa0 = xsrc + ((size_t)n * p.IH * p.IW + iw) * ldx + xch + c4 * 4;
    const size_t x_pitch = (size_t)p.IW * ldx;
    const bool xok0 = iw >= 0, xok1 = true, x2 = tid < 32, xok2 = x2 && iw + 32 < p.IW;      // iw + 16 is always inside
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rd0 = zero, rd1 = zero, rx0 = zero, rx1 = zero, rx2 = zero;
    auto load_dy = [&](int r) {
        rd0 = *reinterpret_cast<const float4*>(dy0 + (size_t)r * dy_pitch);
        rd1 = *reinterpret_cast<const float4*>(dy0 + (size_t)r * dy_pitch + (size_t)16 * p.ldDY);
    };
    auto load_x = [&](int ih) {
        rx0 = rx1 = rx2 = zero;
        if ((unsigned)ih < (unsigned)p.IH) {
            const float* xr = xa0 + (size_t)ih * x_pitch;
            if (xok0) rx0 = *reinterpret_cast<const float4*>(xr);
            if (xok1) rx1 = *reinterpret_cast<const float4*>(xr + (size_t)16 * ldx);
            if (xok2) rx2 = *reinterpret_cast<const float4*>(xr + (size_t)32 * ldx);
        }
    };
    float sX, sD;      // F16X2 operand scales
    plane_scales<NPL, false>(p, first, sX, sD);
    auto put = [&](int off, const float4 v, float sc) { put_planes<NPL, PL>(planes, off, v, sc); };
    auto store_dy = [&](int buf) {
        put(buf * 32 * 64 + w64_off(pxa, c4 * 4), rd0, sD);
        put(buf * 32 * 64 + w64_off(pxa + 16, c4 * 4), rd1, sD);
    };
    auto store_x = [&](int ih) {
        const int ring = 2 * 32 * 64 + ((ih + 4) & 3) * 34 * 64;
        put(ring + w64_off(pxa, c4 * 4), rx0, sX);
        put(ring + w64_off(pxa + 16, c4 * 4), rx1, sX);
        if (x2) put(ring + w64_off(pxa + 32, c4 * 4), rx2, sX);
    };
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int i16 = lane & 15, grp = lane >> 4;
    const int frow = 8 * (grp >> 1) + (i16 >> 2), fcol = 16 * (grp & 1) + 4 * (i16 & 3);
    auto frag = [&](const bf16_t* base, int px, int c) {       // transposed 16-pixel x 32-channel operand at (px, c)
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(base + w64_off(px, c)));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(base + w64_off(px + 4, c)));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };
    ring_prologue(r0, load_dy, load_x, store_dy, store_x);
    for (int r = r0; r < r1; ++r) {
        const int buf = (r - r0) & 1;
        const bool more = r + 1 < r1;
        if (more) {
            load_dy(r + 1);
            load_x(r + 2);
        }
        const bf16_t* ab = planes + buf * 32 * 64;
        if constexpr (NPL == 2) {
            // software pipeline over the 18 (k-step, tap) products of a row step: the transpose reads of product i + 1 are
            // issued BEFORE the three MFMAs of product i (8 more VGPRs)
            const int ca = wa * 32 + fcol, cb = wb * 32 + fcol;
            bf16x8 a_h[2], a_m[2], b_h[2], b_m[2];
            auto rowp = [&](int kh) { return planes + 2 * 32 * 64 + ((r - 1 + kh + 4) & 3) * 34 * 64; };
            a_h[0] = frag(ab, frow, ca);
            a_m[0] = frag(ab + PL, frow, ca);
            b_h[0] = frag(rowp(0), frow, cb);
            b_m[0] = frag(rowp(0) + PL, frow, cb);
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                const int ks = i / 9, t = i % 9, cur = i & 1;
                if (i + 1 < 18) {
                    const int ks1 = (i + 1) / 9, t1 = (i + 1) % 9, kh1 = t1 / 3, kw1 = t1 % 3;
                    // (read order: what the FIRST MFMA of the next product takes comes last - one wait in front of the three
                    //  MFMAs covers them all and nothing stands between MFMAs on one accumulator: ~43 cycles each, MI355X_MICROARCH)
                    if (t1 == 0) {
                        a_h[1] = frag(ab, 16 + frow, ca);
                        a_m[1] = frag(ab + PL, 16 + frow, ca);
                    }
                    b_m[cur ^ 1] = frag(rowp(kh1) + PL, 16 * ks1 + frow + kw1, cb);
                    b_h[cur ^ 1] = frag(rowp(kh1), 16 * ks1 + frow + kw1, cb);
                }
                f32x16 c = acc[t];
                c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a_m[ks]), __builtin_bit_cast(f16x8, b_h[cur]), c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a_h[ks]), __builtin_bit_cast(f16x8, b_m[cur]), c, 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a_h[ks]), __builtin_bit_cast(f16x8, b_h[cur]), c, 0, 0, 0);
                if (i == 8) __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);                                 // reads first ...
                else if (i + 1 < 18) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                            // ... then the MFMAs
                __builtin_amdgcn_sched_barrier(0);
            }
        } else      // three bf16 planes: read, wait, multiply per product
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pa = 16 * ks + frow, ca = wa * 32 + fcol;
            const bf16x8 ah = frag(ab, pa, ca), am = frag(ab + PL, pa, ca), al = frag(ab + (NPL - 1) * PL, pa, ca);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const bf16_t* row = planes + 2 * 32 * 64 + ((r - 1 + kh + 4) & 3) * 34 * 64;      // input row r-1+kh
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int t = kh * 3 + kw, pb = pa + kw, cb = wb * 32 + fcol;
                    const bf16x8 bh = frag(row, pb, cb), bm = frag(row + PL, pb, cb);
                    f32x16 c = acc[t];
                    const bf16x8 bl = frag(row + (NPL - 1) * PL, pb, cb);
#if XV2_T0 == 0
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, c, 0, 0, 0);
#endif
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, c, 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);      // keep the fragment reads of later taps from piling up (144 + ~100 VGPRs)
                }
            }
        }
        if (more) {
            store_dy(buf ^ 1);
            store_x(r + 2);
        }
        __syncthreads();
    }
    // every wave writes its quadrant of the block's slab part[y][co][T][Ctot] (C layout of the 32x32 MFMA)
    const size_t rowlen = (size_t)9 * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
    const int l31 = lane & 31, hh = lane >> 5;
    float iX, iD;
    plane_scales<NPL, true>(p, first, iX, iD);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = co0 + wa * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            slab[(size_t)row * rowlen + (size_t)t * p.Ctot + cn0 + wb * 32 + l31] = NPL == 2 ? acc[t][r] * iX * iD : acc[t][r];
        }
}

// the same 64 x 64 tiling for bf16 storage (wgrad_alltaps_tr_kernel's big sibling): one bf16 plane, 16-byte loads and LDS
// stores of 8 channels, one MFMA per (tap, k-step).  Emulated first (every second row step's producer skipped: -16 ... -31 %).
__global__ void __launch_bounds__(256, 2) wgrad_alltaps64_tr_kernel(const WgradParams p) {
    __shared__ __attribute__((aligned(16))) bf16_t planes[W64_PL];      // 25.6 KB
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx, by;
    wgrad_block(p.xcd_order, bx, by);
    const int wa = wave >> 1, wb = wave & 1;
    const Strip s = alltaps_strip<64>(bx, by, p.tiles_n, p.ktiles, p.kt_per_split, p.OW, p.OH);
    const int co0 = s.co0, cn0 = s.cn0, n = s.n, ow0 = s.ow0, r0 = s.r0, r1 = s.r1;
    const bool first = cn0 < p.C0;
    const bf16_t* xsrc = reinterpret_cast<const bf16_t*>(first ? p.X0 : p.X1);
    const int ldx = first ? p.ldX0 : p.ldX1, xch = first ? cn0 : cn0 - p.C0;
    // loads: 8 lanes x 16 bytes per pixel; every thread one dY element and one X element (pixels 0..31), threads < 16 pixels 32, 33
    const int px = tid >> 3, c8 = tid & 7;
    const bf16_t* dy0 = reinterpret_cast<const bf16_t*>(p.DY) + ((size_t)n * p.OH * p.OW + ow0 + px) * p.ldDY + co0 + c8 * 8;
    const size_t dy_pitch = (size_t)p.OW * p.ldDY;
    const int iw = ow0 - 1 + px;
    const bf16_t* xa0 = xsrc + ((size_t)n * p.IH * p.IW + iw) * ldx + xch + c8 * 8;
    const size_t x_pitch = (size_t)p.IW * ldx;
    const bool xok = iw >= 0, x2 = tid < 16, x2ok = x2 && iw + 32 < p.IW;
    const i32x4 zero = {0, 0, 0, 0};
    i32x4 rd = zero, rx = zero, rx2 = zero;
    auto load_dy = [&](int r) { rd = *reinterpret_cast<const i32x4*>(dy0 + (size_t)r * dy_pitch); };
    auto load_x = [&](int ih) {
        rx = zero;
        rx2 = zero;
        if ((unsigned)ih < (unsigned)p.IH) {
            if (xok) rx = *reinterpret_cast<const i32x4*>(xa0 + (size_t)ih * x_pitch);
            if (x2ok) rx2 = *reinterpret_cast<const i32x4*>(xa0 + (size_t)ih * x_pitch + (size_t)32 * ldx);
        }
    };
    auto store_dy = [&](int buf) { *reinterpret_cast<i32x4*>(planes + buf * 32 * 64 + w64_off(px, c8 * 8)) = rd; };
    auto store_x = [&](int ih) {
        bf16_t* ring = planes + 2 * 32 * 64 + ((ih + 4) & 3) * 34 * 64;
        *reinterpret_cast<i32x4*>(ring + w64_off(px, c8 * 8)) = rx;
        if (x2) *reinterpret_cast<i32x4*>(ring + w64_off(px + 32, c8 * 8)) = rx2;
    };
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int frow = tr_row(lane), fcol = tr_col(lane);
    auto frag = [&](const bf16_t* base, int fp, int c) {
        return tr_frag(base + w64_off(fp, c), base + w64_off(fp + 4, c));
    };
    ring_prologue(r0, load_dy, load_x, store_dy, store_x);
    for (int r = r0; r < r1; ++r) {
        const int buf = (r - r0) & 1;
        const bool more = r + 1 < r1;
        if (more) {
            load_dy(r + 1);
            load_x(r + 2);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pa = 16 * ks + frow;
            const bf16x8 af = frag(planes + buf * 32 * 64, pa, wa * 32 + fcol);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const bf16_t* row = planes + 2 * 32 * 64 + ((r - 1 + kh + 4) & 3) * 34 * 64;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const bf16x8 bf = frag(row, pa + kw, wb * 32 + fcol);
                    acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[kh * 3 + kw], 0, 0, 0);
                }
            }
        }
        if (more) {
            store_dy(buf ^ 1);
            store_x(r + 2);
        }
        __syncthreads();
    }
    const size_t rowlen = (size_t)9 * p.Ctot;
    float* slab = p.part + (size_t)by * p.Cout * rowlen;
    const int l31 = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = co0 + wa * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            slab[(size_t)row * rowlen + (size_t)t * p.Ctot + cn0 + wb * 32 + l31] = acc[t][r];
        }
}

}  // namespace xv2
