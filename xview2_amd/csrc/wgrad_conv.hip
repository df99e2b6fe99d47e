// Weight gradient of a convolution: planners, the kernel table and its launcher, the slab sum and the ABI entry points.  The
// kernels are in wgrad_kernel.h (its head maps the families).
//
//   dW[co][t][c] = sum_{m} dY[m][co] * X[pix(m, t)][c]        (m over N*OH*OW output pixels)
//
// The reduction over pixels is split across gridDim.y (and, for narrow tiles, across the waves of a block); every split
// writes its own slab part[split][Cout][T][Ctot] and a second kernel sums the slabs in a fixed order (deterministic, no
// atomics) while transposing into the reference's OIHW parameter layout.  Replaces the weight-gradient half of autograd for
// every nn.Conv2d / nn.ConvTranspose2d of model/layers.py and of the encoder blocks.
#include "wgrad_kernel.h"
#include <algorithm>

namespace xv2 {

// first stage of a two-level slab sum (many slabs, few elements): out2[g][i] = sum over the g-th group of slabs
__global__ void wgrad_reduce_stage1_kernel(const float* __restrict__ part, int nslab, int per, size_t total,
                                           float* __restrict__ out2) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int z0 = blockIdx.y * per, z1 = min(z0 + per, nslab);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int z = z0;
    for (; z + 4 <= z1; z += 4) {
        s0 += part[(size_t)z * total + i];
        s1 += part[(size_t)(z + 1) * total + i];
        s2 += part[(size_t)(z + 2) * total + i];
        s3 += part[(size_t)(z + 3) * total + i];
    }
    for (; z < z1; ++z) s0 += part[(size_t)z * total + i];
    out2[(size_t)blockIdx.y * total + i] = (s0 + s1) + (s2 + s3);
}

// out_oihw[co][ci][t] = sum_z part[z][co][t][ci]   (ci < cin_real)
// T == 1: input and output orders coincide -> plain streaming sum.
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, int nslab, int Cout, int T, int Ctot,
                                    int cin_real, float* __restrict__ out) {
    const size_t total = (size_t)Cout * T * Ctot;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Ctot);
        const size_t q = i / Ctot;
        const int t = (int)(q % T);
        const int co = (int)(q / T);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;   // 4 independent chains: the slab loads overlap
        int z = 0;
        for (; z + 4 <= nslab; z += 4) {
            s0 += part[(size_t)z * total + i];
            s1 += part[(size_t)(z + 1) * total + i];
            s2 += part[(size_t)(z + 2) * total + i];
            s3 += part[(size_t)(z + 3) * total + i];
        }
        for (; z < nslab; ++z) s0 += part[(size_t)z * total + i];
        const float s = (s0 + s1) + (s2 + s3);
        if (ci < cin_real) out[((size_t)co * cin_real + ci) * T + t] = s;
    }
}
// T > 1: one block per (co, 64-channel chunk): coalesced 256-byte slab reads, LDS transpose to [ci][t], then one
// contiguous 64*T-float store into the OIHW row.
__global__ void __launch_bounds__(256) wgrad_reduce_t_kernel(const float* __restrict__ part, int nslab, int Cout, int T,
                                                              int Ctot, int cin_real, float* __restrict__ out) {
    __shared__ float sh[64 * 52];
    const int chunks = Ctot / 64;
    const int co = blockIdx.x / chunks, ci0 = (blockIdx.x % chunks) * 64;
    const size_t total = (size_t)Cout * T * Ctot;
    const size_t base = ((size_t)co * T) * Ctot + ci0;
    const int n = T * 64;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int t = e >> 6, c = e & 63;
        const float* p = part + base + (size_t)t * Ctot + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int z = 0;
        for (; z + 4 <= nslab; z += 4) {
            s0 += p[(size_t)z * total];
            s1 += p[(size_t)(z + 1) * total];
            s2 += p[(size_t)(z + 2) * total];
            s3 += p[(size_t)(z + 3) * total];
        }
        for (; z < nslab; ++z) s0 += p[(size_t)z * total];
        sh[c * T + t] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    const int valid = min(64, cin_real - ci0);
    float* o = out + ((size_t)co * cin_real + ci0) * T;
    for (int e = threadIdx.x; e < valid * T; e += 256) o[e] = sh[e];
}

// stem_conv.hip
int stem7x7_wgrad_slabs(const xv2_conv_desc* d);
int stem7x7_wgrad_launch(const xv2_conv_desc* d, const float* x, const float* dy, int lddy, float* part, hipStream_t stream);

struct WgradPlan {
    int bm, bn, wk, splitk, kt_per, ktiles, tiles;
    bool smallc;
    bool stem7;        // stem_conv.hip: the 7x7 / stride-2 RGB stem from an LDS-resident input patch
    bool alltaps;      // the all-taps kernels: ktiles = row chunks per strip, kt_per = rows per chunk
    int nslab;         // partial slabs the MFMA kernel writes
    int groups;        // > 0: two-level slab sum with this many intermediate slabs
};

// The fitted constants of the planners, and where each was measured.
static constexpr struct {
    // all-taps cost model: time of one row step with the CU full, in the model's units.  Exact fp32 2.4 us and bf16 0.8 us: measured
    // on the decoder layers, isolated kernels.  The split-product and the 64 x 64 values: re-fitted on the WHOLE step (round 5,
    // scripts/ab_multi.sh, 12-point grid: a plateau at 64 x 64: 0.2 - 0.5, 32 x 32: 0.6 - 1.5 against the isolated-kernel values
    // 5.2 / 2.25 of round 3, cfg2 fp32 21.18 -> 20.71 ms.  The model prices a launch alone on the chip; on the side stream, next
    // to the compute stream's HBM-bound BatchNorm passes, what a plan costs is its slab traffic and the CUs it holds - fewer,
    // fatter blocks and fewer row chunks win.  bf16 storage likewise: 64 x 64 constant 1.144 -> 0.3, cfg2 --precision 16
    // 13.09 -> 12.72 ms, cfg3 16.45 -> 15.9 ms, three same-box pairs)
    double trow32_f32 = 2.4, trow32_bf16 = 0.8, trow32_x3 = 1.0, trow64_x3 = 0.4, trow64_bf16hbm = 0.3;
    // all-taps resident blocks per chip (256 CUs): 2 per CU in fp32 (144 accumulator VGPRs) and for the 64 x 64 tiles, 4 per CU
    // for the bf16 kernels (80 VGPRs), 3 per CU for the split-product ones (134 VGPRs, 38 KB of LDS)
    int cap32_f32 = 512, cap32_bf16 = 1024, cap32_x3 = 768, cap64 = 512;
    // cost of one slab (written by the kernel, re-read by the slab sum) per MB, small slabs sum in parallel: min of the two lines;
    // fitted on dec3 / l4 (bf16)
    double slab_us0 = 0.02, slab_us_mb0 = 0.7, slab_us1 = 1.0, slab_us_mb1 = 0.15;
    // per-tap split search: resident blocks per CU - LDS-limited: 2 for the 128 x 128 tile, 4 otherwise; the split-product and
    // bf16-storage 64 x 64 kernels measured best when planned for 2 as well (1x1 @256^2 layers 0.063 -> 0.054 ms and
    // 0.039 -> 0.031 ms)
    int pertap_per_cu_big = 2, pertap_per_cu = 4;
} WGRAD_FIT{};

static bool plan_stem7(const xv2_conv_desc* d, WgradPlan& pl) {
    const int slabs = stem7x7_wgrad_slabs(d);
    if (!slabs) return false;
    pl.stem7 = true;
    pl.bm = pl.bn = 64;
    pl.wk = pl.splitk = pl.kt_per = pl.ktiles = pl.tiles = 1;
    pl.nslab = slabs;
    if (pl.nslab >= 64) pl.groups = 16;
    return true;
}

// 3x3 / stride 1 / pad 1 on 32-channel multiples with OW % 32 == 0: the all-taps kernels, tile and row chunks by cost model
static bool plan_alltaps(const xv2_conv_desc* d, bool x3, WgradPlan& pl) {
    const int Ctot = d->C0 + d->C1;
    if (pl.smallc || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->dil != 1 || d->OW % 32 != 0 ||
        d->OH != d->IH || d->OW != d->IW || d->Cout % 32 != 0 || d->C0 % 32 != 0 || d->C1 % 32 != 0 || d->C0 <= 0)
        return false;
    pl.alltaps = true;
    pl.wk = 1;
    // split-bf16 / bf16 storage: 64 x 64 tiles (wgrad_alltaps64_*_kernel: half the producer work per FLOP) where the channel
    // counts allow AND the cost model prefers them - layers with few tiles (ResNeSt's grouped 3x3 layers at 64^2 / 32^2) cannot
    // fill the chip with a quarter of the blocks
    const bool can64 = (x3 || d->math == XV2_MATH_BF16_STORE) && d->Cout % 64 == 0 && d->C0 % 64 == 0 && d->C1 % 64 == 0;
    const int strips = d->N * (d->OW / 32);
    const double slab_mb = 1e-6 * (double)d->Cout * 9.0 * Ctot * 4.0;
    const double slab_us = std::min(WGRAD_FIT.slab_us0 + WGRAD_FIT.slab_us_mb0 * slab_mb, WGRAD_FIT.slab_us1 + WGRAD_FIT.slab_us_mb1 * slab_mb);
    const int maxchunks = std::max(1, d->OH / 8);
    // row chunks per strip: the count that minimises (rounds of resident blocks) x (rows per chunk) x (time of one
    // row step with the CU full) + (slabs written by the kernel and re-read by the slab sum)
    auto plan_tiles = [&](bool t64, int& chunks_out) {
        const int tiles = t64 ? (d->Cout / 64) * (Ctot / 64) : (d->Cout / 32) * (Ctot / 32);
        const int cap = t64 ? WGRAD_FIT.cap64 : x3 ? WGRAD_FIT.cap32_x3 : d->math ? WGRAD_FIT.cap32_bf16 : WGRAD_FIT.cap32_f32;
        const double t_row = t64 ? (x3 ? WGRAD_FIT.trow64_x3 : WGRAD_FIT.trow64_bf16hbm)
                                 : x3 ? WGRAD_FIT.trow32_x3 : d->math ? WGRAD_FIT.trow32_bf16 : WGRAD_FIT.trow32_f32;
        double best_cost = 0.0;
        chunks_out = 1;
        for (int c = 1; c <= maxchunks && c <= 64; ++c) {
            const int rows = (int)cdiv(d->OH, c);
            if ((int)cdiv(d->OH, rows) != c) continue;
            const int64_t blocks = (int64_t)tiles * strips * c;
            const int nslab = strips * c;
            const double cost = (double)cdiv(blocks, cap) * rows * t_row + (nslab + (nslab >= 64 ? 16 : 0)) * slab_us;
            if (c == 1 || cost < best_cost) {
                best_cost = cost;
                chunks_out = c;
            }
        }
        return best_cost;
    };
    int chunks = 1, chunks64 = 1;
    const double cost32 = plan_tiles(false, chunks);
    bool t64 = false;
    if (can64 && plan_tiles(true, chunks64) < cost32) {
        t64 = true;
        chunks = chunks64;
    }
    pl.bm = pl.bn = t64 ? 64 : 32;
    pl.tiles = t64 ? (d->Cout / 64) * (Ctot / 64) : (d->Cout / 32) * (Ctot / 32);
    pl.kt_per = (int)cdiv(d->OH, chunks);
    pl.ktiles = (int)cdiv(d->OH, pl.kt_per);
    pl.splitk = strips * pl.ktiles;
    pl.nslab = pl.splitk;
    if (pl.nslab >= 64) pl.groups = 16;
    return true;
}

// every other layer: one tap per block, the largest tile the channel counts allow, the pixel reduction split to fill the chip
static void plan_per_tap(const xv2_conv_desc* d, bool x3, WgradPlan& pl) {
    const int Ctot = d->C0 + d->C1, T = d->KH * d->KW;
    int bm = (d->Cout % 128 == 0) ? 128 : (d->Cout % 64 == 0 ? 64 : 32);
    int bn;
    if (pl.smallc) {
        bn = 64;
        if (bm == 128) bm = 64;
        pl.tiles = (d->Cout / bm) * (int)cdiv(T * 4, bn);
    } else {
        auto fit = [&](int v) { return d->C0 % v == 0 && d->C1 % v == 0; };
        bn = fit(128) ? 128 : (fit(64) ? 64 : 32);
        if (bm == 128 && bn != 128) bm = 64;
        if (bn == 128 && bm != 128) bn = 64;
        pl.tiles = (d->Cout / bm) * (Ctot / bn) * T;
    }
    pl.bm = bm;
    pl.bn = bn;
    pl.wk = tile_wk(bm, bn);
    const int64_t M = (int64_t)d->N * d->OH * d->OW;
    pl.ktiles = (int)cdiv(M, 32);
    // split the pixel reduction so that the grid fills the chip in whole "rounds" of resident blocks; among the split factors
    // that keep >= 8 K-tiles per block take the smallest one whose last round is >= 90 % full (fewer slabs = less reduce traffic)
    const int cap = 256 * ((bm == 128 || x3 || d->math == XV2_MATH_BF16_STORE) ? WGRAD_FIT.pertap_per_cu_big : WGRAD_FIT.pertap_per_cu);
    const int maxsplit = std::max(1, pl.ktiles / 8);
    int best = 1;
    double best_eff = 0.0;
    for (int sk = 1; sk <= maxsplit && sk <= 256; ++sk) {
        const int64_t blocks = (int64_t)pl.tiles * sk;
        const double eff = (double)blocks / (double)(cdiv(blocks, cap) * cap);
        if (eff > best_eff + 1e-9) {
            best_eff = eff;
            best = sk;
        }
        if (eff >= 0.9) {
            best = sk;
            break;
        }
    }
    pl.kt_per = (int)cdiv(pl.ktiles, best);
    pl.splitk = (int)cdiv(pl.ktiles, pl.kt_per);
    pl.nslab = pl.splitk * pl.wk;
}

// d->math: XV2_MATH_F32X3 already replaced by XV2_MATH_F32 and passed as x3
static WgradPlan make_plan(const xv2_conv_desc* d, bool x3) {
    WgradPlan pl;
    pl.smallc = (d->C0 == 4 && d->C1 == 0);
    pl.alltaps = false;
    pl.stem7 = false;
    pl.groups = 0;
    if (!plan_stem7(d, pl) && !plan_alltaps(d, x3, pl)) plan_per_tap(d, x3, pl);
    return pl;
}

// The kernels: one row per device kernel.  Every kernel takes (const WgradParams), 256 threads and the grid (pl.tiles, pl.splitk).
// name: what the row registers with the profiler (tests, scripts and the committed profiles key on it); lds: dynamic LDS bytes;
// ex / ed: bytes per X / dY element and x_in: X priced at input (else output) resolution - what prof_begin prices a launch with.
typedef void (*WgradKernel)(const WgradParams);
struct WgradRow {
    WgradKernel kernel;
    const char* name;
    WForm form;
    int bm, bn;
    unsigned lds;
    int ex, ed;
    bool x_in;
};
constexpr bool X_IN = true, X_OUT = false;
constexpr unsigned tiled_lds(int bm, int bn) { return 2u * 32 * (bm + bn) * 4; }                   // two stages of fp32 [32][BM], [32][BN]
constexpr unsigned tr_lds(int planes, int bm, int bn) { return planes * 32u * (bm + 32 + bn + 32) * 2; }      // bf16 rows of BM + 32, BN + 32
#define XV2_WGRAD_ROW(NAME, FORM, BM, BN, LDS, EX, ED, XRES, ...) {__VA_ARGS__, NAME, WForm::FORM, BM, BN, LDS, EX, ED, XRES},
static const WgradRow WGRAD_ROWS[] = {
    XV2_WGRAD_ROW("wgrad_kernel<64,64,2,2,1,rgb,bf16hbm>", RGB_BF16HBM, 64, 64, tiled_lds(64, 64), 4, 2, X_IN, wgrad_kernel<WForm::RGB_BF16HBM, 64, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<32,64,1,2,2,rgb,bf16hbm>", RGB_BF16HBM, 32, 64, tiled_lds(32, 64), 4, 2, X_IN, wgrad_kernel<WForm::RGB_BF16HBM, 32, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<64,64,2,2,1,rgb>", RGB, 64, 64, tiled_lds(64, 64), 4, 4, X_IN, wgrad_kernel<WForm::RGB, 64, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<32,64,1,2,2,rgb>", RGB, 32, 64, tiled_lds(32, 64), 4, 4, X_IN, wgrad_kernel<WForm::RGB, 32, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<128,128,2,2,1,c32,bf16,bf16hbm>", BF16_BF16HBM, 128, 128, tiled_lds(128, 128), 2, 2, X_IN, wgrad_kernel<WForm::BF16_BF16HBM, 128, 128>)
    XV2_WGRAD_ROW("wgrad_kernel<64,64,2,2,1,c32,bf16,bf16hbm>", BF16_BF16HBM, 64, 64, tiled_lds(64, 64), 2, 2, X_IN, wgrad_kernel<WForm::BF16_BF16HBM, 64, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<64,32,2,1,2,c32,bf16,bf16hbm>", BF16_BF16HBM, 64, 32, tiled_lds(64, 32), 2, 2, X_IN, wgrad_kernel<WForm::BF16_BF16HBM, 64, 32>)
    XV2_WGRAD_ROW("wgrad_kernel<32,64,1,2,2,c32,bf16,bf16hbm>", BF16_BF16HBM, 32, 64, tiled_lds(32, 64), 2, 2, X_IN, wgrad_kernel<WForm::BF16_BF16HBM, 32, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<32,32,1,1,4,c32,bf16hbm>", C32_BF16HBM, 32, 32, tiled_lds(32, 32), 2, 2, X_IN, wgrad_kernel<WForm::C32_BF16HBM, 32, 32>)
    XV2_WGRAD_ROW("wgrad_kernel<128,128,2,2,1,c32,bf16>", BF16, 128, 128, tiled_lds(128, 128), 4, 4, X_IN, wgrad_kernel<WForm::BF16, 128, 128>)
    XV2_WGRAD_ROW("wgrad_kernel<64,64,2,2,1,c32,bf16>", BF16, 64, 64, tiled_lds(64, 64), 4, 4, X_IN, wgrad_kernel<WForm::BF16, 64, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<64,32,2,1,2,c32,bf16>", BF16, 64, 32, tiled_lds(64, 32), 4, 4, X_IN, wgrad_kernel<WForm::BF16, 64, 32>)
    XV2_WGRAD_ROW("wgrad_kernel<32,64,1,2,2,c32,bf16>", BF16, 32, 64, tiled_lds(32, 64), 4, 4, X_IN, wgrad_kernel<WForm::BF16, 32, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<128,128,2,2,1,c32>", C32, 128, 128, tiled_lds(128, 128), 4, 4, X_IN, wgrad_kernel<WForm::C32, 128, 128>)
    XV2_WGRAD_ROW("wgrad_kernel<64,64,2,2,1,c32>", C32, 64, 64, tiled_lds(64, 64), 4, 4, X_IN, wgrad_kernel<WForm::C32, 64, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<64,32,2,1,2,c32>", C32, 64, 32, tiled_lds(64, 32), 4, 4, X_IN, wgrad_kernel<WForm::C32, 64, 32>)
    XV2_WGRAD_ROW("wgrad_kernel<32,64,1,2,2,c32>", C32, 32, 64, tiled_lds(32, 64), 4, 4, X_IN, wgrad_kernel<WForm::C32, 32, 64>)
    XV2_WGRAD_ROW("wgrad_kernel<32,32,1,1,4,c32>", C32, 32, 32, tiled_lds(32, 32), 4, 4, X_IN, wgrad_kernel<WForm::C32, 32, 32>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<128,128,f32x3>", TR_F32X3, 128, 128, tr_lds(3, 128, 128), 4, 4, X_IN, wgrad_tr_x3_kernel<128, 128, 3>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<64,64,f32x3>", TR_F32X3, 64, 64, tr_lds(3, 64, 64), 4, 4, X_IN, wgrad_tr_x3_kernel<64, 64, 3>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<128,128,f16x2>", TR_F16X2, 128, 128, tr_lds(2, 128, 128), 4, 4, X_IN, wgrad_tr_x3_kernel<128, 128, 2>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<64,64,f16x2>", TR_F16X2, 64, 64, tr_lds(2, 64, 64), 4, 4, X_IN, wgrad_tr_x3_kernel<64, 64, 2>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<128,128,bf16hbm>", TR_BF16HBM, 128, 128, tr_lds(2, 128, 128), 2, 2, X_IN, wgrad_tr_kernel<128, 128>)
    XV2_WGRAD_ROW("wgrad_tr_kernel<64,64,bf16hbm>", TR_BF16HBM, 64, 64, tr_lds(2, 64, 64), 2, 2, X_IN, wgrad_tr_kernel<64, 64>)
    XV2_WGRAD_ROW("wgrad_alltaps_kernel", ALLTAPS_C32, 32, 32, 0, 4, 4, X_OUT, wgrad_alltaps_kernel<false>)
    XV2_WGRAD_ROW("wgrad_alltaps_kernel<bf16>", ALLTAPS_BF16, 32, 32, 0, 4, 4, X_OUT, wgrad_alltaps_kernel<true>)
    XV2_WGRAD_ROW("wgrad_alltaps_kernel<bf16hbm>", ALLTAPS_BF16HBM, 32, 32, 0, 2, 2, X_OUT, wgrad_alltaps_tr_kernel)
    XV2_WGRAD_ROW("wgrad_alltaps_kernel<f32x3>", ALLTAPS_F32X3, 32, 32, 0, 4, 4, X_OUT, wgrad_alltaps_x3_kernel<3>)
    XV2_WGRAD_ROW("wgrad_alltaps_kernel<f16x2>", ALLTAPS_F16X2, 32, 32, 0, 4, 4, X_OUT, wgrad_alltaps_x3_kernel<2>)
    XV2_WGRAD_ROW("wgrad_alltaps64_kernel<bf16hbm>", ALLTAPS_BF16HBM, 64, 64, 0, 2, 2, X_OUT, wgrad_alltaps64_tr_kernel)
    XV2_WGRAD_ROW("wgrad_alltaps64_kernel<f32x3>", ALLTAPS_F32X3, 64, 64, 3 * W64_PL * 2, 4, 4, X_OUT, wgrad_alltaps64_x3_kernel<3>)
    XV2_WGRAD_ROW("wgrad_alltaps64_kernel<f16x2>", ALLTAPS_F16X2, 64, 64, 2 * W64_PL * 2, 4, 4, X_OUT, wgrad_alltaps64_x3_kernel<2>)
};
#undef XV2_WGRAD_ROW
constexpr int WGRAD_NROWS = sizeof(WGRAD_ROWS) / sizeof(WGRAD_ROWS[0]);

static const WgradRow* find_row(WForm form, int bm, int bn) {
    for (const WgradRow& r : WGRAD_ROWS)
        if (r.form == form && r.bm == bm && r.bn == bn) return &r;
    return nullptr;      // no kernel for the plan: an error, never another kernel
}

// The row of a plan (not the stem's).  d->math: XV2_MATH_F32X3 already replaced by XV2_MATH_F32 and passed as x3; fast: p.fast;
// h2: x3 with every operand maximum known (F16X2: two scaled fp16 planes, three MFMAs per product).
static const WgradRow* pick_row(const xv2_conv_desc* d, const WgradPlan& pl, bool fast, bool h2, bool x3) {
    const bool hs = d->math == XV2_MATH_BF16_STORE;
    const bool tr_tile = pl.wk == 1 && (pl.bm == 128 || (pl.bm == 64 && pl.bn == 64));      // the transpose-read kernels' tiles
    WForm form;
    if (pl.alltaps) form = h2 ? WForm::ALLTAPS_F16X2 : x3 ? WForm::ALLTAPS_F32X3 : hs ? WForm::ALLTAPS_BF16HBM : d->math ? WForm::ALLTAPS_BF16 : WForm::ALLTAPS_C32;
    else if (pl.smallc) form = hs ? WForm::RGB_BF16HBM : WForm::RGB;
    else if (x3 && fast && tr_tile) form = h2 ? WForm::TR_F16X2 : WForm::TR_F32X3;
    else if (hs && fast && tr_tile) form = WForm::TR_BF16HBM;
    else if (hs) form = (pl.bm == 32 && pl.bn == 32) ? WForm::C32_BF16HBM : WForm::BF16_BF16HBM;
    else if (d->math == XV2_MATH_BF16 && !(pl.bm == 32 && pl.bn == 32)) form = WForm::BF16;
    else form = WForm::C32;      // exact fp32 MFMA: XV2_MATH_F32, the per-tap layers of XV2_MATH_F32X3 off the fast path, 32 x 32 tiles
    return find_row(form, pl.bm, pl.bn);
}

static int launch_row(const WgradRow& row, const WgradParams& p, const WgradPlan& pl, hipStream_t stream) {
    struct Once {
        int kid[WGRAD_NROWS];
        hipError_t attr_rc;
    };
    static const Once once = [] {      // thread-safe one-time registration (function-local static)
        Once o;
        o.attr_rc = hipSuccess;
        for (int i = 0; i < WGRAD_NROWS; ++i) {
            o.kid[i] = prof_register(WGRAD_ROWS[i].name);
            if (WGRAD_ROWS[i].lds <= 48 * 1024) continue;      // more dynamic LDS than a launch gets by default
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(WGRAD_ROWS[i].kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)WGRAD_ROWS[i].lds);
            if (e != hipSuccess) o.attr_rc = e;
        }
        return o;
    }();
    XV2_CHECK_HIP(once.attr_rc);
    const double creal = wform_rgb(row.form) ? 3.0 : (double)p.Ctot;
    const double xpix = row.x_in ? (double)p.M / (p.OH * p.OW) * p.IH * p.IW : (double)p.M;
    prof_begin(once.kid[&row - WGRAD_ROWS], 2.0 * (double)p.M * p.Cout * p.T * creal,
               row.ex * xpix * creal + row.ed * (double)p.M * p.Cout + 4.0 * (double)p.Cout * p.T * creal, stream);
    hipLaunchKernelGGL(row.kernel, dim3(pl.tiles, pl.splitk), dim3(256), row.lds, stream, p);
    prof_end(stream);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

static int wgrad_impl(const xv2_conv_desc* d_in, const float* x0, int ldx0, const float* x1, int ldx1,
                      const float* dy, int lddy, float* dw_oihw, int cin_real, float* workspace,
                      hipStream_t stream) {
    AmaxGuard amax_guard;
    xv2_conv_desc dcopy = *d_in;            // XV2_MATH_F32X3: the all-taps and transpose-read kernels have split-product forms; the
    const bool x3 = dcopy.math == XV2_MATH_F32X3;      // other weight-gradient kernels run the exact fp32 MFMA
    if (x3) dcopy.math = XV2_MATH_F32;
    const xv2_conv_desc* d = &dcopy;
    XV2_CHECK_ARG(d->KH * d->KW <= 52, "too many taps");
    XV2_CHECK_ARG(d->Cout % 32 == 0, "backward_weight: Cout=%d must be a multiple of 32", d->Cout);
    const WgradPlan pl = make_plan(d, x3);
    const bool hs = d->math == XV2_MATH_BF16_STORE;
    XV2_CHECK_ARG(pl.smallc || (d->C0 % 32 == 0 && d->C1 % 32 == 0 && d->C0 > 0),
                  "backward_weight: C0=%d C1=%d must be multiples of 32", d->C0, d->C1);
    WgradParams p;
    p.X0 = x0; p.X1 = x1; p.DY = dy; p.part = workspace;
    p.amaxX0 = amax_ctx().a0; p.amaxX1 = amax_ctx().a1; p.amaxDY = amax_ctx().dy;
    static const int f16x2_on = [] { const char* e = getenv("XV2_F16X2"); return (e ? atoi(e) : 7) & 4; }();
    // F16X2: all operand maxima known (xv2_amax_ctx) - two scaled fp16 planes, three MFMAs per product
    const bool h2 = x3 && f16x2_on && p.amaxX0 && p.amaxDY && (!x1 || p.amaxX1);
    p.C0 = d->C0; p.C1 = d->C1; p.Ctot = d->C0 + d->C1; p.ldX0 = ldx0; p.ldX1 = ldx1; p.ldDY = lddy;
    p.Cout = d->Cout;
    p.IH = d->IH; p.IW = d->IW; p.OH = d->OH; p.OW = d->OW; p.stride = d->stride;
    p.M = d->N * d->OH * d->OW;
    p.T = d->KH * d->KW;
    p.ktiles = pl.ktiles; p.kt_per_split = pl.kt_per;
    p.xcd_order = 1;
    p.tiles_n = pl.smallc ? (int)cdiv(p.T * 4, pl.bn) : p.Ctot / pl.bn;
    const size_t total = (size_t)d->Cout * p.T * p.Ctot;
    {
        const long long ed = hs ? 2 : 4, ex = (hs && !pl.smallc) ? 2 : 4;
        const long long bx0 = (long long)d->N * d->IH * d->IW * ldx0 * ex;
        const long long bx1 = x1 ? (long long)d->N * d->IH * d->IW * ldx1 * ex : 0;
        const long long bdy = (long long)p.M * lddy * ed;
        p.fast = (d->OW % 32 == 0 && bx0 < (1ll << 31) && bx1 < (1ll << 31) && bdy < (1ll << 31)) ? 1 : 0;
        p.bytesX0 = (unsigned)std::min<long long>(bx0, 0x7fffffffll);
        p.bytesX1 = (unsigned)std::min<long long>(bx1, 0x7fffffffll);
        p.bytesDY = (unsigned)std::min<long long>(bdy, 0x7fffffffll);
    }
    for (int kh = 0; kh < d->KH; ++kh)
        for (int kw = 0; kw < d->KW; ++kw) {
            p.taps[kh * d->KW + kw].dh = (short)(kh * d->dil - d->pad);
            p.taps[kh * d->KW + kw].dw = (short)(kw * d->dil - d->pad);
        }
    int rc;
    if (pl.stem7) {
        rc = stem7x7_wgrad_launch(d, x0, dy, lddy, workspace, stream);
    } else {
        const WgradRow* row = pick_row(d, pl, p.fast != 0, h2, x3);
        XV2_CHECK_ARG(row, "backward_weight: no kernel for a %d x %d tile in this math mode", pl.bm, pl.bn);
        rc = launch_row(*row, p, pl, stream);
    }
    if (rc) return rc;
    const float* slabs = workspace;
    int nslab = pl.nslab;
    if (pl.groups > 0) {
        float* out2 = workspace + (size_t)pl.nslab * total;
        const int per = (int)cdiv(pl.nslab, pl.groups);
        const int groups = (int)cdiv(pl.nslab, per);
        hipLaunchKernelGGL(wgrad_reduce_stage1_kernel, dim3((unsigned)cdiv(total, 256), groups), dim3(256), 0, stream,
                           workspace, pl.nslab, per, total, out2);
        slabs = out2;
        nslab = groups;
    }
    if (p.T > 1 && p.Ctot % 64 == 0) {
        hipLaunchKernelGGL(wgrad_reduce_t_kernel, dim3(d->Cout * (p.Ctot / 64)), dim3(256), 0, stream, slabs,
                           nslab, d->Cout, p.T, p.Ctot, cin_real, dw_oihw);
    } else {
        const int grid = (int)std::min<size_t>(cdiv(total, 256), 4096);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid), dim3(256), 0, stream, slabs, nslab,
                           d->Cout, p.T, p.Ctot, cin_real, dw_oihw);
    }
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_conv2d_backward_weight_workspace(const xv2_conv_desc* d_in) {
    xv2_conv_desc dcopy = *d_in;
    if (dcopy.math == XV2_MATH_F32X3) dcopy.math = XV2_MATH_F32;
    const xv2_conv_desc* d = &dcopy;
    const WgradPlan pl = make_plan(d, d_in->math == XV2_MATH_F32X3);
    return (size_t)(pl.nslab + pl.groups) * d->Cout * d->KH * d->KW * (d->C0 + d->C1) * sizeof(float);
}

extern "C" int xv2_conv2d_backward_weight(const xv2_conv_desc* d, const void* x0, int ldx0,
                                          const void* x1, int ldx1, const void* dy, int lddy,
                                          float* dw_oihw, int cin_real, float* workspace, void* stream) {
    return wgrad_impl(d, (const float*)x0, ldx0, (const float*)x1, ldx1, (const float*)dy, lddy, dw_oihw, cin_real, workspace,
                      (hipStream_t)stream);
}

// The same launch on a SIDE stream, ordered behind everything enqueued so far on the caller's stream (the weight gradient
// is only needed by the optimizer / the gradient all-reduce, so it may overlap the rest of the backward pass): event
// record on `stream`, wait on `side_stream`, launch there.  One call instead of the binding's event / stream-switch
// sequence (~20 us of host time per layer in Python).  The caller joins `side_stream` before it reads dw.
extern "C" int xv2_conv2d_backward_weight_async(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                                                const void* dy, int lddy, float* dw_oihw, int cin_real, float* workspace,
                                                void* side_stream, void* stream) {
    XV2_CHECK_ARG(side_stream && side_stream != stream, "backward_weight_async: a distinct side stream is required");
    // one event per (host thread, device): an event belongs to the device that was current when it was created, and a host
    // thread may drive streams of several devices.  Re-recorded per call: a wait captures the record that precedes it.
    static thread_local hipEvent_t evs[64] = {};
    int dev = 0;
    XV2_CHECK_HIP(hipGetDevice(&dev));
    XV2_CHECK_ARG(dev >= 0 && dev < 64, "backward_weight_async: device index %d out of range", dev);
    hipEvent_t& ev = evs[dev];
    if (!ev) XV2_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    XV2_CHECK_HIP(hipEventRecord(ev, (hipStream_t)stream));
    XV2_CHECK_HIP(hipStreamWaitEvent((hipStream_t)side_stream, ev, 0));
    return wgrad_impl(d, (const float*)x0, ldx0, (const float*)x1, ldx1, (const float*)dy, lddy, dw_oihw, cin_real, workspace,
                      (hipStream_t)side_stream);
}

// conv_transpose: the equivalent conv `d` has input = the transposed conv's OUTPUT gradient (large
// tensor, C0 channels) and output-gradient = the transposed conv's INPUT x (Cout channels).
extern "C" int xv2_conv_transpose2d_backward_weight(const xv2_conv_desc* d, const void* x, int ldx,
                                                    const void* dy, int lddy, float* dw, float* workspace,
                                                    void* stream) {
    return wgrad_impl(d, (const float*)dy, lddy, nullptr, 0, (const float*)x, ldx, dw, d->C0, workspace, (hipStream_t)stream);
}
