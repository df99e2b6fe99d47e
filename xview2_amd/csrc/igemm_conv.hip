// Implicit-GEMM convolution, host side: tile / split-K planner, dispatch to the forms of igemm_kernel (igemm_kernel.h: the
// kernel, its forms and the split-K slab sum), preparation of the weight operand (pre-split planes, recorded maxima) and the
// ABI entry points of conv2d / conv_transpose2d forward and backward-data.
#include "igemm_kernel.h"
#include "amax_ctx.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <unordered_map>

namespace xv2 {

template <Form F, int BM, int BN>
constexpr size_t igemm_smem_bytes() {
    return (size_t)igemm_main_floats<F, BM, BN>() * 4 + BM * 4 + 4 * BN * 2 * 4;
}

template <Form F, int BM, int BN>
static int launch_one(const IgemmParams& p, hipStream_t stream) {
    constexpr bool SMALLC = form_traits(F).SMALLC, HS = form_traits(F).HS;
    constexpr size_t smem = igemm_smem_bytes<F, BM, BN>();
    auto kern = igemm_kernel<F, BM, BN>;
    // one-time setup per instantiation; C++11 guarantees the initialiser of a function-local static runs exactly once
    // even with concurrent callers (the library may be driven from several host threads, one stream each)
    static const hipError_t attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    XV2_CHECK_HIP(attr_rc);
    static const int kid = [] {
        char nm[96];
        snprintf(nm, sizeof(nm), "igemm_kernel<%d,%d,%d,%d,%s>", BM, BN, tile_wgm(BN), 4 / tile_wgm(BN), form_traits(F).suffix);
        return prof_register(nm);
    }();
    IgemmParams q = p;
    int maxtiles = 0;
    double flops = 0.0;
    for (int c = 0; c < q.ncls; ++c) {
        q.cls[c].mtiles = (int)cdiv(q.cls[c].M, BM);
        maxtiles = std::max(maxtiles, q.cls[c].mtiles);
        const double kreal = SMALLC ? (double)q.cls[c].ntaps * q.cin_real : (double)q.cls[c].ntaps * q.Ctot;
        flops += 2.0 * (double)q.cls[c].M * q.Nout * kreal;
    }
    const int grid = maxtiles * (q.Nout / BN);
    // algorithmic bytes: input pixels x channels + weights + output, each once
    const double ein = (HS && !SMALLC) ? 2.0 : 4.0, eout = HS ? 2.0 : 4.0;
    double abytes = ein * ((double)q.cls[0].M / std::max(1, q.cls[0].OHl * q.cls[0].OWl) * q.IH * q.IW *
                               (SMALLC ? q.cin_real : q.Ctot) + (double)q.Nout * q.T * (SMALLC ? q.cin_real : q.Ctot));
    for (int c = 0; c < q.ncls; ++c) abytes += eout * (double)q.cls[c].M * q.Nout;
    if (!HS && q.amax_out && q.amax_recorded) *q.amax_recorded = 1;      // (this kernel or, behind a slab launch, the slab sum records)
    prof_begin(kid, flops, abytes, stream);
    hipLaunchKernelGGL(kern, dim3(grid, q.ncls, q.ksplit), dim3(256), smem, stream, q);
    prof_end(stream);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// tile shape and split-K factor; `nkt` = K tiles of the (single-class) problem, 0 disables split-K
static void pick_tile(int64_t M, int Nout, bool smallc, int nkt, int math, int& bm, int& bn, int& ksplit) {
    bn = (Nout % 128 == 0) ? 128 : (Nout % 64 == 0 ? 64 : 32);
    ksplit = 1;
    if (smallc || bn == 32) {
        bm = 128;
        return;
    }
    if (const char* f = getenv("XV2_FORCE_TILE")) {      // tuning sweeps (scripts/sweep_tiles.py): "bm,bn,ksplit"
        int fbm = 0, fbn = 0, fks = 0;
        if (sscanf(f, "%d,%d,%d", &fbm, &fbn, &fks) == 3 && (fbm == 64 || fbm == 128) && (fbn == 64 || fbn == 128) &&
            Nout % fbn == 0 && fks >= 1) {
            bm = fbm;
            bn = fbn;
            if (fks > 1 && fbm == 128 && fbn == 128 && nkt / fks >= 2) ksplit = fks;
            return;
        }
    }
    // Cost model in "rounds": the chip holds `cap` blocks at once (LDS-limited: 2 per CU for the 128x128, 64x128 and
    // 128x64 tiles, 4 per CU for 64x64); a launch takes ceil(blocks / cap) rounds of (tile rows x K share) work.
    // Candidates: 128-row tile, 64-row tile (measured ~8 % less efficient per FLOP), and for bn == 128 the 128-row
    // tile with K split 2..8 ways (partials reduced by splitk_reduce_kernel, charged as extra traffic).
    const int ntn = Nout / bn;
    if (math == XV2_MATH_BF16_STORE) {
        // bf16 storage: the kernels are throughput-bound (LDS / MFMA issue) once a CU holds 3 blocks, so a launch takes
        // (blocks on the fullest CU) x (tile rows x K share), stretched for a last group of fewer than 3 blocks (latency
        // not hidden: 0.55 alone, 0.9 in pairs) and for the 64-row tiles (0.8 per FLOP).  scripts/sweep_tiles.py.
        auto cost = [&](int64_t blocks, double rows, double kshare, double eff) {
            const int64_t n = cdiv(blocks, 256);                 // blocks on the fullest CU, run three at a time
            const int r = (int)(n % 3);
            const double units = (double)(n - r) + (r == 1 ? 1.0 / 0.55 : r == 2 ? 2.0 / 0.9 : 0.0);
            return units * rows * kshare / eff;
        };
        const double kk = (double)std::max(nkt, 1);
        double best = cost(cdiv(M, 128) * ntn, 128.0, kk, 1.0);
        bm = 128;
        const double c64 = cost(cdiv(M, 64) * ntn, 64.0, kk, 0.8);
        if (c64 < best * 0.97) {
            best = c64;
            bm = 64;
        }
        if (bn == 128 && nkt >= 16) {
            // (+ 12 K-tiles' worth of work per split-K block for writing / re-reading its slab, as below)
            for (int ks = 2; ks <= 8 && nkt / ks >= 8; ++ks) {
                const double c = cost(cdiv(M, 128) * ntn * ks, 128.0, (double)cdiv(nkt, ks) + 12.0, 1.0);
                if (c < best * 0.95) {
                    best = c;
                    bm = 128;
                    ksplit = ks;
                }
            }
        }
        return;
    }
    auto rounds = [&](int64_t blocks, int cap) { return (double)cdiv(blocks, cap); };
    const int cap128 = 512, cap64 = (bn == 64) ? 1024 : 512;
    const double k = (double)std::max(nkt, 1);
    double best = rounds(cdiv(M, 128) * ntn, cap128) * 128.0 * k;
    bm = 128;
    // per-FLOP efficiency of the 64-row tiles relative to 128 x 128: 0.92 with the fp32 MFMA; 0.65 in the split-bf16 form
    // (6-12 MFMAs per stage and barrier; measured 143 vs 190 TFLOP/s on the 116-GFLOP decoder layers)
    // (64-channel outputs, round 3: 128 x 64 measured 5 % FASTER than 64 x 64 at equal rounds - dec4.c1 132 vs 126, l1.conv2 104
    //  vs 98 TFLOP/s - so there the 64-row tile only wins when it needs fewer rounds)
    const double eff64 = math == XV2_MATH_F32X3 ? (bn == 64 ? 0.48 : 0.65) : 0.92;
    const double c64 = rounds(cdiv(M, 64) * ntn, cap64) * 64.0 * k / eff64;
    if (c64 < best * 0.97) {
        best = c64;
        bm = 64;
    }
    if (bn == 128 && nkt >= 16) {
        const int64_t blocks128 = cdiv(M, 128) * ntn;
        for (int ks = 2; ks <= 8 && nkt / ks >= 8; ++ks) {
            const double per = (double)cdiv(nkt, ks);
            // + ~6 K-tiles worth of work per block for writing / re-reading the fp32 slab (3 measured against the
            // split-bf16 form's 64-row alternative on the short-K 1x1 layers)
            // (round 4, whole-step sweeps of this charge - profiles/r04_gated_ab.md: the isolated-kernel fit of 3 / 4 K-tiles
            //  left out what the slab-sum LAUNCH costs the step; 9 / 12 measured 1 - 1.5 % faster on cfg2 fp32, cfg2 p16 and cfg3)
            const double c = rounds(blocks128 * ks, cap128) * 128.0 * (per + (math == XV2_MATH_F32X3 ? 9.0 : 6.0));
            if (c < best * 0.95) {
                best = c;
                bm = 128;
                ksplit = ks;
            }
        }
    }
}

// (round 3 could sum the split-K slabs inside the GEMM launch - XV2_SPLITK_FOLD: measured slower than the 32-row slab-sum kernel
//  and removed in round 6 with the other in-launch hand-offs)
int64_t igemm_stats_tiles(int64_t M, int Nout, bool smallc, int nkt, int math) {
    int bm, bn, ks;
    pick_tile(M, Nout, smallc, nkt, math, bm, bn, ks);
    return ks > 1 ? cdiv(M, SPLITK_ROWS) : cdiv(M, bm);
}

int igemm_stats_tile_rows(int64_t M, int Nout, bool smallc, int nkt, int math) {
    int bm, bn, ks;
    pick_tile(M, Nout, smallc, nkt, math, bm, bn, ks);
    return ks > 1 ? SPLITK_ROWS : bm;
}

size_t igemm_splitk_bytes(int64_t M, int Nout, bool smallc, int nkt, int math) {
    int bm, bn, ks;
    pick_tile(M, Nout, smallc, nkt, math, bm, bn, ks);
    return ks > 1 ? (size_t)ks * M * Nout * sizeof(float) : 0;
}

// ---- weights pre-split into bf16 planes (the ..._WX3 / F16X2_HALO forms) ------------------------------------------------------
// x3 layout of a packed fp32 operand B [nrows][T][ctot]:  [nrows / 64][T][ctot / 16][3 planes][64 rows][16] bf16, the two
// 8-element halves of a row swapped on rows with bit 3 set (the LDS image of a weight stage, copied 1:1 by the DMA loads).
struct PresplitEntry {
    const void* x3;
    int nrows, T, ctot;
    const unsigned* amax = nullptr;      // F16X2 entries: the 64 maximum slots the two fp16 planes were scaled with
};
static std::mutex g_presplit_mu;
static std::unordered_map<const void*, PresplitEntry> g_presplit;
static std::unordered_map<const void*, PresplitEntry> g_presplit2;      // packed fp32 operand -> two scaled fp16 planes (F16X2)
static std::unordered_map<const void*, const unsigned*> g_wamax;        // packed fp32 operand -> the slots of its maximum (F16X2)

static bool f16x2_enabled(int bit = 1) {      // XV2_F16X2=0: every launch on the three-plane bf16 form
    // (bit mask for A/B runs: 1 = halo form, 2 = per-tap form; 4 = the weight-gradient kernels, wgrad_conv.hip; default all)
    static const int v = [] { const char* e = getenv("XV2_F16X2"); return e ? atoi(e) : 7; }();
    return (v & bit) != 0;
}

// max |x| of a tensor into 64 slots (zeroed by the caller): the weight operands' maxima, and the test harness
__global__ void __launch_bounds__(256) amax_kernel(const float* __restrict__ x, size_t n4, unsigned* __restrict__ slots) {
    __shared__ float red[4];
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        if (!(v.x == v.x && v.y == v.y && v.z == v.z && v.w == v.w)) m = __uint_as_float(0x7fc00000u);      // NaN stays loud
    }
    amax_record(slots, m, red);
}

// one block = one (64-row unit, 16-channel slice), all taps: 256 threads = 64 rows x 4 channel quads, so that every plane of
// a (tap, slice) is written as ONE contiguous 2 KB run (the first version wrote 32-byte pieces 6 KB apart: 210 us per cfg2
// step; one block per tap spent its time in the table search: 35 K blocks x 7 dependent loads, 110 us)
__device__ __forceinline__ void presplit_block(const float* __restrict__ src, __bf16* __restrict__ dst, int T, int ctot,
                                               int64_t blk) {
    const int nsl = ctot / 16;
    const int cs = (int)(blk % nsl), unit = (int)(blk / nsl);
    const int r = threadIdx.x >> 2, k0 = (threadIdx.x & 3) * 4;
    const int half = (k0 >> 3) ^ ((r >> 3) & 1);      // (rows r and r + 8 share a 256-byte bank window: ds_read_b128 lane groups, MI355X_MICROARCH)
    const float* sp = src + (size_t)(unit * 64 + r) * T * ctot + cs * 16 + k0;
    __bf16* dp = dst + ((size_t)unit * T * nsl + cs) * 3072 + r * 16 + half * 8 + (k0 & 7);
    if (T == 9) {        // (the only supported tap count) all nine taps in flight: one memory round trip per block, not three
        float4 v[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) v[u] = *reinterpret_cast<const float4*>(sp + (size_t)u * ctot);
#pragma unroll
        for (int u = 0; u < 9; ++u) {
            uint2 pk[3];
            split3x4(v[u], pk[0], pk[1], pk[2]);
            __bf16* d = dp + (size_t)u * nsl * 3072;
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(d + q * 1024) = pk[q];
        }
        return;
    }
    for (int t0 = 0; t0 < T; t0 += 3) {        // three taps in flight
        float4 v[3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (t0 + u < T) v[u] = *reinterpret_cast<const float4*>(sp + (size_t)(t0 + u) * ctot);
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (t0 + u < T) {
                uint2 pk[3];
                split3x4(v[u], pk[0], pk[1], pk[2]);
                __bf16* d = dp + (size_t)(t0 + u) * nsl * 3072;
#pragma unroll
                for (int q = 0; q < 3; ++q) *reinterpret_cast<uint2*>(d + q * 1024) = pk[q];
            }
    }
}
// the same image with TWO fp16 planes of w * s (F16X2; 2048 elements per (unit, tap, slice)), s from the operand's recorded maximum
// one block = one (64-row unit, 16-channel slice), all taps - as presplit_block; amax_only: record max |w| of the block instead
template <bool AMAX_ONLY>
__device__ __forceinline__ void presplit2h_block(const float* __restrict__ src, __bf16* __restrict__ dst, int T, int ctot,
                                                 int64_t blk, unsigned* __restrict__ amax) {
    __shared__ float red[4];
    const int nsl = ctot / 16;
    const int r = threadIdx.x >> 2, k0 = (threadIdx.x & 3) * 4;
    const int half = (k0 >> 3) ^ ((r >> 3) & 1);      // (rows r and r + 8 share a 256-byte bank window: ds_read_b128 lane groups, MI355X_MICROARCH)
    const int cs = (int)(blk % nsl), unit = (int)(blk / nsl);
    const float* sp = src + (size_t)(unit * 64 + r) * T * ctot + cs * 16 + k0;
    float s = 1.f, m = 0.f;
    if constexpr (!AMAX_ONLY) s = amax_scale(amax_exponent(amax));
    __bf16* dp = dst + ((size_t)unit * T * nsl + cs) * 2048 + r * 16 + half * 8 + (k0 & 7);
    for (int t0 = 0; t0 < T; t0 += 3) {
        float4 v[3];
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (t0 + u < T) v[u] = *reinterpret_cast<const float4*>(sp + (size_t)(t0 + u) * ctot);
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (t0 + u < T) {
                if constexpr (AMAX_ONLY) {
                    m = amax_acc(m, v[u]);
                } else {
                    uint2 pk[2];
                    split2hx4(v[u], s, pk[0], pk[1]);
                    __bf16* d = dp + (size_t)(t0 + u) * nsl * 2048;
                    *reinterpret_cast<uint2*>(d) = pk[0];
                    *reinterpret_cast<uint2*>(d + 1024) = pk[1];
                }
            }
    }
    if constexpr (AMAX_ONLY) amax_record(amax, m, red, (unsigned)blk);
}
__global__ void __launch_bounds__(256) presplit2h_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, int nrows,
                                                         int T, int ctot, unsigned* __restrict__ amax) {
    const int64_t nb = (int64_t)(nrows / 64) * (ctot / 16);
    for (int64_t blk = blockIdx.x; blk < nb; blk += gridDim.x) presplit2h_block<false>(src, dst, T, ctot, blk, amax);
}
// table[n][7]: {src, dst, nrows, T, ctot, first block, amax slots}
template <bool AMAX_ONLY>
__global__ void __launch_bounds__(256) presplit2h_table_kernel(const int64_t* __restrict__ table, int n) {
    int lo = 0, hi = n - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * 7 + 5] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* e = table + lo * 7;
    presplit2h_block<AMAX_ONLY>(reinterpret_cast<const float*>(e[0]), reinterpret_cast<__bf16*>(e[1]), (int)e[3], (int)e[4], blk - e[5],
                                reinterpret_cast<unsigned*>(e[6]));
}
__global__ void __launch_bounds__(256) presplit_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, int nrows,
                                                       int T, int ctot) {
    const int64_t nb = (int64_t)(nrows / 64) * (ctot / 16);
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) presplit_block(src, dst, T, ctot, b);
}
// table[n][6]: {src, dst, nrows, T, ctot, first block}; a block = one (unit, slice)
__global__ void __launch_bounds__(256) presplit_table_kernel(const int64_t* __restrict__ table, int n) {
    int lo = 0, hi = n - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * 6 + 5] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* e = table + lo * 6;
    presplit_block(reinterpret_cast<const float*>(e[0]), reinterpret_cast<__bf16*>(e[1]), (int)e[3], (int)e[4], blk - e[5]);
}
static bool presplit_lookup(const void* b, int nrows, int T, int ctot, const void** x3) {
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    auto it = g_presplit.find(b);
    if (it == g_presplit.end() || it->second.nrows != nrows || it->second.T != T || it->second.ctot != ctot) return false;
    *x3 = it->second.x3;
    return true;
}
// F16X2 for this launch: the operand maxima of both sides are known and the weights exist as two scaled fp16 planes
static bool f16x2_ready(IgemmParams& p) {
    if (!f16x2_enabled() || p.math != XV2_MATH_F32X3 || !p.amaxA0 || (p.A1 && !p.amaxA1)) return false;
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    auto it = g_presplit2.find(p.B);
    if (it == g_presplit2.end() || it->second.nrows != p.Nout || it->second.T != p.T || it->second.ctot != p.Ctot) return false;
    p.Bx3 = reinterpret_cast<const float*>(it->second.x3);
    p.bytesBx3 = (unsigned)((size_t)p.Nout * p.T * p.Ctot * 4);
    p.amaxB = it->second.amax;
    p.npl = 2;
    return true;
}
// ... of the per-tap form (both operands split in the kernel): the maxima of the sources and of the packed weights
bool f16x2_ready_pertap(IgemmParams& p) {
    if (!f16x2_enabled(2) || p.math != XV2_MATH_F32X3 || !p.amaxA0 || (p.A1 && !p.amaxA1)) return false;
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    auto it = g_wamax.find(p.B);
    if (it == g_wamax.end()) return false;
    p.amaxB = it->second;
    p.npl = 2;
    return true;
}

// the halo form of the F32X3 kernel (Form::F32X3_HALO...): 3x3 taps around the output pixel on a same-size input.
// First version measured 0.93 - 1.03x of the per-tap form; rocprofv3 PMC on it showed why (profiles/r03_pmc_halo.md): the
// effective clock DID rise (1.59 -> 1.87 GHz: the activation operand's loads, splits and plane stores drop 6.4x) but the
// matrix pipe's duty fell from 0.66 to 0.50 - the tap / slice counters, captured by reference in the iteration lambda,
// lived in scratch memory (3 extra VMEM round trips per stage) and the tap table was read with vector loads.  With both
// gone: dec2 / dec3 116-GFLOP layers 0.592 -> 0.547 / 0.605 -> 0.553 ms, dec4 0.565 -> 0.483, l1.conv2 0.093 -> 0.077.
// (Eight channels per thread with 16-byte plane stores - half the store instructions for the same bytes - measured 2-3 %
// slower than the 4-channel / 8-byte form.)
// halo form of the bf16-storage kernel (both operands global -> LDS by DMA, no register path): exact, and measured NOT
// faster than the per-tap form - cfg2 3x3 layers forward 550 -> 526, backward-data 598 -> 559 TFLOP/s (dec1 0.164 -> 0.203 ms,
// dec2 / dec3 equal, l4.conv2 0.029 -> 0.026): that kernel has no split and no conversion to save, its producer is already
// one 16-byte load + one 16-byte LDS store per 8 channels.  Default since the K loop is straight-line code (round 6:
// cfg2 --precision 16 12.06 -> 11.61 ms, cfg3 15.0 -> 14.4 ms, profiles/r06_halo_bf16_straight_line_ab.txt); XV2_HALO_BF16=0: per-tap form.
static bool halo_bf16_enabled() {
    static const int v = [] { const char* e = getenv("XV2_HALO_BF16"); return e ? atoi(e) : 1; }();
    return v != 0;
}
static bool halo_eligible(const IgemmParams& p, bool smallc, int math = XV2_MATH_F32X3) {
    if (math == XV2_MATH_BF16_STORE && !halo_bf16_enabled()) return false;
    if (smallc || p.math != math || p.ncls != 1 || p.s_in != 1 || p.Nout % 64 != 0) return false;
    const ClassInfo& c = p.cls[0];
    if (c.ntaps != 9 || c.tap0 != 0 || c.OHl != p.IH || c.OWl != p.IW || c.OHl % 4 != 0 || c.OWl % 32 != 0) return false;
    if (p.C0 % 32 != 0 || p.Ctot % 32 != 0 || c.nkt != 9 * (p.Ctot / BK)) return false;
    const int sgn = p.taps[0].dh < 0 ? 1 : -1;
    for (int t = 0; t < 9; ++t)       // slot order, (dh, dw) = sgn * (t / 3 - 1, t % 3 - 1): the kernel derives them
        if (p.taps[t].slot != t || p.taps[t].dh != sgn * (t / 3 - 1) || p.taps[t].dw != sgn * (t % 3 - 1)) return false;
    return true;
}

// the five tiles of a per-tap form for the (bm, bn) of pick_tile()
#define XV2_IGEMM_TILES(FORM)                                                                                                      \
    do {                                                                                                                           \
        if (bn == 128) return bm == 128 ? launch_one<Form::FORM, 128, 128>(p, stream) : launch_one<Form::FORM, 64, 128>(p, stream); \
        if (bn == 64) return bm == 128 ? launch_one<Form::FORM, 128, 64>(p, stream) : launch_one<Form::FORM, 64, 64>(p, stream);    \
        return launch_one<Form::FORM, 128, 32>(p, stream);                                                                         \
    } while (0)

int igemm_launch(IgemmParams& p, bool smallc, float* splitk_ws, hipStream_t stream) {
    XV2_CHECK_ARG(p.Nout % 32 == 0, "igemm: Nout=%d must be a multiple of 32", p.Nout);
    XV2_CHECK_ARG(p.ncls >= 1 && p.cls[0].M > 0, "igemm: empty problem");
    int bm, bn, ks;
    int64_t maxM = 0;
    for (int c = 0; c < p.ncls; ++c) maxM = std::max<int64_t>(maxM, p.cls[c].M);
    if (direct3x3_eligible(p, smallc)) return direct3x3_launch(p, stream);
    if (smallc && p.math == XV2_MATH_F32X3) p.math = XV2_MATH_F32; // RGB stem: exact fp32
    pick_tile(maxM * (p.ncls > 1 ? p.ncls : 1), p.Nout, smallc, (p.ncls == 1 && splitk_ws) ? p.cls[0].nkt : 0, p.math, bm, bn, ks);
    if (getenv("XV2_DEBUG_TILE"))
        fprintf(stderr, "igemm M=%lld N=%d nkt=%d ws=%d -> %dx%d ks=%d\n", (long long)maxM, p.Nout, p.cls[0].nkt,
                splitk_ws != nullptr, bm, bn, ks);
    if (!smallc && p.ncls == 1 && (p.math == XV2_MATH_F32X3 || p.math == XV2_MATH_BF16_STORE)) {
        // small grids (the /8 ... /32 encoder levels): sg_conv.hip instead of a 64-row / split-K plan of the tiled kernel.
        // Forward launches with statistics: the descriptor queries (xv2_conv2d_forward_stats_tiles / _tile_rows / _workspace)
        // already answered with sg_planned_rows() for this shape, so the partials have that geometry whichever kernel runs -
        // if the operands are not ready for it (no recorded maxima, no fp16 planes) the tiled kernel takes 64-row tiles, unsplit.
        const int planned = (p.stats && !p.A1 && p.C1 == 0) ? sg_planned_rows(maxM, p.Nout, p.Ctot, p.T, p.math) : 0;
        const int R = planned ? planned : ks > 1 ? SPLITK_ROWS : bm;
        IgemmParams q = p;
        if ((p.math == XV2_MATH_BF16_STORE || f16x2_ready(q)) && sg_conv_eligible(q, smallc, R)) {
            SgGroupCtx& gc = sg_group_ctx();
            if (gc.active && gc.w1) {      // a grouped layer: group 1 in the same grid when its operands are ready as well
                IgemmParams q1 = q;
                q1.B = static_cast<const float*>(gc.w1);
                if (p.math == XV2_MATH_BF16_STORE || f16x2_ready(q1)) {
                    gc.done = 1;
                    return sg_conv_launch(q, R, stream, &q1);
                }
            }
            return sg_conv_launch(q, R, stream);
        }
        if (planned) {
            XV2_CHECK_ARG(planned == 64, "igemm: the small-grid plan expects 64-row statistics tiles");
            bm = 64;
            ks = 1;
        }
    }
    p.ksplit = ks;
    p.part = splitk_ws;
    p.kt_per_split = (int)cdiv(p.cls[0].nkt, ks);
    const bool stem7 = ks == 1 && stem7x7_eligible(p, smallc);
    if (stem7 || (ks == 1 && (bm == 128 || !p.stats) && thin1x1_eligible(p, smallc))) {
        // HBM-bound 1x1 layers: the streaming kernel (thin_conv.hip), and the 7x7 RGB stem (stem_conv.hip); both write the
        // 128-row statistics partials of the BM = 128 plan
        return stem7 ? stem7x7_launch(p, stream) : thin1x1_launch(p, stream);
    }
    if (ks == 1) {
        int mk = 0;
        for (int c = 0; c < p.ncls; ++c) mk = std::max(mk, p.cls[c].nkt);
        p.kt_per_split = mk;
        if (bm == 128 && bn >= 64 && halo_eligible(p, smallc, XV2_MATH_BF16_STORE))
            return bn == 128 ? launch_one<Form::BF16HBM_HALO, 128, 128>(p, stream) : launch_one<Form::BF16HBM_HALO, 128, 64>(p, stream);
        const bool halo1 = bm == 128 && bn >= 64 && halo_eligible(p, smallc);
        if (halo1) {
            if (f16x2_ready(p))
                return bn == 128 ? launch_one<Form::F16X2_HALO, 128, 128>(p, stream) : launch_one<Form::F16X2_HALO, 128, 64>(p, stream);
            const void* x3 = nullptr;
            if (presplit_lookup(p.B, p.Nout, p.T, p.Ctot, &x3)) {
                p.Bx3 = reinterpret_cast<const float*>(x3);
                p.bytesBx3 = (unsigned)((size_t)p.Nout * p.T * p.Ctot * 6);
                return bn == 128 ? launch_one<Form::F32X3_HALO_WX3, 128, 128>(p, stream) : launch_one<Form::F32X3_HALO_WX3, 128, 64>(p, stream);
            }
            return bn == 128 ? launch_one<Form::F32X3_HALO, 128, 128>(p, stream) : launch_one<Form::F32X3_HALO, 128, 64>(p, stream);
        }
    } else {
        p.ksplit = (int)cdiv(p.cls[0].nkt, p.kt_per_split);
        const bool halo16 = halo_eligible(p, smallc, XV2_MATH_BF16_STORE);
        bool halo = halo_eligible(p, smallc) || halo16;
        if (halo) {      // K ranges of whole 32-channel chunks (all nine taps of a halo slice stay in one block)
            const int nch = p.cls[0].nkt / 9, cps = (int)cdiv(nch, p.ksplit), nks = (int)cdiv(nch, cps);
            if (nks > 1) {
                p.kt_per_split = 9 * cps;
                p.ksplit = nks;
                const void* x3 = nullptr;
                if (!halo16 && f16x2_ready(p)) {
                } else if (!halo16 && presplit_lookup(p.B, p.Nout, p.T, p.Ctot, &x3)) {
                    p.Bx3 = reinterpret_cast<const float*>(x3);
                    p.bytesBx3 = (unsigned)((size_t)p.Nout * p.T * p.Ctot * 6);
                }
            } else {
                halo = false;
            }
        }
        // split-K: the slab-sum kernel takes the statistics (32-row tiles)
        int rc = (halo && halo16)              ? launch_one<Form::BF16HBM_HALO, 128, 128>(p, stream)
                 : p.math == XV2_MATH_BF16_STORE ? launch_one<Form::BF16HBM, 128, 128>(p, stream)
                 : (halo && p.npl == 2)        ? launch_one<Form::F16X2_HALO, 128, 128>(p, stream)
                 : (halo && p.Bx3)             ? launch_one<Form::F32X3_HALO_WX3, 128, 128>(p, stream)
                 : halo                        ? launch_one<Form::F32X3_HALO, 128, 128>(p, stream)
                 : f16x2_ready_pertap(p)       ? launch_one<Form::F16X2, 128, 128>(p, stream)
                 : p.math == XV2_MATH_F32X3    ? launch_one<Form::F32X3, 128, 128>(p, stream)
                 : p.math                      ? launch_one<Form::BF16, 128, 128>(p, stream)
                                               : launch_one<Form::C32, 128, 128>(p, stream);
        if (rc) return rc;
        const int M = p.cls[0].M;
        const dim3 rgrid((unsigned)cdiv(M, SPLITK_ROWS), (unsigned)cdiv(p.Nout, 256));
        if (p.math == XV2_MATH_BF16_STORE)
            hipLaunchKernelGGL(splitk_reduce_kernel<bf16_t>, rgrid, dim3(256), 0, stream, splitk_ws, p.ksplit, M, p.Nout,
                               p.bias, (bf16_t*)p.Out0, p.ldo0, p.N0, (bf16_t*)p.Out1, p.ldo1, p.stats, p.accum,
                               p.ep_scale, p.ep_shift, (const bf16_t*)p.ep_res, p.ep_ldres, p.ep_act, (unsigned*)nullptr);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel<float>, rgrid, dim3(256), 0, stream, splitk_ws, p.ksplit, M, p.Nout,
                               p.bias, p.Out0, p.ldo0, p.N0, p.Out1, p.ldo1, p.stats, p.accum, p.ep_scale, p.ep_shift,
                               p.ep_res, p.ep_ldres, p.ep_act, p.amax_out);
        XV2_CHECK_LAUNCH();
        return XV2_OK;
    }
    if (smallc) {      // the image source: 128-row tiles only
        if (p.math == XV2_MATH_BF16_STORE) {
            // (bf16 MFMA on the rounded image was measured SLOWER here, 0.36 vs 0.22 ms: the gather loader sets the pace
            // and the 16 exact-fp32 instructions per K-tile hide it; the weight-gradient twin does use bf16 MFMA)
            if (bn == 128) return launch_one<Form::RGB_BF16OUT, 128, 128>(p, stream);
            if (bn == 64) return launch_one<Form::RGB_BF16OUT, 128, 64>(p, stream);
            return launch_one<Form::RGB_BF16OUT, 128, 32>(p, stream);
        }
        if (bn == 128) return launch_one<Form::RGB, 128, 128>(p, stream);
        if (bn == 64) return launch_one<Form::RGB, 128, 64>(p, stream);
        return launch_one<Form::RGB, 128, 32>(p, stream);
    }
    if (p.math == XV2_MATH_BF16_STORE) XV2_IGEMM_TILES(BF16HBM);
    if (p.math == XV2_MATH_F32X3 && f16x2_ready_pertap(p)) XV2_IGEMM_TILES(F16X2);
    if (p.math == XV2_MATH_F32X3) XV2_IGEMM_TILES(F32X3);
    if (p.math) XV2_IGEMM_TILES(BF16);
    XV2_IGEMM_TILES(C32);
}
#undef XV2_IGEMM_TILES

// python-style floor division for the parity decomposition
static inline int fdiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

static int fill_common(IgemmParams& p, const xv2_conv_desc* d) {
    XV2_CHECK_ARG(d->KH * d->KW <= 52, "kernel %dx%d has too many taps", d->KH, d->KW);
    XV2_CHECK_ARG(d->stride >= 1 && d->dil >= 1, "bad stride/dilation");
    XV2_CHECK_ARG((long long)d->N * d->IH * d->IW < (1ll << 31) && (long long)d->N * d->OH * d->OW < (1ll << 31),
                  "tensor too large for 32-bit pixel indices");
    p.bias = nullptr;
    p.stats = nullptr;
    p.part = nullptr;
    p.Bx3 = nullptr;
    p.bytesBx3 = 0;
    p.npl = 3;
    p.amaxA0 = amax_ctx().a0;      // forward: the activation sources (backward-data replaces them by the gradient's)
    p.amaxA1 = amax_ctx().a1;
    p.amaxB = nullptr;
    p.amax_out = nullptr;
    p.amax_recorded = nullptr;
    p.ksplit = 1;
    p.cin_real = 3;
    p.math = d->math;
    p.accum = 0;
    p.ep_scale = p.ep_shift = p.ep_res = nullptr;
    p.ep_ldres = p.ep_act = 0;
    XV2_CHECK_ARG(d->math >= 0 && d->math <= XV2_MATH_F32X3, "conv: unknown math mode %d", d->math);
    p.A1 = nullptr;
    p.Out1 = nullptr;
    p.ncls = 1;
    return XV2_OK;
}

static inline bool is_rgb(const xv2_conv_desc* d) { return d->C0 == 4 && d->C1 == 0; }
// bytes per element of the activations / packed weights a convolution reads (the RGB image and its weights stay fp32)
static inline long long esz_in(const xv2_conv_desc* d) { return (d->math == XV2_MATH_BF16_STORE && !is_rgb(d)) ? 2 : 4; }
static inline bool out_aligned(const xv2_conv_desc* d, const void* p, int ld) {
    const uintptr_t mask = d->math == XV2_MATH_BF16_STORE ? 7 : 15;      // 4-element vector stores
    return ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & mask) == 0;
}
static inline int fwd_nkt(const xv2_conv_desc* d) {
    return is_rgb(d) ? (int)cdiv(d->KH * d->KW * 4, BK) : d->KH * d->KW * ((d->C0 + d->C1) / BK);
}

}  // namespace xv2

using namespace xv2;

// rows per statistics tile when the forward pass of this descriptor is planned for sg_conv.hip (single source), else 0
static int fwd_sg_rows(const xv2_conv_desc* d) {
    if (is_rgb(d) || d->C1 != 0) return 0;
    return sg_planned_rows((int64_t)d->N * d->OH * d->OW, d->Cout, d->C0, d->KH * d->KW, d->math);
}
extern "C" int64_t xv2_conv2d_forward_stats_tiles(const xv2_conv_desc* d) {
    if (const int r = fwd_sg_rows(d)) return cdiv((int64_t)d->N * d->OH * d->OW, r);
    return igemm_stats_tiles((int64_t)d->N * d->OH * d->OW, d->Cout, is_rgb(d), fwd_nkt(d), d->math);
}
extern "C" int64_t xv2_conv2d_forward_stats_tile_rows(const xv2_conv_desc* d) {
    if (const int r = fwd_sg_rows(d)) return r;
    return igemm_stats_tile_rows((int64_t)d->N * d->OH * d->OW, d->Cout, is_rgb(d), fwd_nkt(d), d->math);
}
extern "C" size_t xv2_conv2d_forward_workspace(const xv2_conv_desc* d) {
    // (a shape planned for sg_conv.hip keeps the tiled plan's workspace: launches WITHOUT statistics whose operands are not
    //  ready for it still run that plan, split K included)
    return igemm_splitk_bytes((int64_t)d->N * d->OH * d->OW, d->Cout, is_rgb(d), fwd_nkt(d), d->math);
}
extern "C" size_t xv2_conv2d_backward_data_workspace(const xv2_conv_desc* d) {
    if (d->stride != 1) return 0;
    return igemm_splitk_bytes((int64_t)d->N * d->IH * d->IW, d->C0 + d->C1, false, d->KH * d->KW * (d->Cout / BK), d->math);
}

struct FwdEpilogue {
    const float* scale;
    const float* shift;
    const float* res;
    int ldres, act;
};
static int amax_rows_into(const float* x, int64_t rows, int C, int64_t ld, unsigned* slots, hipStream_t stream);      // below
static int conv_forward_impl(const xv2_conv_desc* d, const float* x0, int ldx0, const float* x1, int ldx1,
                             const float* w_ohwi, const float* bias, float* y, int ldy, float* stats,
                             float* workspace, void* stream, const FwdEpilogue* ep, int accumulate = 0) {
    AmaxGuard amax_guard;
    IgemmParams p;
    int rc = fill_common(p, d);
    if (rc) return rc;
    p.accum = accumulate & 1;      // ADD the result onto what y holds (the gradient of the tensor's other consumer)
    if (ep) {
        XV2_CHECK_ARG(ep->scale && ep->shift && !stats, "conv2d_forward_fused: scale and shift are required, stats excluded");
        XV2_CHECK_ARG((reinterpret_cast<uintptr_t>(ep->scale) & 15) == 0 && (reinterpret_cast<uintptr_t>(ep->shift) & 15) == 0 &&
                          (!ep->res || out_aligned(d, ep->res, ep->ldres)),
                      "conv2d_forward_fused: epilogue operands must be 16-byte aligned");
        p.ep_scale = ep->scale; p.ep_shift = ep->shift; p.ep_res = ep->res; p.ep_ldres = ep->ldres; p.ep_act = ep->act;
    }
    const bool smallc = is_rgb(d);
    XV2_CHECK_ARG(smallc || (d->C0 % 32 == 0 && d->C1 % 32 == 0 && d->C0 > 0),
                  "conv2d_forward: C0=%d C1=%d must be multiples of 32 (or a single 4-channel source)", d->C0, d->C1);
    XV2_CHECK_ARG(!(stats && bias), "conv2d_forward: stats and bias are mutually exclusive");
    XV2_CHECK_ARG(out_aligned(d, y, ldy), "conv2d_forward: output rows must be aligned to 4 elements");
    // (band form of an RGB stem, xv2_pad_band: pixel stride 4 with an even pixel index on every access keeps 16-byte alignment)
    const bool band = d->C0 == 32 && d->C1 == 0 && ldx0 == 4 && d->KW == 1 && d->stride == 2 && d->pad == 0 && d->IW % 2 == 0;
    XV2_CHECK_ARG(esz_in(d) == 4 || band || (ldx0 % 8 == 0 && (!x1 || ldx1 % 8 == 0) && (reinterpret_cast<uintptr_t>(x0) & 15) == 0 &&
                                     (reinterpret_cast<uintptr_t>(x1) & 15) == 0 && (reinterpret_cast<uintptr_t>(w_ohwi) & 15) == 0),
                  "conv2d_forward: bf16 operands must be 16-byte aligned with row strides that are multiples of 8");
    XV2_CHECK_ARG(!(stats && !workspace && xv2_conv2d_forward_workspace(d) > 0),
                  "conv2d_forward: this shape is planned as split-K; pass the workspace when stats are requested");
    p.A0 = x0; p.A1 = x1; p.B = w_ohwi; p.bias = bias; p.Out0 = y; p.Out1 = nullptr; p.stats = stats;
    p.C0 = d->C0; p.C1 = d->C1; p.Ctot = d->C0 + d->C1;
    p.ldA0 = ldx0; p.ldA1 = ldx1;
    p.IH = d->IH; p.IW = d->IW; p.s_in = d->stride;
    p.osN = d->OH * d->OW; p.osH = d->OW; p.osW = 1;
    p.Nout = d->Cout; p.N0 = d->Cout; p.ldo0 = ldy; p.ldo1 = 0;
    p.T = d->KH * d->KW;
    ClassInfo& c = p.cls[0];
    c.tap0 = 0; c.ntaps = p.T; c.OHl = d->OH; c.OWl = d->OW; c.M = d->N * d->OH * d->OW; c.os0 = 0;
    for (int kh = 0; kh < d->KH; ++kh)
        for (int kw = 0; kw < d->KW; ++kw) {
            Tap& t = p.taps[kh * d->KW + kw];
            t.dh = (short)(kh * d->dil - d->pad);
            t.dw = (short)(kw * d->dil - d->pad);
            t.slot = kh * d->KW + kw;
        }
    p.cpt = smallc ? 1 : p.Ctot / BK;
    c.nkt = fwd_nkt(d);
    {
        const long long pixels = (long long)d->N * d->IH * d->IW;
        const long long es = esz_in(d);
        const long long b0 = pixels * ldx0 * es, b1 = x1 ? pixels * ldx1 * es : 0;
        const long long bw = (long long)d->Cout * p.T * p.Ctot * es;
        XV2_CHECK_ARG(b0 < (1ll << 31) && b1 < (1ll << 31) && bw < (1ll << 31) && p.T <= 32 || smallc,
                      "conv2d_forward: operands of 2 GiB or more (or more than 32 taps) are not supported");
        p.bytesA0 = (unsigned)b0; p.bytesA1 = (unsigned)b1; p.bytesB = (unsigned)bw;
    }
    // F16X2, inference (fused epilogue): record max |z| for the next layer - in the epilogue of the tiled kernels, by a pass
    // of its own behind the direct / streaming / stem kernels
    int amax_recorded = 0;
    if (ep && p.math != XV2_MATH_BF16_STORE && p.math != XV2_MATH_BF16) {
        p.amax_out = amax_ctx().out;
        p.amax_recorded = &amax_recorded;
    }
    if (int rc2 = igemm_launch(p, smallc, workspace, (hipStream_t)stream)) return rc2;
    if (p.amax_out && !amax_recorded)
        return amax_rows_into(y, (int64_t)d->N * d->OH * d->OW, d->Cout, ldy, p.amax_out, (hipStream_t)stream);
    return XV2_OK;
}

extern "C" int xv2_conv2d_forward(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1,
                                  int ldx1, const void* w_ohwi, const float* bias, void* y, int ldy,
                                  float* stats, float* workspace, void* stream) {
    return conv_forward_impl(d, (const float*)x0, ldx0, (const float*)x1, ldx1, (const float*)w_ohwi, bias, (float*)y, ldy,
                             stats, workspace, stream, nullptr);
}

extern "C" int xv2_conv2d_forward_bn(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                                     const void* w_ohwi, void* y, int ldy, float* stats_partials, float* workspace,
                                     int parts, int part_stride, double* sums, double* scratch, double count,
                                     const float* gamma, const float* beta, float eps, float momentum,
                                     float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                                     float* shift, void* stream) {
    XV2_CHECK_ARG(stats_partials && scratch && sums, "conv2d_forward_bn: partials, scratch and sums are required");
    XV2_CHECK_ARG(parts >= 1 && part_stride >= d->Cout, "conv2d_forward_bn: parts=%d part_stride=%d", parts, part_stride);
    XV2_CHECK_ARG(!mean || (invstd && scale && shift), "conv2d_forward_bn: mean, invstd, scale and shift go together");
    // the convolution (with statistics partials per row tile), then per part the reduction of the partials (+ coefficients and
    // running statistics).  (Round 3 folded the reduction into the convolution launch - the last blocks to arrive summed the
    // partials behind a device-scope ticket; with the release fences that hand-off needs it cost +0.65 ms per cfg2 step and was
    // removed in round 6 together with the gated apply that depended on it: a kernel boundary is cheaper)
    int rc = xv2_conv2d_forward(d, x0, ldx0, x1, ldx1, w_ohwi, nullptr, y, ldy, stats_partials, workspace, stream);
    if (rc) return rc;
    const int64_t tiles = xv2_conv2d_forward_stats_tiles(d);
    XV2_CHECK_ARG(tiles % parts == 0, "conv2d_forward_bn: %lld statistics tiles do not split into %d parts", (long long)tiles, parts);
    const int64_t tpp = tiles / parts;
    for (int s = 0; s < parts && !rc; ++s) {
        const float* ps = stats_partials + (size_t)s * tpp * d->Cout * 2;
        double* ss = sums + (size_t)s * part_stride * 2;
        const size_t o = (size_t)s * part_stride;
        rc = mean ? xv2_bn_reduce_finalize(ps, tpp, d->Cout, ss, scratch, count, gamma, beta, eps, momentum, running_mean,
                                           running_var, mean + o, invstd + o, scale + o, shift + o, stream)
                  : xv2_bn_reduce_stats(ps, tpp, d->Cout, ss, scratch, stream);
    }
    return rc;
}

extern "C" int xv2_conv2d_forward_fused(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1,
                                        int ldx1, const void* w_ohwi, const float* scale, const float* shift,
                                        const void* residual, int ldres, int act, void* z, int ldz,
                                        float* workspace, void* stream) {
    FwdEpilogue ep{scale, shift, (const float*)residual, ldres, act};
    return conv_forward_impl(d, (const float*)x0, ldx0, (const float*)x1, ldx1, (const float*)w_ohwi, nullptr, (float*)z, ldz,
                             nullptr, workspace, stream, &ep);
}

// backward-data of conv `d`: A = dy [N][OH][OW][Cout], output = dx [N][IH][IW][C0|C1]
static int dgrad_impl(const xv2_conv_desc* d, const float* dy, int lddy, const float* w_ihwo,
                      float* dx0, int lddx0, float* dx1, int lddx1, float* workspace, hipStream_t stream,
                      int accumulate = 0) {
    AmaxGuard amax_guard;
    IgemmParams p;
    int rc = fill_common(p, d);
    if (rc) return rc;
    p.amaxA0 = amax_ctx().dy;      // the A operand of a backward-data launch is the output gradient
    p.amaxA1 = nullptr;
    int amax_recorded = 0;
    if (d->math == XV2_MATH_F32X3) {      // F16X2: the maximum of dx0 for ITS consumers (a transposed convolution's backward)
        p.amax_out = amax_ctx().out;
        p.amax_recorded = &amax_recorded;
    }
    p.accum = accumulate & (dx1 ? 3 : 1);
    XV2_CHECK_ARG(d->Cout % 32 == 0, "backward_data: Cout=%d must be a multiple of 32", d->Cout);
    XV2_CHECK_ARG(d->C0 % 32 == 0 && d->C1 % 32 == 0, "backward_data: C0=%d/C1=%d must be multiples of 32", d->C0, d->C1);
    const int s = d->stride;
    XV2_CHECK_ARG(s <= 2, "backward_data: stride %d unsupported (1 or 2)", s);
    XV2_CHECK_ARG(out_aligned(d, dx0, lddx0) && (!dx1 || out_aligned(d, dx1, lddx1)),
                  "backward_data: output rows must be aligned to 4 elements");
    const long long es = d->math == XV2_MATH_BF16_STORE ? 2 : 4;
    XV2_CHECK_ARG(es == 4 || (lddy % 8 == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0 && (reinterpret_cast<uintptr_t>(w_ihwo) & 15) == 0),
                  "backward_data: bf16 operands must be 16-byte aligned with row strides that are multiples of 8");
    p.A0 = dy; p.A1 = nullptr; p.B = w_ihwo;
    p.C0 = d->Cout; p.C1 = 0; p.Ctot = d->Cout; p.ldA0 = lddy; p.ldA1 = 0;
    p.IH = d->OH; p.IW = d->OW; p.s_in = 1;
    p.Nout = d->C0 + d->C1; p.N0 = d->C0;
    p.Out0 = dx0; p.ldo0 = lddx0; p.Out1 = dx1; p.ldo1 = lddx1;
    p.T = d->KH * d->KW;
    p.cpt = p.Ctot / BK;
    p.osN = d->IH * d->IW; p.osH = s * d->IW; p.osW = s;
    {
        const long long b0 = (long long)d->N * d->OH * d->OW * lddy * es;
        const long long bw = (long long)(d->C0 + d->C1) * p.T * d->Cout * es;
        XV2_CHECK_ARG(b0 < (1ll << 31) && bw < (1ll << 31) && p.T <= 32,
                      "backward_data: operands of 2 GiB or more (or more than 32 taps) are not supported");
        p.bytesA0 = (unsigned)b0; p.bytesA1 = 0; p.bytesB = (unsigned)bw;
    }
    bool need_zero = false;
    int ncls = 0, ntap = 0;
    for (int pi = 0; pi < s; ++pi)
        for (int pj = 0; pj < s; ++pj) {
            const int OHl = (d->IH - pi + s - 1) / s, OWl = (d->IW - pj + s - 1) / s;
            if (OHl <= 0 || OWl <= 0) continue;
            ClassInfo c;
            c.tap0 = ntap; c.ntaps = 0; c.OHl = OHl; c.OWl = OWl; c.M = d->N * OHl * OWl;
            c.os0 = pi * d->IW + pj;
            for (int kh = 0; kh < d->KH; ++kh) {
                const int nh = pi + d->pad - kh * d->dil;
                if (((nh % s) + s) % s != 0) continue;
                for (int kw = 0; kw < d->KW; ++kw) {
                    const int nw = pj + d->pad - kw * d->dil;
                    if (((nw % s) + s) % s != 0) continue;
                    Tap& t = p.taps[ntap++];
                    t.dh = (short)fdiv(nh, s);
                    t.dw = (short)fdiv(nw, s);
                    t.slot = kh * d->KW + kw;
                    ++c.ntaps;
                }
            }
            if (c.ntaps == 0) {
                need_zero = true;
                continue;
            }
            c.nkt = c.ntaps * p.cpt;
            p.cls[ncls++] = c;
        }
    if (need_zero) {
        XV2_CHECK_ARG(lddx0 == d->C0 && (d->C1 == 0 || lddx1 == d->C1),
                      "backward_data: strided outputs unsupported when parity classes are empty");
        // pixels no tap reaches get a zero gradient - or, when accumulating, keep what they hold
        if (!(p.accum & 1)) XV2_CHECK_HIP(hipMemsetAsync(dx0, 0, (size_t)d->N * d->IH * d->IW * d->C0 * es, stream));
        if (d->C1 && !(p.accum & 2))
            XV2_CHECK_HIP(hipMemsetAsync(dx1, 0, (size_t)d->N * d->IH * d->IW * d->C1 * es, stream));
    }
    if (ncls == 0) return XV2_OK;
    p.ncls = ncls;
    if (int rc2 = igemm_launch(p, false, (s == 1) ? workspace : nullptr, stream)) return rc2;
    if (p.amax_out && !amax_recorded) {      // (direct / streaming kernels: a pass of its own over dx0)
        XV2_CHECK_ARG(lddx0 == d->C0, "backward_data: F16X2 maximum of a strided dx0");
        return xv2_tensor_amax_into(dx0, (int64_t)d->N * d->IH * d->IW * d->C0, p.amax_out, stream);
    }
    return XV2_OK;
}

extern "C" int xv2_conv2d_backward_data(const xv2_conv_desc* d, const void* dy, int lddy,
                                        const void* w_ihwo, void* dx0, int lddx0, void* dx1,
                                        int lddx1, float* workspace, void* stream) {
    return dgrad_impl(d, (const float*)dy, lddy, (const float*)w_ihwo, (float*)dx0, lddx0, (float*)dx1, lddx1, workspace,
                      (hipStream_t)stream);
}

extern "C" int xv2_conv2d_backward_data_acc(const xv2_conv_desc* d, const void* dy, int lddy,
                                            const void* w_ihwo, void* dx0, int lddx0, void* dx1,
                                            int lddx1, int accumulate, float* workspace, void* stream) {
    return dgrad_impl(d, (const float*)dy, lddy, (const float*)w_ihwo, (float*)dx0, lddx0, (float*)dx1, lddx1, workspace,
                      (hipStream_t)stream, accumulate);
}

extern "C" int xv2_conv_transpose2d_forward(const xv2_conv_desc* d, const void* x, int ldx,
                                            const void* w_ihwo, void* y, int ldy, void* stream) {
    XV2_CHECK_ARG(d->C1 == 0, "conv_transpose2d: single output tensor expected");
    AmaxGuard amax_guard;
    // F16X2: the maximum of y (the next convolution's source): the tiled kernels record it in their epilogue (dgrad_impl),
    // the streaming kernel in its store loop (round 6: the pass of its own over the 268 MB of the 1024^2 level took 69 us per step)
    unsigned* slots = (d->math == XV2_MATH_F32X3 && ldy == d->C0) ? amax_ctx().out : nullptr;
    XV2_CHECK_ARG(!amax_ctx().out || slots, "conv_transpose2d: F16X2 maximum of a strided / non-fp32 output");
    const int rc = thin_convT_forward(d, x, ldx, w_ihwo, y, ldy, slots, (hipStream_t)stream);      // thin_conv.hip (records max |y| in its store loop)
    if (rc < 0) return dgrad_impl(d, (const float*)x, ldx, (const float*)w_ihwo, (float*)y, ldy, nullptr, 0, nullptr, (hipStream_t)stream);
    return rc;
}

extern "C" int xv2_conv_transpose2d_backward_data(const xv2_conv_desc* d, const void* dy, int lddy,
                                                  const void* w_ohwi, void* dx, int lddx, void* stream) {
    AmaxGuard amax_guard;      // (the streaming kernel does not read the context: it must still end with this call)
    if (const int rc = thin_convT_backward_data(d, dy, lddy, w_ohwi, dx, lddx, 0, (hipStream_t)stream); rc >= 0) return rc;
    return xv2_conv2d_forward(d, dy, lddy, nullptr, 0, w_ohwi, nullptr, dx, lddx, nullptr, nullptr, stream);
}

extern "C" int xv2_conv_transpose2d_backward_data_acc(const xv2_conv_desc* d, const void* dy, int lddy, const void* w_ohwi,
                                                      void* dx, int lddx, int accumulate, float* workspace, void* stream) {
    AmaxGuard amax_guard;
    if (const int rc = thin_convT_backward_data(d, dy, lddy, w_ohwi, dx, lddx, accumulate, (hipStream_t)stream); rc >= 0) return rc;
    return conv_forward_impl(d, (const float*)dy, lddy, nullptr, 0, (const float*)w_ohwi, nullptr, (float*)dx, lddx, nullptr,
                             workspace, stream, nullptr, accumulate);
}

// ---- pre-split weights (see PresplitEntry) ---------------------------------------------------------------------------
extern "C" size_t xv2_presplit_bytes(int nrows, int T, int ctot) { return (size_t)nrows * T * ctot * 6; }

extern "C" int xv2_presplit_supported(int nrows, int T, int ctot) { return (T == 9 && nrows % 64 == 0 && ctot % 32 == 0) ? 1 : 0; }

static int presplit_register(const float* b_fp32, int nrows, int T, int ctot, void* x3) {
    XV2_CHECK_ARG(b_fp32 && x3 && xv2_presplit_supported(nrows, T, ctot), "presplit: unsupported operand %d x %d x %d", nrows, T, ctot);
    XV2_CHECK_ARG((reinterpret_cast<uintptr_t>(x3) & 15) == 0 && (reinterpret_cast<uintptr_t>(b_fp32) & 15) == 0 &&
                      xv2_presplit_bytes(nrows, T, ctot) < (1ull << 31), "presplit: alignment / size");
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    g_presplit[b_fp32] = PresplitEntry{x3, nrows, T, ctot};
    return XV2_OK;
}

// split the packed fp32 operand `b_fp32` [nrows][T][ctot] into `x3` and remember the pair: convolutions that are handed
// `b_fp32` afterwards read the planes (the caller refreshes them whenever the weights change, on the same stream)
extern "C" int xv2_presplit_weights(const float* b_fp32, int nrows, int T, int ctot, void* x3, void* stream) {
    if (int rc = presplit_register(b_fp32, nrows, T, ctot, x3)) return rc;
    const int64_t nb = (int64_t)(nrows / 64) * (ctot / 16);
    hipLaunchKernelGGL(presplit_kernel, dim3((unsigned)std::min<int64_t>(nb, 16384)), dim3(256), 0, (hipStream_t)stream,
                       b_fp32, reinterpret_cast<__bf16*>(x3), nrows, T, ctot);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
// ... of a row-strided tensor [rows][C] with row pitch ld (a channel slice of a wider tensor)
__global__ void __launch_bounds__(256) amax_rows_kernel(const float* __restrict__ x, int64_t rows, int C4, int64_t ld,
                                                         unsigned* __restrict__ slots) {
    __shared__ float red[4];
    float m = 0.f;
    const int64_t total = rows * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / C4;
        m = amax_acc(m, *reinterpret_cast<const float4*>(x + r * ld + (i - r * C4) * 4));
    }
    amax_record(slots, m, red);
}
static int amax_rows_into(const float* x, int64_t rows, int C, int64_t ld, unsigned* slots, hipStream_t stream) {
    XV2_CHECK_ARG(x && slots && rows > 0 && C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)x & 15) == 0, "amax_rows: 4-element rows");
    const int64_t n4 = rows * (C / 4);
    hipLaunchKernelGGL(amax_rows_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n4, 1024), 1024)), dim3(256), 0, stream, x, rows, C / 4,
                       ld, slots);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
// max |x| ON TOP of what the slots hold (no zeroing): producers whose kernel has no recording form
int xv2_tensor_amax_into(const float* x, int64_t n, void* slots, void* stream) {
    XV2_CHECK_ARG(x && slots && n > 0 && n % 4 == 0 && ((uintptr_t)x & 15) == 0, "tensor_amax: n %% 4 == 0, 16-byte aligned");
    const long long n4 = n / 4;
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)std::min<long long>(cdiv(n4, 1024), 1024)), dim3(256), 0, (hipStream_t)stream, x,
                       (size_t)n4, static_cast<unsigned*>(slots));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
extern "C" int xv2_tensor_amax(const float* x, int64_t n, void* slots, void* stream) {
    XV2_CHECK_ARG(x && slots && n > 0 && n % 4 == 0 && ((uintptr_t)x & 15) == 0, "tensor_amax: n %% 4 == 0, 16-byte aligned");
    XV2_CHECK_HIP(hipMemsetAsync(slots, 0, AMAX_SLOTS * AMAX_STRIDE * sizeof(unsigned), (hipStream_t)stream));
    const long long n4 = n / 4;
    hipLaunchKernelGGL(amax_kernel, dim3((unsigned)std::min<long long>(cdiv(n4, 1024), 1024)), dim3(256), 0, (hipStream_t)stream, x,
                       (size_t)n4, static_cast<unsigned*>(slots));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
extern "C" size_t xv2_presplit_f16_bytes(int nrows, int T, int ctot) { return (size_t)nrows * T * ctot * 4; }
// layouts that get the two fp16 planes: the 3x3 layers (halo form, sg_conv.hip) and, since round 5, the 1x1 layers (sg_conv.hip)
extern "C" int xv2_presplit_f16_supported(int nrows, int T, int ctot) {
    if (T == 9) return xv2_presplit_supported(nrows, T, ctot);
    return (T == 1 && nrows % 64 == 0 && ctot % 16 == 0) ? 1 : 0;
}
extern "C" int xv2_weight_amax_register(const void* b_fp32, const void* amax_slots) {
    XV2_CHECK_ARG(b_fp32 && amax_slots, "weight_amax_register: null");
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    g_wamax[b_fp32] = static_cast<const unsigned*>(amax_slots);
    return XV2_OK;
}
// table[n][4] = {x (fp32, 16-byte aligned), n4 = float4 count, slots, first block}; an entry owns ceil(n4 / 1024) blocks
__global__ void __launch_bounds__(256) amax_table_kernel(const int64_t* __restrict__ table, int n) {
    __shared__ float red[4];
    int lo = 0, hi = n - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * 4 + 3] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* e = table + lo * 4;
    const float4* x = reinterpret_cast<const float4*>(e[0]);
    const int64_t n4 = e[1], b = blk - e[3];
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = b * 1024 + u * 256 + threadIdx.x;
        if (i < n4) m = amax_acc(m, x[i]);
    }
    amax_record(reinterpret_cast<unsigned*>(e[2]), m, red, (unsigned)b);
}
extern "C" int xv2_weight_amax_table(const int64_t* table, int n, int64_t total_blocks, void* amax_base, int64_t amax_bytes,
                                     void* stream) {
    XV2_CHECK_ARG(table && n > 0 && total_blocks > 0 && total_blocks < (1ll << 31) && amax_base && amax_bytes > 0,
                  "weight_amax_table: bad table");
    XV2_CHECK_HIP(hipMemsetAsync(amax_base, 0, (size_t)amax_bytes, (hipStream_t)stream));
    hipLaunchKernelGGL(amax_table_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table, n);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
extern "C" int xv2_presplit_weights_f16(const float* b_fp32, int nrows, int T, int ctot, void* x2, void* amax_slots, void* stream) {
    XV2_CHECK_ARG(b_fp32 && x2 && amax_slots && xv2_presplit_f16_supported(nrows, T, ctot), "presplit_f16: unsupported operand %d x %d x %d",
                  nrows, T, ctot);
    XV2_CHECK_ARG(((uintptr_t)x2 & 15) == 0 && xv2_presplit_f16_bytes(nrows, T, ctot) < (1ull << 31), "presplit_f16: alignment / size");
    {
        std::lock_guard<std::mutex> lk(g_presplit_mu);
        PresplitEntry e{x2, nrows, T, ctot};
        e.amax = static_cast<const unsigned*>(amax_slots);
        g_presplit2[b_fp32] = e;
    }
    const int64_t nb = (int64_t)(nrows / 64) * (ctot / 16);
    hipLaunchKernelGGL(presplit2h_kernel, dim3((unsigned)std::min<int64_t>(nb, 16384)), dim3(256), 0, (hipStream_t)stream, b_fp32,
                       reinterpret_cast<__bf16*>(x2), nrows, T, ctot, static_cast<unsigned*>(amax_slots));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
// every registered F16X2 pair of a device table in one go (after the optimizer step): zero the slots, maxima, planes
extern "C" int xv2_presplit_f16_table(const int64_t* table, int n, int64_t total_blocks, void* stream) {
    XV2_CHECK_ARG(table && n > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "presplit_f16_table: bad table");
    hipLaunchKernelGGL(presplit2h_table_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table, n);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
extern "C" int64_t xv2_presplit_blocks(int nrows, int T, int ctot) { (void)T; return (int64_t)(nrows / 64) * (ctot / 16); }
// every registered pair of a device table in one launch (after the optimizer step); rows as in presplit_table_kernel
extern "C" int xv2_presplit_table(const int64_t* table, int n, int64_t total_blocks, void* stream) {
    XV2_CHECK_ARG(table && n > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "presplit_table: bad table");
    hipLaunchKernelGGL(presplit_table_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, table, n);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
extern "C" int xv2_presplit_forget(const void* b_fp32) {
    std::lock_guard<std::mutex> lk(g_presplit_mu);
    if (b_fp32) {
        g_presplit.erase(b_fp32);
        g_presplit2.erase(b_fp32);
        g_wamax.erase(b_fp32);
    } else {
        g_presplit.clear();
        g_presplit2.clear();
        g_wamax.clear();
    }
    return XV2_OK;
}
