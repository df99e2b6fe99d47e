// Joint histogram behind the sweep of the fusion's thresholds and class scales (xview2_amd/utils/calibrate.py).
//
// The fusion (pp_fuse_kernel) is per pixel: pre = (loc > a) | ((loc > b) & (post_raw > 1)), post = pre ? post_raw : 0, and
// the scorer's 15 counts are sums over pixels of functions of (pre, post, lt, dt).  With an ascending threshold table T and
// k = #{ j : loc > T[j] }, "loc > T[j]" is "k > j", so one pass that counts the pixels per (k, r = post_raw - 1, t = lt > 0,
// d = dt) holds the counts of every pair (a, b) = (T[i], T[j]) at once; the host takes them out by suffix sums.
//
// One block walks a stretch of one tile for one scale vector (blockIdx.z).  The thresholds sit in LDS and k comes from a
// binary search; the block's counts sit in an LDS table of (n + 1) * 40 uint32 and its non-zero bins go out as 64-bit global
// adds.  Integer adds commute, so the histogram is the same whatever the schedule.
//
// Contention: on real tiles most pixels fall into a handful of background bins.  Equal keys can be combined per WAVE before
// they reach LDS: the first lane still holding a key broadcasts it, a ballot finds every lane with that key, one lane adds the
// popcount, and those lanes retire; after `rounds` such rounds the lanes left over add their own ones.  Measured
// (profiles/calibrate_cost.md, S = 27): against one atomic per pixel, ONE round is 1.5 times faster where a stretch is uniform
// and 8-13 % slower where four to forty keys mix; every further round only costs (eight rounds: 1.7-2.1 times the naive time).
// So DEFAULT_ROUNDS is 1: the uniform stretch, whose 64 lanes would queue on one address, is the case worth buying off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"
#include "fuse_px.h"

namespace {

using xv2::K_4CH;
using xv2::K_5CH;
using xv2::K_LABEL;

constexpr int MAX_T = 128;            // thresholds
constexpr int MAX_S = 64;             // scale vectors per launch (gridDim.z)
constexpr int BINS_K = 40;            // bins per k: [r 4][t 2][d 5]
constexpr int DEFAULT_ROUNDS = 1;
constexpr int PX_PER_BLOCK = 1024;    // pixels a block walks at least (when the tile has them)
constexpr int TARGET_BLOCKS = 1792;   // 256 CUs x 7 resident blocks (LDS): one round of blocks, each zeroing and flushing once

// rounds == 0: the naive form, one LDS atomic per pixel (scripts/bench_calibrate.py's comparison)
template <int KIND>
__global__ void __launch_bounds__(256) calibrate_hist_kernel(const float* __restrict__ loc, const void* __restrict__ dmg,
                                                             const uint8_t* __restrict__ lt, const uint8_t* __restrict__ dt,
                                                             int64_t hw, const float* __restrict__ thresholds, int n,
                                                             const float* __restrict__ scales,
                                                             unsigned long long* __restrict__ hist,
                                                             unsigned long long* __restrict__ bad, int rounds) {
    __shared__ float T[MAX_T];
    __shared__ unsigned sh[(MAX_T + 1) * BINS_K];
    __shared__ unsigned sh_bad;
    const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.z;
    const int bins = (n + 1) * BINS_K;
    for (int i = tid; i < bins; i += 256) sh[i] = 0;
    if (tid < n) T[tid] = thresholds[tid];
    if (tid == 0) sh_bad = 0;
    xv2::ClassScale cs = {{1.f, 1.f, 1.f, 1.f}, scales != nullptr};
    if (scales) {
#pragma unroll
        for (int c = 0; c < 4; ++c) cs.s[c] = scales[s * 4 + c];
    }
    __syncthreads();
    const int64_t base = (int64_t)b * hw;
    const int64_t stride = (int64_t)gridDim.x * 256;
    unsigned nbad = 0;
    // i0 is uniform over the block, so every lane of a wave takes every trip and the ballots below see the whole wave
    for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < hw; i0 += stride) {
        const int64_t i = i0 + tid;
        int key = -1;
        if (i < hw) {
            const int raw = xv2::decode_raw<KIND>(dmg, b, hw, i, cs);
            const float l = loc[base + i];
            const unsigned t = lt[base + i], d = dt[base + i];
            int lo = 0, hi = n;   // k = the first j with !(l > T[j]), n if none; NaN compares false: k = 0
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (l > T[mid]) lo = mid + 1; else hi = mid;
            }
            if (t > 4 || d > 4 || (KIND == K_LABEL && (raw < 1 || raw > 4)))
                ++nbad;
            else
                key = lo * BINS_K + (raw - 1) * 10 + (t > 0 ? 5 : 0) + (int)d;
        }
        if (rounds > 0) {
            unsigned long long left = __ballot(key >= 0);
            for (int round = 0; left && round < rounds; ++round) {
                const int first = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(left));
                const int lead = __builtin_amdgcn_readlane(key, first);
                const unsigned long long same = __ballot(key == lead);   // retired lanes hold -1 and never match
                if ((tid & 63) == first) atomicAdd(&sh[lead], (unsigned)__popcll(same));
                if (key == lead) key = -1;
                left &= ~same;
            }
        }
        if (key >= 0) atomicAdd(&sh[key], 1u);
    }
    const unsigned long long mb = __ballot(nbad != 0);
    if (mb) {
        nbad = (unsigned)xv2::wave_sum((int)nbad);
        if ((tid & 63) == 0) atomicAdd(&sh_bad, nbad);
    }
    __syncthreads();
    unsigned long long* out = hist + (int64_t)s * bins;
    for (int i = tid; i < bins; i += 256)
        if (sh[i]) atomicAdd(&out[i], (unsigned long long)sh[i]);
    // every scale vector sees the same bad pixels (the label check has no scales): count them once
    if (tid == 0 && s == 0 && sh_bad) atomicAdd(bad, (unsigned long long)sh_bad);
}

int g_rounds = DEFAULT_ROUNDS;   // xv2_calibrate_hist_rounds: measurement switch of scripts/bench_calibrate.py

}  // namespace

static int cal_kid() {
    static const int id = xv2::prof_register("calibrate_hist_kernel");
    return id;
}

extern "C" int xv2_calibrate_hist_rounds(int rounds) {
    g_rounds = rounds < 0 ? DEFAULT_ROUNDS : std::min(rounds, 64);
    return XV2_OK;
}

extern "C" int xv2_calibrate_hist(const float* loc, const void* dmg, int dmg_kind, const uint8_t* lt, const uint8_t* dt, int B,
                                  int H, int W, const float* thresholds, int n, const float* scales, int S, int64_t* hist,
                                  int64_t* bad, void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "calibrate_hist: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "calibrate_hist: H*W=%lld exceeds 2^30 pixels per tile", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + 63) / 64 <= 65535, "calibrate_hist: B=%d or H=%d too large for one launch", B, H);
    XV2_CHECK_ARG(dmg_kind == XV2_DMG_4CH || dmg_kind == XV2_DMG_5CH || dmg_kind == XV2_DMG_LABEL,
                  "calibrate_hist: dmg_kind=%d unsupported (4- or 5-channel probabilities, or an int32 label map)", dmg_kind);
    XV2_CHECK_ARG(n >= 1 && n <= MAX_T, "calibrate_hist: %d thresholds, must be 1..%d", n, MAX_T);
    XV2_CHECK_ARG(S >= 1 && S <= MAX_S, "calibrate_hist: %d scale vectors, must be 1..%d per call", S, MAX_S);
    XV2_CHECK_ARG(scales || S == 1, "calibrate_hist: S=%d without a scale table (NULL means one unscaled pass)", S);
    XV2_CHECK_ARG(!scales || dmg_kind != XV2_DMG_LABEL,
                  "calibrate_hist: class scales need damage probabilities, a label map has none to scale");
    XV2_CHECK_ARG(loc && dmg && lt && dt && thresholds && hist && bad, "calibrate_hist: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(xv2::cdiv(hw, PX_PER_BLOCK), xv2::cdiv(TARGET_BLOCKS, (int64_t)B * S)));
    const dim3 grid(gx, B, S);
    const double bytes = (double)B * hw * S * (6 + (dmg_kind == XV2_DMG_4CH ? 16 : dmg_kind == XV2_DMG_5CH ? 20 : 4));
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    unsigned long long* bd = reinterpret_cast<unsigned long long*>(bad);
#define CAL_LAUNCH(KIND)                                                                                               \
    XV2_LAUNCH(cal_kid(), bytes, calibrate_hist_kernel<KIND>, grid, dim3(256), 0, st, loc, dmg, lt, dt, hw, thresholds, n, \
               scales, h, bd, g_rounds)
    if (dmg_kind == XV2_DMG_4CH) CAL_LAUNCH(K_4CH);
    else if (dmg_kind == XV2_DMG_5CH) CAL_LAUNCH(K_5CH);
    else CAL_LAUNCH(K_LABEL);
#undef CAL_LAUNCH
    return XV2_OK;
}
