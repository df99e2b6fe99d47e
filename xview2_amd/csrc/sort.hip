// xv2_sort_u32: R independent rows of M uint32 keys, ascending, on the caller's stream.  A least-significant-digit radix
// sort with 8-bit digits: 4 passes of 3 launches each, whatever R and M; rows ride on gridDim.y; nothing returns to the host.
//
// A row is cut into tiles of SORT_TILE keys; block b of a row owns the tpb consecutive tiles [b * tpb, (b + 1) * tpb) (tpb = 1
// up to SORT_MAX_BLOCKS tiles, so the (digit, block) table stays small however long the row is).  Per pass:
//   1. sort_hist_kernel     the block counts the pass's digit over its tiles in LDS (integer adds: order-free) and stores its
//                           256 counts into table[row][digit][block]
//   2. sort_scan_kernel     grid (256 digits, R): exclusive scan of table[row][digit][.] in place, the digit's total aside
//   3. sort_scatter_kernel  the block scans the 256 totals into digit bases, adds its own table entry, and walks its tiles in
//                           order, 256 keys (one per thread) at a time.  The rank of a key among the equal digits of its
//                           256 is STABLE: inside the wave the lanes below it with the same digit (__ballot per digit bit,
//                           64-bit masks, popcount), plus the counts of the waves before it, plus the digit's running
//                           offset in LDS, which moves on after every 256 keys.  No atomic takes part in a position, so
//                           equal digits keep the order the earlier passes gave them, which is what makes the LSD sort right.
// Kernel boundaries are the only hand-off between blocks.  The sorted order of a key-only sort is unique: every call gives the
// same bits.  Buffers alternate keys -> tmp -> out -> tmp -> out, so `out` may be `keys`.
#include "xv2_common.h"
#include <algorithm>

namespace xv2 {

constexpr int SORT_THREADS = 256;
constexpr int SORT_KPT = 8;                               // keys per thread and tile, loaded before the first is ranked
constexpr int SORT_TILE = SORT_THREADS * SORT_KPT;        // 2048
constexpr int SORT_MAX_BLOCKS = 1024;                     // per row
constexpr int SORT_DIGITS = 256;
constexpr int SORT_PASSES = 4;

struct SortPlan {
    int ntiles, tpb, nb;
};
static inline SortPlan sort_plan(int64_t M) {
    SortPlan p;
    p.ntiles = (int)cdiv(M, SORT_TILE);
    p.tpb = (int)cdiv(p.ntiles, SORT_MAX_BLOCKS);
    p.nb = (int)cdiv(p.ntiles, p.tpb);
    return p;
}

// inclusive scan of one int per thread over the block's 256 threads; s is 256 ints of LDS, free on entry and on return
__device__ __forceinline__ int block_scan_incl(int v, int* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < SORT_THREADS; off <<= 1) {
        const int x = t >= off ? s[t - off] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    const int r = s[t];
    __syncthreads();
    return r;
}

// grid (nb, R)
__global__ void __launch_bounds__(SORT_THREADS) sort_hist_kernel(const unsigned* __restrict__ in, int64_t M, int tpb,
                                                                  int shift, int* __restrict__ table) {
    __shared__ int h[SORT_DIGITS];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const unsigned* row = in + (size_t)blockIdx.y * M;
    const int64_t q0 = (int64_t)blockIdx.x * tpb * SORT_TILE, q1 = min(q0 + (int64_t)tpb * SORT_TILE, M);
    for (int64_t q = q0 + t; q < q1; q += SORT_THREADS) atomicAdd(&h[(row[q] >> shift) & 255u], 1);
    __syncthreads();
    table[((size_t)blockIdx.y * SORT_DIGITS + t) * gridDim.x + blockIdx.x] = h[t];
}

// grid (256, R): table[row][digit][0 .. nb) -> its exclusive prefix sums, totals[row][digit] = the sum.  nb <= 1024: four
// consecutive entries per thread.
__global__ void __launch_bounds__(SORT_THREADS) sort_scan_kernel(int* __restrict__ table, int nb, int* __restrict__ totals) {
    __shared__ int s[SORT_THREADS];
    const int t = threadIdx.x;
    int* row = table + ((size_t)blockIdx.y * SORT_DIGITS + blockIdx.x) * nb;
    const int per = (nb + SORT_THREADS - 1) / SORT_THREADS;
    int v[SORT_MAX_BLOCKS / SORT_THREADS], sum = 0;
#pragma unroll
    for (int j = 0; j < SORT_MAX_BLOCKS / SORT_THREADS; ++j) {
        const int i = t * per + j;
        v[j] = (j < per && i < nb) ? row[i] : 0;
        sum += v[j];
    }
    const int incl = block_scan_incl(sum, s);
    int run = incl - sum;
#pragma unroll
    for (int j = 0; j < SORT_MAX_BLOCKS / SORT_THREADS; ++j) {
        const int i = t * per + j;
        if (j < per && i < nb) row[i] = run;
        run += v[j];
    }
    if (t == SORT_THREADS - 1) totals[blockIdx.y * SORT_DIGITS + blockIdx.x] = incl;
}

// grid (nb, R)
__global__ void __launch_bounds__(SORT_THREADS) sort_scatter_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out,
                                                                     int64_t M, int ntiles, int tpb, int shift,
                                                                     const int* __restrict__ table,
                                                                     const int* __restrict__ totals) {
    __shared__ int off[SORT_DIGITS];            // where the next key of each digit goes
    __shared__ int wcnt[4][SORT_DIGITS];        // keys of each digit in each wave's 64 of the current 256
    __shared__ int s[SORT_THREADS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    {
        const int tot = totals[blockIdx.y * SORT_DIGITS + t];
        const int incl = block_scan_incl(tot, s);
        off[t] = incl - tot + table[((size_t)blockIdx.y * SORT_DIGITS + t) * gridDim.x + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
    }
    __syncthreads();
    const unsigned* src = in + (size_t)blockIdx.y * M;
    unsigned* dst = out + (size_t)blockIdx.y * M;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int tile0 = (int)blockIdx.x * tpb, tile1 = min(tile0 + tpb, ntiles);
    for (int tile = tile0; tile < tile1; ++tile) {
        const int64_t base = (int64_t)tile * SORT_TILE;
        unsigned k[SORT_KPT];
#pragma unroll
        for (int j = 0; j < SORT_KPT; ++j) {
            const int64_t q = base + j * SORT_THREADS + t;
            k[j] = q < M ? src[q] : 0u;
        }
#pragma unroll
        for (int j = 0; j < SORT_KPT; ++j) {
            if (base + j * SORT_THREADS >= M) break;      // the same for the whole block
            const bool valid = base + j * SORT_THREADS + t < M;
            const unsigned d = (k[j] >> shift) & 255u;
            unsigned long long m = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long b = __ballot(one);
                m &= one ? b : ~b;
            }
            const int rank = __popcll(m & below);
            if (valid && rank == 0) wcnt[wv][d] = __popcll(m);
            __syncthreads();
            if (valid) {
                int pos = off[d] + rank;
                for (int w = 0; w < wv; ++w) pos += wcnt[w][d];
                dst[pos] = k[j];
            }
            __syncthreads();
            off[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
#pragma unroll
            for (int w = 0; w < 4; ++w) wcnt[w][t] = 0;
            __syncthreads();
        }
    }
}

enum { K_HIST, K_SCAN, K_SCATTER };
static int sort_kid(int k) {
    static const int ids[] = {prof_register("sort_hist_kernel"), prof_register("sort_scan_kernel"),
                              prof_register("sort_scatter_kernel")};
    return ids[k];
}

static bool sort_shape_ok(int R, int64_t M) { return R >= 1 && R <= 65535 && M >= 1 && M < ((int64_t)1 << 30); }

}  // namespace xv2

using namespace xv2;

// workspace: [tmp: R*M uint32][table: R*256*nb int32][totals: R*256 int32]
extern "C" size_t xv2_sort_workspace(int R, int64_t M) {
    if (!sort_shape_ok(R, M)) return 0;
    const SortPlan p = sort_plan(M);
    return ((size_t)R * M + (size_t)R * SORT_DIGITS * p.nb + (size_t)R * SORT_DIGITS) * sizeof(int);
}

extern "C" int xv2_sort_u32(const uint32_t* keys, uint32_t* out, int R, int64_t M, void* workspace, void* stream) {
    XV2_CHECK_ARG(sort_shape_ok(R, M), "sort_u32: R=%d rows of %lld keys unsupported (1 <= R <= 65535, 1 <= keys < 2^30)", R,
                  (long long)M);
    XV2_CHECK_ARG(keys != nullptr && out != nullptr && workspace != nullptr, "sort_u32: keys, out or workspace is NULL");
    hipStream_t st = (hipStream_t)stream;
    const SortPlan p = sort_plan(M);
    unsigned* tmp = reinterpret_cast<unsigned*>(workspace);
    int* table = reinterpret_cast<int*>(tmp + (size_t)R * M);
    int* totals = table + (size_t)R * SORT_DIGITS * p.nb;
    const dim3 grid(p.nb, R);
    const double kb = 4.0 * R * M, tb = 4.0 * R * SORT_DIGITS * p.nb;
    const unsigned* src = keys;
    for (int pass = 0; pass < SORT_PASSES; ++pass) {
        unsigned* dst = (pass & 1) ? out : tmp;
        const int shift = 8 * pass;
        XV2_LAUNCH(sort_kid(K_HIST), kb + tb, sort_hist_kernel, grid, dim3(SORT_THREADS), 0, st, src, M, p.tpb, shift, table);
        XV2_LAUNCH(sort_kid(K_SCAN), 2.0 * tb, sort_scan_kernel, dim3(SORT_DIGITS, R), dim3(SORT_THREADS), 0, st, table, p.nb, totals);
        XV2_LAUNCH(sort_kid(K_SCATTER), 2.0 * kb + tb, sort_scatter_kernel, grid, dim3(SORT_THREADS), 0, st, src, dst, M, p.ntiles, p.tpb,
                   shift, table, totals);
        src = dst;
    }
    return XV2_OK;
}
