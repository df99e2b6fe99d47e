// "lovasz": the Lovasz-softmax loss (Berman et al., CVPR 2018, Algorithm 1) with classes = "present" and per_image = False:
// the whole batch is one set per class.
//
// For a class c over the M considered pixels, fg_i says whether pixel i has label c and the error is e_i = 1 - p_i(c) if fg_i,
// else p_i(c), p the channel softmax.  With the errors in descending order, loss_c = sum_j e_(j) (J_j - J_(j-1)), J_j the
// Jaccard loss of the first j entries.  The increments have closed forms, so a pixel's weight needs only rank counts against
// the sorted foreground and background errors (G foreground pixels; B_>(v) background errors > v; b background errors == v;
// F_>=(v) foreground errors >= v):
//   foreground, error v:  w = 1 / (G + B_>(v))
//   background, error v:  w = (G - F_>=(v)) / ((G + B_>(v)) (G + B_>(v) + b))
// Among equal errors the foreground comes first and tied background pixels share their telescoped sum equally
// (1 / (G + B_>) - 1 / (G + B_> + b) over b entries): the mean over every order of the tied group, a valid subgradient that
// depends on no order.  loss_c = sum e w; the term is the mean of loss_c over the classes in `class_mask` with G > 0, or 0.
//
// One KEY sort per class gives both sorted sets: errors are non-negative, so key = bits(e) | fg << 31 (e canonical: zero is
// +0, NaN the one pattern 0x7fc00000, above 1.0), skipped pixels (post, label 0) the sentinel 0xFFFFFFFF.  Ascending, a row is
// background ascending, foreground ascending, skipped.
//
// Passes (caller's stream, nothing returns to the host, launch count independent of the shape):
//   1. lovasz_key_kernel     keys [C][N H W], per-block integer counts of foreground and skipped pixels per class
//   2. lovasz_count_kernel   the counts added up -> records [C][4] = G, Nb, skipped, included-and-present
//   3. xv2_sort_u32          the rows of the lowest to the highest included class (12 launches)
//   4. lovasz_sum_kernel     over sorted positions: a background entry knows its rank from its position and finds F_>= by a
//                            lower bound in the foreground segment, a foreground entry B_> by an upper bound in the background
//                            segment; e * w in fp64, fp64 partials per block
//   5. lovasz_finish_kernel  the partials in a fixed order, the mean over present classes
// Backward is one pass: per pixel and class it reads the SAVED key (a recomputed error may round differently and land on the
// other side of a neighbour), binary-searches the class's sorted row (the first steps on samples of the row that the block
// keeps in LDS), forms w as above and writes
//   dlogit_k = gscale * p_k (g_k - sum_c g_c p_c),  g_c = -w / n_present (foreground), +w / n_present (background).
#include "xv2_common.h"
#include "loss_px.h"
#include <algorithm>

namespace xv2 {

constexpr unsigned LOV_NAN = 0x7fc00000u, LOV_SIGN = 0x80000000u, LOV_SKIP = 0xffffffffu;
constexpr int LOV_REC = 4;               // int32 per class: G, Nb, skipped, included-and-present
constexpr int LOV_NPRESENT = 4;          // sums[0 .. C) the class losses, sums[4] the number of present classes
constexpr int LOV_CHUNK = 1024;          // entries per block below the caps
constexpr int LOV_KEY_BLOCKS = 1024, LOV_SUM_BLOCKS = 2048;

static inline int lov_blocks(int64_t total, int cap) { return (int)std::min<int64_t>(std::max<int64_t>(cdiv(total, LOV_CHUNK), 1), cap); }

// first index in [lo, hi) whose key is >= v (lower) / > v (upper); hi when there is none
__device__ __forceinline__ int lov_lower(const unsigned* __restrict__ S, int lo, int hi, unsigned v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (S[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int lov_upper(const unsigned* __restrict__ S, int lo, int hi, unsigned v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (S[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// S: a class's sorted row, background keys in [0, Nb), foreground keys (sign bit set) in [Nb, Nb + G); v: error bits.
// hi: the first background position whose key is > v
__device__ __forceinline__ double lov_fg_weight(int G, int Nb, int hi) { return 1.0 / (double)(G + Nb - hi); }
// [lo, hi): the positions of the background keys equal to v; fl: the first foreground position whose error is >= v
__device__ __forceinline__ double lov_bg_weight(int G, int Nb, int lo, int hi, int fl) {
    const int bgt = Nb - hi, b = hi - lo, fge = G - (fl - Nb);
    return (double)(G - fge) / ((double)(G + bgt) * (double)(G + bgt + b));
}

// The backward pass looks every pixel up in its class's sorted row.  The first ten steps of each search run in LDS, on
// LOV_SAMPLES keys taken at even distances from the segment: smp[k] = S[base + k * n / LOV_SAMPLES].
constexpr int LOV_SAMPLES = 1024;
__device__ __forceinline__ int lov_sample_pos(int k, int n) { return (int)((int64_t)k * n / LOV_SAMPLES); }
// lower (UPPER: upper) bound of v in the segment S[base, base + n), as an index into S
template <bool UPPER>
__device__ __forceinline__ int lov_bound(const unsigned* __restrict__ S, int base, int n, const unsigned* smp, unsigned v) {
    if (n == 0) return base;
    int lo = 0, hi = LOV_SAMPLES;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (UPPER ? smp[mid] <= v : smp[mid] < v) lo = mid + 1; else hi = mid;
    }
    // every key up to sample lo - 1 is on the left of the bound, sample lo itself is not
    const int b = lo == LOV_SAMPLES ? n : lov_sample_pos(lo, n);
    const int a = lo == 0 ? 0 : min(lov_sample_pos(lo - 1, n) + 1, b);
    return UPPER ? lov_upper(S, base + a, base + b, v) : lov_lower(S, base + a, base + b, v);
}

// workspace: [sum partials: C * LOV_SUM_BLOCKS doubles][count partials: LOV_KEY_BLOCKS * (C + 1) int32][the sort's]
struct LovWs {
    double* part;
    int* cnt;
    void* sort;
};
static inline LovWs lov_ws(void* ws, int C) {
    LovWs o;
    o.part = reinterpret_cast<double*>(ws);
    o.cnt = reinterpret_cast<int*>(o.part + (size_t)C * LOV_SUM_BLOCKS);
    o.sort = o.cnt + (size_t)LOV_KEY_BLOCKS * (C + 1);
    return o;
}

// grid B: block b owns entries [b * chunk, (b + 1) * chunk) of the N H W pixels
template <int C>
__global__ void __launch_bounds__(256) lovasz_key_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                         int N, int H, int W, int ls, int post, int64_t chunk,
                                                         unsigned* __restrict__ keys, int* __restrict__ cnt_part) {
    __shared__ int sh[4][C + 1];
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const int64_t i0 = blockIdx.x * chunk, i1 = min(i0 + chunk, total);
    int g[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) g[c] = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const Px px = px_decode<C>(i, hw, W);
        const int y = label_at(labels, px.n, px.h, px.w, H, W, ls);
        float p[C], lse;
        softmax_px<C>(logits, px.base, hw, p, lse);
        const bool skip = post && y == 0;
        const int cls = post ? y - 1 : y;
        g[C] += skip ? 1 : 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            unsigned key = LOV_SKIP;
            if (!skip) {
                const bool fg = cls == c;
                float e = fg ? 1.f - p[c] : p[c];
                // canonical form for the sort: NaN is ONE pattern above 1.0, zero is +0 (never -0, never below zero)
                if (!(e > 0.f)) e = (e != e) ? __uint_as_float(LOV_NAN) : 0.f;
                key = __float_as_uint(e) | (fg ? LOV_SIGN : 0u);
                g[c] += fg ? 1 : 0;
            }
            keys[c * total + i] = key;
        }
    }
    block_sum_store(g, sh, cnt_part + (size_t)blockIdx.x * (C + 1));
}

// one block: the B partial counts in a fixed order -> records
__global__ void __launch_bounds__(256) lovasz_count_kernel(const int* __restrict__ cnt_part, int B, int C, int64_t total,
                                                           unsigned class_mask, int* __restrict__ rec) {
    __shared__ int sh[5][4];
    int a[5] = {0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < B; b += 256)
        for (int c = 0; c <= C; ++c) a[c] += cnt_part[(size_t)b * (C + 1) + c];
    for (int c = 0; c <= C; ++c) {
        const int v = wave_sum(a[c]);
        if ((threadIdx.x & 63) == 0) sh[c][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x >= C) return;
    const int c = threadIdx.x;
    const int G = sh[c][0] + sh[c][1] + sh[c][2] + sh[c][3];
    const int skipped = sh[C][0] + sh[C][1] + sh[C][2] + sh[C][3];
    rec[c * LOV_REC + 0] = G;
    rec[c * LOV_REC + 1] = (int)(total - G - skipped);
    rec[c * LOV_REC + 2] = skipped;
    rec[c * LOV_REC + 3] = (((class_mask >> c) & 1u) && G > 0) ? 1 : 0;
}

// grid (B, classes c0 .. c1): block b owns sorted positions [b * chunk, (b + 1) * chunk) of class c0 + blockIdx.y.  The keys of
// a chunk are ascending, so what its first and its last entry find in the other segment bounds every search in between.
__global__ void __launch_bounds__(256) lovasz_sum_kernel(const unsigned* __restrict__ sorted, int64_t total, int64_t chunk, int c0,
                                                         const int* __restrict__ rec, double* __restrict__ part) {
    __shared__ double sh[4][1];
    __shared__ int rng[4];
    const int c = c0 + blockIdx.y;
    const int G = rec[c * LOV_REC], Nb = rec[c * LOV_REC + 1];
    const unsigned* S = sorted + (size_t)c * total;
    double a[1] = {0.0};
    if (rec[c * LOV_REC + 3]) {            // the same for the whole block
        const int64_t j0 = blockIdx.x * chunk, j1 = min(j0 + chunk, (int64_t)Nb + G);
        const int64_t b1 = min(j1, (int64_t)Nb), f0 = max(j0, (int64_t)Nb);
        if (threadIdx.x == 0 && j0 < b1) {
            rng[0] = lov_lower(S, Nb, Nb + G, S[j0] | LOV_SIGN);
            rng[1] = lov_lower(S, Nb, Nb + G, S[b1 - 1] | LOV_SIGN);
        }
        if (threadIdx.x == 64 && f0 < j1) {
            rng[2] = lov_upper(S, 0, Nb, S[f0] & ~LOV_SIGN);
            rng[3] = lov_upper(S, 0, Nb, S[j1 - 1] & ~LOV_SIGN);
        }
        __syncthreads();
        for (int64_t jj = j0 + threadIdx.x; jj < j1; jj += 256) {
            const int j = (int)jj;
            const unsigned key = S[j];
            double w;
            if (j < Nb) {
                // the tied group around j: its neighbours say whether there is one at all
                int lo = j, hi = j + 1;
                if (j > 0 && S[j - 1] == key) lo = lov_lower(S, 0, j, key);
                if (j + 1 < Nb && S[j + 1] == key) hi = lov_upper(S, j + 1, Nb, key);
                w = lov_bg_weight(G, Nb, lo, hi, lov_lower(S, rng[0], rng[1], key | LOV_SIGN));
            } else {
                w = lov_fg_weight(G, Nb, lov_upper(S, rng[2], rng[3], key & ~LOV_SIGN));
            }
            a[0] += (double)__uint_as_float(key & ~LOV_SIGN) * w;
        }
    }
    block_sum_store(a, sh, part + (size_t)c * gridDim.x + blockIdx.x);
}

// one block: each class's partials, strided over the threads and then across them in a fixed order; the mean over present classes
__global__ void __launch_bounds__(256) lovasz_finish_kernel(const double* __restrict__ part, int B, int C,
                                                            const int* __restrict__ rec, double* __restrict__ sums,
                                                            float* __restrict__ loss) {
    __shared__ double sh[4][4];
    for (int c = 0; c < 4; ++c) strided_wave_total(part + (size_t)c * B, (c < C && rec[c * LOV_REC + 3]) ? B : 0, 1, sh[c]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    int np = 0;
    for (int k = 0; k < LOV_NPRESENT; ++k) {
        const double lc = wave4_total(sh[k]);
        sums[k] = lc;
        if (k < C && rec[k * LOV_REC + 3]) {
            tot += lc;
            ++np;
        }
    }
    sums[LOV_NPRESENT] = (double)np;
    loss[0] = np > 0 ? (float)(tot / (double)np) : 0.f;
}

template <int C>
__global__ void __launch_bounds__(256) lovasz_bwd_kernel(const float* __restrict__ logits, int64_t hw, int64_t total,
                                                         const unsigned* __restrict__ keys, const unsigned* __restrict__ sorted,
                                                         const int* __restrict__ rec, const double* __restrict__ sums,
                                                         const float* __restrict__ gscale, float* __restrict__ dlogits) {
    __shared__ unsigned smp[C][2][LOV_SAMPLES];      // per class: samples of the background and of the foreground segment
    const double np = sums[LOV_NPRESENT];
    const float gs = gscale[0];
    int G[C], Nb[C];
    bool on[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        G[c] = rec[c * LOV_REC];
        Nb[c] = rec[c * LOV_REC + 1];
        on[c] = rec[c * LOV_REC + 3] != 0;
        if (!on[c]) continue;
        const unsigned* S = sorted + (size_t)c * total;
        for (int k = threadIdx.x; k < LOV_SAMPLES; k += 256) {
            smp[c][0][k] = Nb[c] > 0 ? S[lov_sample_pos(k, Nb[c])] : 0u;
            smp[c][1][k] = S[Nb[c] + lov_sample_pos(k, G[c])];
        }
    }
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / hw, q = i - n * hw;
        const int64_t base = n * C * hw + q;
        float g[C];
        bool any = false;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = 0.f;
            if (!on[c]) continue;
            const unsigned key = keys[c * total + i];
            if (key == LOV_SKIP) continue;
            const unsigned* S = sorted + (size_t)c * total;
            const unsigned v = key & ~LOV_SIGN;
            double w;
            if (key & LOV_SIGN) {
                w = -lov_fg_weight(G[c], Nb[c], lov_bound<true>(S, 0, Nb[c], smp[c][0], v));
            } else {
                // the key itself is in the row: S[lo] == v; only a tied group needs the second search
                const int lo = lov_bound<false>(S, 0, Nb[c], smp[c][0], v);
                const int hi = (lo + 1 < Nb[c] && S[lo + 1] == v) ? lov_bound<true>(S, 0, Nb[c], smp[c][0], v) : lo + 1;
                w = lov_bg_weight(G[c], Nb[c], lo, hi, lov_bound<false>(S, Nb[c], G[c], smp[c][1], key | LOV_SIGN));
            }
            g[c] = (float)(w / np);
            any = true;
        }
        if (!any) {
            zero_px<C>(dlogits, base, hw);
            continue;
        }
        float p[C], lse;
        softmax_px<C>(logits, base, hw, p, lse);
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dot += g[c] * p[c];
#pragma unroll
        for (int c = 0; c < C; ++c) dlogits[base + c * hw] = gs * p[c] * (g[c] - dot);
    }
}

enum { K_KEY, K_COUNT, K_SUM, K_FINISH, K_BWD };
static int lov_kid(int k) {
    static const int ids[] = {prof_register("lovasz_key_kernel"), prof_register("lovasz_count_kernel"),
                              prof_register("lovasz_sum_kernel"), prof_register("lovasz_finish_kernel"),
                              prof_register("lovasz_bwd_kernel")};
    return ids[k];
}

static int lov_check(int N, int C, int H, int W, int lstride, int64_t& total) {
    if (int rc = loss_check("lovasz", N, C, H, W, lstride)) return rc;
    total = (int64_t)N * H * W;
    XV2_CHECK_ARG(total < ((int64_t)1 << 30), "lovasz: N*H*W=%lld entries unsupported (< 2^30)", (long long)total);
    return XV2_OK;
}

// the rows the sort covers: the lowest to the highest class of the mask
static inline void lov_span(unsigned mask, int& c0, int& c1) {
    c0 = 0;
    while (!((mask >> c0) & 1u)) ++c0;
    c1 = c0;
    for (int c = c0 + 1; c < 4; ++c)
        if ((mask >> c) & 1u) c1 = c;
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_lovasz_workspace(int N, int C, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (C != 2 && C != 4)) return 0;
    const int64_t total = (int64_t)N * H * W;
    if (total >= ((int64_t)1 << 30)) return 0;
    return (size_t)C * LOV_SUM_BLOCKS * sizeof(double) + (size_t)LOV_KEY_BLOCKS * (C + 1) * sizeof(int) +
           xv2_sort_workspace(C, total);
}

extern "C" int xv2_lovasz_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride, int post,
                                  unsigned class_mask, uint32_t* keys, uint32_t* sorted, int* records, double* sums, float* loss,
                                  void* workspace, void* stream) {
    int64_t total = 0;
    if (int rc = lov_check(N, C, H, W, lstride, total)) return rc;
    XV2_CHECK_ARG(class_mask != 0u && class_mask < (1u << C), "lovasz: class_mask=0x%x names no class or one beyond C=%d",
                  class_mask, C);
    hipStream_t st = (hipStream_t)stream;
    const LovWs ws = lov_ws(workspace, C);
    const int Bk = lov_blocks(total, LOV_KEY_BLOCKS), Bs = lov_blocks(total, LOV_SUM_BLOCKS);
    const double npx = (double)total;
    XV2_DISPATCH_C24(C, XV2_LAUNCH(lov_kid(K_KEY), npx * (8 * C + 1), lovasz_key_kernel<CC>, dim3(Bk), dim3(256), 0, st, logits, labels,
                                   N, H, W, lstride, post, cdiv(total, Bk), keys, ws.cnt));
    XV2_LAUNCH(lov_kid(K_COUNT), 4.0 * Bk * (C + 1), lovasz_count_kernel, dim3(1), dim3(256), 0, st, ws.cnt, Bk, C, total, class_mask,
               records);
    int c0, c1;
    lov_span(class_mask, c0, c1);
    const int R = c1 - c0 + 1;
    if (int rc = xv2_sort_u32(keys + (size_t)c0 * total, sorted + (size_t)c0 * total, R, total, ws.sort, stream)) return rc;
    XV2_LAUNCH(lov_kid(K_SUM), npx * R * 4, lovasz_sum_kernel, dim3(Bs, R), dim3(256), 0, st, sorted, total, cdiv(total, Bs), c0, records,
               ws.part);
    XV2_LAUNCH(lov_kid(K_FINISH), 8.0 * Bs * R, lovasz_finish_kernel, dim3(1), dim3(256), 0, st, ws.part, Bs, C, records, sums, loss);
    return XV2_OK;
}

extern "C" int xv2_lovasz_backward(const float* logits, int N, int C, int H, int W, const uint32_t* keys, const uint32_t* sorted,
                                   const int* records, const double* sums, const float* gscale, float* dlogits, void* stream) {
    int64_t total = 0;
    if (int rc = lov_check(N, C, H, W, 1, total)) return rc;      // (the backward pass reads no label)
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    // 8 pixels per thread and more on large inputs: a block fills its sample tables once
    const int grid = (int)std::min<int64_t>(cdiv(total, 2048), 2048);
    const double bytes = (double)total * (8 * C + 4 * C);
    XV2_DISPATCH_C24(C, XV2_LAUNCH(lov_kid(K_BWD), bytes, lovasz_bwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, hw, total, keys,
                                   sorted, records, sums, gscale, dlogits));
    return XV2_OK;
}
