// "ohem_hard": online hard example mining (arXiv 1812.05802) as model/loss.py:24-51 reads once the k hardest negatives
// are really selected (the reference slices the (values, indices) tuple of sort, so its "ohem" keeps every negative;
// that stays XV2_LOSS_CE in loss.hip).
//
// Per image i, with l = logsumexp(x) - x[y] per pixel: positives (y > 0) are all kept, of the Cn negatives (y == 0)
// the k = min(Cn, max(Cn / 4, 5, 2 Cp)) with the largest l.  loss = sum_i (sum l over positives + sum of the k largest
// negative l) / sum_i (Cp + k).
//
// Passes (all on the caller's stream, nothing returns to the host, launch count independent of N):
//   1. ohem_px_kernel    l of every pixel -> px_loss (positives: the sentinel -1), fp64 partial sums of the positives
//   2. 3 x (ohem_hist_kernel + ohem_scan_kernel)   exact k-th largest negative loss t per image: radix select over the
//      fp32 bit pattern (non-negative floats order like their bits; NaN above +Inf), digits of 11 / 11 / 10 bits from
//      the top.  A histogram block counts its chunk of one image in LDS (integer adds: order-free) and stores its
//      table; the scan block of the image adds the tables and walks down from the top bin to the one that holds the
//      k-th entry.  Kernel boundaries are the only hand-off.
//   3. ohem_sum_kernel   sum of the negatives above t, fp32 in a thread, fp64 across, fixed order
//   4. ohem_finish_kernel  + r * t per image (r = k - #{l > t} entries of the tied class {l == t} are kept), the loss
// Backward is one pass that reads px_loss and the record: it never recomputes l for the comparison against t (a second
// evaluation may contract differently and flip a pixel at the threshold).  Tie rule: every negative with l == t gets
// the weight r / c_eq - the mean over all valid choices of the tied subset, independent of any order.
#include "xv2_common.h"
#include "loss_px.h"
#include <algorithm>

namespace xv2 {

constexpr int OHEM_BINS = 2048;          // table stride of every stage (the last one uses 1024 of them)
constexpr int OHEM_MAX_BLOCKS = 128;     // histogram / sum blocks per image
constexpr int OHEM_CHUNK = 4096;         // pixels per block below that cap
constexpr int OHEM_REC = 8;              // int32 per image: Cp, Cn, k, bits(t), c_gt, c_eq, r, 0
constexpr unsigned OHEM_NAN = 0x7fc00000u;

static inline int ohem_blocks(int64_t M) { return (int)std::min<int64_t>(std::max<int64_t>(cdiv(M, OHEM_CHUNK), 1), OHEM_MAX_BLOCKS); }

// Sort key of a stored value: its bit pattern.  Entries with the sign bit set are not candidates (the sentinel of the
// positives), except -0.0, which is a zero.
__device__ __forceinline__ bool ohem_key(unsigned bits, unsigned& key) {
    if (bits == 0x80000000u) bits = 0u;
    key = bits;
    return (bits >> 31) == 0u;
}

// workspace: [pos partial: N*B doubles][neg partial: N*B doubles][tables: N*B*OHEM_BINS int32]
struct OhemWs {
    double* pos;
    double* neg;
    int* tables;
};
static inline OhemWs ohem_ws(void* ws, int N, int B) {
    OhemWs o;
    o.pos = reinterpret_cast<double*>(ws);
    o.neg = o.pos + (size_t)N * B;
    o.tables = reinterpret_cast<int*>(o.neg + (size_t)N * B);
    return o;
}

// grid (B, N): block b owns pixels [b * chunk, (b + 1) * chunk) of image n
template <int C>
__global__ void __launch_bounds__(256) ohem_px_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                       int H, int W, int ls, int64_t chunk, float* __restrict__ px_loss,
                                                       double* __restrict__ pos_part) {
    __shared__ double sh[4][1];
    const int64_t hw = (int64_t)H * W, n = blockIdx.y;
    const int64_t q0 = blockIdx.x * chunk, q1 = min(q0 + chunk, hw);
    float a[1] = {0.f};
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        int h, w;
        px_hw(q, W, h, w);
        const int y = label_at(labels, n, h, w, H, W, ls);
        const int64_t base = n * C * hw + q;
        float x[C], m = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            x[c] = logits[base + c * hw];
            m = fmaxf(m, x[c]);
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += expf(x[c] - m);
        // pick<C>(x, y), spelled out: handed to a function by reference, x[4] is kept in LDS and x[y] read back from there
        // (4 KB per block and a round trip per pixel at C = 4); this chain stays in registers
        float xy = x[0];
#pragma unroll
        for (int c = 1; c < C; ++c) xy = (y == c) ? x[c] : xy;
        // (m - x[y]) + log s, rounded once: the two terms are formed exactly in fp64
        float l = (float)(((double)m - (double)xy) + (double)logf(s));
        // canonical form for the select: NaN is ONE pattern above +Inf, zero is +0 (never -0, never below zero)
        if (!(l > 0.f)) l = (l != l) ? __uint_as_float(OHEM_NAN) : 0.f;
        if (y > 0) {
            a[0] += l;
            l = -1.f;
        }
        px_loss[n * hw + q] = l;
    }
    block_sum_store(a, sh, pos_part + (size_t)n * gridDim.x + blockIdx.x);
}

// grid (B, N).  STAGE 0 / 1 / 2 counts the digit at bits 31..21 / 20..10 / 9..0 of the candidates whose higher digits
// equal those of rec[3] (the prefix the earlier stages fixed).
template <int STAGE>
__global__ void __launch_bounds__(256) ohem_hist_kernel(const unsigned* __restrict__ vals, int64_t M, int64_t chunk,
                                                         const int* __restrict__ rec, int* __restrict__ tables) {
    __shared__ int h[OHEM_BINS];
    const int64_t n = blockIdx.y;
    for (int i = threadIdx.x; i < OHEM_BINS; i += 256) h[i] = 0;
    __syncthreads();
    const unsigned prefix = STAGE > 0 ? (unsigned)rec[n * OHEM_REC + 3] : 0u;
    const int64_t q0 = blockIdx.x * chunk, q1 = min(q0 + chunk, M);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
        unsigned key;
        if (!ohem_key(vals[n * M + q], key)) continue;
        unsigned d;
        if (STAGE == 0) {
            d = key >> 21;
        } else if (STAGE == 1) {
            if ((key >> 21) != (prefix >> 21)) continue;
            d = (key >> 10) & 2047u;
        } else {
            if ((key >> 10) != (prefix >> 10)) continue;
            d = key & 1023u;
        }
        atomicAdd(&h[d], 1);
    }
    __syncthreads();
    int* dst = tables + ((size_t)n * gridDim.x + blockIdx.x) * OHEM_BINS;
    for (int i = threadIdx.x; i < OHEM_BINS; i += 256) dst[i] = h[i];
}

// grid N, 1024 threads.  Adds the image's B tables, then finds the bin d with #{digit > d} < kr <= #{digit >= d} for the
// kr = k - c_gt entries still to place.  Stage 0 also fixes Cn (= the table's total), Cp and k; the last stage c_eq and r.
// kin == nullptr: Cp = M - Cn and k by the mining rule; else Cp = 0 and k = clamp(kin[n], 0, Cn).
__global__ void __launch_bounds__(1024) ohem_scan_kernel(const int* __restrict__ tables, int B, int64_t M,
                                                          const int* __restrict__ kin, int stage, int* __restrict__ rec) {
    __shared__ int h[OHEM_BINS];
    __shared__ int sfx[256];
    const int n = blockIdx.x, t = threadIdx.x;
    int* r = rec + (size_t)n * OHEM_REC;
    // read before the first barrier: the one thread that writes the record does so after the last
    int k = 0, cgt0 = 0;
    unsigned prefix0 = 0u;
    if (stage > 0) {
        k = r[2];
        prefix0 = (unsigned)r[3];
        cgt0 = r[4];
        if (k == 0) return;      // no candidates to place: stage 0 left the final record
    }
    int2 a = make_int2(0, 0);
    const int2* p = reinterpret_cast<const int2*>(tables + (size_t)n * B * OHEM_BINS) + t;
    for (int b = 0; b < B; ++b) {
        const int2 v = p[(size_t)b * (OHEM_BINS / 2)];
        a.x += v.x;
        a.y += v.y;
    }
    h[2 * t] = a.x;
    h[2 * t + 1] = a.y;
    __syncthreads();
    int own = 0;
    if (t < 256) {
#pragma unroll
        for (int j = 0; j < 8; ++j) own += h[8 * t + j];
        sfx[t] = own;
    }
    __syncthreads();
    // inclusive suffix sums over the 256 groups of 8 bins
    for (int off = 1; off < 256; off <<= 1) {
        int v = 0;
        if (t < 256 && t + off < 256) v = sfx[t + off];
        __syncthreads();
        if (t < 256) sfx[t] += v;
        __syncthreads();
    }
    if (t >= 256) return;
    int Cp = 0, Cn = 0;
    if (stage == 0) {
        Cn = sfx[0];
        if (kin) {
            k = min(max(kin[n], 0), Cn);
        } else {
            Cp = (int)(M - Cn);
            k = min(Cn, max(max(Cn / 4, 5), 2 * Cp));
        }
        if (k == 0) {
            if (t == 0) {
                r[0] = Cp;
                r[1] = Cn;
#pragma unroll
                for (int j = 2; j < OHEM_REC; ++j) r[j] = 0;
            }
            return;
        }
    }
    const int kr = k - cgt0;
    int above = sfx[t] - own;            // candidates in the groups above this one
    if (!(above < kr && kr <= above + own)) return;
    int d = 8 * t + 7, c = 0;
    for (; d >= 8 * t; --d) {
        c = h[d];
        if (above + c >= kr) break;
        above += c;
    }
    const int sh = stage == 0 ? 21 : (stage == 1 ? 10 : 0);
    const int cgt = cgt0 + above;
    if (stage == 0) {
        r[0] = Cp;
        r[1] = Cn;
        r[2] = k;
    }
    r[3] = (int)(prefix0 | ((unsigned)d << sh));
    r[4] = cgt;
    r[5] = stage == 2 ? c : 0;
    r[6] = stage == 2 ? k - cgt : 0;
    r[7] = 0;
}

// grid (B, N): fp64 partial sum of the image's candidates above its threshold
__global__ void __launch_bounds__(256) ohem_sum_kernel(const unsigned* __restrict__ vals, int64_t M, int64_t chunk,
                                                        const int* __restrict__ rec, double* __restrict__ neg_part) {
    __shared__ double sh[4][1];
    const int64_t n = blockIdx.y;
    const int k = rec[n * OHEM_REC + 2];
    const unsigned tb = (unsigned)rec[n * OHEM_REC + 3];
    const int64_t q0 = blockIdx.x * chunk, q1 = min(q0 + chunk, M);
    float a[1] = {0.f};
    if (k > 0)
        for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
            unsigned key;
            if (ohem_key(vals[n * M + q], key) && key > tb) a[0] += __uint_as_float(key);
        }
    block_sum_store(a, sh, neg_part + (size_t)n * gridDim.x + blockIdx.x);
}

// one block: the partials strided over the threads, then 256 serial terms (this order is part of the result), r * t per image,
// the loss; sums = {positive sum, selected-negative sum, samples}
__global__ void __launch_bounds__(256) ohem_finish_kernel(const double* __restrict__ pos_part,
                                                           const double* __restrict__ neg_part, int nparts, int N,
                                                           const int* __restrict__ rec, double* __restrict__ sums,
                                                           float* __restrict__ loss) {
    __shared__ double sp[256], sn[256];
    double p = 0.0, g = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        p += pos_part[i];
        g += neg_part[i];
    }
    sp[threadIdx.x] = p;
    sn[threadIdx.x] = g;
    __syncthreads();
    if (threadIdx.x != 0) return;
    p = 0.0;
    g = 0.0;
    for (int i = 0; i < 256; ++i) {
        p += sp[i];
        g += sn[i];
    }
    double cnt = 0.0;
    for (int n = 0; n < N; ++n) {
        const int* r = rec + (size_t)n * OHEM_REC;
        if (r[2] > 0) g += (double)r[6] * (double)__uint_as_float((unsigned)r[3]);
        cnt += (double)r[0] + (double)r[2];
    }
    sums[0] = p;
    sums[1] = g;
    sums[2] = cnt;
    loss[0] = (float)((p + g) / cnt);
}

template <int C>
__global__ void __launch_bounds__(256) ohem_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                        int N, int H, int W, int ls, const unsigned* __restrict__ px_loss,
                                                        const int* __restrict__ rec, const double* __restrict__ sums,
                                                        const float* __restrict__ gscale, float* __restrict__ dlogits) {
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const float gs = gscale[0] * (float)(1.0 / sums[2]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        const int64_t n = px.n, base = px.base;
        unsigned key;
        int y = 0;
        float wgt;
        if (!ohem_key(px_loss[i], key)) {          // a positive: always kept
            y = label_at(labels, n, px.h, px.w, H, W, ls);
            wgt = 1.f;
        } else {
            const int* r = rec + n * OHEM_REC;
            const unsigned tb = (unsigned)r[3];
            wgt = (r[2] == 0 || key < tb) ? 0.f : (key > tb ? 1.f : (float)r[6] / (float)r[5]);
        }
        if (wgt == 0.f) {
            zero_px<C>(dlogits, base, hw);
            continue;
        }
        float p[C], lse;
        softmax_px<C>(logits, base, hw, p, lse);
        const float s = gs * wgt;
#pragma unroll
        for (int c = 0; c < C; ++c) dlogits[base + c * hw] = s * (p[c] - ((y == c) ? 1.f : 0.f));
    }
}

enum { K_PX, K_HIST, K_SCAN, K_SUM, K_FINISH, K_BWD };
static int ohem_kid(int k) {
    static const int ids[] = {prof_register("ohem_px_kernel"), prof_register("ohem_hist_kernel"), prof_register("ohem_scan_kernel"),
                              prof_register("ohem_sum_kernel"), prof_register("ohem_finish_kernel"), prof_register("ohem_bwd_kernel")};
    return ids[k];
}

static int ohem_select(const unsigned* vals, int N, int64_t M, const int* kin, int* rec, const OhemWs& ws, int B,
                       hipStream_t st) {
    const int64_t chunk = cdiv(M, B);
    const dim3 grid(B, N);
    const double tbl = (double)N * B * OHEM_BINS * sizeof(int);
    XV2_LAUNCH(ohem_kid(K_HIST), 4.0 * N * M + tbl, ohem_hist_kernel<0>, grid, dim3(256), 0, st, vals, M, chunk, rec, ws.tables);
    XV2_LAUNCH(ohem_kid(K_SCAN), tbl, ohem_scan_kernel, dim3(N), dim3(1024), 0, st, ws.tables, B, M, kin, 0, rec);
    XV2_LAUNCH(ohem_kid(K_HIST), 4.0 * N * M + tbl, ohem_hist_kernel<1>, grid, dim3(256), 0, st, vals, M, chunk, rec, ws.tables);
    XV2_LAUNCH(ohem_kid(K_SCAN), tbl, ohem_scan_kernel, dim3(N), dim3(1024), 0, st, ws.tables, B, M, kin, 1, rec);
    XV2_LAUNCH(ohem_kid(K_HIST), 4.0 * N * M + tbl, ohem_hist_kernel<2>, grid, dim3(256), 0, st, vals, M, chunk, rec, ws.tables);
    XV2_LAUNCH(ohem_kid(K_SCAN), tbl, ohem_scan_kernel, dim3(N), dim3(1024), 0, st, ws.tables, B, M, kin, 2, rec);
    return XV2_OK;
}

static int ohem_check_shape(int N, int64_t M) {
    XV2_CHECK_ARG(N >= 1 && N <= 65535 && M >= 1 && M < ((int64_t)1 << 30),
                  "ohem: N=%d images of %lld entries unsupported (1 <= N <= 65535, 1 <= entries < 2^30)", N, (long long)M);
    return XV2_OK;
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_ohem_workspace(int N, int64_t M) {
    if (N < 1 || M < 1) return 0;
    const size_t nb = (size_t)N * ohem_blocks(M);
    return nb * (2 * sizeof(double) + OHEM_BINS * sizeof(int));
}

extern "C" int xv2_topk_select(const float* values, int N, int64_t M, const int* k, int* records, void* workspace,
                               void* stream) {
    if (int rc = ohem_check_shape(N, M)) return rc;
    XV2_CHECK_ARG(k != nullptr, "topk_select: k is NULL");
    const int B = ohem_blocks(M);
    return ohem_select(reinterpret_cast<const unsigned*>(values), N, M, k, records, ohem_ws(workspace, N, B), B,
                       (hipStream_t)stream);
}

extern "C" int xv2_ohem_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                                float* px_loss, int* records, double* sums, float* loss, void* workspace, void* stream) {
    if (int rc = loss_check("ohem", N, C, H, W, lstride)) return rc;
    const int64_t M = (int64_t)H * W;
    if (int rc = ohem_check_shape(N, M)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int B = ohem_blocks(M);
    const int64_t chunk = cdiv(M, B);
    const OhemWs ws = ohem_ws(workspace, N, B);
    const dim3 grid(B, N);
    const double npx = (double)N * M;
    XV2_DISPATCH_C24(C, XV2_LAUNCH(ohem_kid(K_PX), npx * (4 * C + 5), ohem_px_kernel<CC>, grid, dim3(256), 0, st, logits, labels, H,
                                   W, lstride, chunk, px_loss, ws.pos));
    const unsigned* vals = reinterpret_cast<const unsigned*>(px_loss);
    if (int rc = ohem_select(vals, N, M, nullptr, records, ws, B, st)) return rc;
    XV2_LAUNCH(ohem_kid(K_SUM), npx * 4, ohem_sum_kernel, grid, dim3(256), 0, st, vals, M, chunk, records, ws.neg);
    XV2_LAUNCH(ohem_kid(K_FINISH), 16.0 * N * B, ohem_finish_kernel, dim3(1), dim3(256), 0, st, ws.pos, ws.neg, N * B, N, records, sums,
               loss);
    return XV2_OK;
}

extern "C" int xv2_ohem_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                                 const float* px_loss, const int* records, const double* sums, const float* gscale,
                                 float* dlogits, void* stream) {
    if (int rc = loss_check("ohem", N, C, H, W, lstride)) return rc;
    XV2_CHECK_ARG(logits && labels && px_loss && records && sums && gscale && dlogits, "ohem: null tensor");
    const int64_t M = (int64_t)H * W;
    if (int rc = ohem_check_shape(N, M)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * M;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), 4096);
    const unsigned* vals = reinterpret_cast<const unsigned*>(px_loss);
    const double bytes = (double)total * (8 * C + 4);
    XV2_DISPATCH_C24(C, XV2_LAUNCH(ohem_kid(K_BWD), bytes, ohem_bwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, labels, N, H,
                                   W, lstride, vals, records, sums, gscale, dlogits));
    return XV2_OK;
}
