// What the per-pixel loss kernels share (loss.hip, ohem.hip, lovasz.hip, wce.hip).  Device side: the walk from a flat pixel
// index to its image, row, column and label, the channel softmax of one NCHW pixel, the zero-gradient store, the select of a
// class's entry and the block sums.  Host side: the argument checks of an entry point and the C = 2 / 4 dispatch.
// What a term does with a label (clamp a class beyond C, drop it, count it) stays in the term's own file.
#pragma once
#include "xv2_common.h"

namespace xv2 {

// ---- the pixel walk ------------------------------------------------------------------------------------------------------
// index of the label (and of anything else kept at label resolution) behind pixel (n, h, w) of a head whose labels are
// ls times finer: deep supervision reads every ls-th label of every ls-th row
#define XV2_LABEL_INDEX(n, h, w, H, W, ls) (((n) * (int64_t)(H) * (ls) + (int64_t)(h) * (ls)) * ((int64_t)(W) * (ls)) + (int64_t)(w) * (ls))
__device__ __forceinline__ int64_t label_index(int64_t n, int h, int w, int H, int W, int ls) {
    return XV2_LABEL_INDEX(n, h, w, H, W, ls);
}
// the one spelling above, but inside the subscript and not label_index's value: only there does the compiler split the column
// term off the address and keep the rest in scalar registers; through label_index's value that arithmetic moves into the
// per-pixel vector code of every kernel that calls label_at
__device__ __forceinline__ int label_at(const uint8_t* __restrict__ labels, int64_t n, int h, int w, int H, int W,
                                        int ls) {
    return labels[XV2_LABEL_INDEX(n, h, w, H, W, ls)];
}

// pixel q of an image -> row and column
__device__ __forceinline__ void px_hw(int64_t q, int W, int& h, int& w) {
    h = (int)(q / W);
    w = (int)(q - (int64_t)h * W);
}
// pixel i of an [N][C][H][W] batch: image n, pixel q = h * W + w of it, base = the offset of its channel 0
struct Px {
    int64_t n, q, base;
    int h, w;
};
template <int C>
__device__ __forceinline__ Px px_decode(int64_t i, int64_t hw, int W) {
    Px p;
    p.n = i / hw;
    p.q = i - p.n * hw;
    px_hw(p.q, W, p.h, p.w);
    p.base = p.n * C * hw + p.q;
    return p;
}

template <int C>
__device__ __forceinline__ void softmax_px(const float* __restrict__ logits, int64_t base, int64_t hw, float* p,
                                           float& lse) {
    float l[C];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        l[c] = logits[base + c * hw];
        m = fmaxf(m, l[c]);
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        p[c] = expf(l[c] - m);
        s += p[c];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    lse = m + logf(s);
}

// a pixel that takes no part: zero gradient in every channel
template <int C>
__device__ __forceinline__ void zero_px(float* dlogits, int64_t base, int64_t hw) {
#pragma unroll
    for (int c = 0; c < C; ++c) dlogits[base + c * hw] = 0.f;
}

// v[c] as a chain of selects; c outside [1, C) gives v[0].  Where v is a per-thread array the compiler may still turn the
// chain into an indexed read of a copy in LDS (it does in wce's kernels at C = 4): see ohem_px_kernel before using it there
template <int C>
__device__ __forceinline__ float pick(const float (&v)[C], int c) {
    float r = v[0];
#pragma unroll
    for (int k = 1; k < C; ++k) r = (c == k) ? v[k] : r;
    return r;
}

// ---- block sums (256 threads = 4 waves; the order of every addition is part of the result) -------------------------------
// the type a thread's accumulator is added up in across lanes, waves and blocks
template <typename T> struct Wide { typedef T type; };
template <> struct Wide<float> { typedef double type; };

// K per-thread accumulators -> dst[0 .. K): widened, then added across the wave, then the four waves in order
template <int K, typename T>
__device__ __forceinline__ void block_sum_store(const T (&a)[K], typename Wide<T>::type (&sh)[4][K],
                                                typename Wide<T>::type* dst) {
    typedef typename Wide<T>::type WT;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const WT v = wave_sum((WT)a[k]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K)
        dst[threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

// one-block finish kernels: n partials src[b * stride], b strided over the 256 threads, then added across the wave; lane 0
// leaves its wave's sum in sh4[wave].  After a barrier wave4_total(sh4) is the block's total.
__device__ __forceinline__ void strided_wave_total(const double* src, int n, size_t stride, double* sh4) {
    double a = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) a += src[(size_t)b * stride];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = a;
}
__device__ __forceinline__ double wave4_total(const double* sh4) { return sh4[0] + sh4[1] + sh4[2] + sh4[3]; }

// ---- host side -----------------------------------------------------------------------------------------------------------
// what every per-pixel loss entry checks before its first launch; c_set: bit c set for every class count the entry takes.
// Limits that belong to one term (a 2^30 range, a 65535 grid) stay with the term.
constexpr unsigned LOSS_C24 = (1u << 2) | (1u << 4);
static inline int loss_check(const char* what, int N, int C, int H, int W, int lstride, unsigned c_set = LOSS_C24) {
    XV2_CHECK_ARG(C >= 0 && C < 32 && ((c_set >> C) & 1u), "%s: C=%d unsupported", what, C);
    XV2_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N=%d H=%d W=%d", what, N, H, W);
    XV2_CHECK_ARG(lstride >= 1, "%s: bad lstride=%d", what, lstride);
    return XV2_OK;
}

// run `call` with the constexpr int CC bound to 2 for C == 2 and to 4 otherwise: after loss_check(..., LOSS_C24) that is C
// itself; xv2_loss_backward, which also takes C = 1 and 3 for mse and coral, sends any other C with composed terms to 4
#define XV2_DISPATCH_C24(C, ...)                \
    do {                                        \
        if ((C) == 2) {                         \
            constexpr int CC = 2;               \
            __VA_ARGS__;                        \
        } else {                                \
            constexpr int CC = 4;               \
            __VA_ARGS__;                        \
        }                                       \
    } while (0)

}  // namespace xv2
