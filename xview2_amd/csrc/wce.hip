// "wce": cross-entropy with a per-pixel weight w(p) = cw[class(p)] + b(p) (include/xv2.h): class weights plus the border
// map of the U-Net paper (Ronneberger et al. 2015), b = w0 exp(-(d1 + d2)^2 / (2 sigma^2)) with d1 / d2 the distances from a
// background pixel to the nearest and the second-nearest building.
//
//   loss = sum_p w(p) l(p) / sum_p w(p),  l = logsumexp(x) - x[class];  dlogits = gscale w (softmax - onehot) / sum_p w
//
// Distances (xv2_border_distances): xv2_label_components numbers the 4-connected components of label > 0, then one block per
// 32 x 32 output tile stages the tile's (32 + 2R)^2 component labels in LDS (zero outside the image) and every thread scans the
// disc dy^2 + dx^2 <= R^2 around its background pixels, keeping the two smallest squared distances to two DIFFERENT
// components: (a1, L1), (a2, L2), L1 != L2.  A disc pixel of component L at squared distance d:
//   1. L == L1        a1 = min(a1, d)
//   2. else d < a1    (a2, L2) = (a1, L1), (a1, L1) = (d, L)
//   3. else L == L2   a2 = min(a2, d)
//   4. else d < a2    (a2, L2) = (d, L)
// a1 / a2 are then the smallest / second smallest of the per-component minima, whatever the scan order and whichever of two
// tied components is called nearest.  A pixel with d >= a2 changes nothing in any branch and is rejected first; behind that
// test rules 3 and 4 both end in a2 = d, so the kernel keeps no L2.  A tile whose window holds no building writes 0xFFFF
// without scanning.  Nothing is read back, the launches do not depend on the content.
//
// The weight itself is wce_px.h: one function for the map entry, the forward and the backward pass.
// Sums: fp32 inside a thread, fp64 across lanes, waves and blocks in a fixed order: two calls give the same bits.
#include "xv2_common.h"
#include "loss_px.h"
#include "wce_px.h"
#include <algorithm>
#include <cmath>

namespace xv2 {

constexpr int BT = 32;                  // output tile edge of the distance kernel
constexpr int BR_MAX = 32;              // largest radius: a window of 96 x 96 int32 = 36,864 bytes of LDS
constexpr int WCE_BLOCKS = 1024;        // cap of the forward grid-stride loop
constexpr int WCE_BWD_BLOCKS = 4096;
constexpr int BIG = 0x7fffffff;

// grid (tiles_x, tiles_y, B), 256 threads: thread t owns column t & 31 and rows (t >> 5) + 8 k, k < 4, of its tile
__global__ void __launch_bounds__(256) border_dist_kernel(const int32_t* __restrict__ comp, int H, int W, int R,
                                                          uint16_t* __restrict__ d1o, uint16_t* __restrict__ d2o) {
    extern __shared__ int win[];            // [S][S] component labels, origin (y0 - R, x0 - R)
    __shared__ int half[BR_MAX + 1];        // half[|dy|]: the largest |dx| inside the disc
    const int tid = threadIdx.x, S = BT + 2 * R;
    const int x0 = blockIdx.x * BT, y0 = blockIdx.y * BT;
    const int64_t base = (int64_t)blockIdx.z * H * W;
    int any = 0;
    for (int i = tid; i < S * S; i += 256) {
        const int wy = i / S, wx = i - wy * S;
        const int gy = y0 - R + wy, gx = x0 - R + wx;
        int L = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) L = comp[base + (int64_t)gy * W + gx];
        win[i] = L;
        any |= L;
    }
    if (tid <= R) {
        const int rem = R * R - tid * tid;
        int h = (int)sqrtf((float)rem);
        while (h * h > rem) --h;
        while ((h + 1) * (h + 1) <= rem) ++h;
        half[tid] = h;
    }
    any = __syncthreads_or(any);
    const int lx = tid & (BT - 1), x = x0 + lx;
    if (x >= W) return;
#pragma unroll 1
    for (int k = 0; k < BT * BT / 256; ++k) {
        const int ly = (tid >> 5) + 8 * k, y = y0 + ly;
        if (y >= H) break;
        const int64_t o = base + (int64_t)y * W + x;
        int a1 = BIG, a2 = BIG;
        if (any && win[(ly + R) * S + lx + R] == 0) {
            int L1 = 0;
            for (int dy = -R; dy <= R; ++dy) {
                const int h = half[dy < 0 ? -dy : dy], dy2 = dy * dy;
                const int* row = win + (ly + R + dy) * S + lx + R;
                for (int dx = -h; dx <= h; ++dx) {
                    const int L = row[dx];
                    const int d = dy2 + dx * dx;
                    if (L == 0 || d >= a2) continue;
                    if (L == L1) {
                        a1 = min(a1, d);
                    } else if (d < a1) {
                        a2 = a1;
                        a1 = d;
                        L1 = L;
                    } else {            // rules 3 and 4: d < a2 already
                        a2 = d;
                    }
                }
            }
        }
        d1o[o] = (uint16_t)(a1 == BIG ? WCE_NONE : (unsigned)a1);
        d2o[o] = (uint16_t)(a2 == BIG ? WCE_NONE : (unsigned)a2);
    }
}

__global__ void __launch_bounds__(256) border_weights_kernel(const uint16_t* __restrict__ d1, const uint16_t* __restrict__ d2,
                                                             int64_t n, float w0, float sigma, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = wce_border(d1[i], d2[i], w0, sigma);
}

// the pixel's class, or -1 for a pixel that takes no part (post: label 0; a class beyond C)
__device__ __forceinline__ int wce_class(int y, int post, int C) {
    if (post) y -= 1;
    return y < C ? y : -1;
}

template <int C>
__global__ void __launch_bounds__(256) wce_fwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                      int N, int H, int W, int ls, int post,
                                                      const float* __restrict__ class_w, const uint16_t* __restrict__ d1,
                                                      const uint16_t* __restrict__ d2, float w0, float sigma,
                                                      double* __restrict__ part) {
    __shared__ double sh[4][2];
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    float cw[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cw[c] = class_w[c];
    float a[2] = {0.f, 0.f};      // sum of w l, sum of w
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        const int64_t li = label_index(px.n, px.h, px.w, H, W, ls);      // of the label and of its D1 / D2 entries
        const int cls = wce_class(labels[li], post, C);
        if (cls < 0) continue;
        const float wt = wce_weight(pick<C>(cw, cls), d1 ? wce_border(d1[li], d2[li], w0, sigma) : 0.f);
        const int64_t base = px.base;
        float p[C], lse;
        softmax_px<C>(logits, base, hw, p, lse);
        const float l = lse - logits[base + cls * hw];
        a[0] += wt * l;
        a[1] += wt;
    }
    block_sum_store(a, sh, part + (size_t)blockIdx.x * 2);
}

// one block: the block partials strided over the threads, then across them in a fixed order
__global__ void __launch_bounds__(256) wce_finish_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ sums,
                                                         float* __restrict__ loss) {
    __shared__ double sh[2][4];
    strided_wave_total(part, nblocks, 2, sh[0]);
    strided_wave_total(part + 1, nblocks, 2, sh[1]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double wl = wave4_total(sh[0]), sw = wave4_total(sh[1]);
    sums[0] = wl;
    sums[1] = sw;
    loss[0] = sw > 0.0 ? (float)(wl / sw) : 0.f;
}

template <int C>
__global__ void __launch_bounds__(256) wce_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                                      int N, int H, int W, int ls, int post,
                                                      const float* __restrict__ class_w, const uint16_t* __restrict__ d1,
                                                      const uint16_t* __restrict__ d2, float w0, float sigma,
                                                      const double* __restrict__ sums, const float* __restrict__ gscale,
                                                      float* __restrict__ dlogits) {
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const double sw = sums[1];
    const bool live = sw > 0.0;
    const float inv = live ? (float)(1.0 / sw) : 0.f;
    const float gs = gscale[0];
    float cw[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cw[c] = class_w[c];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        const int64_t li = label_index(px.n, px.h, px.w, H, W, ls);
        const int cls = wce_class(labels[li], post, C);
        const int64_t base = px.base;
        if (cls < 0 || !live) {
            zero_px<C>(dlogits, base, hw);
            continue;
        }
        const float wt = wce_weight(pick<C>(cw, cls), d1 ? wce_border(d1[li], d2[li], w0, sigma) : 0.f);
        float p[C], lse;
        softmax_px<C>(logits, base, hw, p, lse);
        const float k = gs * (wt * inv);
#pragma unroll
        for (int c = 0; c < C; ++c) dlogits[base + c * hw] = k * (p[c] - ((cls == c) ? 1.f : 0.f));
    }
}

enum { K_DIST, K_MAP, K_FWD, K_FINISH, K_BWD };
static int wce_kid(int k) {
    static const int ids[] = {prof_register("border_dist_kernel"), prof_register("border_weights_kernel"),
                              prof_register("wce_fwd_kernel"), prof_register("wce_finish_kernel"),
                              prof_register("wce_bwd_kernel")};
    return ids[k];
}

static int border_check(const char* what, int B, int H, int W) {
    XV2_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d", what, B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < ((int64_t)1 << 30), "%s: H*W=%lld pixels per image unsupported (< 2^30)", what,
                  (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && cdiv(H, BT) <= 65535, "%s: B=%d or H=%d too large for one launch", what, B, H);
    return XV2_OK;
}

static int map_check(const char* what, float w0, float sigma) {
    XV2_CHECK_ARG(std::isfinite(w0) && w0 >= 0.f, "%s: border weight w0=%g must be finite and >= 0", what, (double)w0);
    XV2_CHECK_ARG(std::isfinite(sigma) && sigma > 0.f, "%s: border sigma=%g must be finite and > 0", what, (double)sigma);
    return XV2_OK;
}

static int wce_check(int N, int C, int H, int W, int lstride, int post, const void* d1, const void* d2, float w0, float sigma) {
    if (int rc = loss_check("wce", N, C, H, W, lstride)) return rc;
    XV2_CHECK_ARG(N <= 65535, "wce: N=%d images unsupported (<= 65535)", N);
    XV2_CHECK_ARG((int64_t)H * W < ((int64_t)1 << 30), "wce: H*W=%lld pixels per image unsupported (< 2^30)", (long long)H * W);
    XV2_CHECK_ARG((d1 == nullptr) == (d2 == nullptr), "wce: d1 and d2 come together (both NULL: no border term)");
    if (d1) {
        XV2_CHECK_ARG(!post, "wce: the border term is defined for post == 0 only (post=%d with distance maps)", post);
        if (int rc = map_check("wce", w0, sigma)) return rc;
    }
    return XV2_OK;
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_border_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || B > 65535 || (int64_t)H * W >= ((int64_t)1 << 30)) return 0;
    return (size_t)B * H * W * sizeof(int32_t);
}

extern "C" int xv2_border_distances(const uint8_t* labels, int B, int H, int W, int R, void* workspace, uint16_t* d1,
                                    uint16_t* d2, void* stream) {
    if (int rc = border_check("border_distances", B, H, W)) return rc;
    XV2_CHECK_ARG(R >= 1 && R <= BR_MAX, "border_distances: radius R=%d unsupported (1..%d)", R, BR_MAX);
    XV2_CHECK_ARG(labels && workspace && d1 && d2, "border_distances: null tensor");
    int32_t* comp = reinterpret_cast<int32_t*>(workspace);
    if (int rc = xv2_label_components(labels, B, H, W, nullptr, comp, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(W, BT), (unsigned)cdiv(H, BT), (unsigned)B);
    const int S = BT + 2 * R;
    XV2_LAUNCH(wce_kid(K_DIST), (double)B * H * W * 8, border_dist_kernel, grid, dim3(256), (size_t)S * S * sizeof(int), st, comp, H, W,
               R, d1, d2);
    return XV2_OK;
}

extern "C" int xv2_border_weights(const uint16_t* d1, const uint16_t* d2, int64_t n, float w0, float sigma, float* out,
                                  void* stream) {
    XV2_CHECK_ARG(n >= 1, "border_weights: n=%lld must be positive", (long long)n);
    if (int rc = map_check("border_weights", w0, sigma)) return rc;
    XV2_CHECK_ARG(d1 && d2 && out, "border_weights: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)std::min<int64_t>(cdiv(n, 256), 4096);
    XV2_LAUNCH(wce_kid(K_MAP), (double)n * 8, border_weights_kernel, dim3(grid), dim3(256), 0, st, d1, d2, n, w0, sigma, out);
    return XV2_OK;
}

extern "C" size_t xv2_wce_workspace(int N, int C, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (C != 2 && C != 4)) return 0;
    return (size_t)WCE_BLOCKS * 2 * sizeof(double);
}

extern "C" int xv2_wce_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride, int post,
                               const float* class_w, const uint16_t* d1, const uint16_t* d2, float w0, float sigma,
                               double* sums, float* loss, void* workspace, void* stream) {
    if (int rc = wce_check(N, C, H, W, lstride, post, d1, d2, w0, sigma)) return rc;
    XV2_CHECK_ARG(logits && labels && class_w && sums && loss && workspace, "wce: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * H * W;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), WCE_BLOCKS);
    double* part = reinterpret_cast<double*>(workspace);
    const double bytes = (double)total * (4 * C + 1 + (d1 ? 4 : 0));
    XV2_DISPATCH_C24(C, XV2_LAUNCH(wce_kid(K_FWD), bytes, wce_fwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W,
                                   lstride, post, class_w, d1, d2, w0, sigma, part));
    XV2_LAUNCH(wce_kid(K_FINISH), 16.0 * grid, wce_finish_kernel, dim3(1), dim3(256), 0, st, part, grid, sums, loss);
    return XV2_OK;
}

extern "C" int xv2_wce_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride, int post,
                                const float* class_w, const uint16_t* d1, const uint16_t* d2, float w0, float sigma,
                                const double* sums, const float* gscale, float* dlogits, void* stream) {
    if (int rc = wce_check(N, C, H, W, lstride, post, d1, d2, w0, sigma)) return rc;
    XV2_CHECK_ARG(logits && labels && class_w && sums && gscale && dlogits, "wce: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * H * W;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), WCE_BWD_BLOCKS);
    const double bytes = (double)total * (8 * C + 1 + (d1 ? 4 : 0));
    XV2_DISPATCH_C24(C, XV2_LAUNCH(wce_kid(K_BWD), bytes, wce_bwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W,
                                   lstride, post, class_w, d1, d2, w0, sigma, sums, gscale, dlogits));
    return XV2_OK;
}
