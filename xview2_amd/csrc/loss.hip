// The composed loss (model/loss.py:78-101 with monai 0.4.0 DiceLoss / FocalLoss restated, Ohem == mean CE
// because of the tuple-slice at model/loss.py:45), its mse / coral forms, argmax label maps and the F1 counts
// (utils/f1.py:14,36).
//
// Forward: one streaming pass over the NCHW logits computes every sum the composed loss needs
//   per class c: I_c = sum p_c*[y==c], G_c = sum [y==c], P_c = sum p_c      (Dice, batch=True)
//   F = sum -(1-p_t)^2 log p_t,  E = sum -log p_t,  n = number of (masked-in) pixels
// fp32 inside a thread, fp64 across threads/blocks, fixed order -> acc[] -> scalar loss.
// Backward: a second streaming pass forms dL/dlogits analytically from acc[] (no autograd graph).
#include "xv2_common.h"
#include "loss_px.h"
#include <algorithm>

namespace xv2 {

constexpr int LOSS_BLOCKS = 1024;
// acc layout (doubles): [0..3] I_c, [4..7] G_c, [8..11] P_c, [12] F, [13] E, [14] n
constexpr int NACC = 15;
// the composed terms take C = 2 or 4, mse C = 1, coral C = 3
constexpr unsigned LOSS_C1234 = (1u << 1) | (1u << 2) | (1u << 3) | (1u << 4);

template <int C>
__global__ void __launch_bounds__(256) loss_fwd_kernel(const float* __restrict__ logits,
                                                        const uint8_t* __restrict__ labels, int N, int H, int W,
                                                        int ls, int post, double* __restrict__ part) {
    __shared__ double sh[4][NACC];
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    float a[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) a[k] = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        int y = label_at(labels, px.n, px.h, px.w, H, W, ls);
        if (post) {
            if (y == 0) continue;
            y -= 1;
        }
        float p[C], lse;
        softmax_px<C>(logits, px.base, hw, p, lse);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float t = (y == c) ? 1.f : 0.f;
            a[c] += p[c] * t;
            a[4 + c] += t;
            a[8 + c] += p[c];
        }
        const float lt = logits[px.base + (int64_t)(y < C ? y : 0) * hw] - lse;  // log p_t
        const float pt = expf(lt);
        a[12] += -(1.f - pt) * (1.f - pt) * lt;
        a[13] += -lt;
        a[14] += 1.f;
    }
    block_sum_store(a, sh, part + (size_t)blockIdx.x * NACC);
}

__global__ void __launch_bounds__(256) loss_finish_kernel(const double* __restrict__ part, int nblocks, int C,
                                                           int terms, double* __restrict__ acc,
                                                           float* __restrict__ loss) {
    __shared__ double sh[16][16];
    __shared__ double tot[NACC];
    // 16 lanes per accumulator, each summing every 16th block partial, then a 16-term tail: this order is part of the result
    const int k = threadIdx.x & 15, lane = threadIdx.x >> 4;
    double s = 0.0;
    if (k < NACC)
        for (int b = lane; b < nblocks; b += 16) s += part[(size_t)b * NACC + k];
    sh[lane][k] = s;
    __syncthreads();
    if (threadIdx.x < NACC) {
        double t = 0.0;
        for (int l = 0; l < 16; ++l) t += sh[l][threadIdx.x];
        tot[threadIdx.x] = t;
        acc[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double L = 0.0;
        const double n = tot[14];
        if (terms & XV2_LOSS_DICE) {
            // monai DiceLoss(softmax, to_onehot_y, batch): include_background=False iff C == 2
            // (model/loss.py:18-19)
            const int c0 = (C == 2) ? 1 : 0;
            double f = 0.0;
            for (int c = c0; c < C; ++c) f += 1.0 - (2.0 * tot[c] + 1e-5) / (tot[4 + c] + tot[8 + c] + 1e-5);
            L += f / (double)(C - c0);
        }
        if (terms & XV2_LOSS_FOCAL) L += tot[12] / n;
        if (terms & XV2_LOSS_CE) L += tot[13] / n;
        if (terms & (XV2_LOSS_MSE | XV2_LOSS_CORAL)) L = tot[12] / n;
        loss[0] = (float)L;
    }
}

template <int C>
__global__ void __launch_bounds__(256) loss_bwd_kernel(const float* __restrict__ logits,
                                                        const uint8_t* __restrict__ labels, int N, int H, int W,
                                                        int ls, int post, int terms, const double* __restrict__ acc,
                                                        const float* __restrict__ gscale, float weight,
                                                        float* __restrict__ dlogits) {
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const float gs = gscale[0] * weight;
    const int c0 = (C == 2) ? 1 : 0;
    // dice: dL/dI_c = -2/(den_c)/K ; dL/dP_c = (2I_c+eps)/den_c^2/K  with den = G+P+eps
    float dI[C], dP[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        dI[c] = 0.f;
        dP[c] = 0.f;
        if ((terms & XV2_LOSS_DICE) && c >= c0) {
            const double den = acc[4 + c] + acc[8 + c] + 1e-5;
            dI[c] = (float)(-2.0 / den / (double)(C - c0));
            dP[c] = (float)((2.0 * acc[c] + 1e-5) / (den * den) / (double)(C - c0));
        }
    }
    const float inv_n = (float)(1.0 / acc[14]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        int y = label_at(labels, px.n, px.h, px.w, H, W, ls);
        const int64_t base = px.base;
        bool drop = false;
        if (post) {
            if (y == 0) drop = true;
            y -= 1;
        }
        if (drop) {
            zero_px<C>(dlogits, base, hw);
            continue;
        }
        float p[C], lse;
        softmax_px<C>(logits, base, hw, p, lse);
        // dL/dp_c from dice
        float dp[C];
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            dp[c] = dI[c] * ((y == c) ? 1.f : 0.f) + dP[c];
            dot += dp[c] * p[c];
        }
        // focal / ce act through log p_t: d(log p_t)/dl_c = [c==t] - p_c
        float dlt = 0.f;
        const float pt = p[y < C ? y : 0];
        const float lt = logf(fmaxf(pt, 1e-45f));
        if (terms & XV2_LOSS_FOCAL) dlt += (2.f * (1.f - pt) * pt * lt - (1.f - pt) * (1.f - pt)) * inv_n;
        if (terms & XV2_LOSS_CE) dlt += -inv_n;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float g = p[c] * (dp[c] - dot) + dlt * (((y == c) ? 1.f : 0.f) - p[c]);
            dlogits[base + c * hw] = gs * g;
        }
    }
}

// "mse" (model/loss.py:92-94: relu(y_pred[:,0]) vs label-1 on building pixels) and "coral" (model/loss.py:54-65:
// ordinal levels [1]*k+[0]*(3-k), sum_k logsig(x_k)*lv_k + (logsig(x_k)-x_k)*(1-lv_k)); --type post only.
// MODE 0 = mse (C = 1), MODE 1 = coral (C = 3).  acc[12] = sum of per-pixel losses, acc[14] = pixel count.
template <int MODE>
__global__ void __launch_bounds__(256) loss_aux_fwd_kernel(const float* __restrict__ logits,
                                                            const uint8_t* __restrict__ labels, int N, int H, int W,
                                                            int ls, int post, double* __restrict__ part) {
    __shared__ double sh[4][2];
    constexpr int C = MODE == 0 ? 1 : 3;
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    float a = 0.f, cnt = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        int y = label_at(labels, px.n, px.h, px.w, H, W, ls);
        if (post) {
            if (y == 0) continue;
            y -= 1;
        }
        const int64_t base = px.base;
        if (MODE == 0) {
            const float x = logits[base];
            const float p = x <= 0.f ? 0.f : x;      // relu that keeps a NaN (fmaxf would drop it: a finite loss of a NaN logit)
            const float d = p - (float)y;
            a += d * d;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = logits[base + k * hw];
                const float ls_ = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));   // logsigmoid(x)
                // 0 * x: +-0 for a finite x (the sum keeps its bits), NaN for x = +Inf on a reached level, where ls_ is 0 and the
                // reference's logpt * levels + (logpt - x) * (1 - levels) is NaN as well: no finite loss of a non-finite logit
                a -= (k < y) ? (ls_ + 0.f * x) : (ls_ - x);
            }
        }
        cnt += 1.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double va = wave_sum((double)a), vc = wave_sum((double)cnt);
    if (lane == 0) {
        sh[wave][0] = va;
        sh[wave][1] = vc;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double v = 0.0;
        if (threadIdx.x == 12) v = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        if (threadIdx.x == 14) v = sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1];
        part[(size_t)blockIdx.x * NACC + threadIdx.x] = v;
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) loss_aux_bwd_kernel(const float* __restrict__ logits,
                                                            const uint8_t* __restrict__ labels, int N, int H, int W,
                                                            int ls, int post, const double* __restrict__ acc,
                                                            const float* __restrict__ gscale, float weight,
                                                            float* __restrict__ dlogits) {
    constexpr int C = MODE == 0 ? 1 : 3;
    const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
    const float gs = gscale[0] * weight * (float)(1.0 / acc[14]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Px px = px_decode<C>(i, hw, W);
        int y = label_at(labels, px.n, px.h, px.w, H, W, ls);
        const int64_t base = px.base;
        const bool drop = post && y == 0;
        y -= post ? 1 : 0;
        if (MODE == 0) {
            const float x = logits[base];
            dlogits[base] = (drop || x <= 0.f) ? 0.f : gs * 2.f * (x - (float)y);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float x = logits[base + k * hw];
                const float sg = 1.f / (1.f + expf(-x));
                dlogits[base + k * hw] = drop ? 0.f : gs * (sg - ((k < y) ? 1.f : 0.f));
            }
        }
    }
}

template <int C>
__global__ void argmax_kernel(const float* __restrict__ logits, int64_t total, int64_t hw, int add,
                              uint8_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / hw, q = i - n * hw;
        float best = logits[n * C * hw + q];
        int bi = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) {
            const float v = logits[(n * C + c) * hw + q];
            // first maximum wins and a NaN is the maximum (the first NaN wins), like torch.argmax
            if (v > best || (v != v && best == best)) {
                best = v;
                bi = c;
            }
        }
        out[i] = (uint8_t)(bi + add);
    }
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_loss_workspace(int N, int C, int H, int W) {
    (void)N; (void)C; (void)H; (void)W;
    return (size_t)LOSS_BLOCKS * NACC * sizeof(double);
}

extern "C" int xv2_loss_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                                int post, int terms, double* acc, float* loss, float* workspace, void* stream) {
    const bool aux = terms == XV2_LOSS_MSE || terms == XV2_LOSS_CORAL;
    XV2_CHECK_ARG(terms != 0 && (aux || (terms & ~7) == 0), "loss: bad terms mask %d", terms);
    XV2_CHECK_ARG(aux ? (C == (terms == XV2_LOSS_MSE ? 1 : 3)) : (C == 2 || C == 4),
                  "loss: C=%d does not fit the requested terms (dice/focal/ce: 2 or 4, mse: 1, coral: 3)", C);
    if (int rc = loss_check("loss", N, C, H, W, lstride, LOSS_C1234)) return rc;
    XV2_CHECK_ARG(logits && labels && acc && loss && workspace, "loss: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * H * W;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), LOSS_BLOCKS);
    double* part = reinterpret_cast<double*>(workspace);
    if (terms == XV2_LOSS_MSE)
        hipLaunchKernelGGL(loss_aux_fwd_kernel<0>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride, post, part);
    else if (terms == XV2_LOSS_CORAL)
        hipLaunchKernelGGL(loss_aux_fwd_kernel<1>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride, post, part);
    else
        XV2_DISPATCH_C24(C, hipLaunchKernelGGL(loss_fwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride,
                                               post, part));
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, part, grid, C, terms, acc, loss);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_loss_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                                 int post, int terms, const double* acc, const float* gscale, float weight,
                                 float* dlogits, void* stream) {
    if (int rc = loss_check("loss", N, C, H, W, lstride, LOSS_C1234)) return rc;
    XV2_CHECK_ARG(logits && labels && acc && gscale && dlogits, "loss: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * H * W;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), 4096);
    if (terms == XV2_LOSS_MSE)
        hipLaunchKernelGGL(loss_aux_bwd_kernel<0>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride, post,
                           acc, gscale, weight, dlogits);
    else if (terms == XV2_LOSS_CORAL)
        hipLaunchKernelGGL(loss_aux_bwd_kernel<1>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride, post,
                           acc, gscale, weight, dlogits);
    else
        XV2_DISPATCH_C24(C, hipLaunchKernelGGL(loss_bwd_kernel<CC>, dim3(grid), dim3(256), 0, st, logits, labels, N, H, W, lstride,
                                               post, terms, acc, gscale, weight, dlogits));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// tp / fn / fp per class over label maps (utils/f1.py:27-47): counts[(c-1)*3 + {0,1,2}] += #{pred==c & tgt==c},
// #{pred!=c & tgt==c}, #{pred==c & tgt!=c} for c = 1..ncls-1; masked != 0 restricts to pixels with tgt > 0 (damage
// task).  Integer atomics: exact and order-independent.
__global__ void __launch_bounds__(256) f1_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ tgt,
                                                        int64_t total, int ncls, int masked,
                                                        unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sh[12];
    if (threadIdx.x < 12) sh[threadIdx.x] = 0;
    __syncthreads();
    unsigned int loc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) loc[k] = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = pred[i], t = tgt[i];
        if (masked && t == 0) continue;
#pragma unroll
        for (int c = 1; c <= 4; ++c) {
            if (c >= ncls) break;
            loc[(c - 1) * 3 + 0] += (p == c && t == c);
            loc[(c - 1) * 3 + 1] += (p != c && t == c);
            loc[(c - 1) * 3 + 2] += (p == c && t != c);
        }
    }
    const int n = (ncls - 1) * 3;
    for (int k = 0; k < n; ++k) {
        unsigned int v = loc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[k], v);
    }
    __syncthreads();
    if (threadIdx.x < n && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

extern "C" int xv2_f1_counts(const uint8_t* pred, const uint8_t* target, int64_t total, int n_class, int masked,
                             int64_t* counts, void* stream) {
    XV2_CHECK_ARG(n_class >= 2 && n_class <= 5 && total > 0, "f1_counts: n_class=%d unsupported (2..5)", n_class);
    const int grid = (int)std::min<int64_t>(cdiv(total, 256 * 8), 2048);
    hipLaunchKernelGGL(f1_counts_kernel, dim3(std::max(grid, 1)), dim3(256), 0, (hipStream_t)stream, pred, target, total,
                       n_class, masked, reinterpret_cast<unsigned long long*>(counts));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_argmax_nchw(const float* logits, int N, int C, int64_t hw, int add, uint8_t* labels,
                               void* stream) {
    XV2_CHECK_ARG(C >= 2 && C <= 4, "argmax: C=%d unsupported (2..4)", C);
    const int64_t total = (int64_t)N * hw;
    const int grid = (int)std::min<int64_t>(cdiv(total, 256), 4096);
    if (C == 2)
        hipLaunchKernelGGL(argmax_kernel<2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, total, hw, add, labels);
    else if (C == 3)
        hipLaunchKernelGGL(argmax_kernel<3>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, total, hw, add, labels);
    else
        hipLaunchKernelGGL(argmax_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, total, hw, add, labels);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
