// Per-pixel pieces shared by the loss kernels (loss_optim.hip, ohem.hip): the channel softmax of one NCHW pixel and the
// strided label fetch of deep supervision.
#pragma once
#include "xv2_common.h"

namespace xv2 {

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

__device__ __forceinline__ int label_at(const uint8_t* __restrict__ labels, int64_t n, int h, int w, int H, int W,
                                        int ls) {
    return labels[(n * (int64_t)H * ls + (int64_t)h * ls) * ((int64_t)W * ls) + (int64_t)w * ls];
}

}  // namespace xv2
