// The per-pixel decode of the prediction fusion (reference utils/post_process.py:31-34), shared by pp_fuse_kernel
// (postproc.hip) and calibrate_hist_kernel (calibrate.hip) so that the sweep counts exactly what the fusion writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xv2 {

enum { K_4CH = 0, K_5CH = 1, K_LABEL = 2, K_MASK = 3 };

// per-class factors of the damage argmax; on == 0: the channels are compared as they are, no multiplication
struct ClassScale {
    float s[4];
    int on;
};

// post of the reference: argmax(dmg) + 1 over four fp32 channels, the first maximum on ties (np.argmax); with scales
// over the float32 products scale[c] * p_c, each rounded once
__device__ __forceinline__ int argmax4(const float* d, int64_t plane, const ClassScale& cs) {
    float m = cs.on ? __fmul_rn(cs.s[0], d[0]) : d[0];
    int k = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const float v = cs.on ? __fmul_rn(cs.s[c], d[c * plane]) : d[c * plane];
        if (v > m) { m = v; k = c; }
    }
    return k + 1;
}

// post before masking of pixel `off` of tile b: KIND K_4CH / K_5CH (fp32 [B,C,H,W]; five channels: the background
// channel dropped, the 4-channel rule on channels 1..4) or K_LABEL (int32 [B,H,W], the value itself, unscaled)
template <int KIND>
__device__ __forceinline__ int decode_raw(const void* dmg, int b, int64_t hw, int64_t off, const ClassScale& cs) {
    if (KIND == K_4CH) return argmax4(reinterpret_cast<const float*>(dmg) + (int64_t)b * 4 * hw + off, hw, cs);
    if (KIND == K_5CH) return argmax4(reinterpret_cast<const float*>(dmg) + (int64_t)b * 5 * hw + hw + off, hw, cs);
    return reinterpret_cast<const int32_t*>(dmg)[(int64_t)b * hw + off];
}

// pre of the reference: float32 comparisons, as numpy compares a float32 array with a Python float
__device__ __forceinline__ int fuse_pre(float l, int raw, float t_loc, float t_dmg) {
    return (l > t_loc) || ((l > t_dmg) && raw > 1);
}

}  // namespace xv2
