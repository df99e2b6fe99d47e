// The per-pixel weight of the "wce" term (include/xv2.h): w(p) = cw[class(p)] + b(p).  ONE definition, used by the map entry
// (xv2_border_weights), the forward pass and the backward pass, so that the three hold identical bits: every operation is an
// explicitly rounded intrinsic, which the compiler can neither fuse with a neighbour nor reorder, whatever it is inlined into.
#pragma once
#include "xv2_common.h"

namespace xv2 {

constexpr unsigned WCE_NONE = 0xFFFFu;      // "no component within R" in the D1 / D2 maps

// b = w0 * exp(-(sqrt(D1) + sqrt(D2))^2 / (2 sigma^2)), the square as D1 + D2 + 2 sqrtf(D1 D2): D1, D2 <= 1024, so the sum
// and the product (<= 2^20) are exact fp32 integers.  0 where there is no second component within R.
__device__ __forceinline__ float wce_border(unsigned d1, unsigned d2, float w0, float sigma) {
    if (d2 == WCE_NONE || d1 == WCE_NONE) return 0.f;
    const float s = __fadd_rn((float)(d1 + d2), __fmul_rn(2.f, __fsqrt_rn((float)(d1 * d2))));
    const float den = __fmul_rn(2.f, __fmul_rn(sigma, sigma));
    return __fmul_rn(w0, expf(-__fdiv_rn(s, den)));
}

__device__ __forceinline__ float wce_weight(float cw, float border) { return __fadd_rn(cw, border); }

}  // namespace xv2
