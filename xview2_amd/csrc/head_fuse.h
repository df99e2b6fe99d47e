// Per-lane arithmetic of the <= 4-channel 1x1 head (model/layers.py:177,180) and of the BatchNorm apply in front of it, shared by
// the stand-alone kernels (pointwise.hip head_*_kernel, norm_act.hip bn_act_fwd_kernel) and by the BatchNorm passes that absorb
// the head of the last decoder layer (norm_act.hip: bn_act_head_fwd_kernel, ColOp mode 2, the head form of
// bn_act_bwd_rows_kernel).  One definition per expression: the fused and the unfused path round identically.
// Lane <-> channel ownership of the head: a lane owns 4 consecutive channels, L = Cin / 4 lanes share a pixel.
#pragma once
#include "xv2_common.h"

namespace xv2 {

// z = act(y * scale + shift [+ residual]) for 4 channels
__device__ __forceinline__ float4 bn_act_apply4(const float4& v, const float4& sc, const float4& sh, const float4* r, int act) {
    float4 o;
    o.x = __fmaf_rn(v.x, sc.x, sh.x); o.y = __fmaf_rn(v.y, sc.y, sh.y);
    o.z = __fmaf_rn(v.z, sc.z, sh.z); o.w = __fmaf_rn(v.w, sc.w, sh.w);
    if (r) {
        o.x += r->x; o.y += r->y; o.z += r->z; o.w += r->w;
    }
    o.x = apply_act(o.x, act); o.y = apply_act(o.y, act);
    o.z = apply_act(o.z, act); o.w = apply_act(o.w, act);
    return o;
}

// the values a store of v in the storage type T holds
template <typename T>
__device__ __forceinline__ float4 stored4(const float4& v) {
    return make_float4(Elem<T>::round(v.x), Elem<T>::round(v.y), Elem<T>::round(v.z), Elem<T>::round(v.w));
}

// A value the unfused path STORES and reads back (z, the head's input gradient) reaches the fused kernels' arithmetic through this:
// the optimiser then sees it as it sees a loaded value and cannot contract the expressions on either side of it differently
// (fma formation across the would-be store) - the one way the two paths' bits could part although they share every expression.
__device__ __forceinline__ float4 as_loaded(float4 v) {
    asm("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
}

template <int COUT>
__device__ __forceinline__ void head_load_w(const float* __restrict__ w, int Cin, int c, float4 (&ww)[COUT]) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) ww[o] = *reinterpret_cast<const float4*>(w + o * Cin + c);
}

// forward: this lane's 4 channels of every output's dot product
template <int COUT>
__device__ __forceinline__ void head_dot4(const float4& v, const float4 (&ww)[COUT], float (&acc)[COUT]) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] += v.x * ww[o].x + v.y * ww[o].y + v.z * ww[o].z + v.w * ww[o].w;
}

// the L lanes of a pixel (L a power of two <= 64, lanes consecutive): xor-shuffle tree, every lane ends with the sum
template <int COUT>
__device__ __forceinline__ void head_lane_sum(float (&acc)[COUT], int L) {
#pragma unroll
    for (int o = 0; o < COUT; ++o)
        for (int s = L >> 1; s > 0; s >>= 1) acc[o] += __shfl_xor(acc[o], s, 64);
}

// where the Cout values of pixel p live in a logits-shaped fp32 tensor ([N][Cout][hw] when nchw, else [npix][Cout]): element index
// of output 0 and the stride between outputs
struct HeadIdx {
    int64_t base, stride;
};
__device__ __forceinline__ HeadIdx head_index(int nchw, int64_t p, int64_t hw, int cout) {
    if (!nchw) return HeadIdx{p * cout, 1};
    const int64_t n = p / hw, q = p - n * hw;
    return HeadIdx{n * cout * hw + q, hw};
}
// the same index without the 64-bit division (two hundred instructions on this ISA - more than the rest of a streaming pass
// spends per row): hw_div >= 0: hw = 1 << hw_div; -1: npix < 2^31, a 32-bit division; -2: head_index
__device__ __forceinline__ HeadIdx head_index_fast(int nchw, int64_t p, int64_t hw, int cout, int hw_div) {
    if (!nchw) return HeadIdx{p * cout, 1};
    if (hw_div == -2) return head_index(nchw, p, hw, cout);
    const int64_t n = hw_div >= 0 ? (p >> hw_div) : (int64_t)((unsigned)p / (unsigned)hw);
    return HeadIdx{n * cout * hw + (p - n * hw), hw};
}
static inline int head_hw_div(int64_t npix, int64_t hw) {
    if (hw > 0 && (hw & (hw - 1)) == 0) {
        int s = 0;
        while (((int64_t)1 << s) < hw) ++s;
        return s;
    }
    return npix < 0x7fffffff ? -1 : -2;
}

template <int COUT>
__device__ __forceinline__ void head_store(float* __restrict__ y, const float (&acc)[COUT], const float* __restrict__ bias,
                                           const HeadIdx& at) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) y[at.base + o * at.stride] = acc[o] + (bias ? bias[o] : 0.f);
}

// backward: the pixel's output gradients
template <int COUT>
__device__ __forceinline__ void head_load_g(const float* __restrict__ dy, const HeadIdx& at, float (&g)[COUT]) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) g[o] = dy[at.base + o * at.stride];
}

// dx[c .. c+3] = sum_o g[o] * w[o][c .. c+3], o ascending
template <int COUT>
__device__ __forceinline__ float4 head_dx4(const float (&g)[COUT], const float4 (&ww)[COUT]) {
    float4 d = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        d.x += g[o] * ww[o].x; d.y += g[o] * ww[o].y; d.z += g[o] * ww[o].z; d.w += g[o] * ww[o].w;
    }
    return d;
}

// dw[o][c .. c+3] += g[o] * x[c .. c+3]
template <int COUT>
__device__ __forceinline__ void head_dw4(const float (&g)[COUT], const float4& v, float4 (&dwacc)[COUT]) {
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        dwacc[o].x = __fmaf_rn(g[o], v.x, dwacc[o].x); dwacc[o].y = __fmaf_rn(g[o], v.y, dwacc[o].y);
        dwacc[o].z = __fmaf_rn(g[o], v.z, dwacc[o].z); dwacc[o].w = __fmaf_rn(g[o], v.w, dwacc[o].w);
    }
}

// lanes per pixel of the head kernels: min(64, Cin / 4) rounded down to a power of two
static inline int head_lanes(int Cin) {
    int L = 1;
    while (L * 2 <= 64 && L * 2 * 4 <= Cin) L *= 2;
    return L;
}
constexpr int HEAD_MAX_COUT = 4;
constexpr int HEAD_BLOCKS = 1024;      // grid cap of the head's backward pass = rows of its partial buffer

// per-block partials [nblocks][Cout][Cin + 1] (dw row, then db) -> dw, db: fp64 across blocks in a fixed order (pointwise.hip)
int head_bwd_reduce_launch(const float* part, int nblocks, int Cout, int Cin, float* dw, float* db, hipStream_t stream);

// profiler ids of the head path (errors.cpp prof_*; zero flops / bytes: they only name what ran)
int head_prof_id(int which);      // 0 head_fwd_kernel, 1 head_bwd_kernel, 2 bn_act_head_fwd_kernel, 3 column_partials_kernel<head>, 4 bn_act_bwd_rows_head_kernel

}  // namespace xv2
