// The --optimizer choices (model/plt.py:150-161) on the flat fp32 parameter / gradient buffers of xview2_amd.optim: AdamW
// (model/plt.py:154; adamw_kernel with the step on the host, adamw_dev_kernel the device-state form) and the others.
// Every entry point but xv2_adamw_step (learning rate and step are host arguments there) reads the learning rate and the step
// counter from device memory and increments the counter in its last launch, so a captured training step stays valid while the
// schedule advances.
//
// Elementwise rules (sgd, radam, adabelief, adabound): one grid-stride launch, the per-step scalars (bias corrections,
// RAdam's rho_t and its branch, AdaBound's bounds) computed per thread in double from the step counter.
//
// Rules with per-tensor / per-output-channel reductions (adamp, novograd): a segment table built once per optimizer cuts
// the buffer into rows (dim 0 of a tensor with >= 2 dims, else the whole tensor).  One wave per row sums a row's
// products into `partials` (a fixed lane-strided order and a fixed butterfly: no atomics, bitwise-reproducible steps),
// one wave per tensor folds its rows in a fixed order, one wave per row applies the update.
//
// Gradient guard (xv2_grad_guard): two launches in front of any rule - a grid-stride sum of squares of the whole gradient
// buffer in double (one partial per block, fixed lane order and butterfly), then a one-block fold that adds the partials in
// index order and writes the guard record (include/xv2.h): the clipped global norm's coefficient and the skip flag of a
// non-finite gradient.  Every rule kernel is a template on GUARDED: that form multiplies the gradient scale by the record's
// coefficient and returns before touching anything when the record says skip; the other form is the code without a guard.
//
// EMA of the weights (xv2_ema_update_dev): a kernel of its own behind the rule, never fused into one - one streaming launch over
// the average and the parameter buffer plus the counter increment, with the guard record passed explicitly.
//
// Gradient accumulation (xv2_grad_accumulate): one streaming launch over a second flat buffer and the gradient buffer, one
// rounded addition per element in micro-batch order; no rule, guard or backward kernel knows about it.
#include "xv2_common.h"
#include "optim_ctx.h"
#include <algorithm>
#include <cmath>

namespace xv2 {

enum FlatRule { RULE_SGD = 0, RULE_SGD_MOMENTUM = 1, RULE_RADAM = 2, RULE_ADABELIEF = 3, RULE_ADABOUND = 4 };

// GUARDED kernels: true when the record says skip (block-uniform); otherwise the gradient scale times the clip coefficient
template <bool GUARDED>
__device__ __forceinline__ bool guard_skips(const float* __restrict__ guard, float& gscale) {
    if (GUARDED) {
        if (reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return true;
        gscale *= guard[GUARD_COEF];
    }
    return false;
}

// the per-step scalars of one rule, computed in double from lr and the 1-based step, handed to the element loop as float
struct StepScalars {
    float a, b, c, d;
};

template <int R>
__device__ __forceinline__ StepScalars step_scalars(double lr, double t, double b1, double b2, double wd, double mu,
                                                    double base_lr, double final_lr, double gamma) {
    StepScalars s{};
    if (R == RULE_SGD) {
        s.a = (float)lr;
    } else if (R == RULE_SGD_MOMENTUM) {
        s.a = (float)lr;
        s.b = (float)mu;
        s.c = t == 1.0 ? 0.f : 1.f;                 // the buffer starts as a copy of the first gradient
    } else {
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        if (R == RULE_RADAM) {
            const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
            const double rho_t = rho_inf - 2.0 * t * pow(b2, t) / bc2;
            s.a = (float)(1.0 - lr * wd);
            if (rho_t >= 5.0) {
                const double rt = sqrt(bc2 * (rho_t - 4.0) * (rho_t - 2.0) * rho_inf /
                                       ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
                s.b = (float)(lr * rt / bc1);
                s.c = 1.f;                          // adaptive branch
            } else {
                s.b = (float)(lr / bc1);
                s.c = 0.f;                          // un-rectified (momentum only) branch
            }
        } else if (R == RULE_ADABELIEF) {
            s.a = (float)(lr / bc1);
            s.b = (float)sqrt(bc2);
        } else {                                    // RULE_ADABOUND
            const double f = final_lr * lr / base_lr;
            s.a = (float)(lr * sqrt(bc2) / bc1);
            s.b = (float)(f * (1.0 - 1.0 / (gamma * t + 1.0)));
            s.c = (float)(f * (1.0 + 1.0 / (gamma * t)));
        }
    }
    return s;
}

// one element's update (shared by the 16-byte and the scalar loops: the same operations in the same order)
template <int R>
__device__ __forceinline__ void rule_one(float& p, float g, float& s0, float& s1, const StepScalars& k, float b1, float b2,
                                         float c1, float c2, float eps, float wd, float gscale) {
    float gi = g * gscale;
    if (R == RULE_SGD) {
        p -= k.a * gi;
    } else if (R == RULE_SGD_MOMENTUM) {
        const float buf = k.c != 0.f ? k.b * s0 + gi : gi;
        s0 = buf;
        p -= k.a * buf;
    } else if (R == RULE_RADAM) {
        const float pi = p * k.a;
        const float mi = b1 * s0 + c1 * gi;
        const float vi = b2 * s1 + c2 * gi * gi;
        s0 = mi;
        s1 = vi;
        p = k.c != 0.f ? pi - k.b * (mi / (sqrtf(vi) + eps)) : pi - k.b * mi;
    } else if (R == RULE_ADABELIEF) {
        gi += wd * p;
        const float mi = b1 * s0 + c1 * gi;
        const float d = gi - mi;
        const float si = (b2 * s1 + c2 * d * d) + eps;
        s0 = mi;
        s1 = si;
        p -= k.a * (mi / (sqrtf(si) / k.b + eps));
    } else {                                        // RULE_ADABOUND
        gi += wd * p;
        const float mi = b1 * s0 + c1 * gi;
        const float vi = b2 * s1 + c2 * gi * gi;
        s0 = mi;
        s1 = vi;
        const float step = fminf(fmaxf(k.a / (sqrtf(vi) + eps), k.b), k.c);
        p -= step * mi;
    }
}

template <int R, bool GUARDED>
__global__ void __launch_bounds__(256) flat_rule_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ s0, float* __restrict__ s1, int64_t n,
                                                         const float* __restrict__ lr_dev, const int* __restrict__ step_dev,
                                                         double b1d, double b2d, float eps, float wd, float mu,
                                                         float base_lr, float final_lr, float gamma, float gscale,
                                                         const float* __restrict__ guard) {
    if (guard_skips<GUARDED>(guard, gscale)) return;
    const double t = (double)(step_dev[0] + 1);
    const StepScalars k = step_scalars<R>((double)lr_dev[0], t, b1d, b2d, wd, mu, base_lr, final_lr, gamma);
    // the betas and their complements rounded once from double (1 - 0.999f would be 1.3e-5 off 0.001)
    const float b1 = (float)b1d, b2 = (float)b2d, c1 = (float)(1.0 - b1d), c2 = (float)(1.0 - b2d);
    constexpr bool has0 = R != RULE_SGD, has1 = R != RULE_SGD && R != RULE_SGD_MOMENTUM;
    float z0 = 0.f, z1 = 0.f;                        // stand-ins for the state a rule does not keep
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s0) |
                         reinterpret_cast<uintptr_t>(s1)) & 15) ? 0 : n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 a = has0 ? reinterpret_cast<float4*>(s0)[i] : float4{0.f, 0.f, 0.f, 0.f};
        float4 b = has1 ? reinterpret_cast<float4*>(s1)[i] : float4{0.f, 0.f, 0.f, 0.f};
        rule_one<R>(pp.x, gg.x, a.x, b.x, k, b1, b2, c1, c2, eps, wd, gscale);
        rule_one<R>(pp.y, gg.y, a.y, b.y, k, b1, b2, c1, c2, eps, wd, gscale);
        rule_one<R>(pp.z, gg.z, a.z, b.z, k, b1, b2, c1, c2, eps, wd, gscale);
        rule_one<R>(pp.w, gg.w, a.w, b.w, k, b1, b2, c1, c2, eps, wd, gscale);
        if (has0) reinterpret_cast<float4*>(s0)[i] = a;
        if (has1) reinterpret_cast<float4*>(s1)[i] = b;
        reinterpret_cast<float4*>(p)[i] = pp;
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        rule_one<R>(p[i], g[i], has0 ? s0[i] : z0, has1 ? s1[i] : z1, k, b1, b2, c1, c2, eps, wd, gscale);
}

template <bool GUARDED>
__global__ void inc_step_kernel(int* p, const float* __restrict__ guard) {
    if (GUARDED && reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return;     // a skipped step is not counted
    p[0] += 1;
}

// ---- segmented rules --------------------------------------------------------------------------------------------
// rows  [rows_total][3] int64: {first element, length, tensor}
// tens  [ntensors][4]   int64: {first row, rows, numel, dims >= 2}
// partials [rows_total][SEG_K] float
constexpr int SEG_K = 4;
constexpr int SEG_WAVES = 4;                         // waves (rows or tensors) per 256-thread block
enum SegRule { SEG_ADAMP = 0, SEG_NOVOGRAD = 1 };

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

struct AdamPScalars {
    float b1, b2, c1, c2, eps, bc2s, gscale;
};

// AdamP's row pass for one element: moments updated, then sum p*g, g*g, p*p, p*u (u the Adam direction)
__device__ __forceinline__ void adamp_row_one(float p, float g, float& m, float& v, const AdamPScalars& c, double (&acc)[SEG_K]) {
    const float gi = g * c.gscale;
    const float mi = c.b1 * m + c.c1 * gi;
    const float vi = c.b2 * v + c.c2 * gi * gi;
    m = mi;
    v = vi;
    const float u = mi / (sqrtf(vi) / c.bc2s + c.eps);
    acc[0] += (double)p * gi;
    acc[1] += (double)gi * gi;
    acc[2] += (double)p * p;
    acc[3] += (double)p * u;
}

template <int S, bool GUARDED>
__global__ void __launch_bounds__(256) seg_row_kernel(const int64_t* __restrict__ rows, int64_t rows_total,
                                                       const float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ partials, const int* __restrict__ step_dev,
                                                       double b1, double b2, float eps, float gscale,
                                                       const float* __restrict__ guard) {
    if (guard_skips<GUARDED>(guard, gscale)) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (row >= rows_total) return;
    const int64_t start = rows[row * 3], len = rows[row * 3 + 1];
    double acc[SEG_K] = {0.0, 0.0, 0.0, 0.0};
    const bool vec = (len & 3) == 0 && (start & 3) == 0;
    if (S == SEG_ADAMP) {
        const double t = (double)(step_dev[0] + 1);
        const AdamPScalars c{(float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), eps, (float)sqrt(1.0 - pow(b2, t)), gscale};
        if (vec) {
            const int64_t l4 = len >> 2, s4 = start >> 2;
            for (int64_t i = lane; i < l4; i += 64) {
                const float4 pp = reinterpret_cast<const float4*>(p)[s4 + i];
                const float4 gg = reinterpret_cast<const float4*>(g)[s4 + i];
                float4 mm = reinterpret_cast<float4*>(m)[s4 + i], vv = reinterpret_cast<float4*>(v)[s4 + i];
                adamp_row_one(pp.x, gg.x, mm.x, vv.x, c, acc);
                adamp_row_one(pp.y, gg.y, mm.y, vv.y, c, acc);
                adamp_row_one(pp.z, gg.z, mm.z, vv.z, c, acc);
                adamp_row_one(pp.w, gg.w, mm.w, vv.w, c, acc);
                reinterpret_cast<float4*>(m)[s4 + i] = mm;
                reinterpret_cast<float4*>(v)[s4 + i] = vv;
            }
        } else {
            for (int64_t i = lane; i < len; i += 64) adamp_row_one(p[start + i], g[start + i], m[start + i], v[start + i], c, acc);
        }
    } else {                                         // SEG_NOVOGRAD: the squared norm of the scaled gradient
        if (vec) {
            const int64_t l4 = len >> 2, s4 = start >> 2;
            for (int64_t i = lane; i < l4; i += 64) {
                const float4 gg = reinterpret_cast<const float4*>(g)[s4 + i];
                const float x = gg.x * gscale, y = gg.y * gscale, z = gg.z * gscale, w = gg.w * gscale;
                acc[1] += (double)x * x + (double)y * y + (double)z * z + (double)w * w;
            }
        } else {
            for (int64_t i = lane; i < len; i += 64) {
                const float x = g[start + i] * gscale;
                acc[1] += (double)x * x;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) acc[k] = wave_sum(acc[k]);
    if (lane < SEG_K) partials[row * SEG_K + lane] = (float)acc[lane];
}

// |cos| as F.cosine_similarity(g, p, eps) computes it: each norm clamped below at eps
__device__ __forceinline__ double abs_cos(double pg, double gg, double pp, double eps) {
    return fabs(pg) / (fmax(sqrt(gg), eps) * fmax(sqrt(pp), eps));
}

// one wave per tensor.  AdamP: decision[t] (0 no projection, 1 channel view, 2 layer view) and aux[t] = {layer-view
// coefficient sum(p*u) / (|p| + eps)^2, weight-decay ratio}.  NovoGrad: the blended gradient norm norm_avg[t].
template <int S, bool GUARDED>
__global__ void __launch_bounds__(256) seg_fold_kernel(const int64_t* __restrict__ tens, int ntensors,
                                                        const float* __restrict__ partials, int* __restrict__ decision,
                                                        float* __restrict__ aux, float* __restrict__ norm_avg,
                                                        const int* __restrict__ step_dev, double b2, float eps, float delta,
                                                        float wd_ratio, const float* __restrict__ guard) {
    if (GUARDED && reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return;
    const int lane = threadIdx.x & 63;
    const int tsr = blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (tsr >= ntensors) return;                     // (wave-uniform: a wave owns one tensor)
    const int64_t r0 = tens[tsr * 4], nr = tens[tsr * 4 + 1], numel = tens[tsr * 4 + 2];
    const bool multi_dim = tens[tsr * 4 + 3] != 0;
    double acc[SEG_K] = {0.0, 0.0, 0.0, 0.0};
    double mx = 0.0;
    for (int64_t r = lane; r < nr; r += 64) {
        const float* q = partials + (r0 + r) * SEG_K;
#pragma unroll
        for (int k = 0; k < SEG_K; ++k) acc[k] += (double)q[k];
        if (S == SEG_ADAMP) mx = fmax(mx, abs_cos(q[0], q[1], q[2], eps));
    }
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) acc[k] = wave_sum(acc[k]);
    if (S == SEG_ADAMP) mx = wave_max(mx);
    if (lane != 0) return;
    if (S == SEG_ADAMP) {
        const int64_t rowlen = numel / nr;
        int dec = 0;
        double coef = 0.0;
        if (multi_dim) {
            if (mx < (double)delta / sqrt((double)rowlen)) {
                dec = 1;                             // channel view: the apply pass takes each row's own coefficient
            } else if (abs_cos(acc[0], acc[1], acc[2], eps) < (double)delta / sqrt((double)numel)) {
                dec = 2;
                const double pn = sqrt(acc[2]) + eps;
                coef = acc[3] / (pn * pn);
            }
        }
        decision[tsr] = dec;
        aux[tsr * 2] = (float)coef;
        aux[tsr * 2 + 1] = dec ? wd_ratio : 1.f;
    } else {
        const double n = sqrt(acc[1]);
        const double prev = norm_avg[tsr];
        norm_avg[tsr] = step_dev[0] == 0 ? (float)n : (float)sqrt(b2 * prev * prev + (1.0 - b2) * n * n);
    }
}

struct ApplyScalars {
    float lr, step_size, bc2s, b1, c1, eps, wd, gscale;
};

// AdamP: u from the moments the row pass stored, projected by `coef`, decoupled decay scaled by the tensor's ratio
__device__ __forceinline__ void adamp_apply_one(float& p, float m, float v, float coef, float decay, const ApplyScalars& c) {
    const float u = m / (sqrtf(v) / c.bc2s + c.eps) - coef * p;
    p = p * decay - c.step_size * u;
}
// NovoGrad (grad averaging, decay outside the moment): `den` = norm_avg / sqrt(1 - b2^t) + eps of the tensor
__device__ __forceinline__ void novograd_apply_one(float& p, float g, float& m, float den, const ApplyScalars& c) {
    const float gi = g * c.gscale;
    const float mi = c.b1 * m + c.c1 * gi;
    m = mi;
    p = p - c.lr * ((mi * c.step_size) / den + c.wd * p);
}

template <int S, bool GUARDED>
__global__ void __launch_bounds__(256) seg_apply_kernel(const int64_t* __restrict__ rows, int64_t rows_total,
                                                         float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, const float* __restrict__ v,
                                                         const float* __restrict__ partials,
                                                         const int* __restrict__ decision, const float* __restrict__ aux,
                                                         const float* __restrict__ norm_avg,
                                                         const float* __restrict__ lr_dev, const int* __restrict__ step_dev,
                                                         double b1, double b2, float eps, float wd, float gscale,
                                                         const float* __restrict__ guard) {
    if (guard_skips<GUARDED>(guard, gscale)) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (row >= rows_total) return;
    const int64_t start = rows[row * 3], len = rows[row * 3 + 1], tsr = rows[row * 3 + 2];
    const double lr = lr_dev[0], t = (double)(step_dev[0] + 1);
    const double bc1 = 1.0 - pow(b1, t), bc2s = sqrt(1.0 - pow(b2, t));
    ApplyScalars c{(float)lr, 0.f, (float)bc2s, (float)b1, (float)(1.0 - b1), eps, wd, gscale};
    const bool vec = (len & 3) == 0 && (start & 3) == 0;
    const int64_t l4 = len >> 2, s4 = start >> 2;
    if (S == SEG_ADAMP) {
        c.step_size = (float)(lr / bc1);
        const int dec = decision[tsr];
        float coef = 0.f;
        if (dec == 1) {
            const float* q = partials + row * SEG_K;
            const double pn = sqrt((double)q[2]) + eps;
            coef = (float)((double)q[3] / (pn * pn));
        } else if (dec == 2) {
            coef = aux[tsr * 2];
        }
        const float decay = (float)(1.0 - lr * wd * (double)aux[tsr * 2 + 1]);
        if (vec) {
            for (int64_t i = lane; i < l4; i += 64) {
                float4 pp = reinterpret_cast<float4*>(p)[s4 + i];
                const float4 mm = reinterpret_cast<const float4*>(m)[s4 + i], vv = reinterpret_cast<const float4*>(v)[s4 + i];
                adamp_apply_one(pp.x, mm.x, vv.x, coef, decay, c);
                adamp_apply_one(pp.y, mm.y, vv.y, coef, decay, c);
                adamp_apply_one(pp.z, mm.z, vv.z, coef, decay, c);
                adamp_apply_one(pp.w, mm.w, vv.w, coef, decay, c);
                reinterpret_cast<float4*>(p)[s4 + i] = pp;
            }
        } else {
            for (int64_t i = lane; i < len; i += 64) adamp_apply_one(p[start + i], m[start + i], v[start + i], coef, decay, c);
        }
    } else {
        c.step_size = (float)(1.0 / bc1);
        const float den = (float)((double)norm_avg[tsr] / bc2s + eps);
        if (vec) {
            for (int64_t i = lane; i < l4; i += 64) {
                float4 pp = reinterpret_cast<float4*>(p)[s4 + i], mm = reinterpret_cast<float4*>(m)[s4 + i];
                const float4 gg = reinterpret_cast<const float4*>(g)[s4 + i];
                novograd_apply_one(pp.x, gg.x, mm.x, den, c);
                novograd_apply_one(pp.y, gg.y, mm.y, den, c);
                novograd_apply_one(pp.z, gg.z, mm.z, den, c);
                novograd_apply_one(pp.w, gg.w, mm.w, den, c);
                reinterpret_cast<float4*>(m)[s4 + i] = mm;
                reinterpret_cast<float4*>(p)[s4 + i] = pp;
            }
        } else {
            for (int64_t i = lane; i < len; i += 64) novograd_apply_one(p[start + i], g[start + i], m[start + i], den, c);
        }
    }
}

// ---- gradient guard ---------------------------------------------------------------------------------------------
constexpr int GUARD_MAX_BLOCKS = 1024;               // partials the one-block fold adds serially (4 blocks per CU)

// blocks of the sum-of-squares pass: a function of n alone, so the summation order (and the result's bits) is too
static inline int guard_blocks(int64_t n) { return (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), GUARD_MAX_BLOCKS); }

__device__ __forceinline__ void sq_acc4(const float4 v, double (&acc)[4]) {
    acc[0] = fma((double)v.x, (double)v.x, acc[0]);
    acc[1] = fma((double)v.y, (double)v.y, acc[1]);
    acc[2] = fma((double)v.z, (double)v.z, acc[2]);
    acc[3] = fma((double)v.w, (double)v.w, acc[3]);
}

// partial[block] = sum of g[i]^2 over the block's grid-stride share, in double: a thread's elements in index order into four
// accumulators (one per float4 component; the scalar tail into the first), those added pairwise, the wave butterfly, then
// the block's four waves in wave order.  A finite float squared is at most 1.2e77: the sum cannot overflow, so a non-finite
// sum means a non-finite element.
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
    __shared__ double wsum[4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t n4 = (reinterpret_cast<uintptr_t>(g) & 15) ? 0 : n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {      // four 16-byte loads in flight per thread
        const float4 a = reinterpret_cast<const float4*>(g)[i], b = reinterpret_cast<const float4*>(g)[i + stride];
        const float4 c = reinterpret_cast<const float4*>(g)[i + 2 * stride], d = reinterpret_cast<const float4*>(g)[i + 3 * stride];
        sq_acc4(a, acc);
        sq_acc4(b, acc);
        sq_acc4(c, acc);
        sq_acc4(d, acc);
    }
    for (; i < n4; i += stride) sq_acc4(reinterpret_cast<const float4*>(g)[i], acc);
    for (int64_t j = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += stride)
        acc[0] = fma((double)g[j], (double)g[j], acc[0]);
    const double v = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one block: the partials added in index order, then the record.  torch.nn.utils.clip_grad_norm_'s arithmetic in double,
// stored as float: coef = min(max_norm / (norm + 1e-6), 1) - a NaN stays a NaN, as torch.clamp keeps it.
__global__ void __launch_bounds__(256) grad_guard_fold_kernel(const double* __restrict__ partial, int blocks, double grad_scale,
                                                              double max_norm, int skip_nonfinite, float* __restrict__ guard) {
    __shared__ double sh[GUARD_MAX_BLOCKS];
    for (int i = threadIdx.x; i < blocks; i += 256) sh[i] = partial[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < blocks; ++i) sum += sh[i];
    const double norm = grad_scale * sqrt(sum);
    const float norm_f = (float)norm;
    const bool finite = isfinite(norm);              // (of the double: finite elements whose norm exceeds fp32 still clip)
    double coef = 1.0;
    if (max_norm > 0.0) {
        coef = max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    const bool skip = skip_nonfinite != 0 && !finite;
    int* gi = reinterpret_cast<int*>(guard);
    int64_t* gl = reinterpret_cast<int64_t*>(guard);
    guard[GUARD_NORM] = norm_f;
    guard[GUARD_COEF] = (float)coef;
    gi[GUARD_SKIP] = skip ? 1 : 0;
    gi[GUARD_SKIPPED_ROW] = skip ? gi[GUARD_SKIPPED_ROW] + 1 : 0;
    gl[GUARD_STEPS64] += 1;
    if (!skip && coef < 1.0) gl[GUARD_STEPS64 + 1] += 1;
    if (skip) gl[GUARD_STEPS64 + 2] += 1;
    if (isfinite(norm_f) && norm_f > guard[GUARD_NORM_MAX]) guard[GUARD_NORM_MAX] = norm_f;
}

// ---- EMA of the weights -----------------------------------------------------------------------------------------
// ema += (1 - d) * (param - ema) over the flat parameter buffer: 12 bytes per element, one launch plus the counter increment.
// d = min(decay, (1 + t) / (10 + t)) under warm-up, t the updates applied so far (read from the device), else decay; the
// complement is formed in double and rounded once.  One rounded subtraction and one fused multiply-add per element, spelled
// out so that the result does not hang on the compiler's contraction: param == ema is a fixed point bit for bit (an average
// of -0 alone comes back as +0: +0 + -0 = +0), and a non-finite parameter reaches only its own element.
__device__ __forceinline__ float ema_one(float e, float p, float om) { return fmaf(om, p - e, e); }

template <bool GUARDED>
__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param, int64_t n,
                                                          double decay, int warmup, const int* __restrict__ count_dev,
                                                          const float* __restrict__ guard) {
    if (GUARDED && reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return;     // a skipped step does not pull the average
    double d = decay;
    if (warmup) {
        const double t = (double)count_dev[0];
        d = fmin(decay, (1.0 + t) / (10.0 + t));
    }
    const float om = (float)(1.0 - d);
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(param)) & 15) ? 0 : n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 e = reinterpret_cast<float4*>(ema)[i];
        const float4 p = reinterpret_cast<const float4*>(param)[i];
        e.x = ema_one(e.x, p.x, om);
        e.y = ema_one(e.y, p.y, om);
        e.z = ema_one(e.z, p.z, om);
        e.w = ema_one(e.w, p.w, om);
        reinterpret_cast<float4*>(ema)[i] = e;
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        ema[i] = ema_one(ema[i], param[i], om);
}

// ---- gradient accumulation over micro-batches -------------------------------------------------------------------
// One rounded fp32 addition per element, acc[i] + grad[i] in that operand order (there is no product, so nothing contracts):
// open copies grad into acc, add stores the sum into acc, close stores it into grad and only reads acc.  ema_update_kernel's
// loop: 16-byte loads and stores when both pointers are 16-byte aligned, the same operation per element for the tail and
// otherwise.
enum AccumMode { ACCUM_OPEN = 0, ACCUM_ADD = 1, ACCUM_CLOSE = 2 };

template <int MODE>
__global__ void __launch_bounds__(256) grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ grad, int64_t n) {
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(grad)) & 15) ? 0 : n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 g = reinterpret_cast<const float4*>(grad)[i];
        if (MODE == ACCUM_OPEN) {
            reinterpret_cast<float4*>(acc)[i] = g;
        } else {
            float4 a = reinterpret_cast<const float4*>(acc)[i];
            a.x = a.x + g.x;
            a.y = a.y + g.y;
            a.z = a.z + g.z;
            a.w = a.w + g.w;
            reinterpret_cast<float4*>(MODE == ACCUM_ADD ? acc : grad)[i] = a;
        }
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (MODE == ACCUM_OPEN)
            acc[i] = grad[i];
        else
            (MODE == ACCUM_ADD ? acc : grad)[i] = acc[i] + grad[i];
    }
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt, float gscale) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gscale;
        float pi = p[i];
        pi *= 1.f - lr * wd;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pi - (lr / bc1) * (mi / denom);
    }
}

// graph-capturable form: learning rate and step counter live in device memory, so a captured launch stays valid
// while the host-side schedule / step count advance
// one element's update (shared by the scalar and the 16-byte forms: the same operations in the same order)
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps,
                                          float wd, float bc1, float bc2_sqrt, float gscale) {
    const float gi = g * gscale;
    float pi = p;
    pi *= 1.f - lr * wd;
    const float mi = b1 * m + (1.f - b1) * gi;
    const float vi = b2 * v + (1.f - b2) * gi * gi;
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p = pi - (lr / bc1) * (mi / denom);
}
// GUARDED (include/xv2.h "gradient guard"): the record's skip flag returns before anything is touched, its clip coefficient
// multiplies the gradient scale; the other instantiation is the kernel without a guard
template <bool GUARDED>
__global__ void __launch_bounds__(256) adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                         const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                         float wd, const int* __restrict__ step_dev, float gscale,
                                                         const float* __restrict__ guard) {
    if (GUARDED) {
        if (reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return;
        gscale *= guard[GUARD_COEF];
    }
    const float lr = lr_dev[0];
    const float step = (float)(step_dev[0] + 1);
    const float bc1 = 1.f - powf(b1, step);
    const float bc2_sqrt = sqrtf(1.f - powf(b2, step));
    // 16-byte accesses (the flat buffers are allocation-aligned): four tensors x 16 bytes in flight per thread and iteration;
    // with 4-byte accesses the pass ran at 3.6 TB/s (0.2 ms for the 25.5 M parameters of cfg2, 1.9 ms for cfg5's)
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v)) & 15) ? 0 : n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        adamw_one(pp.x, gg.x, mm.x, vv.x, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        adamw_one(pp.y, gg.y, mm.y, vv.y, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        adamw_one(pp.z, gg.z, mm.z, vv.z, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        adamw_one(pp.w, gg.w, mm.w, vv.w, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        reinterpret_cast<float4*>(p)[i] = pp;
    }
    for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adamw_one(p[i], g[i], m[i], v[i], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
}
template <bool GUARDED>
__global__ void inc_i32_kernel(int* p, const float* __restrict__ guard) {
    if (GUARDED && reinterpret_cast<const int*>(guard)[GUARD_SKIP] != 0) return;     // a skipped step is not counted
    p[0] += 1;
}

}  // namespace xv2

using namespace xv2;

extern "C" int xv2_grad_accumulate(float* acc, float* grad, int64_t n, int mode, void* stream) {
    XV2_CHECK_ARG(n >= 0, "grad_accumulate: n = %lld, must not be negative", (long long)n);
    XV2_CHECK_ARG(mode >= ACCUM_OPEN && mode <= ACCUM_CLOSE, "grad_accumulate: unknown mode %d (0 open, 1 add, 2 close)", mode);
    if (n == 0) return XV2_OK;
    XV2_CHECK_ARG(acc && grad, "grad_accumulate: null accumulator or gradient buffer");
    const uintptr_t a = reinterpret_cast<uintptr_t>(acc), g = reinterpret_cast<uintptr_t>(grad), bytes = (uintptr_t)n * sizeof(float);
    XV2_CHECK_ARG(a + bytes <= g || g + bytes <= a, "grad_accumulate: the accumulator and the gradient buffer overlap");
    // ema_update_kernel's grid: one float4 per thread up to 4096 blocks, grid-stride beyond 2^22 elements
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), 4096);
    hipStream_t s = (hipStream_t)stream;
    if (mode == ACCUM_OPEN)
        hipLaunchKernelGGL(grad_accumulate_kernel<ACCUM_OPEN>, dim3(grid), dim3(256), 0, s, acc, grad, n);
    else if (mode == ACCUM_ADD)
        hipLaunchKernelGGL(grad_accumulate_kernel<ACCUM_ADD>, dim3(grid), dim3(256), 0, s, acc, grad, n);
    else
        hipLaunchKernelGGL(grad_accumulate_kernel<ACCUM_CLOSE>, dim3(grid), dim3(256), 0, s, acc, grad, n);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" size_t xv2_grad_guard_workspace(int64_t n) { return n > 0 ? (size_t)guard_blocks(n) * sizeof(double) : 0; }

extern "C" int xv2_grad_guard(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite,
                              void* workspace, void* guard, void* stream) {
    XV2_CHECK_ARG(grad && guard, "grad_guard: null gradient buffer or guard record");
    XV2_CHECK_ARG(n > 0, "grad_guard: n = %lld, must be positive", (long long)n);
    XV2_CHECK_ARG(std::isfinite(max_norm) && max_norm >= 0.f, "grad_guard: max_norm = %g, must be finite and >= 0 (0: no clipping)",
                  (double)max_norm);
    XV2_CHECK_ARG(workspace, "grad_guard: a guard needs its workspace (xv2_grad_guard_workspace bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int blocks = guard_blocks(n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, s, grad, n, static_cast<double*>(workspace));
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_guard_fold_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(workspace), blocks,
                       (double)grad_scale, (double)max_norm, skip_nonfinite, static_cast<float*>(guard));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_flat_step_dev(int rule, float* param, const float* grad, float* state0, float* state1, int64_t n,
                                 const float* lr_dev, int* step_dev, double beta1, double beta2, float eps,
                                 float weight_decay, float momentum, float base_lr, float final_lr, float gamma,
                                 float grad_scale, void* stream) {
    OptimGuardScope scope;          // (the guard named for this call, cleared on every way out)
    XV2_CHECK_ARG(param && grad && lr_dev && step_dev && n > 0, "flat_step_dev: null buffer or empty");
    XV2_CHECK_ARG(rule >= RULE_SGD && rule <= RULE_ADABOUND, "flat_step_dev: unknown rule %d", rule);
    XV2_CHECK_ARG(rule == RULE_SGD || state0, "flat_step_dev: rule %d keeps a first state buffer", rule);
    XV2_CHECK_ARG(rule == RULE_SGD || rule == RULE_SGD_MOMENTUM || state1, "flat_step_dev: rule %d keeps two state buffers", rule);
    XV2_CHECK_ARG(rule != RULE_ADABOUND || base_lr > 0.f, "flat_step_dev: adabound needs base_lr > 0");
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), 4096);
    hipStream_t s = (hipStream_t)stream;
    const float* guard = scope.guard;
#define XV2_RULE_LAUNCH_G(R, G)                                                                                        \
    hipLaunchKernelGGL((flat_rule_kernel<R, G>), dim3(grid), dim3(256), 0, s, param, grad, state0, state1, n, lr_dev, \
                       step_dev, beta1, beta2, eps, weight_decay, momentum, base_lr, final_lr, gamma, grad_scale, guard)
#define XV2_RULE_LAUNCH(R)                   \
    do {                                     \
        if (guard)                           \
            XV2_RULE_LAUNCH_G(R, true);      \
        else                                 \
            XV2_RULE_LAUNCH_G(R, false);     \
    } while (0)
    switch (rule) {
        case RULE_SGD: XV2_RULE_LAUNCH(RULE_SGD); break;
        case RULE_SGD_MOMENTUM: XV2_RULE_LAUNCH(RULE_SGD_MOMENTUM); break;
        case RULE_RADAM: XV2_RULE_LAUNCH(RULE_RADAM); break;
        case RULE_ADABELIEF: XV2_RULE_LAUNCH(RULE_ADABELIEF); break;
        default: XV2_RULE_LAUNCH(RULE_ADABOUND);
    }
#undef XV2_RULE_LAUNCH
#undef XV2_RULE_LAUNCH_G
    XV2_CHECK_LAUNCH();
    if (guard)
        hipLaunchKernelGGL(inc_step_kernel<true>, dim3(1), dim3(1), 0, s, step_dev, guard);
    else
        hipLaunchKernelGGL(inc_step_kernel<false>, dim3(1), dim3(1), 0, s, step_dev, guard);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                  int* step_dev, float grad_scale, void* stream) {
    OptimGuardScope scope;          // (the guard named for this call, cleared on every way out)
    const float* guard = scope.guard;
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), 4096);
    if (guard)
        hipLaunchKernelGGL(adamw_dev_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, n, lr_dev, beta1, beta2, eps, weight_decay, step_dev, grad_scale, guard);
    else
        hipLaunchKernelGGL(adamw_dev_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                           exp_avg_sq, n, lr_dev, beta1, beta2, eps, weight_decay, step_dev, grad_scale, guard);
    XV2_CHECK_LAUNCH();
    if (guard)
        hipLaunchKernelGGL(inc_i32_kernel<true>, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, guard);
    else
        hipLaunchKernelGGL(inc_i32_kernel<false>, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, guard);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                              void* stream) {
    OptimGuardScope scope;
    // (a skipped step must not advance the step: only the device-counter forms can honour a guard)
    XV2_CHECK_ARG(!scope.guard, "adamw_step: a gradient guard needs the device-state form (xv2_adamw_step_dev)");
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2 = 1.f - powf(beta2, (float)step);
    const int grid = (int)std::min<int64_t>(cdiv(n, 256), 4096);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       n, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2), grad_scale);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

template <bool G>
static int adamp_launch(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors, float* param,
                        const float* grad, float* exp_avg, float* exp_avg_sq, float* partials, int* decision, float* aux,
                        const float* lr_dev, int* step_dev, double beta1, double beta2, float eps, float weight_decay,
                        float delta, float wd_ratio, float grad_scale, const float* guard, hipStream_t s) {
    const unsigned rgrid = (unsigned)cdiv(rows_total, SEG_WAVES), tgrid = (unsigned)cdiv(ntensors, SEG_WAVES);
    hipLaunchKernelGGL((seg_row_kernel<SEG_ADAMP, G>), dim3(rgrid), dim3(256), 0, s, rows, rows_total, param, grad, exp_avg,
                       exp_avg_sq, partials, step_dev, beta1, beta2, eps, grad_scale, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL((seg_fold_kernel<SEG_ADAMP, G>), dim3(tgrid), dim3(256), 0, s, tensors, ntensors, partials, decision, aux,
                       (float*)nullptr, step_dev, beta2, eps, delta, wd_ratio, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL((seg_apply_kernel<SEG_ADAMP, G>), dim3(rgrid), dim3(256), 0, s, rows, rows_total, param, grad, exp_avg,
                       exp_avg_sq, partials, decision, aux, (const float*)nullptr, lr_dev, step_dev, beta1, beta2, eps,
                       weight_decay, grad_scale, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(inc_step_kernel<G>, dim3(1), dim3(1), 0, s, step_dev, guard);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_adamp_step_dev(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors,
                                  float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* partials,
                                  int* decision, float* aux, const float* lr_dev, int* step_dev, double beta1, double beta2,
                                  float eps, float weight_decay, float delta, float wd_ratio, float grad_scale,
                                  void* stream) {
    OptimGuardScope scope;
    XV2_CHECK_ARG(rows && tensors && param && grad && exp_avg && exp_avg_sq && partials && decision && aux && lr_dev &&
                  step_dev && rows_total > 0 && ntensors > 0, "adamp_step_dev: null buffer or empty table");
    return scope.guard
               ? adamp_launch<true>(rows, rows_total, tensors, ntensors, param, grad, exp_avg, exp_avg_sq, partials, decision,
                                    aux, lr_dev, step_dev, beta1, beta2, eps, weight_decay, delta, wd_ratio, grad_scale,
                                    scope.guard, (hipStream_t)stream)
               : adamp_launch<false>(rows, rows_total, tensors, ntensors, param, grad, exp_avg, exp_avg_sq, partials, decision,
                                     aux, lr_dev, step_dev, beta1, beta2, eps, weight_decay, delta, wd_ratio, grad_scale,
                                     nullptr, (hipStream_t)stream);
}

template <bool G>
static int novograd_launch(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors, float* param,
                           const float* grad, float* exp_avg, float* norm_avg, float* partials, const float* lr_dev,
                           int* step_dev, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                           const float* guard, hipStream_t s) {
    const unsigned rgrid = (unsigned)cdiv(rows_total, SEG_WAVES), tgrid = (unsigned)cdiv(ntensors, SEG_WAVES);
    hipLaunchKernelGGL((seg_row_kernel<SEG_NOVOGRAD, G>), dim3(rgrid), dim3(256), 0, s, rows, rows_total, param, grad,
                       (float*)nullptr, (float*)nullptr, partials, step_dev, beta1, beta2, eps, grad_scale, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL((seg_fold_kernel<SEG_NOVOGRAD, G>), dim3(tgrid), dim3(256), 0, s, tensors, ntensors, partials,
                       (int*)nullptr, (float*)nullptr, norm_avg, step_dev, beta2, eps, 0.f, 1.f, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL((seg_apply_kernel<SEG_NOVOGRAD, G>), dim3(rgrid), dim3(256), 0, s, rows, rows_total, param, grad,
                       exp_avg, (const float*)nullptr, partials, (const int*)nullptr, (const float*)nullptr, norm_avg,
                       lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale, guard);
    XV2_CHECK_LAUNCH();
    hipLaunchKernelGGL(inc_step_kernel<G>, dim3(1), dim3(1), 0, s, step_dev, guard);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_novograd_step_dev(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors,
                                     float* param, const float* grad, float* exp_avg, float* norm_avg, float* partials,
                                     const float* lr_dev, int* step_dev, double beta1, double beta2, float eps,
                                     float weight_decay, float grad_scale, void* stream) {
    OptimGuardScope scope;
    XV2_CHECK_ARG(rows && tensors && param && grad && exp_avg && norm_avg && partials && lr_dev && step_dev &&
                  rows_total > 0 && ntensors > 0, "novograd_step_dev: null buffer or empty table");
    return scope.guard ? novograd_launch<true>(rows, rows_total, tensors, ntensors, param, grad, exp_avg, norm_avg, partials,
                                               lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale, scope.guard,
                                               (hipStream_t)stream)
                       : novograd_launch<false>(rows, rows_total, tensors, ntensors, param, grad, exp_avg, norm_avg, partials,
                                                lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale, nullptr,
                                                (hipStream_t)stream);
}

extern "C" int xv2_ema_update_dev(float* ema, const float* param, int64_t n, double decay, int warmup, int* count_dev,
                                  const void* guard, void* stream) {
    XV2_CHECK_ARG(decay >= 0.0 && decay < 1.0, "ema_update_dev: decay = %g, must lie in [0, 1)", decay);
    XV2_CHECK_ARG(n >= 0, "ema_update_dev: n = %lld, must not be negative", (long long)n);
    if (n == 0) return XV2_OK;
    XV2_CHECK_ARG(ema && param && count_dev, "ema_update_dev: null average, parameter buffer or counter");
    // flat_rule_kernel's grid: one float4 per thread up to 4096 blocks, grid-stride beyond 4096 * 256 * 4 = 2^22 elements
    const int grid = (int)std::min<int64_t>(cdiv(cdiv(n, 4), 256), 4096);
    hipStream_t s = (hipStream_t)stream;
    const float* g = static_cast<const float*>(guard);
    if (g) {
        hipLaunchKernelGGL(ema_update_kernel<true>, dim3(grid), dim3(256), 0, s, ema, param, n, decay, warmup, count_dev, g);
        XV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(inc_step_kernel<true>, dim3(1), dim3(1), 0, s, count_dev, g);
    } else {
        hipLaunchKernelGGL(ema_update_kernel<false>, dim3(grid), dim3(256), 0, s, ema, param, n, decay, warmup, count_dev, g);
        XV2_CHECK_LAUNCH();
        hipLaunchKernelGGL(inc_step_kernel<false>, dim3(1), dim3(1), 0, s, count_dev, g);
    }
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
