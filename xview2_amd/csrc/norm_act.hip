// BatchNorm2d (training and eval) fused with ReLU / LeakyReLU(0.01) / sigmoid and the residual add,
// NHWC.  HBM-bound streaming kernels: 16-byte accesses, channel = fastest index, deterministic
// two-level reductions (fp32 inside a row chunk, fp64 across chunks).
// Reference sites: nn.BatchNorm2d + activation at model/layers.py:16-17,36-37,72,93-94 and in the
// un-vendored ResNet/ResNeSt blocks; torch semantics (biased batch variance for normalisation,
// unbiased for running_var, momentum 0.1, eps 1e-5).
#include "bn_fold.h"
#include "amax_ctx.h"
#include "head_fuse.h"
#include <type_traits>
#include <mutex>
#include <cstring>
#include <algorithm>

namespace xv2 {

// ---------------------------------------------------------------------------------------------
// column partials: for every chunk of `rpb` rows, part[chunk][C][2] = (sum f0, sum f1) per channel.
// F(row, c4 or c, vec) returns the two quantities to accumulate.
struct ChunkGeom {
    int rpb;        // rows per block
    int64_t chunks;
    int cgw;        // channels per block (vector path): C, or 256-channel groups for wide tensors; 0 = generic path
    int groups;
};

// Vector path: a block covers `cgw` channels (cgw/4 float4 lanes x 256/(cgw/4) row lanes) and `rpb` rows; wide
// tensors (C a multiple of 256) are cut into 256-channel groups along grid.y so that a block keeps 4 row lanes and
// the number of row chunks - hence the partial-sum traffic - stays a small fraction of the tensor.
// W = channels per lane of the vector path: 4 (fp32, 16-byte accesses) or 8 (bf16, 16-byte accesses)
static ChunkGeom chunk_geom(int64_t npix, int C, int W = 4) {
    ChunkGeom g;
    g.cgw = 0;
    g.groups = 1;
    if (C % W == 0) {
        if (C > 256 && C % 256 == 0) g.cgw = 256;
        else if (C / W <= 256 && 256 % (C / W) == 0) g.cgw = C;
    }
    if (g.cgw) g.groups = C / g.cgw;
    const int64_t rows_per_pass = g.cgw ? 256 / (g.cgw / W) : 4;
    // (bf16 tensors - W = 8 channels per 16-byte lane - are half the bytes: half the blocks; whole-step sweeps of the block cap,
    //  cfg3 15.75 -> 15.66 ms, cfg2 --precision 16 12.53 -> 12.44 ms; fp32 tensors are indifferent between 1024 and 8192)
    int64_t rpb = cdiv(npix * g.groups, W == 8 ? 1024 : 2048);
    rpb = cdiv(rpb, rows_per_pass) * rows_per_pass;
    if (rpb < rows_per_pass * 8) rpb = rows_per_pass * 8;
    g.rpb = (int)rpb;
    g.chunks = cdiv(npix, rpb);
    return g;
}

// the head behind the last decoder layer (head_fuse.h), as the BatchNorm backward passes see it: dz is never stored, a lane
// rebuilds its 4 channels of it from the pixel's <= 4 logit gradients
struct HeadGrad {
    const float* dl;     // d loss / d logits, [N][Cout][hw] (nchw) or [npix][Cout]
    const float* w;      // head weights [Cout][C]
    int64_t hw;
    int nchw, hw_div;    // hw_div: head_index_fast
};

// MODE 0: tensor stats (x, x*x).  MODE 1: BN backward (g, g*xhat).  MODE 2: MODE 1 with dz = head_dx4(dlogits, w) computed per
// element, the activation mask recomputed from y (COUT = the head's
// output channels; vector path only).
template <int MODE, typename T, int COUT = 0>
struct ColOp {
    struct NoHead {};
    typename std::conditional<MODE == 2, HeadGrad, NoHead>::type head;   // MODE2 only: no kernel argument bytes elsewhere
    const T* a;   // MODE0: x          MODE1: dz
    const T* z;   // MODE1
    const T* y;   // MODE1
    const float* mean;
    const float* invstd;
    const float* scale;   // MODE1 with z == nullptr: the activation mask is recomputed from y*scale+shift
    const float* shift;
    int lda, ldz, ldy, act;
    int zbits;   // z is not the activated output but a byte per float4 of it: bit k = (z[4*j + k] > 0)
    int c4tot;   // float4 per row (mask indexing)
    __device__ __forceinline__ void apply(int64_t row, int c, float& f0, float& f1) const {
        static_assert(MODE != 2 || COUT > 0, "mode 2 needs the head's channel count");
        static_assert(MODE != 2, "mode 2 has no generic form: vector path only (xv2_bn_act_head_supported), rows through applyh");
        if constexpr (MODE == 0) {
            // shifted sums (shift = the tensor's first row): avoids the E[x^2]-E[x]^2 cancellation when
            // |mean| >> std (e.g. split-attention bn1 over a handful of near-equal GAP values)
            const float v = ld1(a + row * lda + c) - ld1(a + c);
            f0 += v;
            f1 += v * v;
        } else {
            const float yv = ld1(y + row * ldy + c);
            const float ag = z ? act_grad_from_output(ld1(z + row * ldz + c), act)
                               : act_grad_from_pre(__fmaf_rn(yv, scale[c], shift[c]), act);
            const float g = ld1(a + row * lda + c) * ag;
            const float xh = (yv - mean[c]) * invstd[c];
            f0 += g;
            f1 += g * xh;
        }
    }
    // one 16-byte access per tensor: NV float4 groups = 4 (fp32) or 8 (bf16) consecutive channels starting at c
    __device__ __forceinline__ void applyv(int64_t row, int c, float4 (&f0)[Vec16<T>::NV], float4 (&f1)[Vec16<T>::NV],
                                           const float4 (&mu)[Vec16<T>::NV], const float4 (&is)[Vec16<T>::NV],
                                           const float4 (&sc)[Vec16<T>::NV], const float4 (&sf)[Vec16<T>::NV]) const {
        constexpr int NV = Vec16<T>::NV;
        static_assert(MODE != 2, "mode 2 rows go through applyh");
        if constexpr (MODE == 0) {
            float4 v[NV];
            Vec16<T>::ld(a + row * lda + c, v);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                v[q].x -= mu[q].x; v[q].y -= mu[q].y; v[q].z -= mu[q].z; v[q].w -= mu[q].w;   // mu = first row (shift)
                f0[q].x += v[q].x; f0[q].y += v[q].y; f0[q].z += v[q].z; f0[q].w += v[q].w;
                f1[q].x += v[q].x * v[q].x; f1[q].y += v[q].y * v[q].y; f1[q].z += v[q].z * v[q].z; f1[q].w += v[q].w * v[q].w;
            }
        } else {
            float4 d[NV], yy[NV], zz[NV];
            Vec16<T>::ld(a + row * lda + c, d);
            Vec16<T>::ld(y + row * ldy + c, yy);
            unsigned m = 0;
            if (z && zbits) {
                const uint8_t* mp = reinterpret_cast<const uint8_t*>(z) + row * c4tot + (c >> 2);
                m = NV == 2 ? *reinterpret_cast<const unsigned short*>(mp) : *mp;
            } else if (z) {
                Vec16<T>::ld(z + row * ldz + c, zz);
            }
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                float gx, gy, gz, gw;
                if (z && zbits) {
                    const unsigned mq = m >> (8 * q);
                    gx = d[q].x * act_grad_from_output((mq & 1u) ? 1.f : -1.f, act); gy = d[q].y * act_grad_from_output((mq & 2u) ? 1.f : -1.f, act);
                    gz = d[q].z * act_grad_from_output((mq & 4u) ? 1.f : -1.f, act); gw = d[q].w * act_grad_from_output((mq & 8u) ? 1.f : -1.f, act);
                } else if (z) {
                    gx = d[q].x * act_grad_from_output(zz[q].x, act); gy = d[q].y * act_grad_from_output(zz[q].y, act);
                    gz = d[q].z * act_grad_from_output(zz[q].z, act); gw = d[q].w * act_grad_from_output(zz[q].w, act);
                } else {
                    gx = d[q].x * act_grad_from_pre(__fmaf_rn(yy[q].x, sc[q].x, sf[q].x), act);
                    gy = d[q].y * act_grad_from_pre(__fmaf_rn(yy[q].y, sc[q].y, sf[q].y), act);
                    gz = d[q].z * act_grad_from_pre(__fmaf_rn(yy[q].z, sc[q].z, sf[q].z), act);
                    gw = d[q].w * act_grad_from_pre(__fmaf_rn(yy[q].w, sc[q].w, sf[q].w), act);
                }
                f0[q].x += gx; f0[q].y += gy; f0[q].z += gz; f0[q].w += gw;
                f1[q].x += gx * ((yy[q].x - mu[q].x) * is[q].x); f1[q].y += gy * ((yy[q].y - mu[q].y) * is[q].y);
                f1[q].z += gz * ((yy[q].z - mu[q].z) * is[q].z); f1[q].w += gw * ((yy[q].w - mu[q].w) * is[q].w);
            }
        }
    }
    // MODE 2: one row of this lane's 4 channels.  dz takes the values the unfused path stores and reads back (rounded to T);
    // the (g, g * xhat) expressions are those of MODE 1 with z == nullptr.
    __device__ __forceinline__ void applyh(int64_t row, int c, float4& f0, float4& f1, const float4& mu, const float4& is,
                                           const float4& sc, const float4& sf, const float4 (&ww)[COUT > 0 ? COUT : 1]) const {
        if constexpr (MODE == 2) {
            float g[COUT];
            head_load_g<COUT>(head.dl, head_index_fast(head.nchw, row, head.hw, COUT, head.hw_div), g);
            const float4 yy = ld4(y + row * ldy + c);
            const float4 d = as_loaded(stored4<T>(head_dx4<COUT>(g, ww)));
            // (MODE 1's sums as the compiler contracts them - the product of f0's term unrounded inside an fma, f1's g rounded first -
            //  spelled out, so that this instantiation cannot contract them any other way: dgamma / dbeta stay bit-equal)
            const float ax = act_grad_from_pre(__fmaf_rn(yy.x, sc.x, sf.x), act), ay = act_grad_from_pre(__fmaf_rn(yy.y, sc.y, sf.y), act);
            const float az = act_grad_from_pre(__fmaf_rn(yy.z, sc.z, sf.z), act), aw = act_grad_from_pre(__fmaf_rn(yy.w, sc.w, sf.w), act);
            const float4 gg = as_loaded(make_float4(d.x * ax, d.y * ay, d.z * az, d.w * aw));
            f0.x = __fmaf_rn(d.x, ax, f0.x); f0.y = __fmaf_rn(d.y, ay, f0.y); f0.z = __fmaf_rn(d.z, az, f0.z); f0.w = __fmaf_rn(d.w, aw, f0.w);
            const float4 xh = as_loaded(make_float4((yy.x - mu.x) * is.x, (yy.y - mu.y) * is.y, (yy.z - mu.z) * is.z, (yy.w - mu.w) * is.w));
            f1.x = __fmaf_rn(gg.x, xh.x, f1.x); f1.y = __fmaf_rn(gg.y, xh.y, f1.y); f1.z = __fmaf_rn(gg.z, xh.z, f1.z); f1.w = __fmaf_rn(gg.w, xh.w, f1.w);
        }
    }
};

// walk order of the streaming kernels (their `rev` argument): the backward apply and the forward apply walk their tensors
// last-to-first, the column sums first-to-last.  `rev` stays a run-time argument of the kernels: the launch sites pass
// these constants, and the kernels' code is the code that was measured.
// (rounds 3 - 5 could fold the chunk / tile partials inside the producing launch - XV2_BN_FOLD, device-scope tickets; removed in
//  round 6: +0.65 ms per cfg2 step once fenced correctly)
constexpr int BN_REV_BWD_APPLY = 1, BN_REV_FWD_APPLY = 1, BN_REV_COLUMN_SUMS = 0;

template <int MODE, typename T, int COUT = 0>
__global__ void __launch_bounds__(256) column_partials_kernel(ColOp<MODE, T, COUT> op, int64_t npix, int C, int rpb, int cgw,
                                                              double* __restrict__ part, int rev) {
    __shared__ float sh[256 * 8 * Vec16<T>::NV];
    const int tid = threadIdx.x;
    // rev: the row chunks are dispatched last-to-first (same chunk -> rows -> partial-row mapping, same sums): the
    // kernel that produced the tensors finished with their last rows
    const int chunk = rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int64_t r0 = (int64_t)chunk * rpb;
    const int64_t r1 = min(r0 + (int64_t)rpb, npix);
    double* out = part + (size_t)chunk * C * 2;
    if (cgw) {
        constexpr int NV = Vec16<T>::NV, W = 4 * NV;
        const int CW = cgw / W;
        const int rpp = 256 / CW;
        const int tx = tid % CW, ty = tid / CW;
        const int cb = blockIdx.y * cgw + tx * W;     // first of this thread's W channels
        float4 f0[NV], f1[NV], g0[NV], g1[NV], mu[NV], is[NV], sc[NV], sf[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            f0[q] = f1[q] = g0[q] = g1[q] = mu[q] = is[q] = sc[q] = sf[q] = make_float4(0, 0, 0, 0);
            if constexpr (MODE >= 1) {
                mu[q] = *reinterpret_cast<const float4*>(op.mean + cb + 4 * q);
                is[q] = *reinterpret_cast<const float4*>(op.invstd + cb + 4 * q);
                if (MODE == 2 || !op.z) {
                    sc[q] = *reinterpret_cast<const float4*>(op.scale + cb + 4 * q);
                    sf[q] = *reinterpret_cast<const float4*>(op.shift + cb + 4 * q);
                }
            } else {
                mu[q] = ld4(op.a + cb + 4 * q);
            }
        }
        // two rows in flight per iteration (independent accumulators): more bytes outstanding per lane
        int64_t r = r0 + ty;
        constexpr int HC = COUT > 0 ? COUT : 1;
        float4 hww[HC];      // MODE 2: the head's weights of this lane's channels
        if constexpr (MODE == 2) {
            static_assert(NV == 1, "the head owns 4 channels per lane");
            head_load_w<COUT>(op.head.w, C, cb, hww);
            for (; r + rpp < r1; r += 2 * rpp) {
                op.applyh(r, cb, f0[0], f1[0], mu[0], is[0], sc[0], sf[0], hww);
                op.applyh(r + rpp, cb, g0[0], g1[0], mu[0], is[0], sc[0], sf[0], hww);
            }
            if (r < r1) op.applyh(r, cb, f0[0], f1[0], mu[0], is[0], sc[0], sf[0], hww);
        } else {
            for (; r + rpp < r1; r += 2 * rpp) {
                op.applyv(r, cb, f0, f1, mu, is, sc, sf);
                op.applyv(r + rpp, cb, g0, g1, mu, is, sc, sf);
            }
            if (r < r1) op.applyv(r, cb, f0, f1, mu, is, sc, sf);
        }
        // per 4-channel group q: the fold below is the one the 4-wide layout performs (same order, same result)
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            f0[q].x += g0[q].x; f0[q].y += g0[q].y; f0[q].z += g0[q].z; f0[q].w += g0[q].w;
            f1[q].x += g1[q].x; f1[q].y += g1[q].y; f1[q].z += g1[q].z; f1[q].w += g1[q].w;
            float* s = sh + (tid * NV + q) * 8;
            s[0] = f0[q].x; s[1] = f0[q].y; s[2] = f0[q].z; s[3] = f0[q].w;
            s[4] = f1[q].x; s[5] = f1[q].y; s[6] = f1[q].z; s[7] = f1[q].w;
        }
        __syncthreads();
        if (tid < CW * NV) {          // one thread per 4-channel group of the block's cgw channels
            const int lane = tid / NV, q = tid % NV;
            double a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0};
            for (int rr = 0; rr < rpp; ++rr) {
                const float* t = sh + ((rr * CW + lane) * NV + q) * 8;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a0[k] += t[k];
                    a1[k] += t[4 + k];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double* o = out + (blockIdx.y * cgw + tid * 4 + k) * 2;
                o[0] = a0[k];
                o[1] = a1[k];
            }
        }
    } else if constexpr (MODE != 2) {
        // generic fallback: 64 channel lanes x 4 row lanes
        const int tx = tid & 63, ty = tid >> 6;
        for (int cb = 0; cb < C; cb += 64) {
            const int c = cb + tx;
            // narrow / odd channel counts (e.g. the 1-channel psi BN): few lanes, long columns -> fp64 running
            // sums, flushed from fp32 every 16 rows
            double d0 = 0.0, d1 = 0.0;
            if (c < C) {
                float f0 = 0.f, f1 = 0.f;
                int k = 0;
                for (int64_t r = r0 + ty; r < r1; r += 4) {
                    op.apply(r, c, f0, f1);
                    if (++k == 16) {
                        d0 += f0; d1 += f1;
                        f0 = f1 = 0.f;
                        k = 0;
                    }
                }
                d0 += f0; d1 += f1;
            }
            double* shd = reinterpret_cast<double*>(sh);
            shd[tid * 2] = d0;
            shd[tid * 2 + 1] = d1;
            __syncthreads();
            if (ty == 0 && c < C) {
                double a0 = 0.0, a1 = 0.0;
                for (int q = 0; q < 4; ++q) {
                    a0 += shd[(q * 64 + tx) * 2];
                    a1 += shd[(q * 64 + tx) * 2 + 1];
                }
                out[c * 2] = a0;
                out[c * 2 + 1] = a1;
            }
            __syncthreads();
        }
    }
}

// Tile partials -> per-channel sums in ONE launch.  grid (ceil(C/32), S): block (g, s) folds its contiguous range of
// tiles for 32 channels into scratch[s][C][2]; the LAST block of a channel group to arrive (device-scope ticket)
// then adds the S scratch rows in index order - so the result does not depend on which block that is - and, when
// `fin.mean` is set, derives the BatchNorm coefficients and running statistics for its channels on the spot.
template <typename T>
__global__ void __launch_bounds__(256) reduce_stats_kernel(const T* __restrict__ part, int64_t tiles, int C, int S,
                                                           double* __restrict__ scratch, unsigned* __restrict__ tickets,
                                                           double* __restrict__ sums, float* __restrict__ f0,
                                                           float* __restrict__ f1, const BnFinalize fin) {
    __shared__ double sh[256 * 2];
    __shared__ int is_last;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 channels x 8 row lanes
    const int c = blockIdx.x * 32 + tx;
    const int64_t per = cdiv(tiles, S);
    const int64_t t0 = (int64_t)blockIdx.y * per, t1 = min(t0 + per, tiles);
    double a0 = 0.0, a1 = 0.0;
    if (c < C) {
        double e0 = 0.0, e1 = 0.0;
        int64_t t = t0 + ty;
        for (; t + 8 < t1; t += 16) {     // two tiles in flight
            a0 += (double)part[((size_t)t * C + c) * 2];
            a1 += (double)part[((size_t)t * C + c) * 2 + 1];
            e0 += (double)part[((size_t)(t + 8) * C + c) * 2];
            e1 += (double)part[((size_t)(t + 8) * C + c) * 2 + 1];
        }
        if (t < t1) {
            a0 += (double)part[((size_t)t * C + c) * 2];
            a1 += (double)part[((size_t)t * C + c) * 2 + 1];
        }
        a0 += e0;
        a1 += e1;
    }
    sh[threadIdx.x * 2] = a0;
    sh[threadIdx.x * 2 + 1] = a1;
    __syncthreads();
    if (ty == 0 && c < C) {
        double b0 = 0.0, b1 = 0.0;
        for (int q = 0; q < 8; ++q) {
            b0 += sh[(q * 32 + tx) * 2];
            b1 += sh[(q * 32 + tx) * 2 + 1];
        }
        // device-scope (write-through) stores: a release FENCE here would write back the whole L2 of this XCD,
        // which still holds the conv output of the previous kernel (measured: +25 us per launch)
        __hip_atomic_store(&scratch[((size_t)blockIdx.y * C + c) * 2], b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&scratch[((size_t)blockIdx.y * C + c) * 2 + 1], b1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (S > 1) {
        __builtin_amdgcn_s_waitcnt(0);   // the row has reached the device coherence point ...
        __syncthreads();
        if (threadIdx.x == 0) {          // ... before the ticket is drawn
            const unsigned prev = __hip_atomic_fetch_add(&tickets[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            is_last = (prev == (unsigned)(S - 1));
            if (is_last) {
                __hip_atomic_store(&tickets[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // the scratch rows are re-used launch after launch: drop what this CU / XCD still caches of them
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
        }
        __syncthreads();
        if (!is_last) return;
    } else {
        __syncthreads();
    }
    // last block: 4 row quarters x (32 channels x 2 statistics); each thread adds its quarter of the S rows with four
    // loads in flight (device-scope loads cost a memory round trip each), then the quarters are combined in order
    const int t64 = threadIdx.x & 63, quarter = threadIdx.x >> 6;
    const int ch = blockIdx.x * 32 + (t64 >> 1), which = t64 & 1;
    double a = 0.0;
    if (ch < C) {
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
        const size_t i = (size_t)ch * 2 + which, stride = (size_t)C * 2;
        auto ld = [&](int row) {   // device-scope loads: the rows were written by blocks on other XCDs
            return __hip_atomic_load(&scratch[(size_t)row * stride + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        const int rq = (S + 3) >> 2;
        int r = quarter * rq;
        const int rend = min(r + rq, S);
        for (; r + 4 <= rend; r += 4) {
            q0 += ld(r);
            q1 += ld(r + 1);
            q2 += ld(r + 2);
            q3 += ld(r + 3);
        }
        for (; r < rend; ++r) q0 += ld(r);
        a = (q0 + q1) + (q2 + q3);
    }
    __syncthreads();          // sh[] (phase 1) is free again
    sh[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    a = (sh[t64] + sh[64 + t64]) + (sh[128 + t64] + sh[192 + t64]);
    if (ch < C) {
        const size_t i = (size_t)ch * 2 + which;
        sums[i] = a;
        if (f0 && !which) f0[ch] = (float)a;   // BN backward: dbeta = sum g
        if (f1 && which) f1[ch] = (float)a;    //              dgamma = sum g*xhat
    }
    if (fin.mean) {
        const double other = __shfl_xor(a, 1, 64);
        if (ch < C && !which) bn_finalize_channel(fin, ch, a, other);
    }
}

// The same reduction for the layers whose partial count is small (<= RS1_MAX_TILES: every layer of the /4 ... /32 levels at
// batch 2) in ONE phase: a block of 1024 threads = 32 channels x 32 row lanes reads all rows of its channels with eight 8-byte
// loads in flight per lane (one or two memory round trips), folds the lanes through LDS in lane order and finalises.  No scratch
// rows, no ticket, no device-scope hand-off: the two-phase kernel above spends 5 - 8 us per launch on exactly those (a dependent
// atomic, an acquire fence, a second round of device-scope loads) for a few hundred KB of partials - 126 launches per cfg2 step,
// ~60 per resnest50 encoder forward, 1200 per cfg5 step, each on the compute stream's critical path.  fp64 sums in a fixed order
// (lane r adds rows r, r + 32, ... in row order; lanes in lane order), like every reduction here.
constexpr int64_t RS1_MAX_TILES = 1024;
template <typename T>
__global__ void __launch_bounds__(1024) reduce_stats_1phase_kernel(const T* __restrict__ part, int64_t tiles, int C,
                                                                    double* __restrict__ sums, float* __restrict__ f0,
                                                                    float* __restrict__ f1, const BnFinalize fin) {
    __shared__ double sh[1024 * 2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + tx;
    double a0 = 0.0, a1 = 0.0;
    if (c < C) {
        typedef T T2 __attribute__((ext_vector_type(2)));
        const T2* p2 = reinterpret_cast<const T2*>(part) + c;
        for (int64_t t = ty; t < tiles; t += 32 * 8) {
            T2 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t tt = t + 32 * i;
                v[i] = p2[(size_t)(tt < tiles ? tt : t) * C];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (t + 32 * i < tiles) {
                    a0 += (double)v[i].x;
                    a1 += (double)v[i].y;
                }
        }
    }
    sh[threadIdx.x * 2] = a0;
    sh[threadIdx.x * 2 + 1] = a1;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int t64 = threadIdx.x, ch = blockIdx.x * 32 + (t64 >> 1), which = t64 & 1;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;      // four chains over the 32 row lanes, combined in a fixed order
#pragma unroll
    for (int q = 0; q < 32; q += 4) {
        q0 += sh[((q + 0) * 32 + (t64 >> 1)) * 2 + which];
        q1 += sh[((q + 1) * 32 + (t64 >> 1)) * 2 + which];
        q2 += sh[((q + 2) * 32 + (t64 >> 1)) * 2 + which];
        q3 += sh[((q + 3) * 32 + (t64 >> 1)) * 2 + which];
    }
    const double a = (q0 + q1) + (q2 + q3);
    if (ch < C) {
        const size_t i = (size_t)ch * 2 + which;
        sums[i] = a;
        if (f0 && !which) f0[ch] = (float)a;   // BN backward: dbeta = sum g
        if (f1 && which) f1[ch] = (float)a;    //              dgamma = sum g*xhat
    }
    if (fin.mean) {
        const double other = __shfl_xor(a, 1, 64);
        if (ch < C && !which) bn_finalize_channel(fin, ch, a, other);
    }
}

// ticket counters for reduce_stats_kernel: a zero-initialised device pool handed out round-robin; every user
// returns its counters to zero, so concurrent launches on different streams never share a live ticket.
unsigned* take_tickets(int n) {
    // one pool per device (a host thread may drive several devices; the counters must live on the device that launches)
    constexpr size_t POOL = 1 << 16;
    constexpr int MAXDEV = 16;
    static unsigned* pool[MAXDEV] = {};
    static size_t cursor[MAXDEV] = {};
    static std::mutex mu;
    int dev = 0;
    if (n <= 0 || (size_t)n > POOL || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;   // callers check
    std::lock_guard<std::mutex> lk(mu);
    if (!pool[dev]) {
        unsigned* p = nullptr;
        if (hipMalloc(&p, POOL * sizeof(unsigned)) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, POOL * sizeof(unsigned)) != hipSuccess) {
            (void)hipFree(p);
            return nullptr;
        }
        pool[dev] = p;
    }
    if (cursor[dev] + (size_t)n > POOL) cursor[dev] = 0;
    unsigned* p = pool[dev] + cursor[dev];
    cursor[dev] += (size_t)n;
    return p;
}

// sums of (x - s) and (x - s)^2  ->  sums of x and x^2, in fp64 (no cancellation at this precision)
__global__ void unshift_stats_kernel(double* __restrict__ sums, const float* __restrict__ x, double n, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double sh = (double)x[c], s1 = sums[c * 2], s2 = sums[c * 2 + 1];
    sums[c * 2] = s1 + n * sh;
    sums[c * 2 + 1] = s2 + 2.0 * sh * s1 + n * sh * sh;
}

template <typename T>
static int reduce_stats(const T* partial, int64_t tiles, int C, double* sums, double* scratch, hipStream_t st,
                        float* f0 = nullptr, float* f1 = nullptr, const BnFinalize* fin = nullptr) {
    int S = (int)std::min<int64_t>(XV2_BN_SCRATCH_ROWS, cdiv(tiles, 16));
    if (S < 1) S = 1;
    const int groups = (int)cdiv(C, 32);
    XV2_CHECK_ARG(groups <= 4096, "reduce_stats: C=%d too large", C);
    if (tiles <= RS1_MAX_TILES) {
        BnFinalize none1;
        memset(&none1, 0, sizeof(none1));
        hipLaunchKernelGGL(reduce_stats_1phase_kernel<T>, dim3((unsigned)groups), dim3(1024), 0, st, partial, tiles, C, sums, f0, f1,
                           fin ? *fin : none1);
        XV2_CHECK_LAUNCH();
        return XV2_OK;
    }
    unsigned* tickets = S > 1 ? take_tickets(groups) : nullptr;
    XV2_CHECK_ARG(S == 1 || tickets, "reduce_stats: ticket pool allocation failed");
    BnFinalize none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(reduce_stats_kernel<T>, dim3((unsigned)groups, S), dim3(256), 0, st, partial, tiles, C, S,
                       scratch, tickets, sums, f0, f1, fin ? *fin : none);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

__global__ void bn_finalize_kernel(const double* __restrict__ sums, const BnFinalize fin, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(fin, c, sums[c * 2], sums[c * 2 + 1]);
}

__global__ void bn_eval_coeffs_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                      float* __restrict__ scale, float* __restrict__ shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float is = 1.f / sqrtf(rv[c] + eps);
    const float sc = (gamma ? gamma[c] : 1.f) * is;
    scale[c] = sc;
    shift[c] = (beta ? beta[c] : 0.f) - rm[c] * sc;
}

template <bool VEC, typename T>
__global__ void __launch_bounds__(256) bn_act_fwd_kernel(const T* __restrict__ y, int ldy,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const T* __restrict__ res, int ldr, int act,
                                                          T* __restrict__ z, int ldz, int64_t npix, int C,
                                                          uint8_t* __restrict__ zmask, int rev, unsigned* __restrict__ amax) {
    __shared__ float amax_red[4];
    float zmax = 0.f;       // F16X2: max |z| of this block's elements (recorded for the convolutions that read z)
    if constexpr (VEC) {
        constexpr int NV = Vec16<T>::NV, W = 4 * NV;     // 16-byte accesses: 4 (fp32) / 8 (bf16) channels per lane
        const int CW = C / W;
        const int64_t total = npix * CW;
        // rev: last element first - the convolution that wrote y finished with its last rows, and the convolution that
        // reads z starts with the first ones: both ends of this pass then meet data the memory-side cache still holds
        for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = rev ? total - 1 - j : j;
            const int64_t row = i / CW;
            const int c = (int)(i - row * CW) * W;
            float4 v[NV], r[NV], o[NV];
            Vec16<T>::ld(y + row * ldy + c, v);
            if (res) Vec16<T>::ld(res + row * ldr + c, r);
            unsigned mbits = 0;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const float4 sc = *reinterpret_cast<const float4*>(scale + c + 4 * q);
                const float4 sh = *reinterpret_cast<const float4*>(shift + c + 4 * q);
                o[q] = bn_act_apply4(v[q], sc, sh, res ? &r[q] : nullptr, act);
                mbits |= (unsigned)((o[q].x > 0.f) | ((o[q].y > 0.f) << 1) | ((o[q].z > 0.f) << 2) | ((o[q].w > 0.f) << 3)) << (8 * q);
                zmax = amax_acc(zmax, o[q]);
            }
            Vec16<T>::st(z + row * ldz + c, o);
            if (zmask) {      // one byte per 4 channels, dense rows: byte index = row * C/4 + c/4
                if constexpr (NV == 2) reinterpret_cast<unsigned short*>(zmask)[i] = (unsigned short)mbits;
                else zmask[i] = (uint8_t)mbits;
            }
        }
    } else {
        const int64_t total = npix * C;
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int64_t row = i / C;
            const int c = (int)(i - row * C);
            float o = __fmaf_rn(ld1(y + row * ldy + c), scale[c], shift[c]);
            if (res) o += ld1(res + row * ldr + c);
            o = apply_act(o, act);
            zmax = amax_acc(zmax, make_float4(o, o, o, o));
            st1(z + row * ldz + c, o);
        }
    }
    if (amax) amax_record(amax, zmax, amax_red);
}

// BatchNorm apply + activation + the <= 4-channel head of the last decoder layer in ONE pass (model/layers.py:93-94 ConvLayer's norm
// and activation, then OutputBlock's 1x1 convolution, model/layers.py:177,180): z = act(y * scale + shift) lives in registers only -
// the head is its single consumer and the BatchNorm backward recomputes the activation mask from y - and only the logits are
// written.  head_fwd_kernel's lane <-> channel ownership (4 channels per lane, L = C / 4 lanes per pixel, the same shuffle tree)
// and the shared per-lane functions of head_fuse.h: the logits are bit-identical to bn_act_fwd_kernel + head_fwd_kernel.  C = 4 * L,
// so a lane keeps its coefficients and head weights in registers.  Pixels are walked last-to-first like bn_act_fwd_kernel (rev):
// the convolution that wrote y finished with its last rows.  No amax record: no MFMA kernel reads z.
template <int COUT, typename T>
__global__ void __launch_bounds__(256) bn_act_head_fwd_kernel(const T* __restrict__ y, int ldy, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int act, int64_t npix, int64_t hw,
                                                               int C, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ logits, int nchw, int hw_div, int L, int rev) {
    const int lane_in = threadIdx.x % L;
    const int gpb = 256 / L;
    const int c = lane_in * 4;
    const float4 sc = *reinterpret_cast<const float4*>(scale + c), sh = *reinterpret_cast<const float4*>(shift + c);
    float4 ww[COUT];
    head_load_w<COUT>(w, C, c, ww);
    const int64_t gstride = (int64_t)gridDim.x * gpb;
    auto pixel = [&](int64_t p, const float4& v) {
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
        head_dot4<COUT>(as_loaded(stored4<T>(bn_act_apply4(v, sc, sh, nullptr, act))), ww, acc);
        head_lane_sum<COUT>(acc, L);
        if (lane_in == 0) head_store<COUT>(logits, acc, bias, head_index_fast(nchw, p, hw, COUT, hw_div));
    };
    // two pixels in flight per lane: the loads are all this pass waits for
    int64_t j = (int64_t)blockIdx.x * gpb + threadIdx.x / L;
    for (; j + gstride < npix; j += 2 * gstride) {
        const int64_t p0 = rev ? npix - 1 - j : j, p1 = rev ? npix - 1 - (j + gstride) : j + gstride;
        const float4 v0 = ld4(y + p0 * ldy + c), v1 = ld4(y + p1 * ldy + c);
        pixel(p0, v0);
        pixel(p1, v1);
    }
    if (j < npix) {
        const int64_t p0 = rev ? npix - 1 - j : j;
        pixel(p0, ld4(y + p0 * ldy + c));
    }
}

template <bool VEC, typename T>
__global__ void __launch_bounds__(256) bn_act_bwd_kernel(const T* __restrict__ dz, int lddz,
                                                          const T* __restrict__ z, int ldz,
                                                          const T* __restrict__ y, int ldy,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const double* __restrict__ sums2, double count, int act,
                                                          int train, T* __restrict__ dy, int lddy,
                                                          T* __restrict__ dres, int lddres, int64_t npix, int C,
                                                          int zbits) {
    const float inv_count = (float)(1.0 / count);
    constexpr int V = VEC ? 4 : 1;
    const int CV = C / V;
    const int64_t total = npix * CV;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / CV;
        const int c = (int)(i - row * CV) * V;
        float d[V], zz[V], yy[V], o[V], g[V];
        const bool need_y = train || !z;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(d) = ld4(dz + row * lddz + c);
            if (z && zbits) {
                const unsigned m = reinterpret_cast<const uint8_t*>(z)[i];
#pragma unroll
                for (int k = 0; k < V; ++k) zz[k] = ((m >> k) & 1u) ? 1.f : -1.f;
            } else if (z) {
                *reinterpret_cast<float4*>(zz) = ld4(z + row * ldz + c);
            }
            if (need_y) *reinterpret_cast<float4*>(yy) = ld4(y + row * ldy + c);
        } else {
            d[0] = ld1(dz + row * lddz + c);
            if (z) zz[0] = ld1(z + row * ldz + c);
            if (need_y) yy[0] = ld1(y + row * ldy + c);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            g[k] = d[k] * (z ? act_grad_from_output(zz[k], act)
                             : act_grad_from_pre(__fmaf_rn(yy[k], scale[c + k], shift[c + k]), act));
            const float gi = (gamma ? gamma[c + k] : 1.f) * invstd[c + k];
            if (train) {
                const float xh = (yy[k] - mean[c + k]) * invstd[c + k];
                const float sg = (float)sums2[(c + k) * 2] * inv_count;
                const float sgx = (float)sums2[(c + k) * 2 + 1] * inv_count;
                o[k] = gi * (g[k] - sg - xh * sgx);
            } else {
                o[k] = gi * g[k];
            }
        }
        if constexpr (VEC) {
            st4(dy + row * lddy + c, *reinterpret_cast<float4*>(o));
            if (dres) st4(dres + row * lddres + c, *reinterpret_cast<float4*>(g));
        } else {
            st1(dy + row * lddy + c, o[0]);
            if (dres) st1(dres + row * lddres + c, g[0]);
        }
    }
}

// Streaming form for C % 4 == 0 with C/4 dividing 256 (every conv layer of the U-Net): a thread owns ONE group of
// 4 channels for its whole life, so the seven per-channel coefficient vectors are loaded once into registers and
// the loop body is 2-3 16-byte loads + one 16-byte store per element vector (HBM-bound).
template <typename T>
__global__ void __launch_bounds__(256) bn_act_bwd_rows_kernel(const T* __restrict__ dz, int lddz,
                                                               const T* __restrict__ z, int ldz,
                                                               const T* __restrict__ y, int ldy,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const double* __restrict__ sums2, double count, int act,
                                                               int train, T* __restrict__ dy, int lddy,
                                                               T* __restrict__ dres, int lddres, int64_t npix, int cgw,
                                                               int rows_per_block, int zbits, int c4tot, int rev,
                                                               unsigned* __restrict__ amax) {
    __shared__ float amax_red[4];
    float dmax = 0.f;       // F16X2: max |dy| of this block (recorded for the backward-data / weight-gradient launches)
    constexpr int NV = Vec16<T>::NV, W = 4 * NV;      // 16-byte accesses: 4 (fp32) / 8 (bf16) channels per lane
    const int CW = cgw / W, rpp = 256 / CW;
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int c = blockIdx.y * cgw + tx * W;
    const float inv_count = (float)(1.0 / count);
    float gi[W], mu[W], is[W], sg[W], sgx[W], sc[W], sf[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        is[k] = invstd[c + k];
        mu[k] = mean[c + k];
        gi[k] = (gamma ? gamma[c + k] : 1.f) * is[k];
        sg[k] = train ? (float)sums2[(c + k) * 2] * inv_count : 0.f;
        sgx[k] = train ? (float)sums2[(c + k) * 2 + 1] * inv_count : 0.f;
        sc[k] = z ? 0.f : scale[c + k];
        sf[k] = z ? 0.f : shift[c + k];
    }
    // row blocks run LAST-to-first: the column-sum pass that precedes this one walked dz / y first-to-last, so the tail
    // of both tensors is what the memory-side cache (256 MB) still holds
    const int64_t r0 = (int64_t)(rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * rows_per_block;
    const int64_t r1 = min(r0 + (int64_t)rows_per_block, npix);
    const bool need_y = train || !z;
    auto row = [&](int64_t r, const float4 (&dv)[NV], const float4 (&zv)[NV], const float4 (&yv)[NV], unsigned m) {
        float4 ov[NV], gv[NV];
        const float* d = reinterpret_cast<const float*>(dv);
        const float* yy = reinterpret_cast<const float*>(yv);
        float* o = reinterpret_cast<float*>(ov);
        float* g = reinterpret_cast<float*>(gv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float zz;
            if (z && zbits) zz = ((m >> (8 * (k >> 2) + (k & 3))) & 1u) ? 1.f : -1.f;
            else if (z) zz = reinterpret_cast<const float*>(zv)[k];
            else zz = 0.f;
            g[k] = d[k] * (z ? act_grad_from_output(zz, act) : act_grad_from_pre(__fmaf_rn(yy[k], sc[k], sf[k]), act));
            if (train) {
                const float xh = (yy[k] - mu[k]) * is[k];
                o[k] = gi[k] * (g[k] - sg[k] - xh * sgx[k]);
            } else {
                o[k] = gi[k] * g[k];
            }
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) dmax = amax_acc(dmax, ov[q]);
        Vec16<T>::st(dy + r * lddy + c, ov);
        if (dres) Vec16<T>::st(dres + r * lddres + c, gv);
    };
    auto fetch = [&](int64_t r, float4 (&dv)[NV], float4 (&zv)[NV], float4 (&yv)[NV], unsigned& m) {
        Vec16<T>::ld(dz + r * lddz + c, dv);
        m = 0;
        if (z && zbits) {
            const uint8_t* mp = reinterpret_cast<const uint8_t*>(z) + r * c4tot + (c >> 2);
            m = NV == 2 ? *reinterpret_cast<const unsigned short*>(mp) : *mp;
        } else if (z) {
            Vec16<T>::ld(z + r * ldz + c, zv);
        }
        if (need_y) Vec16<T>::ld(y + r * ldy + c, yv);
    };
    // (two rows in flight per iteration were measured SLOWER here - 2.30 -> 2.42 ms per cfg2 step in fp32, 1.48 -> 1.69 in
    // bf16: the extra registers cost more occupancy than the deeper per-lane queue buys)
    for (int64_t r = r0 + ty; r < r1; r += rpp) {
        float4 d0[NV], z0[NV], y0[NV];
        unsigned m0;
        fetch(r, d0, z0, y0, m0);
        row(r, d0, z0, y0, m0);
    }
    if (amax) amax_record(amax, dmax, amax_red);
}

// The head form of the apply pass (training mode, no residual; C = 4 * L): dz is not read but rebuilt per element from the pixel's
// logit gradients (head_dx4, rounded to the storage type like the tensor head_bwd_kernel would have stored), dy is the expression
// of bn_act_bwd_rows_kernel, and - dy being elementwise, the pass is free to walk the tensor as it likes - the walk is
// head_bwd_kernel's: block b, group grp takes pixels b * gpb + grp, + gridDim * gpb, ...; the head's dw / db partials (z recomputed
// from the y this pass reads anyway) are therefore head_bwd_kernel's sums in head_bwd_kernel's order, folded over the block's
// groups in the same order: dw / db come out bit-identical to the unfused path.  part: [gridDim][COUT][C + 1].
template <int COUT, typename T>
__global__ void __launch_bounds__(256) bn_act_bwd_rows_head_kernel(const HeadGrad head, const T* __restrict__ y, int ldy,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                    const float* __restrict__ gamma, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, const double* __restrict__ sums2,
                                                                    double count, int act, T* __restrict__ dy, int lddy, int64_t npix,
                                                                    int C, int L, float* __restrict__ part, unsigned* __restrict__ amax) {
    __shared__ float sh[256 * 4 * COUT];      // [gpb][COUT][4 * L]
    __shared__ float amax_red[4];
    float dmax = 0.f;       // F16X2: max |dy| of this block
    const int tid = threadIdx.x;
    const int lane_in = tid % L, grp = tid / L, gpb = 256 / L;
    const int c = lane_in * 4;
    const float inv_count = (float)(1.0 / count);
    const float4 mu = *reinterpret_cast<const float4*>(mean + c), is = *reinterpret_cast<const float4*>(invstd + c);
    const float4 sc = *reinterpret_cast<const float4*>(scale + c), sf = *reinterpret_cast<const float4*>(shift + c);
    float gi[4], sg[4], sgx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        gi[k] = (gamma ? gamma[c + k] : 1.f) * invstd[c + k];
        sg[k] = (float)sums2[(c + k) * 2] * inv_count;
        sgx[k] = (float)sums2[(c + k) * 2 + 1] * inv_count;
    }
    float4 ww[COUT], dwacc[COUT];
    float dbacc[COUT];
    head_load_w<COUT>(head.w, C, c, ww);
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        dwacc[o] = make_float4(0, 0, 0, 0);
        dbacc[o] = 0.f;
    }
    const int64_t gstride = (int64_t)gridDim.x * gpb;
    for (int64_t p = (int64_t)blockIdx.x * gpb + grp; p < npix; p += gstride) {
        float g[COUT];
        head_load_g<COUT>(head.dl, head_index_fast(head.nchw, p, head.hw, COUT, head.hw_div), g);
        const float4 yy = ld4(y + p * ldy + c);
        const float4 d = as_loaded(stored4<T>(head_dx4<COUT>(g, ww)));
        const float4 pre = make_float4(__fmaf_rn(yy.x, sc.x, sf.x), __fmaf_rn(yy.y, sc.y, sf.y), __fmaf_rn(yy.z, sc.z, sf.z),
                                       __fmaf_rn(yy.w, sc.w, sf.w));
        // dy = gi * (g - sg - xhat * sgx), spelled as bn_act_bwd_rows_kernel compiles it: g and xhat rounded, then one fma
        const float4 gg = as_loaded(make_float4(d.x * act_grad_from_pre(pre.x, act), d.y * act_grad_from_pre(pre.y, act),
                                                d.z * act_grad_from_pre(pre.z, act), d.w * act_grad_from_pre(pre.w, act)));
        const float4 xh = as_loaded(make_float4((yy.x - mu.x) * is.x, (yy.y - mu.y) * is.y, (yy.z - mu.z) * is.z, (yy.w - mu.w) * is.w));
        float4 o;
        o.x = gi[0] * __fmaf_rn(-xh.x, sgx[0], gg.x - sg[0]); o.y = gi[1] * __fmaf_rn(-xh.y, sgx[1], gg.y - sg[1]);
        o.z = gi[2] * __fmaf_rn(-xh.z, sgx[2], gg.z - sg[2]); o.w = gi[3] * __fmaf_rn(-xh.w, sgx[3], gg.w - sg[3]);
        dmax = amax_acc(dmax, o);
        st4(dy + p * lddy + c, o);
        // the head's own gradients, as head_bwd_kernel takes them from the stored z
        const float4 z = as_loaded(stored4<T>(make_float4(apply_act(pre.x, act), apply_act(pre.y, act), apply_act(pre.z, act),
                                                           apply_act(pre.w, act))));
        head_dw4<COUT>(g, z, dwacc);
        if (lane_in == 0) {
#pragma unroll
            for (int o2 = 0; o2 < COUT; ++o2) dbacc[o2] += g[o2];
        }
    }
    // fold over the groups of this block: head_bwd_kernel's, in its order
    float* mypart = part + (size_t)blockIdx.x * COUT * (C + 1);
#pragma unroll
    for (int o = 0; o < COUT; ++o) *reinterpret_cast<float4*>(sh + ((grp * COUT + o) * L + lane_in) * 4) = dwacc[o];
    __syncthreads();
    for (int i = tid; i < COUT * L * 4; i += 256) {
        const int o = i / (L * 4), k = i % (L * 4);
        float s = 0.f;
        for (int q = 0; q < gpb; ++q) s += sh[((q * COUT + o) * L) * 4 + k];
        mypart[o * (C + 1) + k] = s;
    }
    __syncthreads();
    if (lane_in == 0) {
#pragma unroll
        for (int o = 0; o < COUT; ++o) sh[grp * COUT + o] = dbacc[o];
    }
    __syncthreads();
    if (tid < COUT) {
        float s = 0.f;
        for (int q = 0; q < gpb; ++q) s += sh[q * COUT + tid];
        mypart[tid * (C + 1) + C] = s;
    }
    if (amax) amax_record(amax, dmax, amax_red);
}

// ---- the projection shortcut of a bottleneck block inside the block's last BatchNorm passes (include/xv2.h "shortcut fusion") ----
// z = act(BN3(y3) + BN_ds(y_ds)): the shortcut's normalised output r (forward) and the residual gradient (backward) are pure
// functions of what the neighbouring pass of BN3 already holds in registers, so neither tensor is stored.  Every value the unfused
// launches store and read back (r, the residual gradient) passes through stored4<T> + as_loaded here; the sums and dy are spelled
// with explicit fmas the way the unfused kernels contract them: all results are bit-identical to the launches replaced.
// Dense tensors, the vector path of chunk_geom, 4 channels per lane.

// forward apply of both BatchNorms: bn_act_fwd_kernel<true>'s walk (rev), mask byte and maximum record
template <typename T>
__global__ void __launch_bounds__(256) bn_act_shortcut_fwd_kernel(const T* __restrict__ y3, const T* __restrict__ yd,
                                                                   const float* __restrict__ scale3, const float* __restrict__ shift3,
                                                                   const float* __restrict__ scaled, const float* __restrict__ shiftd,
                                                                   int act, T* __restrict__ z, int64_t npix, int C,
                                                                   uint8_t* __restrict__ zmask, int rev, unsigned* __restrict__ amax) {
    __shared__ float amax_red[4];
    float zmax = 0.f;
    const int CW = C / 4;
    const int64_t total = npix * CW;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = rev ? total - 1 - j : j;
        const int64_t row = i / CW;
        const int c = (int)(i - row * CW) * 4;
        const float4 v3 = ld4(y3 + row * C + c), vd = ld4(yd + row * C + c);
        const float4 sc3 = *reinterpret_cast<const float4*>(scale3 + c), sh3 = *reinterpret_cast<const float4*>(shift3 + c);
        const float4 scd = *reinterpret_cast<const float4*>(scaled + c), shd = *reinterpret_cast<const float4*>(shiftd + c);
        // the shortcut's output as its own apply pass stores it (no residual, no activation) and BN3's apply pass loads it
        const float4 r = as_loaded(stored4<T>(bn_act_apply4(vd, scd, shd, nullptr, XV2_ACT_NONE)));
        const float4 o = bn_act_apply4(v3, sc3, sh3, &r, act);
        zmax = amax_acc(zmax, o);
        st4(z + row * C + c, o);
        zmask[i] = (uint8_t)((o.x > 0.f) | ((o.y > 0.f) << 1) | ((o.z > 0.f) << 2) | ((o.w > 0.f) << 3));
    }
    if (amax) amax_record(amax, zmax, amax_red);
}

struct ShortcutBn {      // one BatchNorm of the pair, as the backward passes see it
    const float* mean;
    const float* invstd;
    const float* gamma;
};

// Column pass with two sum pairs: column_partials_kernel<1>'s chunk -> rows -> partial-row mapping, its two rows in flight and
// its in-block fold, once for BN3 (sum g, sum g * xhat3: mode 1 with the byte mask) and once for the shortcut (sum gs, sum gs *
// xhat_ds: mode 1 with act = NONE and z == nullptr, reading the stored residual gradient gs).  part: [chunk][2C][2], BN3's channels
// first - reduce_stats<double> then folds both layers in one launch over 2C channels.
template <typename T>
__global__ void __launch_bounds__(256) column_partials_shortcut_kernel(const T* __restrict__ dz, const uint8_t* __restrict__ zmask,
                                                                        const T* __restrict__ y3, const T* __restrict__ yd,
                                                                        const ShortcutBn b3, const ShortcutBn bd, int act,
                                                                        int64_t npix, int C, int rpb, int cgw,
                                                                        double* __restrict__ part, int rev) {
    __shared__ float sh3[256 * 8];
    __shared__ float shd[256 * 8];
    const int tid = threadIdx.x;
    const int chunk = rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x;
    const int64_t r0 = (int64_t)chunk * rpb;
    const int64_t r1 = min(r0 + (int64_t)rpb, npix);
    double* out = part + (size_t)chunk * C * 4;
    const int CW = cgw / 4, c4tot = C / 4;
    const int rpp = 256 / CW;
    const int tx = tid % CW, ty = tid / CW;
    const int cb = blockIdx.y * cgw + tx * 4;
    const float4 mu3 = *reinterpret_cast<const float4*>(b3.mean + cb), is3 = *reinterpret_cast<const float4*>(b3.invstd + cb);
    const float4 mud = *reinterpret_cast<const float4*>(bd.mean + cb), isd = *reinterpret_cast<const float4*>(bd.invstd + cb);
    const float4 zero = make_float4(0, 0, 0, 0);
    float4 f0 = zero, f1 = zero, g0 = zero, g1 = zero;      // BN3: two rows in flight
    float4 h0 = zero, h1 = zero, k0 = zero, k1 = zero;      // shortcut
    auto rowsum = [&](int64_t r, float4& a0, float4& a1, float4& s0, float4& s1) {
        const float4 d = ld4(dz + r * C + cb), v3 = ld4(y3 + r * C + cb), vd = ld4(yd + r * C + cb);
        const unsigned m = zmask[r * c4tot + (cb >> 2)];
        const float ax = act_grad_from_output((m & 1u) ? 1.f : -1.f, act), ay = act_grad_from_output((m & 2u) ? 1.f : -1.f, act);
        const float az = act_grad_from_output((m & 4u) ? 1.f : -1.f, act), aw = act_grad_from_output((m & 8u) ? 1.f : -1.f, act);
        // BN3's sums as mode 1 contracts them: the product of a0's term unrounded inside an fma, a1's g rounded first
        const float4 g = as_loaded(make_float4(d.x * ax, d.y * ay, d.z * az, d.w * aw));
        a0.x = __fmaf_rn(d.x, ax, a0.x); a0.y = __fmaf_rn(d.y, ay, a0.y); a0.z = __fmaf_rn(d.z, az, a0.z); a0.w = __fmaf_rn(d.w, aw, a0.w);
        const float4 x3 = as_loaded(make_float4((v3.x - mu3.x) * is3.x, (v3.y - mu3.y) * is3.y, (v3.z - mu3.z) * is3.z, (v3.w - mu3.w) * is3.w));
        a1.x = __fmaf_rn(g.x, x3.x, a1.x); a1.y = __fmaf_rn(g.y, x3.y, a1.y); a1.z = __fmaf_rn(g.z, x3.z, a1.z); a1.w = __fmaf_rn(g.w, x3.w, a1.w);
        // the shortcut's: gs = the residual gradient as stored and read back; its activation gradient is 1 (gs * 1 is exact)
        const float4 gs = as_loaded(stored4<T>(g));
        s0.x = __fmaf_rn(gs.x, 1.f, s0.x); s0.y = __fmaf_rn(gs.y, 1.f, s0.y); s0.z = __fmaf_rn(gs.z, 1.f, s0.z); s0.w = __fmaf_rn(gs.w, 1.f, s0.w);
        const float4 xd = as_loaded(make_float4((vd.x - mud.x) * isd.x, (vd.y - mud.y) * isd.y, (vd.z - mud.z) * isd.z, (vd.w - mud.w) * isd.w));
        s1.x = __fmaf_rn(gs.x, xd.x, s1.x); s1.y = __fmaf_rn(gs.y, xd.y, s1.y); s1.z = __fmaf_rn(gs.z, xd.z, s1.z); s1.w = __fmaf_rn(gs.w, xd.w, s1.w);
    };
    int64_t r = r0 + ty;
    for (; r + rpp < r1; r += 2 * rpp) {
        rowsum(r, f0, f1, h0, h1);
        rowsum(r + rpp, g0, g1, k0, k1);
    }
    if (r < r1) rowsum(r, f0, f1, h0, h1);
    f0.x += g0.x; f0.y += g0.y; f0.z += g0.z; f0.w += g0.w;
    f1.x += g1.x; f1.y += g1.y; f1.z += g1.z; f1.w += g1.w;
    h0.x += k0.x; h0.y += k0.y; h0.z += k0.z; h0.w += k0.w;
    h1.x += k1.x; h1.y += k1.y; h1.z += k1.z; h1.w += k1.w;
    *reinterpret_cast<float4*>(sh3 + tid * 8) = f0;
    *reinterpret_cast<float4*>(sh3 + tid * 8 + 4) = f1;
    *reinterpret_cast<float4*>(shd + tid * 8) = h0;
    *reinterpret_cast<float4*>(shd + tid * 8 + 4) = h1;
    __syncthreads();
    if (tid < 2 * CW) {          // one thread per 4-channel group and BatchNorm
        const int lane = tid % CW;
        const float* s = tid < CW ? sh3 : shd;
        double a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0};
        for (int rr = 0; rr < rpp; ++rr) {
            const float* t = s + (rr * CW + lane) * 8;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a0[k] += t[k];
                a1[k] += t[4 + k];
            }
        }
        double* o = out + ((tid < CW ? 0 : C) + blockIdx.y * cgw + lane * 4) * 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = a0[k];
            o[2 * k + 1] = a1[k];
        }
    }
}

// Backward apply with two outputs: bn_act_bwd_rows_kernel's geometry, walk (rev) and expressions (g and xhat rounded, then one
// fma), dy3 from g and dy_ds from the stored form gs of the same g; the residual gradient itself is not written.  sums2: [2C][2],
// BN3's channels first.  The two maxima go to two slot sets; dgamma / dbeta of each layer go to that layer's own vector.
template <typename T>
__global__ void __launch_bounds__(256) bn_act_shortcut_bwd_rows_kernel(const T* __restrict__ dz, const uint8_t* __restrict__ zmask,
                                                                        const T* __restrict__ y3, const T* __restrict__ yd,
                                                                        const ShortcutBn b3, const ShortcutBn bd,
                                                                        const double* __restrict__ sums2, double count, int act,
                                                                        T* __restrict__ dy3, T* __restrict__ dyd, int64_t npix, int C,
                                                                        int cgw, int rows_per_block, int rev,
                                                                        float* __restrict__ dgamma3, float* __restrict__ dbeta3,
                                                                        float* __restrict__ dgammad, float* __restrict__ dbetad,
                                                                        unsigned* __restrict__ amax3, unsigned* __restrict__ amaxd) {
    __shared__ float amax_red[4];
    float max3 = 0.f, maxd = 0.f;
    const int CW = cgw / 4, rpp = 256 / CW, c4tot = C / 4;
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int c = blockIdx.y * cgw + tx * 4;
    const float inv_count = (float)(1.0 / count);
    float gi3[4], mu3[4], is3[4], sg3[4], sgx3[4], gid[4], mud[4], isd[4], sgd[4], sgxd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        is3[k] = b3.invstd[c + k];
        mu3[k] = b3.mean[c + k];
        gi3[k] = (b3.gamma ? b3.gamma[c + k] : 1.f) * is3[k];
        sg3[k] = (float)sums2[(c + k) * 2] * inv_count;
        sgx3[k] = (float)sums2[(c + k) * 2 + 1] * inv_count;
        isd[k] = bd.invstd[c + k];
        mud[k] = bd.mean[c + k];
        gid[k] = (bd.gamma ? bd.gamma[c + k] : 1.f) * isd[k];
        sgd[k] = (float)sums2[(C + c + k) * 2] * inv_count;
        sgxd[k] = (float)sums2[(C + c + k) * 2 + 1] * inv_count;
        // the parameter gradients are the fp64 sums rounded to fp32 (what reduce_stats writes next to them): the first row block
        // delivers them to the two layers' own vectors
        if (blockIdx.x == 0 && ty == 0) {
            if (dbeta3) dbeta3[c + k] = (float)sums2[(c + k) * 2];
            if (dgamma3) dgamma3[c + k] = (float)sums2[(c + k) * 2 + 1];
            if (dbetad) dbetad[c + k] = (float)sums2[(C + c + k) * 2];
            if (dgammad) dgammad[c + k] = (float)sums2[(C + c + k) * 2 + 1];
        }
    }
    const int64_t r0 = (int64_t)(rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * rows_per_block;
    const int64_t r1 = min(r0 + (int64_t)rows_per_block, npix);
    for (int64_t r = r0 + ty; r < r1; r += rpp) {
        const float4 dv = ld4(dz + r * C + c), v3 = ld4(y3 + r * C + c), vd = ld4(yd + r * C + c);
        const unsigned m = zmask[r * c4tot + (c >> 2)];
        const float* d = reinterpret_cast<const float*>(&dv);
        const float* yy3 = reinterpret_cast<const float*>(&v3);
        const float* yyd = reinterpret_cast<const float*>(&vd);
        float4 gv;
        float* g = reinterpret_cast<float*>(&gv);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = d[k] * act_grad_from_output(((m >> k) & 1u) ? 1.f : -1.f, act);
        gv = as_loaded(gv);
        const float4 gsv = as_loaded(stored4<T>(gv));      // the residual gradient as stored and read back
        const float* gs = reinterpret_cast<const float*>(&gsv);
        float4 x3v, xdv;
        float* x3 = reinterpret_cast<float*>(&x3v);
        float* xd = reinterpret_cast<float*>(&xdv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x3[k] = (yy3[k] - mu3[k]) * is3[k];
            xd[k] = (yyd[k] - mud[k]) * isd[k];
        }
        x3v = as_loaded(x3v);
        xdv = as_loaded(xdv);
        float4 o3v, odv;
        float* o3 = reinterpret_cast<float*>(&o3v);
        float* od = reinterpret_cast<float*>(&odv);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o3[k] = gi3[k] * __fmaf_rn(-x3[k], sgx3[k], g[k] - sg3[k]);
            od[k] = gid[k] * __fmaf_rn(-xd[k], sgxd[k], gs[k] - sgd[k]);
        }
        max3 = amax_acc(max3, o3v);
        maxd = amax_acc(maxd, odv);
        st4(dy3 + r * C + c, o3v);
        st4(dyd + r * C + c, odv);
    }
    if (amax3) amax_record(amax3, max3, amax_red);
    if (amaxd) {
        __syncthreads();      // amax_red is read by thread 0 of the first record
        amax_record(amaxd, maxd, amax_red);
    }
}

// BatchNorm over a HANDFUL of rows (split attention's bn1 on the [N, inter] vector of pooled features, N = the batch:
// ResNeSt SplAtConv2d, model/unet.py:52): statistics, running-statistics update, coefficients, normalise + activation in
// ONE launch, one thread per channel (two-pass fp64 statistics over its <= 64 rows).  Replaces the five launches of the
// general path (column partials, fold, un-shift, finalise, apply) - ~4 us each on a [2, 256] tensor, 16 .. 66 times per
// forward.  S parts = S independent BatchNorm batches back to back (ops.BN_SPLIT), running statistics in part order.
// (the arithmetic of ONE channel, shared with the fused fc1 + bn1 kernel of split attention's tail below: bit-identical by construction)
__device__ __forceinline__ void bn_rows_channel(const float* __restrict__ y, int rows, int C, int S, int act, int train,
                                                const BnFinalize& fin, float* __restrict__ z, int c) {
    const float g = fin.gamma ? fin.gamma[c] : 1.f, b = fin.beta ? fin.beta[c] : 0.f;
    for (int s = 0; s < S; ++s) {
        const float* ys = y + (size_t)s * rows * C + c;
        double m, var;
        if (train) {
            double a = 0.0;
            for (int r = 0; r < rows; ++r) a += (double)ys[(size_t)r * C];
            m = a / rows;
            double v = 0.0;
            for (int r = 0; r < rows; ++r) {
                const double d = (double)ys[(size_t)r * C] - m;
                v += d * d;
            }
            var = v / rows;
        } else {
            m = (double)fin.running_mean[c];
            var = (double)fin.running_var[c];
        }
        const float is = (float)(1.0 / sqrt(var + (double)fin.eps));
        const float sc = g * is;
        const float sh = b - (float)m * sc;
        fin.mean[s * C + c] = (float)m;
        fin.invstd[s * C + c] = is;
        fin.scale[s * C + c] = sc;
        fin.shift[s * C + c] = sh;
        if (train && fin.running_mean) {
            const double unb = rows > 1 ? var * rows / (rows - 1.0) : var;
            fin.running_mean[c] = (1.f - fin.momentum) * fin.running_mean[c] + fin.momentum * (float)m;
            fin.running_var[c] = (1.f - fin.momentum) * fin.running_var[c] + fin.momentum * (float)unb;
        }
        for (int r = 0; r < rows; ++r)
            z[((size_t)s * rows + r) * C + c] = apply_act(__fmaf_rn(ys[(size_t)r * C], sc, sh), act);
    }
}
__global__ void __launch_bounds__(256) bn_rows_fwd_kernel(const float* __restrict__ y, int rows, int C, int S, int act,
                                                           int train, BnFinalize fin, float* __restrict__ z) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    bn_rows_channel(y, rows, C, S, act, train, fin, z, c);
}

// Split attention's tail, forward (ResNeSt SplAtConv2d: fc1 -> bn1 -> ReLU -> fc2 -> rSoftMax on [N, C]-vectors; reference call site
// model/unet.py:52): two launches instead of four.
//   splat_fc1_bn_kernel: wave j = output channel j of fc1: h1[n][j] for every sample n - the dot product of linear_fwd_kernel (same
//   lane assignment, same shuffle tree) - then lane 0 runs bn_rows_fwd_kernel's arithmetic for that channel on the values it has
//   just stored (a thread reads its own earlier stores).
//   splat_fc2_rsoftmax_kernel: wave (n, c): the two logits of channel c (rows c and C + c of fc2), then rsoftmax_fwd_kernel's
//   arithmetic for the pair.
__global__ void __launch_bounds__(256) splat_fc1_bn_kernel(const float* __restrict__ gap, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, int N, int C, int inter, int S, int train,
                                                            BnFinalize fin, float* __restrict__ h1, float* __restrict__ a1) {
    const int lane = threadIdx.x & 63;
    const int j = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (j >= inter) return;
    for (int n = 0; n < N; ++n) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += gap[n * C + c] * w1[(size_t)j * C + c];
        s = wave_sum(s);
        if (lane == 0) h1[(size_t)n * inter + j] = s + (b1 ? b1[j] : 0.f);
    }
    if (lane == 0) bn_rows_channel(h1, N / S, inter, S, XV2_ACT_RELU, train, fin, a1, j);
}
__global__ void __launch_bounds__(256) splat_fc2_rsoftmax_kernel(const float* __restrict__ a1, const float* __restrict__ w2,
                                                                  const float* __restrict__ b2, int N, int inter, int C,
                                                                  float* __restrict__ logits, float* __restrict__ att) {
    const int lane = threadIdx.x & 63;
    const int wid = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (wid >= N * C) return;
    const int n = wid / C, c = wid % C;
    float l[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int o = r * C + c;
        float s = 0.f;
        for (int k = lane; k < inter; k += 64) s += a1[n * inter + k] * w2[(size_t)o * inter + k];
        s = wave_sum(s);
        l[r] = s + (b2 ? b2[o] : 0.f);
    }
    if (lane == 0) {
        logits[n * 2 * C + c] = l[0];
        logits[n * 2 * C + C + c] = l[1];
        const float m = fmaxf(l[0], l[1]);
        const float e0 = expf(l[0] - m), e1 = expf(l[1] - m);
        const float inv = 1.f / (e0 + e1);
        att[n * 2 * C + c] = e0 * inv;
        att[n * 2 * C + C + c] = e1 * inv;
    }
}
int splat_fc1_bn_launch(const float* gap, const float* w1, const float* b1, int N, int C, int inter, int parts, int train,
                        const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                        float* mean, float* invstd, float* scale, float* shift, float* h1, float* a1, hipStream_t stream) {
    XV2_CHECK_ARG(gap && w1 && h1 && a1 && mean && invstd && scale && shift && N >= 1 && parts >= 1 && N % parts == 0 && N / parts <= 64,
                  "splat fc1 + bn1: N=%d parts=%d", N, parts);
    XV2_CHECK_ARG(train || (running_mean && running_var), "splat fc1 + bn1: eval mode needs the running statistics");
    BnFinalize f;
    f.count = N / parts; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.running_mean = running_mean; f.running_var = running_var;
    f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
    hipLaunchKernelGGL(splat_fc1_bn_kernel, dim3((unsigned)cdiv((int64_t)inter * 64, 256)), dim3(256), 0, stream, gap, w1, b1, N, C, inter,
                       parts, train, f, h1, a1);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
int splat_fc2_rsoftmax_launch(const float* a1, const float* w2, const float* b2, int N, int inter, int C, float* logits, float* att,
                              hipStream_t stream) {
    XV2_CHECK_ARG(a1 && w2 && logits && att && N >= 1 && C >= 1 && inter >= 1, "splat fc2 + rsoftmax: null argument");
    hipLaunchKernelGGL(splat_fc2_rsoftmax_kernel, dim3((unsigned)cdiv((int64_t)N * C * 64, 256)), dim3(256), 0, stream, a1, w2, b2, N, inter,
                       C, logits, att);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// backward of the same: dy = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), g = dz * act'(z); dgamma / dbeta are the
// sums over all parts
__global__ void __launch_bounds__(256) bn_rows_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ z,
                                                           const float* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           int rows, int C, int S, int act, int train,
                                                           float* __restrict__ dy, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float gm = gamma ? gamma[c] : 1.f;
    float tg = 0.f, tb = 0.f;
    for (int s = 0; s < S; ++s) {
        const size_t o = (size_t)s * rows * C + c;
        const float mu = mean[s * C + c], is = invstd[s * C + c];
        float sg = 0.f, sgx = 0.f;
        for (int r = 0; r < rows; ++r) {
            const size_t i = o + (size_t)r * C;
            const float g = dz[i] * act_grad_from_output(z[i], act);
            sg += g;
            sgx += g * ((y[i] - mu) * is);
        }
        const float invn = 1.f / (float)rows;
        for (int r = 0; r < rows; ++r) {
            const size_t i = o + (size_t)r * C;
            const float g = dz[i] * act_grad_from_output(z[i], act);
            const float xh = (y[i] - mu) * is;
            dy[i] = train ? gm * is * (g - sg * invn - xh * sgx * invn) : gm * is * g;
        }
        tg += sgx;
        tb += sg;
    }
    dgamma[c] = tg;
    dbeta[c] = tb;
}

static inline int ew_grid(int64_t total) {
    int64_t b = cdiv(total, 256);
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace xv2

using namespace xv2;

extern "C" int xv2_bn_reduce_stats(const float* partial, int64_t tiles, int C, double* sums, double* scratch,
                                   void* stream) {
    XV2_CHECK_ARG(tiles > 0 && C > 0, "bn_reduce_stats: empty");
    return reduce_stats<float>(partial, tiles, C, sums, scratch, (hipStream_t)stream);
}

extern "C" int xv2_bn_reduce_finalize(const float* partial, int64_t tiles, int C, double* sums, double* scratch,
                                      double count, const float* gamma, const float* beta, float eps, float momentum,
                                      float* running_mean, float* running_var, float* mean, float* invstd,
                                      float* scale, float* shift, void* stream) {
    XV2_CHECK_ARG(tiles > 0 && C > 0, "bn_reduce_finalize: empty");
    XV2_CHECK_ARG(mean && invstd && scale && shift, "bn_reduce_finalize: coefficient outputs are required");
    BnFinalize f;
    f.count = count; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.running_mean = running_mean; f.running_var = running_var;
    f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
    return reduce_stats<float>(partial, tiles, C, sums, scratch, (hipStream_t)stream, nullptr, nullptr, &f);
}

extern "C" size_t xv2_bn_tensor_stats_workspace(int64_t npix, int C) {
    const ChunkGeom g4 = chunk_geom(npix, C, 4), g8 = chunk_geom(npix, C, 8);    // fp32 / bf16 lane layouts
    size_t part = (size_t)std::max(g4.chunks, g8.chunks) * C * 2 * sizeof(double);
    part = (part + 15) & ~(size_t)15;
    return part + (size_t)XV2_BN_SCRATCH_ROWS * C * 2 * sizeof(double);
}
extern "C" size_t xv2_bn_backward_workspace(int64_t npix, int C) { return xv2_bn_tensor_stats_workspace(npix, C); }

template <int MODE, typename T>
static int column_sums(const ColOp<MODE, T>& op, int64_t npix, int C, double* sums, float* workspace, hipStream_t st,
                       float* f0 = nullptr, float* f1 = nullptr) {
    const ChunkGeom g = chunk_geom(npix, C, 4 * Vec16<T>::NV);
    size_t part = (size_t)g.chunks * C * 2 * sizeof(double);
    part = (part + 15) & ~(size_t)15;
    double* dpart = reinterpret_cast<double*>(workspace);
    double* scratch = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + part);
    hipLaunchKernelGGL((column_partials_kernel<MODE, T>), dim3((unsigned)g.chunks, g.groups), dim3(256), 0, st, op, npix,
                       C, g.rpb, g.cgw, dpart, BN_REV_COLUMN_SUMS);
    XV2_CHECK_LAUNCH();
    return reduce_stats<double>(dpart, g.chunks, C, sums, scratch, st, f0, f1);
}

// W-channel vector accesses of `esz`-byte elements (W * esz bytes, aligned)
static inline bool vec_ok(int C, size_t esz, std::initializer_list<int> lds, std::initializer_list<const void*> ptrs,
                          int W = 4) {
    if (C % W) return false;
    for (int l : lds)
        if (l % W) return false;
    for (const void* p : ptrs)
        if (p && (reinterpret_cast<uintptr_t>(p) & (W * esz - 1))) return false;
    return true;
}

extern "C" int xv2_bn_tensor_stats(const float* x, int ldx, int64_t npix, int C, double* sums, float* workspace,
                                   void* stream) {
    XV2_CHECK_ARG(npix > 0 && C > 0, "bn_tensor_stats: empty");
    // the column form is chosen from C alone and the workspace was sized for it: rejected, not re-routed
    XV2_CHECK_ARG(C % 4 != 0 || vec_ok(C, sizeof(float), {ldx}, {x}), "bn_tensor_stats: C %% 4 == 0 needs ldx %% 4 == 0 and a 16-byte aligned x");
    ColOp<0, float> op;
    op.a = x; op.lda = ldx; op.z = nullptr; op.y = nullptr; op.mean = nullptr; op.invstd = nullptr;
    op.scale = op.shift = nullptr;
    op.ldz = op.ldy = 0; op.act = 0; op.zbits = 0; op.c4tot = 0;
    int rc = column_sums<0, float>(op, npix, C, sums, workspace, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(unshift_stats_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, sums, x,
                       (double)npix, C);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_finalize(const double* sums, double count, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, int C, void* stream) {
    BnFinalize f;
    f.count = count; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.running_mean = running_mean; f.running_var = running_var;
    f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, sums, f, C);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* scale, float* shift, int C,
                                  void* stream) {
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma,
                       beta, running_mean, running_var, eps, scale, shift, C);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

template <typename T>
static int bn_act_forward_impl(const T* y, int ldy, const float* scale, const float* shift, const T* residual,
                               int ldr, int act, T* z, int ldz, int64_t npix, int C, uint8_t* zmask, void* stream) {
    XV2_CHECK_ARG(npix > 0 && C > 0, "bn_act_forward: empty");
    AmaxGuard amax_guard;
    unsigned* amax = std::is_same<T, float>::value ? amax_ctx().out : nullptr;      // F16X2: record max |z| (fp32 tensors)
    constexpr int W = 4 * Vec16<T>::NV;
    const bool vec = vec_ok(C, sizeof(T), {ldy, ldz, residual ? ldr : 0}, {y, z, residual}, W) &&
                     vec_ok(C, 4, {}, {scale, shift});
    XV2_CHECK_ARG(!zmask || (vec && act != XV2_ACT_SIGMOID), "bn_act_forward_mask: needs C %% %d == 0, aligned rows, ReLU-type activation", W);
    const int grid = ew_grid(npix * (vec ? C / W : C));
    if (vec)
        hipLaunchKernelGGL((bn_act_fwd_kernel<true, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, y, ldy, scale,
                           shift, residual, ldr, act, z, ldz, npix, C, zmask, BN_REV_FWD_APPLY, amax);
    else
        hipLaunchKernelGGL((bn_act_fwd_kernel<false, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, y, ldy, scale,
                           shift, residual, ldr, act, z, ldz, npix, C, (uint8_t*)nullptr, 0, amax);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_act_forward(const void* y, int ldy, const float* scale, const float* shift,
                                  const void* residual, int ldr, int act, void* z, int ldz, int64_t npix, int C,
                                  int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_act_forward_impl<T>((const T*)y, ldy, scale, shift, (const T*)residual, ldr, act,
                                                           (T*)z, ldz, npix, C, nullptr, stream));
}

extern "C" int xv2_bn_act_forward_mask(const void* y, int ldy, const float* scale, const float* shift,
                                       const void* residual, int ldr, int act, void* z, int ldz, int64_t npix,
                                       int C, uint8_t* zmask, int dtype, void* stream) {
    XV2_CHECK_ARG(zmask, "bn_act_forward_mask: mask output is required");
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_act_forward_impl<T>((const T*)y, ldy, scale, shift, (const T*)residual, ldr, act,
                                                           (T*)z, ldz, npix, C, zmask, stream));
}

template <typename T>
static int bn_bwd_reduce_impl(const T* dz, int lddz, const T* z, int ldz, int zbits, const T* y, int ldy,
                              const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                              int64_t npix, int C, double* sums2, float* dgamma, float* dbeta, float* workspace,
                              void* stream) {
    XV2_CHECK_ARG(npix > 0 && C > 0, "bn_act_backward_reduce: empty");
    XV2_CHECK_ARG(!zbits || (C % 4 == 0 && chunk_geom(npix, C, 4 * Vec16<T>::NV).cgw && act != XV2_ACT_SIGMOID),
                  "bn backward (mask form): unsupported channel count %d / activation", C);
    XV2_CHECK_ARG(C % 4 != 0 || (lddz % 4 == 0 && (!z || ldz % 4 == 0) && ldy % 4 == 0), "bn backward: strides must be multiples of 4");
    // (pointers as well: the column form is chosen from C alone and the workspace was sized for it - rejected, not re-routed)
    XV2_CHECK_ARG(C % 4 != 0 || (vec_ok(C, sizeof(T), {}, {dz, zbits ? nullptr : z, y}) && vec_ok(C, sizeof(float), {}, {mean, invstd, scale, shift})),
                  "bn backward: C %% 4 == 0 needs operands aligned to 4 elements");
    XV2_CHECK_ARG(z || (scale && shift), "bn backward: either z or (scale, shift) is required for the activation mask");
    ColOp<1, T> op;
    op.a = dz; op.lda = lddz; op.z = z; op.ldz = ldz; op.y = y; op.ldy = ldy; op.mean = mean; op.invstd = invstd;
    op.scale = scale; op.shift = shift;
    op.act = act;
    op.zbits = zbits; op.c4tot = C / 4;
    return column_sums<1, T>(op, npix, C, sums2, workspace, (hipStream_t)stream, dbeta, dgamma);
}

extern "C" int xv2_bn_act_backward_reduce(const void* dz, int lddz, const void* z, int ldz, const void* y, int ldy,
                                          const float* mean, const float* invstd, const float* scale,
                                          const float* shift, int act, int64_t npix, int C, double* sums2,
                                          float* dgamma, float* dbeta, float* workspace, int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_bwd_reduce_impl<T>((const T*)dz, lddz, (const T*)z, ldz, 0, (const T*)y, ldy, mean,
                                                          invstd, scale, shift, act, npix, C, sums2, dgamma, dbeta,
                                                          workspace, stream));
}

extern "C" int xv2_bn_act_backward_reduce_mask(const void* dz, int lddz, const uint8_t* zmask, const void* y, int ldy,
                                               const float* mean, const float* invstd, int act, int64_t npix, int C,
                                               double* sums2, float* dgamma, float* dbeta, float* workspace,
                                               int dtype, void* stream) {
    XV2_CHECK_ARG(zmask, "bn_act_backward_reduce_mask: mask is required");
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_bwd_reduce_impl<T>((const T*)dz, lddz, reinterpret_cast<const T*>(zmask), 4, 1,
                                                          (const T*)y, ldy, mean, invstd, nullptr, nullptr, act, npix, C,
                                                          sums2, dgamma, dbeta, workspace, stream));
}

template <typename T>
static int bn_bwd_apply_impl(const T* dz, int lddz, const T* z, int ldz, int zbits, const T* y, int ldy,
                             const float* mean, const float* invstd, const float* gamma, const float* scale,
                             const float* shift, const double* sums2, double count, int act, int train, T* dy,
                             int lddy, T* dres, int lddres, int64_t npix, int C, void* stream) {
    XV2_CHECK_ARG(npix > 0 && C > 0, "bn_act_backward_apply: empty");
    AmaxGuard amax_guard;
    unsigned* amax = std::is_same<T, float>::value ? amax_ctx().out : nullptr;      // F16X2: record max |dy| (fp32 tensors)
    XV2_CHECK_ARG(z || (scale && shift), "bn backward: either z or (scale, shift) is required for the activation mask");
    constexpr int W = 4 * Vec16<T>::NV;
    const bool vecw = vec_ok(C, sizeof(T), {lddz, (z && !zbits) ? ldz : 0, ldy, lddy, dres ? lddres : 0},
                             {dz, zbits ? nullptr : z, y, dy, dres}, W);
    const bool vec = vecw || vec_ok(C, sizeof(T), {lddz, (z && !zbits) ? ldz : 0, ldy, lddy, dres ? lddres : 0},
                                    {dz, zbits ? nullptr : z, y, dy, dres}, 4);
    XV2_CHECK_ARG(!zbits || (vec && act != XV2_ACT_SIGMOID), "bn backward (mask form): needs C %% 4 == 0, aligned rows, ReLU-type activation");
    const ChunkGeom cg = chunk_geom(npix, C, W);
    if (vecw && cg.cgw) {
        const int rpp = 256 / (cg.cgw / W);
        int64_t rpb = cdiv(npix * cg.groups, sizeof(T) == 2 ? 2048 : 4096);
        rpb = std::max<int64_t>(cdiv(rpb, rpp) * rpp, rpp * 4);
        hipLaunchKernelGGL(bn_act_bwd_rows_kernel<T>, dim3((unsigned)cdiv(npix, rpb), cg.groups), dim3(256), 0,
                           (hipStream_t)stream, dz, lddz, z, ldz, y, ldy, mean, invstd, gamma, scale, shift, sums2,
                           count, act, train, dy, lddy, dres, lddres, npix, cg.cgw, (int)rpb, zbits, C / 4, BN_REV_BWD_APPLY, amax);
        XV2_CHECK_LAUNCH();
        return XV2_OK;
    }
    // (the generic forms do not record: take the maximum of what they wrote in a pass of its own - rare shapes)
    struct AmaxAfter {
        unsigned* slots; const void* dy; int lddy, C; int64_t npix; void* stream;
        ~AmaxAfter() {
            if (slots && lddy == C) xv2_tensor_amax_into(static_cast<const float*>(dy), npix * C, slots, stream);
        }
    } amax_after{amax, dy, lddy, C, npix, stream};
    XV2_CHECK_ARG(!amax || (lddy == C && (npix * C) % 4 == 0), "bn_act_backward_apply: F16X2 maximum of a strided / odd-sized dy");
    const int grid = ew_grid(npix * (vec ? C / 4 : C));
    if (vec)
        hipLaunchKernelGGL((bn_act_bwd_kernel<true, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, dz, lddz, z, ldz,
                           y, ldy, mean, invstd, gamma, scale, shift, sums2, count, act, train, dy, lddy, dres, lddres, npix, C,
                           zbits);
    else
        hipLaunchKernelGGL((bn_act_bwd_kernel<false, T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, dz, lddz, z, ldz,
                           y, ldy, mean, invstd, gamma, scale, shift, sums2, count, act, train, dy, lddy, dres, lddres, npix, C,
                           0);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_act_backward_apply(const void* dz, int lddz, const void* z, int ldz, const void* y, int ldy,
                                         const float* mean, const float* invstd, const float* gamma,
                                         const float* scale, const float* shift, const double* sums2, double count,
                                         int act, int train, void* dy, int lddy, void* dres, int lddres,
                                         int64_t npix, int C, int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_bwd_apply_impl<T>((const T*)dz, lddz, (const T*)z, ldz, 0, (const T*)y, ldy, mean,
                                                         invstd, gamma, scale, shift, sums2, count, act, train, (T*)dy,
                                                         lddy, (T*)dres, lddres, npix, C, stream));
}

extern "C" int xv2_bn_act_backward_apply_mask(const void* dz, int lddz, const uint8_t* zmask, const void* y, int ldy,
                                              const float* mean, const float* invstd, const float* gamma,
                                              const double* sums2, double count, int act, int train, void* dy,
                                              int lddy, void* dres, int lddres, int64_t npix, int C, int dtype,
                                              void* stream) {
    XV2_CHECK_ARG(zmask, "bn_act_backward_apply_mask: mask is required");
    XV2_CHECK_DTYPE(dtype);
    XV2_DISPATCH_DTYPE(dtype, return bn_bwd_apply_impl<T>((const T*)dz, lddz, reinterpret_cast<const T*>(zmask), 4, 1,
                                                         (const T*)y, ldy, mean, invstd, gamma, nullptr, nullptr, sums2,
                                                         count, act, train, (T*)dy, lddy, (T*)dres, lddres, npix, C,
                                                         stream));
}

// ---- the head of the last decoder layer inside the BatchNorm passes (include/xv2.h "head fusion") ----
extern "C" int xv2_bn_act_head_supported(int64_t npix, int C, int Cout) {
    if (npix <= 0 || C < 4 || C > 256 || (C & (C - 1)) || Cout < 1 || Cout > HEAD_MAX_COUT) return 0;
    // C / 4 lanes per pixel = the head's L = the BatchNorm kernels' lanes per row, one 4-channel group per lane, one channel group
    const ChunkGeom g = chunk_geom(npix, C, 4);
    return (head_lanes(C) * 4 == C && g.cgw == C && g.groups == 1) ? 1 : 0;
}

template <typename T>
static int bn_act_head_forward_impl(const T* y, int ldy, const float* scale, const float* shift, int act, int64_t npix, int64_t hw,
                                    int C, int Cout, const float* w, const float* bias, float* logits, int nchw_out, void* stream) {
    XV2_CHECK_ARG(y && scale && shift && w && logits && hw > 0, "bn_act_head_forward: null argument");
    XV2_CHECK_ARG(xv2_bn_act_head_supported(npix, C, Cout), "bn_act_head_forward: no fused form for C=%d Cout=%d", C, Cout);
    XV2_CHECK_ARG(vec_ok(C, sizeof(T), {ldy}, {y}, 4) && vec_ok(C, 4, {}, {scale, shift, w}), "bn_act_head_forward: unaligned operand");
    const int L = C / 4;
    // (a pixel group per thread group, two pixels in flight per lane: the grid of bn_act_fwd_kernel over half the elements)
    const int grid = ew_grid(cdiv(npix * L, 2));
    hipStream_t st = (hipStream_t)stream;
    prof_begin(head_prof_id(2), 0.0, 0.0, st);
#define LAUNCH_BHF(CO)                                                                                                     \
    hipLaunchKernelGGL((bn_act_head_fwd_kernel<CO, T>), dim3(grid), dim3(256), 0, st, y, ldy, scale, shift, act, npix, hw, C, w, \
                       bias, logits, nchw_out, head_hw_div(npix, hw), L, BN_REV_FWD_APPLY)
    switch (Cout) {
        case 1: LAUNCH_BHF(1); break;
        case 2: LAUNCH_BHF(2); break;
        case 3: LAUNCH_BHF(3); break;
        default: LAUNCH_BHF(4); break;
    }
#undef LAUNCH_BHF
    prof_end(st);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_act_head_forward(const void* y, int ldy, const float* scale, const float* shift, int act, int64_t npix,
                                       int64_t hw, int C, int Cout, const float* w, const float* bias, float* logits,
                                       int nchw_out, int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    AmaxGuard amax_guard;      // (nothing is recorded: z is never stored)
    XV2_DISPATCH_DTYPE(dtype, return bn_act_head_forward_impl<T>((const T*)y, ldy, scale, shift, act, npix, hw, C, Cout, w, bias,
                                                                logits, nchw_out, stream));
}

static size_t bn_head_part_offset(int64_t npix, int C) {
    return (xv2_bn_backward_workspace(npix, C) + 15) & ~(size_t)15;
}
extern "C" size_t xv2_bn_act_head_backward_workspace(int64_t npix, int C, int Cout) {
    return bn_head_part_offset(npix, C) + (size_t)HEAD_BLOCKS * Cout * (C + 1) * sizeof(float);
}

template <typename T, int COUT>
static int bn_act_head_backward_impl(const float* dlogits, int nchw, int64_t hw, const float* w, const T* y, int ldy, const float* mean,
                                     const float* invstd, const float* gamma, const float* scale, const float* shift, int act,
                                     double count, T* dy, int lddy, int64_t npix, int C, double* sums2, float* dgamma, float* dbeta,
                                     float* dw, float* dbias, float* workspace, hipStream_t st) {
    unsigned* amax = std::is_same<T, float>::value ? amax_ctx().out : nullptr;      // F16X2: record max |dy| (fp32 tensors)
    const ChunkGeom g = chunk_geom(npix, C, 4);
    HeadGrad hg;
    hg.dl = dlogits; hg.w = w; hg.hw = hw; hg.nchw = nchw; hg.hw_div = head_hw_div(npix, hw);
    float* hpart = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + bn_head_part_offset(npix, C));
    ColOp<2, T, COUT> op;
    op.head = hg;
    op.a = nullptr; op.lda = 0; op.z = nullptr; op.ldz = 0; op.y = y; op.ldy = ldy; op.mean = mean; op.invstd = invstd;
    op.scale = scale; op.shift = shift; op.act = act; op.zbits = 0; op.c4tot = C / 4;
    size_t part = (size_t)g.chunks * C * 2 * sizeof(double);
    part = (part + 15) & ~(size_t)15;
    double* dpart = reinterpret_cast<double*>(workspace);
    double* scratch = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + part);
    // pass 1: (sum g, sum g * xhat) per channel, in the unfused pass's row chunks; then its fold
    prof_begin(head_prof_id(3), 0.0, 0.0, st);
    hipLaunchKernelGGL((column_partials_kernel<2, T, COUT>), dim3((unsigned)g.chunks, 1), dim3(256), 0, st, op, npix, C, g.rpb, g.cgw,
                       dpart, BN_REV_COLUMN_SUMS);
    prof_end(st);
    XV2_CHECK_LAUNCH();
    int rc = reduce_stats<double>(dpart, g.chunks, C, sums2, scratch, st, dbeta, dgamma);
    if (rc) return rc;
    // pass 2: dy and the head's dw / db partials in head_bwd_kernel's geometry; then head_bwd_kernel's fold
    const int L = C / 4;
    const int grid = (int)std::min<int64_t>(cdiv(npix, 256 / L), HEAD_BLOCKS);
    prof_begin(head_prof_id(4), 0.0, 0.0, st);
    hipLaunchKernelGGL((bn_act_bwd_rows_head_kernel<COUT, T>), dim3(grid), dim3(256), 0, st, hg, y, ldy, mean, invstd, gamma, scale,
                       shift, sums2, count, act, dy, lddy, npix, C, L, hpart, amax);
    prof_end(st);
    XV2_CHECK_LAUNCH();
    return head_bwd_reduce_launch(hpart, grid, COUT, C, dw, dbias, st);
}

extern "C" int xv2_bn_act_head_backward(const float* dlogits, int nchw_dl, int64_t hw, const float* w, int Cout, const void* y, int ldy,
                                        const float* mean, const float* invstd, const float* gamma, const float* scale,
                                        const float* shift, int act, double count, void* dy, int lddy, int64_t npix, int C,
                                        double* sums2, float* dgamma, float* dbeta, float* dw, float* dbias, float* workspace,
                                        int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    AmaxGuard amax_guard;
    XV2_CHECK_ARG(dlogits && w && y && mean && invstd && scale && shift && dy && sums2 && dw && workspace && hw > 0,
                  "bn_act_head_backward: null argument");
    XV2_CHECK_ARG(xv2_bn_act_head_supported(npix, C, Cout), "bn_act_head_backward: no fused form for C=%d Cout=%d", C, Cout);
    const size_t es = dtype == XV2_BF16 ? 2 : 4;
    XV2_CHECK_ARG(vec_ok(C, es, {ldy, lddy}, {y, dy}, 4) && vec_ok(C, 4, {}, {w, mean, invstd, scale, shift, gamma}),
                  "bn_act_head_backward: unaligned operand");
    hipStream_t st = (hipStream_t)stream;
#define BHB(CO)                                                                                                                   \
    XV2_DISPATCH_DTYPE(dtype, return (bn_act_head_backward_impl<T, CO>(dlogits, nchw_dl, hw, w, (const T*)y, ldy, mean, invstd, gamma, \
                                                                      scale, shift, act, count, (T*)dy, lddy, npix, C, sums2, dgamma, \
                                                                      dbeta, dw, dbias, workspace, st)))
    switch (Cout) {
        case 1: BHB(1);
        case 2: BHB(2);
        case 3: BHB(3);
        default: BHB(4);
    }
#undef BHB
    return XV2_OK;      // (not reached: every case returns)
}

extern "C" int xv2_bn_rows_forward(const float* y, int rows, int C, int parts, const float* gamma, const float* beta, float eps,
                                   float momentum, float* running_mean, float* running_var, int train, int act,
                                   float* mean, float* invstd, float* scale, float* shift, float* z, void* stream) {
    XV2_CHECK_ARG(y && z && mean && invstd && scale && shift && rows >= 1 && rows <= 64 && C >= 1 && parts >= 1,
                  "bn_rows_forward: rows=%d (1..64) C=%d parts=%d", rows, C, parts);
    XV2_CHECK_ARG(train || (running_mean && running_var), "bn_rows_forward: eval mode needs the running statistics");
    BnFinalize f;
    f.count = rows; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.running_mean = running_mean; f.running_var = running_var;
    f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
    hipLaunchKernelGGL(bn_rows_fwd_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, y, rows, C, parts,
                       act, train, f, z);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_rows_backward(const float* dz, const float* z, const float* y, const float* mean, const float* invstd,
                                    const float* gamma, int rows, int C, int parts, int act, int train, float* dy,
                                    float* dgamma, float* dbeta, void* stream) {
    XV2_CHECK_ARG(dz && z && y && mean && invstd && dy && dgamma && dbeta && rows >= 1 && rows <= 64 && C >= 1 && parts >= 1,
                  "bn_rows_backward: rows=%d (1..64) C=%d parts=%d", rows, C, parts);
    hipLaunchKernelGGL(bn_rows_bwd_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, dz, z, y, mean,
                       invstd, gamma, rows, C, parts, act, train, dy, dgamma, dbeta);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// ---- the projection shortcut's BatchNorm inside the block's last BatchNorm passes (include/xv2.h "shortcut fusion") ----
static int shortcut_prof_id(int which) {      // bench-time profiler names of the three fused kernels
    static const int ids[3] = {prof_register("bn_act_shortcut_fwd_kernel"), prof_register("column_partials_shortcut_kernel"),
                               prof_register("bn_act_shortcut_bwd_rows_kernel")};
    return ids[which];
}

extern "C" int xv2_bn_act_shortcut_supported(int64_t npix, int C, int dtype) {
    if (npix <= 0 || C <= 0 || (dtype != XV2_F32 && dtype != XV2_BF16)) return 0;
    // the vector path of the column sums (4 channels per lane for both storage types: Vec16), which is also the shape rule of the
    // byte mask and of the streaming apply pass
    return chunk_geom(npix, C, 4).cgw ? 1 : 0;
}

template <typename T>
static int bn_act_shortcut_forward_impl(const T* y3, const T* yd, const float* scale3, const float* shift3, const float* scaled,
                                        const float* shiftd, int act, T* z, uint8_t* zmask, int64_t npix, int C, hipStream_t st) {
    XV2_CHECK_ARG(vec_ok(C, sizeof(T), {}, {y3, yd, z}, 4) && vec_ok(C, 4, {}, {scale3, shift3, scaled, shiftd}),
                  "bn_act_shortcut_forward: unaligned operand");
    unsigned* amax = std::is_same<T, float>::value ? amax_ctx().out : nullptr;      // F16X2: record max |z| (fp32 tensors)
    const int grid = ew_grid(npix * (C / 4));
    prof_begin(shortcut_prof_id(0), 0.0, 0.0, st);
    hipLaunchKernelGGL(bn_act_shortcut_fwd_kernel<T>, dim3(grid), dim3(256), 0, st, y3, yd, scale3, shift3, scaled, shiftd, act, z,
                       npix, C, zmask, BN_REV_FWD_APPLY, amax);
    prof_end(st);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_act_shortcut_forward(const void* y3, const void* y_ds, const float* scale3, const float* shift3,
                                           const float* scale_ds, const float* shift_ds, int act, void* z, uint8_t* zmask,
                                           int64_t npix, int C, int dtype, void* stream) {
    XV2_CHECK_DTYPE(dtype);
    AmaxGuard amax_guard;
    XV2_CHECK_ARG(y3 && y_ds && scale3 && shift3 && scale_ds && shift_ds && z && zmask, "bn_act_shortcut_forward: null argument");
    XV2_CHECK_ARG(act == XV2_ACT_RELU || act == XV2_ACT_LEAKY, "bn_act_shortcut_forward: ReLU-type activation only (got %d)", act);
    XV2_CHECK_ARG(xv2_bn_act_shortcut_supported(npix, C, dtype), "bn_act_shortcut_forward: no fused form for C=%d", C);
    XV2_DISPATCH_DTYPE(dtype, return bn_act_shortcut_forward_impl<T>((const T*)y3, (const T*)y_ds, scale3, shift3, scale_ds, shift_ds,
                                                                    act, (T*)z, zmask, npix, C, (hipStream_t)stream));
}

// partials [chunks][2C][2] doubles, then reduce_stats' scratch rows for 2C channels
static size_t bn_shortcut_part_bytes(int64_t npix, int C) {
    const size_t part = (size_t)chunk_geom(npix, C, 4).chunks * C * 4 * sizeof(double);
    return (part + 15) & ~(size_t)15;
}
extern "C" size_t xv2_bn_act_shortcut_backward_workspace(int64_t npix, int C) {
    if (npix <= 0 || C <= 0) return 0;
    return bn_shortcut_part_bytes(npix, C) + (size_t)XV2_BN_SCRATCH_ROWS * C * 4 * sizeof(double);
}

template <typename T>
static int bn_act_shortcut_backward_impl(const T* dz, const uint8_t* zmask, const T* y3, const T* yd, const ShortcutBn& b3,
                                         const ShortcutBn& bd, int act, double count, T* dy3, T* dyd, int64_t npix, int C,
                                         double* sums2, float* dgamma3, float* dbeta3, float* dgammad, float* dbetad,
                                         unsigned* amax_dyd, float* workspace, hipStream_t st) {
    XV2_CHECK_ARG(vec_ok(C, sizeof(T), {}, {dz, y3, yd, dy3, dyd}, 4) &&
                      vec_ok(C, 4, {}, {b3.mean, b3.invstd, b3.gamma, bd.mean, bd.invstd, bd.gamma}),
                  "bn_act_shortcut_backward: unaligned operand");
    const bool f32 = std::is_same<T, float>::value;      // F16X2: record max |dy3| / max |dy_ds| (fp32 tensors)
    unsigned* amax3 = f32 ? amax_ctx().out : nullptr;
    unsigned* amaxd = f32 ? amax_dyd : nullptr;
    const ChunkGeom g = chunk_geom(npix, C, 4);
    double* dpart = reinterpret_cast<double*>(workspace);
    double* scratch = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + bn_shortcut_part_bytes(npix, C));
    // pass 1: both layers' (sum g, sum g * xhat) per channel in the unfused passes' row chunks; one fold over 2C channels
    prof_begin(shortcut_prof_id(1), 0.0, 0.0, st);
    hipLaunchKernelGGL(column_partials_shortcut_kernel<T>, dim3((unsigned)g.chunks, g.groups), dim3(256), 0, st, dz, zmask, y3, yd, b3,
                       bd, act, npix, C, g.rpb, g.cgw, dpart, BN_REV_COLUMN_SUMS);
    prof_end(st);
    XV2_CHECK_LAUNCH();
    int rc = reduce_stats<double>(dpart, g.chunks, 2 * C, sums2, scratch, st);
    if (rc) return rc;
    // pass 2: dy3 and dy_ds in the row blocks of bn_act_bwd_rows_kernel
    const int rpp = 256 / (g.cgw / 4);
    int64_t rpb = cdiv(npix * g.groups, sizeof(T) == 2 ? 2048 : 4096);
    rpb = std::max<int64_t>(cdiv(rpb, rpp) * rpp, rpp * 4);
    prof_begin(shortcut_prof_id(2), 0.0, 0.0, st);
    hipLaunchKernelGGL(bn_act_shortcut_bwd_rows_kernel<T>, dim3((unsigned)cdiv(npix, rpb), g.groups), dim3(256), 0, st, dz, zmask, y3,
                       yd, b3, bd, sums2, count, act, dy3, dyd, npix, C, g.cgw, (int)rpb, BN_REV_BWD_APPLY, dgamma3, dbeta3, dgammad,
                       dbetad, amax3, amaxd);
    prof_end(st);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_bn_act_shortcut_backward(const void* dz, const uint8_t* zmask, const void* y3, const void* y_ds,
                                            const float* mean3, const float* invstd3, const float* gamma3, const float* mean_ds,
                                            const float* invstd_ds, const float* gamma_ds, int act, double count, void* dy3,
                                            void* dy_ds, int64_t npix, int C, double* sums2, float* dgamma3, float* dbeta3,
                                            float* dgamma_ds, float* dbeta_ds, void* amax_dy_ds, float* workspace, int dtype,
                                            void* stream) {
    XV2_CHECK_DTYPE(dtype);
    AmaxGuard amax_guard;
    XV2_CHECK_ARG(dz && zmask && y3 && y_ds && mean3 && invstd3 && mean_ds && invstd_ds && dy3 && dy_ds && sums2 && workspace,
                  "bn_act_shortcut_backward: null argument");
    XV2_CHECK_ARG(act == XV2_ACT_RELU || act == XV2_ACT_LEAKY, "bn_act_shortcut_backward: ReLU-type activation only (got %d)", act);
    XV2_CHECK_ARG(xv2_bn_act_shortcut_supported(npix, C, dtype), "bn_act_shortcut_backward: no fused form for C=%d", C);
    ShortcutBn b3, bd;
    b3.mean = mean3; b3.invstd = invstd3; b3.gamma = gamma3;
    bd.mean = mean_ds; bd.invstd = invstd_ds; bd.gamma = gamma_ds;
    XV2_DISPATCH_DTYPE(dtype, return bn_act_shortcut_backward_impl<T>((const T*)dz, zmask, (const T*)y3, (const T*)y_ds, b3, bd, act,
                                                                     count, (T*)dy3, (T*)dy_ds, npix, C, sums2, dgamma3, dbeta3,
                                                                     dgamma_ds, dbeta_ds, (unsigned*)amax_dy_ds, workspace,
                                                                     (hipStream_t)stream));
}
