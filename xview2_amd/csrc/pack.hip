// Weight repacking: OIHW fp32 master weights -> the OHWI / IHWO layouts (fp32 or bf16) the convolution kernels read,
// one tensor per launch (xv2_pack_weight) or every tensor of a table in one launch (xv2_pack_weights_table).
#include "xv2_common.h"
#include <algorithm>

namespace xv2 {

template <typename OT>
__global__ void pack_weight_kernel(const float* __restrict__ w, int Cout, int Cin, int T, int CinP,
                                   OT* __restrict__ ohwi, OT* __restrict__ ihwo) {
    const size_t total = (size_t)Cout * T * CinP;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % CinP);
        const size_t q = i / CinP;
        const int t = (int)(q % T);
        const int co = (int)(q / T);
        const float v = ci < Cin ? w[((size_t)co * Cin + ci) * T + t] : 0.f;
        if (ohwi) st1(ohwi + i, v);
        if (ihwo) st1(ihwo + ((size_t)ci * T + t) * Cout + co, v);
    }
}

// Many weight tensors in one launch (after the optimizer step every packed layout is stale at once).
// table[n][8]: {src OIHW pointer, ohwi pointer or 0, ihwo pointer or 0, Cout, Cin, T, cin_pad, first tile};
// a tile = 32 output channels x 32 (padded) input channels x up to 9 taps, staged through LDS so that the OIHW
// reads AND both transposed writes move whole 128-byte lines.
constexpr int PK_TC = 9;
__host__ __device__ inline int64_t pack_tiles(int Cout, int CinP, int T) {
    return (int64_t)((Cout + 31) / 32) * ((CinP + 31) / 32) * ((T + PK_TC - 1) / PK_TC);
}
// TCC: taps per tile as a compile-time constant (1, 4, 9: every index division below becomes a multiply-shift; the
// runtime-divisor form spent more time in integer division than in memory: 226 us for the 25.5 M parameters of cfg2), 0 = generic
template <int TCC>
__device__ __forceinline__ void pack_tile(float* sh, const float* __restrict__ w, float* __restrict__ ohwi,
                                          float* __restrict__ ihwo, int Cout, int Cin, int T, int CinP, bool half, int t0,
                                          int tcr, int co0, int ci0) {
    const int tc = TCC ? TCC : tcr;
    const int ldco = 32 * tc + 1;
    const int cnt = 32 * 32 * tc;
    // OIHW -> LDS[co][ci][t]  (a co row of the tile is 32*tc consecutive floats when tc == T)
    if constexpr (TCC > 0) {
        // compile-time trip count: ALL 4 * tc loads of a thread in flight (from indices clamped into the tensor), then the
        // LDS stores - the rolled loop waited for every single load (s_waitcnt vmcnt(0) per element: 36 dependent memory
        // round trips per thread and 3x3 tile, the whole table at 1 - 1.5 TB/s)
        constexpr int IT = 4 * TCC;
        float v[IT];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * 256;
            const int col = i / (32 * TCC), r = i - col * (32 * TCC);
            const int cil = r / TCC, tl = r - cil * TCC;
            const int co = min(co0 + col, Cout - 1), ci = min(ci0 + cil, Cin - 1);
            v[k] = w[((size_t)co * Cin + ci) * T + t0 + tl];
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = threadIdx.x + k * 256;
            const int col = i / (32 * TCC), r = i - col * (32 * TCC);
            const int cil = r / TCC;
            sh[col * ldco + r] = (co0 + col < Cout && ci0 + cil < Cin) ? v[k] : 0.f;
        }
    } else
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int col = i / (32 * tc), r = i - col * (32 * tc);
        const int cil = r / tc, tl = r - cil * tc;
        const int co = co0 + col, ci = ci0 + cil;
        sh[col * ldco + r] = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * T + t0 + tl] : 0.f;
    }
    __syncthreads();
    if (ohwi)
        for (int i = threadIdx.x; i < cnt; i += 256) {       // (co, t, ci): ci fastest
            const int cil = i & 31, q = i >> 5;
            const int col = q / tc, tl = q - col * tc;
            const int co = co0 + col, ci = ci0 + cil;
            if (co < Cout && ci < CinP) {
                const size_t o = ((size_t)co * T + t0 + tl) * CinP + ci;
                if (half) reinterpret_cast<bf16_t*>(ohwi)[o] = f32_to_bf16(sh[col * ldco + cil * tc + tl]);
                else ohwi[o] = sh[col * ldco + cil * tc + tl];
            }
        }
    if (ihwo)
        for (int i = threadIdx.x; i < cnt; i += 256) {       // (ci, t, co): co fastest
            const int col = i & 31, q = i >> 5;
            const int cil = q / tc, tl = q - cil * tc;
            const int co = co0 + col, ci = ci0 + cil;
            if (co < Cout && ci < CinP) {
                const size_t o = ((size_t)ci * T + t0 + tl) * Cout + co;
                if (half) reinterpret_cast<bf16_t*>(ihwo)[o] = f32_to_bf16(sh[col * ldco + cil * tc + tl]);
                else ihwo[o] = sh[col * ldco + cil * tc + tl];
            }
        }
}

__global__ void __launch_bounds__(256) pack_weights_table_kernel(const int64_t* __restrict__ table, int n) {
    __shared__ float sh[32 * (32 * PK_TC + 1)];
    int lo = 0, hi = n - 1;
    const int64_t tile = blockIdx.x;
    while (lo < hi) {            // last entry whose first tile is <= this block's tile
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * 8 + 7] <= tile) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* e = table + lo * 8;
    const float* w = reinterpret_cast<const float*>(e[0]);
    float* ohwi = reinterpret_cast<float*>(e[1]);
    float* ihwo = reinterpret_cast<float*>(e[2]);
    const int Cout = (int)e[3], Cin = (int)e[4], T = (int)(e[5] & 0xffff), CinP = (int)e[6];
    const bool half = ((e[5] >> 16) & 0xff) == XV2_BF16;      // packed layouts of this entry are bf16
    int j = (int)(tile - e[7]);
    const int tcs = (T + PK_TC - 1) / PK_TC, cis = (CinP + 31) / 32;
    const int tcb = j % tcs;
    j /= tcs;
    const int cib = j % cis, cob = j / cis;
    const int t0 = tcb * PK_TC, tc = min(PK_TC, T - t0);
    const int co0 = cob * 32, ci0 = cib * 32;
    switch (tc) {       // block-uniform
        case 1: pack_tile<1>(sh, w, ohwi, ihwo, Cout, Cin, T, CinP, half, t0, tc, co0, ci0); break;
        case 4: pack_tile<4>(sh, w, ohwi, ihwo, Cout, Cin, T, CinP, half, t0, tc, co0, ci0); break;
        case 9: pack_tile<9>(sh, w, ohwi, ihwo, Cout, Cin, T, CinP, half, t0, tc, co0, ci0); break;
        default: pack_tile<0>(sh, w, ohwi, ihwo, Cout, Cin, T, CinP, half, t0, tc, co0, ci0);
    }
}

}  // namespace xv2

using namespace xv2;

extern "C" int xv2_pack_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, int cin_pad, void* w_ohwi,
                               void* w_ihwo, int dtype, void* stream) {
    XV2_CHECK_ARG(cin_pad >= Cin, "pack_weight: cin_pad < Cin");
    XV2_CHECK_DTYPE(dtype);
    const size_t total = (size_t)Cout * KH * KW * cin_pad;
    const int grid = (int)std::min<size_t>(cdiv(total, 256), 4096);
    XV2_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(pack_weight_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w_oihw,
                                                 Cout, Cin, KH * KW, cin_pad, (T*)w_ohwi, (T*)w_ihwo));
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int64_t xv2_pack_weights_tiles(int Cout, int KH, int KW, int cin_pad) {
    return pack_tiles(Cout, cin_pad, KH * KW);
}

extern "C" int xv2_pack_weights_table(const int64_t* table, int n, int64_t total_tiles, void* stream) {
    XV2_CHECK_ARG(table && n > 0 && total_tiles > 0 && total_tiles < (1ll << 31), "pack_weights_table: bad table");
    hipLaunchKernelGGL(pack_weights_table_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, table, n);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
