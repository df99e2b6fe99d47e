// Resizing a whole device scene, down and up, and the way back for the fp32 maps predicted at another size (call sites:
// xview2_amd/ops.py resize_u8 / resize_f32, xview2_amd/scene.py ScenePredictor.predict(scales=...)).  Two entry points:
//   xv2_resize_u8    uint8 [H][W][C] -> [h][w][C], bit for bit Pillow's Image.resize((w, h), Image.BICUBIC)
//   xv2_resize_f32   fp32 planar [C][Hs][Ws] -> [C][H][W] with Pillow's bilinear (triangle) filter in this project's own exact
//                    fp32 rule, written to dst, added to dst, or added and divided by the number of scales
//
// Both are the separable resampler of libImaging/Resample.c: per output index a first source index, a tap count and
// coefficients; horizontal pass first, vertical pass second.  Down-scaling widens the filter (support = base * max(in / out, 1),
// antialiasing), so the tap count grows with the ratio: ceil(support) * 2 + 1 slots, 17 (bicubic) / 9 (bilinear) under the
// limit in <= 4 out, out <= 4 in per axis.  The host builds the tables in fp64 (xview2_amd/resize.py axis_table_u8 /
// axis_table_f32): rows of {start, count, k[taps]} int32 words, k in 22-bit fixed point (uint8) or the bits of an fp32 (maps).
// An axis that keeps its size carries the identity table {i, 1, one}, which gives the source value itself: the same bytes as
// Pillow's skipped pass.
//   uint8:  t = clip8((2^21 + sum_j s[start + j] k[j]) >> 22) after EACH pass; |sum| < 255 * 1.5 * 2^22 < 2^31, int32 as Pillow
//   fp32:   t = k[0] s[start]; t = t + k[j] s[start + j] for j = 1 .. count - 1 in tap order, every product and every sum
//           rounded to fp32 on its own (no fused multiply-add: see the pragma below); the intermediate is fp32
//
// The form kept is zoom.hip's, ONE launch and no intermediate in HBM: one 256-thread block per output tile (32 x 32 pixels
// uint8, 32 rows x 64 columns fp32).  Phase 1 runs the horizontal pass of the source rows the tile's rows need, for the tile's
// columns only, into LDS; phase 2 runs the vertical pass out of LDS with (x, c) - x for the planar maps - on the lanes, so a
// wave stores contiguous bytes.  The rows a tile needs are start[last] + count[last] - start[first] <= ceil(31 in / out) + taps:
// the entry point sizes the dynamic LDS by that bound from the sizes alone (at 4:1 down-scaling 142 rows, 13.3 KB at C = 3, and
// 134 rows, 33.5 KB, for a map tile; when up-scaling under 5 KB), and the kernel clamps the row count to it.  Neighbouring tiles of a
// column repeat the horizontal pass of the rows their tap windows share (taps of every ceil(32 in / out) rows).
//
// Every table-derived index is clamped into the image, the tap count into the slots and the row count into the LDS buffer: a
// corrupt table reads a wrong pixel, never another allocation.  Offsets are 64-bit.
#include "xv2_common.h"

// HIP's default -ffp-contract=fast fuses a product into the sum that follows it, one rounding instead of two - also through
// __fmul_rn / __fadd_rn, which the HIP headers define as plain * and + compiled under that default.  The fp32 rule rounds
// every product and every sum, so contraction is off for this file and the three operations are written here, under the pragma.
#pragma clang fp contract(off)

namespace xv2 {

__device__ __forceinline__ float rz_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rz_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rz_div(float a, float b) { return a / b; }      // IEEE division (hipcc's default for fp32 /)

constexpr int RZ_TH = 32;                                   // output rows per tile
constexpr int RZ_TW_U8 = 32, RZ_TW_F32 = 64;                // output columns per tile
constexpr int RZ_ROW_U8 = 2 + XV2_RESIZE_U8_TAPS;           // table row: start, count, coefficients (19 and 11 words: odd
constexpr int RZ_ROW_F32 = 2 + XV2_RESIZE_F32_TAPS;         // strides, conflict-free with the output index on the lanes)

__device__ __forceinline__ uint8_t rz_clip8(int acc) { return (uint8_t)min(max(acc >> 22, 0), 255); }
// the three bytes at off in the low 24 bits: one dword load at any alignment (gfx950 global loads need none), except where the
// dword would end past the image's `total` bytes - its last pixel
__device__ __forceinline__ uint32_t rz_ld3(const uint8_t* __restrict__ base, size_t off, size_t total) {
    if (off + 4 <= total) {
        uint32_t v;
        __builtin_memcpy(&v, base + off, 4);
        return v;
    }
    return (uint32_t)base[off] | ((uint32_t)base[off + 1] << 8) | ((uint32_t)base[off + 2] << 16);
}

// source rows a tile's RZ_TH output rows can need on an axis in -> out whose tables hold `taps` slots
static inline int rz_max_rows(int in, int out, int taps) { return (int)cdiv((int64_t)(RZ_TH - 1) * in, out) + taps + 1; }
// the slots Pillow allocates: ceil(base support * max(in / out, 1)) * 2 + 1
static inline int rz_taps(int in, int out, int base) { return 2 * (in > out ? (int)cdiv((int64_t)base * in, out) : base) + 1; }

template <int C>
__global__ void __launch_bounds__(256) resize_u8_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                         const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab,
                                                         int h, int w, int ntx, int maxrows, uint8_t* __restrict__ dst) {
    __shared__ int sx[RZ_TW_U8 * RZ_ROW_U8], sy[RZ_TH * RZ_ROW_U8];
    extern __shared__ uint8_t rz_mid_u8[];                   // [maxrows][32][C]: the horizontal pass of the tile's source rows
    constexpr int STRIDE = RZ_TW_U8 * C;
    uint8_t* mid = rz_mid_u8;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int tx0 = tx * RZ_TW_U8, ty0 = ty * RZ_TH;
    const int tw = min(RZ_TW_U8, w - tx0), th = min(RZ_TH, h - ty0), line = tw * C;
    for (int i = tid; i < tw * RZ_ROW_U8; i += 256) sx[i] = xtab[(size_t)tx0 * RZ_ROW_U8 + i];
    for (int i = tid; i < th * RZ_ROW_U8; i += 256) sy[i] = ytab[(size_t)ty0 * RZ_ROW_U8 + i];
    __syncthreads();
    // start and start + count are non-decreasing in the output index: the tile's source rows are [r0, r0 + nrows)
    const int r0 = sy[0];
    const int nrows = min(max(sy[(th - 1) * RZ_ROW_U8] + sy[(th - 1) * RZ_ROW_U8 + 1] - r0, 1), maxrows);
    if (C % 3 == 0) {
        // three channels per thread and ONE load per tap: the dword at the pixel's first byte holds its three channels (one
        // byte load per channel and tap made this pass wait on the texture addresser, 0.3 of xv2_translate_u8's rate)
        constexpr int G = C / 3;
        const size_t total = (size_t)H * W * C;
        const int units = tw * G;
        for (int i = tid; i < nrows * units; i += 256) {
            const int r = i / units, u = i - r * units, x = u / G, g = u - x * G;
            const int* t = sx + x * RZ_ROW_U8;
            const int s0 = t[0], n = min(max(t[1], 0), XV2_RESIZE_U8_TAPS);
            const size_t row = (size_t)min(max(r0 + r, 0), H - 1) * W * C + 3 * g;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int j = 0; j < n; ++j) {
                const uint32_t v = rz_ld3(src, row + (size_t)min(max(s0 + j, 0), W - 1) * C, total);
                const int k = t[2 + j];
                a0 += (int)(v & 255u) * k;
                a1 += (int)((v >> 8) & 255u) * k;
                a2 += (int)((v >> 16) & 255u) * k;
            }
            uint8_t* m = mid + r * STRIDE + x * C + 3 * g;
            m[0] = rz_clip8(a0);
            m[1] = rz_clip8(a1);
            m[2] = rz_clip8(a2);
        }
    } else {
        for (int i = tid; i < nrows * line; i += 256) {
            const int r = i / line, q = i - r * line, x = q / C, c = q - x * C;
            const int* t = sx + x * RZ_ROW_U8;
            const int s0 = t[0], n = min(max(t[1], 0), XV2_RESIZE_U8_TAPS);
            const uint8_t* p = src + (size_t)min(max(r0 + r, 0), H - 1) * W * C + c;
            int acc = 1 << 21;
            for (int j = 0; j < n; ++j) acc += (int)p[(size_t)min(max(s0 + j, 0), W - 1) * C] * t[2 + j];
            mid[r * STRIDE + q] = rz_clip8(acc);
        }
    }
    __syncthreads();
    // four output bytes per lane: one dword of LDS per tap (rows of mid are STRIDE bytes apart, a multiple of 4, so the dword is
    // aligned; bytes past `line` are unused and dropped) and one dword store, at any alignment - one byte store per lane held
    // up-scaling at 0.3 of xv2_translate_u8's rate.  mid is declared as bytes, so its dwords are read with memcpy.
    const int words = (line + 3) >> 2;
    for (int i = tid; i < th * words; i += 256) {
        const int y = i / words, q = (i - y * words) * 4;
        const int* t = sy + y * RZ_ROW_U8;
        const int r = t[0] - r0, n = min(max(t[1], 0), XV2_RESIZE_U8_TAPS);
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int j = 0; j < n; ++j) {
            uint32_t v;
            __builtin_memcpy(&v, mid + min(max(r + j, 0), nrows - 1) * STRIDE + q, 4);
            const int k = t[2 + j];
            a0 += (int)(v & 255u) * k;
            a1 += (int)((v >> 8) & 255u) * k;
            a2 += (int)((v >> 16) & 255u) * k;
            a3 += (int)(v >> 24) * k;
        }
        uint8_t* o = dst + ((size_t)(ty0 + y) * w + tx0) * C + q;
        const uint32_t v = (uint32_t)rz_clip8(a0) | ((uint32_t)rz_clip8(a1) << 8) | ((uint32_t)rz_clip8(a2) << 16) |
                           ((uint32_t)rz_clip8(a3) << 24);
        if (q + 4 <= line) {
            __builtin_memcpy(o, &v, 4);
        } else {
            o[0] = (uint8_t)v;
            if (q + 1 < line) o[1] = (uint8_t)(v >> 8);
            if (q + 2 < line) o[2] = (uint8_t)(v >> 16);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) resize_f32_kernel(const float* __restrict__ src, int Hs, int Ws,
                                                          const int32_t* __restrict__ xtab, const int32_t* __restrict__ ytab,
                                                          int H, int W, int ntx, int nty, int maxrows, float divisor,
                                                          float* __restrict__ dst) {
    __shared__ int sx[RZ_TW_F32 * RZ_ROW_F32], sy[RZ_TH * RZ_ROW_F32];
    extern __shared__ float rz_mid_f32[];                    // [maxrows][RZ_TW_F32]
    float* mid = rz_mid_f32;
    const int tid = threadIdx.x;
    const int tiles = ntx * nty;
    const int c = blockIdx.x / tiles, rem = blockIdx.x - c * tiles;
    const int ty = rem / ntx, tx = rem - ty * ntx;
    const int tx0 = tx * RZ_TW_F32, ty0 = ty * RZ_TH;
    const int tw = min(RZ_TW_F32, W - tx0), th = min(RZ_TH, H - ty0);
    for (int i = tid; i < tw * RZ_ROW_F32; i += 256) sx[i] = xtab[(size_t)tx0 * RZ_ROW_F32 + i];
    for (int i = tid; i < th * RZ_ROW_F32; i += 256) sy[i] = ytab[(size_t)ty0 * RZ_ROW_F32 + i];
    __syncthreads();
    const int r0 = sy[0];
    const int nrows = min(max(sy[(th - 1) * RZ_ROW_F32] + sy[(th - 1) * RZ_ROW_F32 + 1] - r0, 1), maxrows);
    const float* plane = src + (size_t)c * Hs * Ws;
    const int x = tid & (RZ_TW_F32 - 1);                     // one wave per row, x on the lanes
    if (x < tw) {
        const int* t = sx + x * RZ_ROW_F32;
        const int s0 = t[0], n = min(max(t[1], 1), XV2_RESIZE_F32_TAPS);
        for (int r = tid / RZ_TW_F32; r < nrows; r += 256 / RZ_TW_F32) {
            const float* p = plane + (size_t)min(max(r0 + r, 0), Hs - 1) * Ws;
            float acc = rz_mul(__int_as_float(t[2]), p[min(max(s0, 0), Ws - 1)]);
            for (int j = 1; j < n; ++j)
                acc = rz_add(acc, rz_mul(__int_as_float(t[2 + j]), p[min(max(s0 + j, 0), Ws - 1)]));
            mid[r * RZ_TW_F32 + x] = acc;
        }
    }
    __syncthreads();
    if (x >= tw) return;
    float* out = dst + (size_t)c * H * W + tx0 + x;
    for (int y = tid / RZ_TW_F32; y < th; y += 256 / RZ_TW_F32) {
        const int* t = sy + y * RZ_ROW_F32;
        const int r = t[0] - r0, n = min(max(t[1], 1), XV2_RESIZE_F32_TAPS);
        float acc = rz_mul(__int_as_float(t[2]), mid[min(max(r, 0), nrows - 1) * RZ_TW_F32 + x]);
        for (int j = 1; j < n; ++j)
            acc = rz_add(acc, rz_mul(__int_as_float(t[2 + j]), mid[min(max(r + j, 0), nrows - 1) * RZ_TW_F32 + x]));
        float* o = out + (size_t)(ty0 + y) * W;
        if (MODE == XV2_RESIZE_ACCUMULATE) acc = rz_add(*o, acc);
        if (MODE == XV2_RESIZE_FINISH) acc = rz_div(rz_add(*o, acc), divisor);
        *o = acc;
    }
}

static int check_resize(const char* what, int in_h, int in_w, int out_h, int out_w) {
    XV2_CHECK_ARG(in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "%s: %d x %d -> %d x %d: sizes must be positive", what, in_h,
                  in_w, out_h, out_w);
    XV2_CHECK_ARG((int64_t)in_h * in_w < (1ll << 30) && (int64_t)out_h * out_w < (1ll << 30),
                  "%s: %d x %d -> %d x %d exceeds 2^30 pixels per image", what, in_h, in_w, out_h, out_w);
    XV2_CHECK_ARG((int64_t)out_h <= 4ll * in_h && (int64_t)in_h <= 4ll * out_h && (int64_t)out_w <= 4ll * in_w &&
                      (int64_t)in_w <= 4ll * out_w,
                  "%s: %d x %d -> %d x %d: per axis out <= 4 in and in <= 4 out are required", what, in_h, in_w, out_h, out_w);
    return XV2_OK;
}

}  // namespace xv2

using namespace xv2;

extern "C" int xv2_resize_u8(const uint8_t* src, int H, int W, int C, const int32_t* xtab, const int32_t* ytab, int h, int w,
                             uint8_t* dst, void* stream) {
    if (int rc = check_resize("resize_u8", H, W, h, w)) return rc;
    XV2_CHECK_ARG(C == 1 || C == 3 || C == 6, "resize_u8: C=%d must be 1, 3 or 6", C);
    XV2_CHECK_ARG(src && xtab && ytab && dst, "resize_u8: null tensor");
    const int ntx = (int)cdiv(w, RZ_TW_U8), nty = (int)cdiv(h, RZ_TH);
    const int maxrows = rz_max_rows(H, h, rz_taps(H, h, 2));
    const dim3 grid((unsigned)((int64_t)ntx * nty));
    const size_t lds = (size_t)maxrows * RZ_TW_U8 * C;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1)
        hipLaunchKernelGGL(resize_u8_kernel<1>, grid, dim3(256), lds, st, src, H, W, xtab, ytab, h, w, ntx, maxrows, dst);
    else if (C == 3)
        hipLaunchKernelGGL(resize_u8_kernel<3>, grid, dim3(256), lds, st, src, H, W, xtab, ytab, h, w, ntx, maxrows, dst);
    else
        hipLaunchKernelGGL(resize_u8_kernel<6>, grid, dim3(256), lds, st, src, H, W, xtab, ytab, h, w, ntx, maxrows, dst);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

extern "C" int xv2_resize_f32(const float* src, int C, int Hs, int Ws, const int32_t* xtab, const int32_t* ytab, int H, int W,
                              int mode, int k, float* dst, void* stream) {
    if (int rc = check_resize("resize_f32", Hs, Ws, H, W)) return rc;
    XV2_CHECK_ARG(C >= 1 && C <= 8, "resize_f32: C=%d must be in 1..8", C);
    XV2_CHECK_ARG(mode == XV2_RESIZE_WRITE || mode == XV2_RESIZE_ACCUMULATE || mode == XV2_RESIZE_FINISH,
                  "resize_f32: unknown mode %d (write 0, accumulate 1, accumulate and finish 2)", mode);
    XV2_CHECK_ARG(k >= 1 && k <= 8, "resize_f32: k=%d maps in the average must be in 1..8", k);
    XV2_CHECK_ARG(src && xtab && ytab && dst, "resize_f32: null tensor");
    const int ntx = (int)cdiv(W, RZ_TW_F32), nty = (int)cdiv(H, RZ_TH);
    const int maxrows = rz_max_rows(Hs, H, rz_taps(Hs, H, 1));
    const dim3 grid((unsigned)((int64_t)ntx * nty * C));
    const size_t lds = (size_t)maxrows * RZ_TW_F32 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const float divisor = (float)k;
    if (mode == XV2_RESIZE_WRITE)
        hipLaunchKernelGGL(resize_f32_kernel<XV2_RESIZE_WRITE>, grid, dim3(256), lds, st, src, Hs, Ws, xtab, ytab, H, W, ntx, nty,
                           maxrows, divisor, dst);
    else if (mode == XV2_RESIZE_ACCUMULATE)
        hipLaunchKernelGGL(resize_f32_kernel<XV2_RESIZE_ACCUMULATE>, grid, dim3(256), lds, st, src, Hs, Ws, xtab, ytab, H, W, ntx,
                           nty, maxrows, divisor, dst);
    else
        hipLaunchKernelGGL(resize_f32_kernel<XV2_RESIZE_FINISH>, grid, dim3(256), lds, st, src, Hs, Ws, xtab, ytab, H, W, ntx,
                           nty, maxrows, divisor, dst);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
