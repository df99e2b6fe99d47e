// `--autoaugment` ON THE DEVICE (reference: data_loading/autoaugment.py ImageNetPolicy as used by pytorch_loader.py:75-84,
// :125-138; this project's worker path runs it through Pillow, xview2_amd/data_loading/autoaugment.py, and THAT is what these
// kernels reproduce bit for bit): the two-operation sub-policy of every sample of a batch, applied in place to the cropped
// uint8 tiles [N][h][w][C] and masks [N][h][w] that xv2_augment_u8 has just written.
//
// The DECISIONS are drawn on the host (autoaugment.draw_policy) and travel as one [N][2][8] int32 table: per sample and stage
// an operation id and its operands.  The ten operations of the POLICY table are three kinds of byte arithmetic, all restated
// in numpy by xview2_amd/data_loading/device_autoaug.py (autoaug_numpy):
//   point tables  posterize / solarize / invert: 256-byte tables the host builds (as ImageOps does);
//                 autocontrast / equalize: tables this file builds from the per-channel histogram of the stage's input -
//                 equalize in integers, autocontrast as ONE fp64 multiply and ONE add per entry (ImageOps.autocontrast)
//   blends        color / contrast / sharpness = Image.blend(degenerate, image, f): float32 d + f * (i - d), truncated
//                 (libImaging/Blend.c); the degenerate image is L replicated / the rounded mean of L / ImageFilter.SMOOTH
//   gathers       rotate: NEAREST gather through a 16.16 fixed-point affine map, zero fill (Geometry.c affine_fixed);
//                 shearX: BICUBIC in fp64 (Geometry.c affine_transform + bicubic_filter), image AND mask
// hipcc contracts a * b + c into one fused operation by default and Pillow's C is compiled without, so this file switches
// contraction OFF (the pragma below) and spells every float32 / fp64 step with plain operators in Pillow's operand order.  The
// __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn intrinsics do not serve: in this toolchain's headers they ARE plain operators,
// compiled with contraction on, and a __fadd_rn(d, __fmul_rn(f, x)) comes out as one v_fma (the blend then differs from Pillow
// in ~1 % of the bytes).  Histograms and sums are integer atomics: order-independent.
//
// Per stage at most three launches, ordered by the stream alone: statistics (LDS histograms / L sums of the samples whose
// operation needs them, flushed with one global atomic per non-empty bin and block), tables (one block per sample and
// channel) and apply (one thread per pixel, the sample's operation selected from its parameter row - uniform per block).
// A gather cannot run in place, so stage 1 writes the workspace's copy of the batch and stage 2 writes the batch back; a sample
// without an operation in a stage is copied.  HBM-bound byte kernels: 2 x (C + 1) bytes per pixel and stage.
#include "xv2_common.h"

#pragma clang fp contract(off)

namespace xv2 {

enum { AA_NONE, AA_TABLE, AA_AUTOCONTRAST, AA_EQUALIZE, AA_COLOR, AA_CONTRAST, AA_SHARPNESS, AA_ROTATE, AA_SHEARX, AA_OPS };

struct AaStage {            // one row of the parameter table (8 x int32)
    int op;
    int a[6];               // blends: a[0] = bits of the float32 factor; rotate: a0 .. a5; shearX: a[1], a[2] = the fp64 coefficient
    int reserved;
};
static_assert(sizeof(AaStage) == 32, "8 x 4 bytes");

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
    return v;
}

// convert("L") of one stored 3-channel pixel (Convert.c L24)
__device__ __forceinline__ int luma(const uint8_t* p) { return (p[0] * 19595 + p[1] * 38470 + p[2] * 7471 + 0x8000) >> 16; }

template <int C>
__global__ void __launch_bounds__(256) autoaug_stats_kernel(const AaStage* __restrict__ prm, int stage,
                                                             const uint8_t* __restrict__ src, int hw,
                                                             unsigned* __restrict__ hist, unsigned* __restrict__ lsum) {
    __shared__ unsigned sh[C * 256];
    const int n = blockIdx.y, tid = threadIdx.x, op = prm[n * 2 + stage].op;
    const uint8_t* s = src + (size_t)n * hw * C;
    if (op == AA_CONTRAST) {                    // sum of L per image: hw <= 2^24 pixels, 2^24 * 255 < 2^32
        unsigned acc[C / 3] = {};
        for (int p = blockIdx.x * 256 + tid; p < hw; p += gridDim.x * 256) {
#pragma unroll
            for (int k = 0; k < C / 3; ++k) acc[k] += (unsigned)luma(s + (size_t)p * C + 3 * k);
        }
#pragma unroll
        for (int k = 0; k < C / 3; ++k) {
            const unsigned v = wave_sum_u(acc[k]);
            if ((tid & 63) == 0 && v) atomicAdd(lsum + n * 2 + k, v);
        }
        return;
    }
    if (op != AA_AUTOCONTRAST && op != AA_EQUALIZE) return;
    for (int i = tid; i < C * 256; i += 256) sh[i] = 0;
    __syncthreads();
    for (int p = blockIdx.x * 256 + tid; p < hw; p += gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < C; ++c) atomicAdd(sh + c * 256 + s[(size_t)p * C + c], 1u);
    }
    __syncthreads();
    for (int i = tid; i < C * 256; i += 256)
        if (sh[i]) atomicAdd(hist + (size_t)n * C * 256 + i, sh[i]);
}

// one block per (channel, sample), thread i builds entry i
__global__ void __launch_bounds__(256) autoaug_table_kernel(const AaStage* __restrict__ prm, int stage, int C, int hw,
                                                             const unsigned* __restrict__ hist, uint8_t* __restrict__ tables) {
    __shared__ unsigned sh[256];
    __shared__ int lohi[2];
    const int n = blockIdx.y, c = blockIdx.x, i = threadIdx.x, op = prm[n * 2 + stage].op;
    if (op != AA_AUTOCONTRAST && op != AA_EQUALIZE) return;
    sh[i] = hist[((size_t)n * C + c) * 256 + i];
    if (i == 0) lohi[0] = 255, lohi[1] = 0;
    __syncthreads();
    if (sh[i]) atomicMin(lohi, i), atomicMax(lohi + 1, i);
    __syncthreads();
    const int lo = lohi[0], hi = lohi[1];       // first and last non-empty bin
    int v = i;                                  // one non-empty bin, or equalize's step == 0: the channel is unchanged
    if (hi > lo) {
        if (op == AA_AUTOCONTRAST) {
            const double scale = 255.0 / (double)(hi - lo);         // (fp64 division is correctly rounded)
            const double offset = -(double)lo * scale;
            v = min(max((int)((double)i * scale + offset), 0), 255);
        } else {
            const unsigned step = ((unsigned)hw - sh[hi]) / 255u;
            if (step) {
                unsigned acc = step / 2;
                for (int j = 0; j < i; ++j) acc += sh[j];      // (every lane reads the same word: an LDS broadcast)
                v = (int)min(acc / step, 255u);                 // Image.point clips the table
            }
        }
    }
    tables[((size_t)n * C + c) * 256 + i] = (uint8_t)v;
}

__device__ __forceinline__ uint8_t clip_trunc(float t) { return t <= 0.f ? 0 : t >= 255.f ? 255 : (uint8_t)(int)t; }

// Blend.c: (UINT8)(d + f * (i - d)) for 0 <= f <= 1 (the value cannot leave 0 .. 255), clipped otherwise
__device__ __forceinline__ uint8_t blend8(int d, int i, float f, bool inside) {
    const float t = (float)d + f * (float)(i - d);
    return inside ? (uint8_t)(int)t : clip_trunc(t);
}

// ImageFilter.SMOOTH at an interior pixel (Filter.c ImagingFilter3x3): 0.5, then rows y + 1, y, y - 1, each summed left to right
__device__ __forceinline__ int smooth8(const uint8_t* p, int rowstride, int C) {
    constexpr float K1 = 1.0f / 13.0f, K5 = 5.0f / 13.0f;
    float ss = 0.5f;
#pragma unroll
    for (int r = 1; r >= -1; --r) {
        const uint8_t* q = p + r * rowstride;
        const float kc = r == 0 ? K5 : K1;
        ss = ss + (((float)q[-C] * K1 + (float)q[0] * kc) + (float)q[C] * K1);
    }
    return min((int)ss, 255);       // ss >= 0.5: truncation is floor
}

// one row of Geometry.c's BICUBIC at fraction d: the four taps are integers, p2 .. p4 exact
__device__ __forceinline__ uint8_t cubic8(int v1, int v2, int v3, int v4, double d) {
    const double p2 = (double)(-v1 + v3), p3 = (double)(2 * (v1 - v2) + v3 - v4), p4 = (double)(-v1 + v2 - v3 + v4);
    const double v = (double)v2 + d * (p2 + d * (p3 + d * p4));
    return v <= 0.0 ? 0 : v >= 255.0 ? 255 : (uint8_t)(int)v;
}

template <int C>
__global__ void __launch_bounds__(256) autoaug_apply_kernel(const AaStage* __restrict__ prm, int stage,
                                                             const uint8_t* __restrict__ luts, const uint8_t* __restrict__ tables,
                                                             const unsigned* __restrict__ lsum, int h, int w,
                                                             const uint8_t* __restrict__ src, const uint8_t* __restrict__ srcm,
                                                             uint8_t* __restrict__ dst, uint8_t* __restrict__ dstm) {
    const int n = blockIdx.y, hw = h * w;
    const AaStage a = prm[n * 2 + stage];
    const uint8_t* si = src + (size_t)n * hw * C;
    const uint8_t* sm = srcm + (size_t)n * hw;
    uint8_t* di = dst + (size_t)n * hw * C;
    uint8_t* dm = dstm + (size_t)n * hw;
    const float f = __int_as_float(a.a[0]);
    const bool inside = f >= 0.f && f <= 1.f;
    const double shear = __hiloint2double(a.a[2], a.a[1]);
    int mean[C / 3] = {};
    if (a.op == AA_CONTRAST) {
        // int(sum / hw + 0.5) = (2 sum + hw) / (2 hw) in integers: sum / hw is a multiple of 1 / hw, never within an fp64
        // rounding error of a half-integer without being one (hw <= 2^24)
#pragma unroll
        for (int k = 0; k < C / 3; ++k) mean[k] = (int)((2ull * lsum[n * 2 + k] + (unsigned)hw) / (2ull * (unsigned)hw));
    }
    for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
        const int y = p / w, x = p - y * w;
        const uint8_t* s = si + (size_t)p * C;
        uint8_t o[C];
        uint8_t om = sm[p];
        switch (a.op) {
        case AA_TABLE:
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = luts[((size_t)n * 2 + stage) * 256 + s[c]];
            break;
        case AA_AUTOCONTRAST:
        case AA_EQUALIZE:
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = tables[((size_t)n * C + c) * 256 + s[c]];
            break;
        case AA_COLOR:
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = blend8(luma(s + 3 * (c / 3)), s[c], f, inside);
            break;
        case AA_CONTRAST:
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = blend8(mean[c / 3], s[c], f, inside);
            break;
        case AA_SHARPNESS: {
            const bool interior = x > 0 && y > 0 && x < w - 1 && y < h - 1;        // SMOOTH copies the 1-pixel border
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = blend8(interior ? smooth8(s + c, w * C, C) : (int)s[c], s[c], f, inside);
            break;
        }
        case AA_ROTATE: {
            const long long xs = ((long long)a.a[2] + (long long)a.a[1] * y + (long long)a.a[0] * x) >> 16;
            const long long ys = ((long long)a.a[5] + (long long)a.a[4] * y + (long long)a.a[3] * x) >> 16;
            const bool ok = xs >= 0 && xs < w && ys >= 0 && ys < h;
            const size_t q = ok ? (size_t)ys * w + (size_t)xs : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = ok ? si[q * C + c] : 0;
            om = ok ? sm[q] : 0;
            break;
        }
        case AA_SHEARX: {
            // xin = 1 * (x + 0.5) + c * (y + 0.5) + 0, yin = y + 0.5: the row fraction is 0 and bicubic's column pass
            // p1 + 0 * (...) returns the row's value unchanged - only the pass along row y is left
            double xin = 1.0 * ((double)x + 0.5) + shear * ((double)y + 0.5) + 0.0;
            const bool ok = xin >= 0.0 && xin < (double)w;
            xin = xin - 0.5;
            const double xf = floor(xin), d = xin - xf;
            const int xb = ok ? (int)xf - 1 : 0;
            const int x1 = min(max(xb, 0), w - 1), x2 = min(max(xb + 1, 0), w - 1), x3 = min(max(xb + 2, 0), w - 1),
                      x4 = min(max(xb + 3, 0), w - 1);
            const uint8_t* r = si + (size_t)y * w * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = ok ? cubic8(r[x1 * C + c], r[x2 * C + c], r[x3 * C + c], r[x4 * C + c], d) : 0;
            const uint8_t* rm = sm + (size_t)y * w;
            om = ok ? cubic8(rm[x1], rm[x2], rm[x3], rm[x4], d) : 0;       // the reference interpolates the labels
            break;
        }
        default:
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = s[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) di[(size_t)p * C + c] = o[c];
        dm[p] = om;
    }
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct AaLayout {
    size_t hist, lsum, tables, img, mask, total;        // byte offsets; hist and lsum hold both stages and are zeroed together
    AaLayout(int N, int C, int h, int w) {
        hist = 0;
        lsum = hist + up256((size_t)2 * N * C * 256 * sizeof(unsigned));
        tables = lsum + up256((size_t)2 * N * 2 * sizeof(unsigned));
        img = tables + up256((size_t)N * C * 256);
        mask = img + up256((size_t)N * h * w * C);
        total = mask + up256((size_t)N * h * w);
    }
};

static bool aa_shape_ok(int N, int C, int h, int w) {
    return N > 0 && N <= 65535 && (C == 3 || C == 6) && h > 0 && w > 0 && (int64_t)h * w <= (1 << 24);
}

}  // namespace xv2

using namespace xv2;

extern "C" size_t xv2_autoaugment_workspace(int N, int C, int h, int w) {
    return aa_shape_ok(N, C, h, w) ? AaLayout(N, C, h, w).total : 0;
}

// host_params: the [N][2][8] int32 table in HOST memory (validated here, and it decides which launches a stage needs);
// params: the same table in device memory; luts: [N][2][256] uint8 host-built tables in device memory (NULL: no sample uses
// one); img [N][h][w][C] and mask [N][h][w] in place
extern "C" int xv2_autoaugment_u8(const int32_t* host_params, const void* params, const uint8_t* luts, int N, int C, int h, int w,
                                  uint8_t* img, uint8_t* mask, void* workspace, void* stream) {
    XV2_CHECK_ARG(host_params && params && img && mask && workspace && aa_shape_ok(N, C, h, w),
                  "autoaugment_u8: N=%d C=%d h=%d w=%d (or a null pointer)", N, C, h, w);
    bool active = false, stats[2] = {false, false}, tabs[2] = {false, false};
    for (int n = 0; n < N; ++n)
        for (int s = 0; s < 2; ++s) {
            const int op = host_params[(n * 2 + s) * 8];
            XV2_CHECK_ARG(op >= 0 && op < AA_OPS, "autoaugment_u8: unknown operation id %d (sample %d, stage %d)", op, n, s);
            XV2_CHECK_ARG(op != AA_TABLE || luts, "autoaugment_u8: sample %d uses a point table and luts is null", n);
            active |= op != AA_NONE;
            tabs[s] |= op == AA_AUTOCONTRAST || op == AA_EQUALIZE;
            stats[s] |= op == AA_AUTOCONTRAST || op == AA_EQUALIZE || op == AA_CONTRAST;
        }
    if (!active) return XV2_OK;
    const AaLayout L(N, C, h, w);
    const hipStream_t st = (hipStream_t)stream;
    const AaStage* prm = (const AaStage*)params;
    uint8_t* ws = (uint8_t*)workspace;
    uint8_t* tables = ws + L.tables;
    const int hw = h * w;
    if (stats[0] || stats[1]) XV2_CHECK_HIP(hipMemsetAsync(ws, 0, L.tables, st));
    const dim3 sgrid((unsigned)std::min<int64_t>(cdiv(hw, 4096), 64), (unsigned)N);
    const dim3 agrid((unsigned)std::min<int64_t>(cdiv(hw, 256), 1024), (unsigned)N);
    for (int s = 0; s < 2; ++s) {
        const uint8_t* si = s == 0 ? img : ws + L.img;
        const uint8_t* sm = s == 0 ? mask : ws + L.mask;
        uint8_t* di = s == 0 ? ws + L.img : img;
        uint8_t* dm = s == 0 ? ws + L.mask : mask;
        unsigned* hist = (unsigned*)(ws + L.hist) + (size_t)s * N * C * 256;
        unsigned* lsum = (unsigned*)(ws + L.lsum) + (size_t)s * N * 2;
        if (stats[s]) {
            if (C == 3)
                hipLaunchKernelGGL(autoaug_stats_kernel<3>, sgrid, dim3(256), 0, st, prm, s, si, hw, hist, lsum);
            else
                hipLaunchKernelGGL(autoaug_stats_kernel<6>, sgrid, dim3(256), 0, st, prm, s, si, hw, hist, lsum);
            XV2_CHECK_LAUNCH();
        }
        if (tabs[s]) {
            hipLaunchKernelGGL(autoaug_table_kernel, dim3((unsigned)C, (unsigned)N), dim3(256), 0, st, prm, s, C, hw, hist, tables);
            XV2_CHECK_LAUNCH();
        }
        if (C == 3)
            hipLaunchKernelGGL(autoaug_apply_kernel<3>, agrid, dim3(256), 0, st, prm, s, luts, tables, lsum, h, w, si, sm, di, dm);
        else
            hipLaunchKernelGGL(autoaug_apply_kernel<6>, agrid, dim3(256), 0, st, prm, s, luts, tables, lsum, h, w, si, sm, di, dm);
        XV2_CHECK_LAUNCH();
    }
    return XV2_OK;
}
