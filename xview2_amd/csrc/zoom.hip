// A.RandomScale of the training recipe ON THE DEVICE (reference: data_loading/pytorch_loader.py:57-63, A.RandomScale(p=0.2,
// scale_limit=(0, 0.3), interpolation=INTER_CUBIC); this project's worker path resizes with Pillow, pytorch_loader.apply_scale,
// and THAT is what this kernel reproduces bit for bit): the crop window of the bicubic-resized uint8 tile and of the
// nearest-resized mask, for every zoomed sample of a batch in one launch.  Its outputs are one-off sources of xv2_augment_u8.
//
// Pillow's uint8 resampler is integer arithmetic (libImaging/Resample.c, 8bpc): per output index a first source index, a tap
// count and coefficients rounded to 22-bit fixed point; two separable passes,
//   horizontal:  t[r][x] = clip8((2^21 + sum_j src[r][xstart[x] + j] * xk[x][j]) >> 22)      for every source row r needed
//   vertical:    o[y][x] = clip8((2^21 + sum_j   t[ystart[y] + j][x] * yk[y][j]) >> 22)
// with the uint8 round-and-clip BETWEEN the passes.  Only the coefficient tables are floating point (fp64): the host builds them
// for the window's columns and rows (xview2_amd/data_loading/device_aug.py resample_tables) and this kernel never sees a float.
// |sum| <= 255 * sum_j |k_j| < 255 * 1.5 * 2^22 < 2^31: int32 as in Pillow; >> on a negative int is arithmetic.
//
// One 256-thread block per 32 x 32 output tile of one sample.  Up-scaling only, so the tap windows of consecutive outputs
// advance by <= 1 source index and hold <= 4 taps: the tile's 32 rows read <= 31 + 4 source rows.  Phase 1 runs the horizontal
// pass for those rows and the tile's 32 columns into LDS (36 x 32 x C bytes: 6.75 KB at C = 6), phase 2 the vertical pass out
// of LDS with the (x, c) index on the lanes: 96 / 192 contiguous bytes per tile row in the loads of phase 1's taps and in the
// stores.  Per tile 36/32 of the horizontal work of a full-image pass and none of its HBM round trip; a 512 x 512 x 6 window is
// 256 tiles, one per CU.
#include "xv2_common.h"

namespace xv2 {

struct ZoomSample {         // one row of the parameter table (8 x int32)
    int src;                // row of the pointer tables
    int H, W;               // source tile size
    int xoff, yoff;         // [w][7] / [h][7] {start, count, k[5]} of the window's columns / rows, offsets into `tables`
    int nxoff, nyoff;       // [w] / [h] nearest source column / row of the mask
    int reserved;
};
static_assert(sizeof(ZoomSample) == 32, "8 x 4 bytes");

constexpr int ZT = 32;              // output tile edge
constexpr int ZROWS = ZT + 4;       // source rows a tile can need (see above)
constexpr int ZTAB = 7;             // start, count, 5 coefficients

__device__ __forceinline__ uint8_t clip8(int acc) { return (uint8_t)min(max(acc >> 22, 0), 255); }

template <int C>
__global__ void __launch_bounds__(256) zoom_crop_u8_kernel(const ZoomSample* __restrict__ prm, const int* __restrict__ tab,
                                                            const uint8_t* const* __restrict__ src_img,
                                                            const uint8_t* const* __restrict__ src_mask, int h, int w,
                                                            uint8_t* __restrict__ img, uint8_t* __restrict__ mask) {
    __shared__ int sx[ZT * ZTAB], sy[ZT * ZTAB];        // 7-word rows: an odd stride, conflict-free with x on the lanes
    __shared__ uint8_t mid[ZROWS * ZT * C];             // the horizontal pass of the tile's source rows: [row][x][c]
    const int z = blockIdx.z, tid = threadIdx.x;
    const ZoomSample a = prm[z];
    const int tx0 = blockIdx.x * ZT, ty0 = blockIdx.y * ZT;
    const int tw = min(ZT, w - tx0), th = min(ZT, h - ty0), line = tw * C;
    for (int i = tid; i < tw * ZTAB; i += 256) sx[i] = tab[a.xoff + tx0 * ZTAB + i];
    for (int i = tid; i < th * ZTAB; i += 256) sy[i] = tab[a.yoff + ty0 * ZTAB + i];
    __syncthreads();
    // start and start + count are non-decreasing in the output index: the tile's source rows are [r0, r1)
    const int r0 = sy[0];
    const int nrows = min(max(sy[(th - 1) * ZTAB] + sy[(th - 1) * ZTAB + 1] - r0, 1), ZROWS);
    const uint8_t* si = src_img[a.src];
    // (indices are clamped into the tile: a corrupt table reads a wrong pixel, never another allocation)
    for (int i = tid; i < nrows * line; i += 256) {
        const int r = i / line, q = i - r * line, x = q / C, c = q - x * C;
        const int* t = sx + x * ZTAB;
        const uint8_t* p = si + (size_t)min(max(r0 + r, 0), a.H - 1) * a.W * C + c;
        int acc = 1 << 21;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (j < t[1]) acc += (int)p[(size_t)min(max(t[0] + j, 0), a.W - 1) * C] * t[2 + j];
        mid[i] = clip8(acc);
    }
    __syncthreads();
    for (int i = tid; i < th * line; i += 256) {
        const int y = i / line, q = i - y * line;
        const int* t = sy + y * ZTAB;
        const int r = t[0] - r0;
        int acc = 1 << 21;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (j < t[1]) acc += (int)mid[min(max(r + j, 0), nrows - 1) * line + q] * t[2 + j];
        img[(((size_t)z * h + ty0 + y) * w + tx0) * C + q] = clip8(acc);
    }
    const uint8_t* sm = src_mask[a.src];
    for (int i = tid; i < th * tw; i += 256) {
        const int y = i / tw, x = i - y * tw;
        const int ys = min(max(tab[a.nyoff + ty0 + y], 0), a.H - 1), xs = min(max(tab[a.nxoff + tx0 + x], 0), a.W - 1);
        mask[((size_t)z * h + ty0 + y) * w + tx0 + x] = sm[(size_t)ys * a.W + xs];
    }
}

}  // namespace xv2

using namespace xv2;

// params: [Z][8] int32 (ZoomSample) and the packed int32 tables in device memory; src_img / src_mask: the device pointer tables
// of xv2_augment_u8; outputs img [Z][h][w][C], mask [Z][h][w]
extern "C" int xv2_zoom_crop_u8(const void* params, const int32_t* tables, const void* src_img, const void* src_mask, int Z, int C,
                                int h, int w, uint8_t* img, uint8_t* mask, void* stream) {
    XV2_CHECK_ARG(params && tables && src_img && src_mask && img && mask && Z > 0 && Z <= 65535 && (C == 3 || C == 6) && h > 0 &&
                      w > 0 && cdiv(h, ZT) <= 65535,
                  "zoom_crop_u8: Z=%d C=%d h=%d w=%d", Z, C, h, w);
    const dim3 grid((unsigned)cdiv(w, ZT), (unsigned)cdiv(h, ZT), (unsigned)Z);
    if (C == 3)
        hipLaunchKernelGGL(zoom_crop_u8_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, (const ZoomSample*)params, tables,
                           (const uint8_t* const*)src_img, (const uint8_t* const*)src_mask, h, w, img, mask);
    else
        hipLaunchKernelGGL(zoom_crop_u8_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, (const ZoomSample*)params, tables,
                           (const uint8_t* const*)src_img, (const uint8_t* const*)src_mask, h, w, img, mask);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
