// Polygons -> masks (include/xv2.h xv2_rasterize_polygons): the even-odd, closed-boundary fill of every feature of a batch of
// tiles, painted in table order with the last feature winning.  The contract (sample points, on-edge, crossing, painting) is
// the header's; this file is one method for it.
//
// Every value is an integer and the only atomic is an integer max into the order map, so no result depends on the order in
// which blocks run: the same bits come out of every run.  Three launches, nothing is read back:
//   clear              order map uint32 [B,H,W] = 0 (hipMemsetAsync on the stream)
//   rs_cover_kernel    one block per work item (a 32 x 32 window of a feature's clipped box), four pixels of one row per
//                      thread; the feature's edges pass through LDS in stages of 256; every covered pixel does
//                      atomicMax(order, feature index + 1)
//   rs_resolve_kernel  out = value of feature order - 1, or 0
// The order map holds the feature's index in the table, not its position within its tile: features are sorted by tile and
// keep file order inside one, and a pixel belongs to one tile, so the largest index is the last feature of the file that
// covers the pixel, and the resolve pass needs no per-tile offset.
//
// The cross products run in int64: |coordinate| <= 2^24 and samples <= 2^24 + 2^7 keep every factor below 2^26 and every
// product below 2^52.  A thread's four samples differ in x alone, so one pair of products per edge serves all four (the
// next sample's cr is the last one's minus (by - ay) << k), and the y-range test that skips an edge comes before any multiply.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

constexpr int STAGE = 256;             // edges per LDS stage, one per thread (a window is 32 x 32 pixels: 256 threads x 4)
constexpr int FEAT_COLS = 8, WORK_COLS = 4;
constexpr int COORD_MAX = 1 << 24;

__global__ void __launch_bounds__(256) rs_cover_kernel(const int4* __restrict__ edges, long long n_edges,
                                                       const int32_t* __restrict__ features, int n_features,
                                                       const int4* __restrict__ work, int k, int off, int B, int H, int W,
                                                       unsigned* __restrict__ order) {
    __shared__ int4 E[STAGE];
    const int4 item = work[blockIdx.x];
    const int f = item.x;
    if (f < 0 || f >= n_features) return;                            // (block-uniform; the host copy was validated, this only
    const int32_t* ft = features + (int64_t)f * FEAT_COLS;           //  keeps a table that changed under the call inside bounds)
    const int4 fa = *reinterpret_cast<const int4*>(ft), box = *reinterpret_cast<const int4*>(ft + 4);
    const int b = fa.x;
    const long long e0 = fa.z;
    const int ne = fa.w;
    if (b < 0 || b >= B || e0 < 0 || ne < 0 || e0 + ne > n_edges) return;
    const int y = item.z + (int)(threadIdx.x >> 3), x0 = item.y + (int)(threadIdx.x & 7u) * 4;
    const int step = 1 << k;
    const long long sy = ((long long)y << k) + off, sx0 = ((long long)x0 << k) + off;
    const bool inside = y >= 0 && y <= box.w && y < H && x0 <= box.z && x0 < W;   // some pixel of the thread lies in the box
    unsigned par = 0, on = 0;                                        // bit j: pixel x0 + j
    for (int s0 = 0; s0 < ne; s0 += STAGE) {
        __syncthreads();
        if (s0 + (int)threadIdx.x < ne) E[threadIdx.x] = edges[e0 + s0 + threadIdx.x];
        __syncthreads();
        const int n = inside ? min(STAGE, ne - s0) : 0;
        for (int i = 0; i < n; ++i) {
            const int4 e = E[i];                                     // (ax, ay, bx, by)
            const int ylo = min(e.y, e.w), yhi = max(e.y, e.w);
            if (sy < ylo || sy > yhi) continue;
            const long long dx = (long long)e.z - e.x, dy = (long long)e.w - e.y;
            long long cr = dx * (sy - e.y) - dy * (sx0 - e.x);
            const long long dcr = dy * step;
            const int xlo = min(e.x, e.z), xhi = max(e.x, e.z);
            const bool spans = sy < yhi;                             // ylo <= sy < yhi: not horizontal, may cross
            const bool up = e.w > e.y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long sx = sx0 + (long long)j * step;
                if (cr == 0 && sx >= xlo && sx <= xhi) on |= 1u << j;
                if (spans && (up ? cr > 0 : cr < 0)) par ^= 1u << j;
                cr -= dcr;
            }
        }
    }
    const unsigned cov = par | on;
    if (cov == 0 || y < box.y) return;
    unsigned* row = order + ((int64_t)b * H + y) * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (((cov >> j) & 1u) && x >= 0 && x >= box.x && x <= box.z && x < W) atomicMax(row + x, (unsigned)f + 1u);
    }
}

__global__ void __launch_bounds__(256) rs_resolve_kernel(const unsigned* __restrict__ order, const int32_t* __restrict__ features,
                                                         int n_features, long long total, uint8_t* __restrict__ out) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    auto value = [&](unsigned o) -> unsigned {
        return (o == 0 || o > (unsigned)n_features) ? 0u : (unsigned)features[(int64_t)(o - 1) * FEAT_COLS + 1] & 0xffu;
    };
    if (i0 + 3 < total) {
        const uint4 o = *reinterpret_cast<const uint4*>(order + i0);
        *reinterpret_cast<unsigned*>(out + i0) = value(o.x) | (value(o.y) << 8) | (value(o.z) << 16) | (value(o.w) << 24);
    } else {
        for (long long i = i0; i < total; ++i) out[i] = (uint8_t)value(order[i]);
    }
}

bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535;
}

}  // namespace

extern "C" size_t xv2_rasterize_workspace(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return 0;
    return 4 * (size_t)B * H * W;
}

// the host copy of the tables: every index the kernels follow and every bound the int64 argument rests on
static int rs_validate(const int32_t* t, int64_t n_edges, int n_features, int64_t n_work, int B, int H, int W) {
    const int32_t* edges = t;
    const int32_t* feats = t + 4 * n_edges;
    const int32_t* work = feats + (int64_t)FEAT_COLS * n_features;
    for (int64_t i = 0; i < 4 * n_edges; ++i)
        XV2_CHECK_ARG(edges[i] >= -COORD_MAX && edges[i] <= COORD_MAX, "rasterize_polygons: edge %lld holds coordinate %d outside "
                      "+-2^24", (long long)(i / 4), edges[i]);
    int last_tile = 0;
    for (int f = 0; f < n_features; ++f) {
        const int32_t* r = feats + (int64_t)FEAT_COLS * f;
        XV2_CHECK_ARG(r[0] >= 0 && r[0] < B, "rasterize_polygons: feature %d names tile %d of %d", f, r[0], B);
        XV2_CHECK_ARG(r[0] >= last_tile, "rasterize_polygons: feature %d (tile %d) follows tile %d: features must be sorted by tile",
                      f, r[0], last_tile);
        last_tile = r[0];
        XV2_CHECK_ARG(r[1] >= 0 && r[1] <= 255, "rasterize_polygons: feature %d has value %d outside 0..255", f, r[1]);
        XV2_CHECK_ARG(r[2] >= 0 && r[3] >= 0 && (int64_t)r[2] + r[3] <= n_edges, "rasterize_polygons: feature %d has edges %d + %d "
                      "of %lld", f, r[2], r[3], (long long)n_edges);
        XV2_CHECK_ARG(r[4] >= 0 && r[4] <= r[6] && r[6] < W && r[5] >= 0 && r[5] <= r[7] && r[7] < H, "rasterize_polygons: feature "
                      "%d has box x %d..%d y %d..%d outside the %d x %d tile", f, r[4], r[6], r[5], r[7], H, W);
    }
    for (int64_t i = 0; i < n_work; ++i) {
        const int32_t* w = work + WORK_COLS * i;
        XV2_CHECK_ARG(w[0] >= 0 && w[0] < n_features, "rasterize_polygons: work item %lld names feature %d of %d", (long long)i,
                      w[0], n_features);
        const int32_t* r = feats + (int64_t)FEAT_COLS * w[0];
        XV2_CHECK_ARG(w[1] >= r[4] && w[1] <= r[6] && w[2] >= r[5] && w[2] <= r[7], "rasterize_polygons: work item %lld has its "
                      "window at (%d, %d) outside the box of feature %d", (long long)i, w[1], w[2], w[0]);
        XV2_CHECK_ARG(w[3] == 0, "rasterize_polygons: work item %lld has %d in its last column", (long long)i, w[3]);
    }
    return XV2_OK;
}

static int rs_kid(int which) {
    static const int ids[] = {xv2::prof_register("rs_cover_kernel"), xv2::prof_register("rs_resolve_kernel")};
    return ids[which];
}

extern "C" int xv2_rasterize_polygons(const int32_t* dev_tables, const int32_t* host_tables, int64_t n_edges, int n_features,
                                      int64_t n_work, int frac_bits, int off, int B, int H, int W, void* workspace,
                                      uint8_t* out, void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "rasterize_polygons: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "rasterize_polygons: H*W=%lld exceeds 2^30 pixels per tile", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535, "rasterize_polygons: B=%d too large for one launch", B);
    XV2_CHECK_ARG(frac_bits >= 0 && frac_bits <= 8, "rasterize_polygons: frac_bits=%d outside 0..8", frac_bits);
    XV2_CHECK_ARG(off == 0 || (frac_bits >= 1 && off == (1 << (frac_bits - 1))), "rasterize_polygons: off=%d is neither 0 (lattice "
                  "points) nor 2^(frac_bits-1) (pixel centres, frac_bits >= 1)", off);
    XV2_CHECK_ARG(((int64_t)(H > W ? H : W) << frac_bits) <= COORD_MAX, "rasterize_polygons: max(H, W) << frac_bits exceeds 2^24");
    XV2_CHECK_ARG(n_edges >= 0 && n_edges < (1ll << 31) && n_features >= 0 && n_work >= 0 && n_work < (1ll << 31),
                  "rasterize_polygons: n_edges=%lld n_features=%d n_work=%lld outside 0 .. 2^31 - 1", (long long)n_edges,
                  n_features, (long long)n_work);
    XV2_CHECK_ARG(workspace && out, "rasterize_polygons: null workspace or out");
    XV2_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 3) == 0, "rasterize_polygons: workspace must be 16-byte "
                  "and out 4-byte aligned");
    const bool empty = n_features == 0 || n_work == 0;
    if (n_edges > 0 || n_features > 0 || n_work > 0) {
        XV2_CHECK_ARG(host_tables && (empty || dev_tables), "rasterize_polygons: null tables");
        XV2_CHECK_ARG(((uintptr_t)dev_tables & 15) == 0, "rasterize_polygons: the device tables must be 16-byte aligned");
        if (int rc = rs_validate(host_tables, n_edges, n_features, n_work, B, H, W)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * H * W;
    XV2_CHECK_ARG((total + 1023) / 1024 < (1ll << 31), "rasterize_polygons: B*H*W=%lld too large for one launch", total);
    if (empty) {
        XV2_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)total, st));
        return XV2_OK;
    }
    unsigned* order = static_cast<unsigned*>(workspace);
    XV2_CHECK_HIP(hipMemsetAsync(order, 0, 4 * (size_t)total, st));
    const int32_t* feats = dev_tables + 4 * n_edges;
    const int32_t* work = feats + (int64_t)FEAT_COLS * n_features;
    XV2_LAUNCH(rs_kid(0), 16.0 * n_work + 4096.0 * n_work, rs_cover_kernel, dim3((unsigned)n_work), dim3(256), 0, st,
               reinterpret_cast<const int4*>(dev_tables), (long long)n_edges, feats, n_features,
               reinterpret_cast<const int4*>(work), frac_bits, off, B, H, W, order);
    XV2_LAUNCH(rs_kid(1), 5.0 * total, rs_resolve_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, st, order, feats,
               n_features, total, out);
    return XV2_OK;
}
