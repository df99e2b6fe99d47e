// Splitting touching buildings (include/xv2.h, "split touching buildings"): a capped exact squared distance transform,
// seeds where the mask survives an erosion by a disc, geodesic growth of the seed labels inside the mask, and a 1-pixel
// cut where two grown pieces meet.  Everything is integer work with a unique result.
//
// Layout as postproc.hip: B tiles of H x W, one 64 x 64 pixel region per 256-thread block, grid (regions_x, regions_y, B).
//
// Distance (sp_edt_kernel, one launch): the region plus a halo of cap - 1 pixels is staged in LDS as bytes (1 = mask or
// outside the tile, 0 = background).  Column pass: g = the row distance to the nearest zero of the pixel's column within
// cap - 1 rows, cap if there is none, for the region's rows over the widened columns.  Row pass:
// d2 = min(cap^2, min over |dx| < cap of dx^2 + g(x + dx)^2).  Both are windowed minima of at most 2 cap - 1 candidates
// per pixel; a wave reads consecutive bytes of one LDS row in either pass (four lanes share a bank word: a broadcast).
//
// Growth state: one uint64 key per pixel, (g << 32) | label with g the geodesic distance to the seed; KEY_BG for
// background, KEY_INF for mask pixels no seed has reached.  Keys only ever decrease, and the fixed point of
// key(p) = min(key(p), key(q) + (1, 0)) over the 4-neighbours q is unique, so the order of relaxations is free.
// A sweep (sp_grow_kernel) reads buffer A and writes buffer B: a block loads its region plus a 1-pixel ring, relaxes in
// LDS until the region is stable against that ring, and writes its interior.  No block reads what another writes, so the
// state after s sweeps is a function of the input alone.  A per-region flag (two arrays, swapped like the keys) says
// whether the region changed in the previous sweep.  A block that neither changed then nor changes now finds both buffers
// equal on its region already and writes nothing: an idle region costs one read.  A block whose region and four
// neighbouring regions all rested in the previous sweep sees the input of that sweep again and does not even load.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

constexpr int RG = 64;              // region edge (pixels)
constexpr int RPT = RG * RG / 256;  // pixels per thread
constexpr int MAX_CAP = 64;
constexpr int GE = RG + 2;          // region plus ring (sp_grow_kernel)
typedef unsigned long long u64;
constexpr u64 KEY_BG = ~0ull;       // not part of the mask
constexpr u64 KEY_INF = ~0ull - 1;  // mask, no seed reached it yet
constexpr u64 STEP = 1ull << 32;    // one pixel further from the seed

// OUT_SEED: seed[p] = mask[p] != 0 && d2 > r2 (uint8), else d2 (uint16)
template <bool OUT_SEED>
__global__ void __launch_bounds__(256) sp_edt_kernel(const uint8_t* __restrict__ mask, int H, int W, int cap, int r2,
                                                     uint16_t* __restrict__ d2, uint8_t* __restrict__ seed) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sp_lds[];
    const int h = cap - 1, E = RG + 2 * h;
    uint8_t* em = sp_lds;          // [E][E]
    uint8_t* g = sp_lds + E * E;   // [RG][E]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    for (int i = tid; i < E * E; i += 256) {
        const int ey = i / E, ex = i - ey * E, y = y0 - h + ey, x = x0 - h + ex;
        uint8_t v = 1;   // pixels outside the tile are not background
        if (x >= 0 && x < W && y >= 0 && y < H) v = mask[base + (int64_t)y * W + x] != 0;
        em[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < RG * E; i += 256) {
        const int oy = i / E, ex = i - oy * E;
        const uint8_t* c = em + (oy + h) * E + ex;
        int gv = 0;
        if (*c) {
            gv = cap;
            for (int d = 1; d <= h; ++d)
                if (!c[-d * E] || !c[d * E]) {
                    gv = d;
                    break;
                }
        }
        g[i] = (uint8_t)gv;
    }
    __syncthreads();
    const int lx = tid & (RG - 1), x = x0 + lx;
#pragma unroll 1
    for (int k = 0; k < RPT; ++k) {
        const int ly = (tid >> 6) + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const uint8_t* row = g + ly * E + lx + h;
        int best = cap * cap;
        for (int dx = -h; dx <= h; ++dx) {
            const int gv = row[dx];
            best = min(best, dx * dx + gv * gv);
        }
        const int64_t p = base + (int64_t)y * W + x;
        if (OUT_SEED)
            seed[p] = (uint8_t)(best > r2 && row[0] != 0);
        else
            d2[p] = (uint16_t)best;
    }
}

// growth state from the seed labels: seeds (0, label), other mask pixels KEY_INF, background KEY_BG; every region's
// flag raised (in the array the first sweep reads) so that the first sweep writes all of buffer B
__global__ void __launch_bounds__(256) sp_init_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                      int64_t hw, u64* __restrict__ keys, int32_t* __restrict__ flags,
                                                      int64_t regions) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i < regions) flags[b * regions + i] = 1;   // (a tile has fewer regions than pixels)
    if (i >= hw) return;
    const int64_t p = b * hw + i;
    u64 k = KEY_BG;
    if (mask[p]) {
        const int32_t l = labels[p];
        k = l > 0 ? (u64)(uint32_t)l : KEY_INF;
    }
    keys[p] = k;
}

__device__ __forceinline__ u64 lds_ld(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One relaxation of the pixel at LDS index i: the smallest reached neighbour, one step further.  A stale neighbour value
// is an upper bound of its final one, so a racing read only delays.  Only the owner writes a pixel.
__device__ __forceinline__ int relax(u64* t, int i) {
    const u64 own = lds_ld(&t[i]);
    if (own < STEP || own == KEY_BG) return 0;   // a seed, or no mask
    u64 m = lds_ld(&t[i - 1]);
    m = min(m, lds_ld(&t[i + 1]));
    m = min(m, lds_ld(&t[i - GE]));
    m = min(m, lds_ld(&t[i + GE]));
    if (m >= KEY_INF) return 0;
    m += STEP;
    if (m >= own) return 0;
    __hip_atomic_store(&t[i], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return 1;
}

__global__ void __launch_bounds__(256) sp_grow_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int H, int W,
                                                      const int32_t* __restrict__ flags_prev,
                                                      int32_t* __restrict__ flags_now, int32_t* __restrict__ pending) {
    __shared__ u64 t[GE * GE];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    const int gx = gridDim.x, gy = gridDim.y;
    const int64_t fi = ((int64_t)b * gy + blockIdx.y) * gx + blockIdx.x;
    // the previous sweep left this region stable against the ring it saw; if neither the region nor a neighbour that
    // supplies the ring changed in that sweep, the input is the same again: nothing to load
    const int before = flags_prev[fi];
    int moved = before;
    if (blockIdx.x > 0) moved |= flags_prev[fi - 1];
    if ((int)blockIdx.x + 1 < gx) moved |= flags_prev[fi + 1];
    if (blockIdx.y > 0) moved |= flags_prev[fi - gx];
    if ((int)blockIdx.y + 1 < gy) moved |= flags_prev[fi + gx];
    if (!moved) {
        if (tid == 0) flags_now[fi] = 0;
        return;
    }
    for (int i = tid; i < GE * GE; i += 256) {
        const int ey = i / GE, ex = i - ey * GE, y = y0 - 1 + ey, x = x0 - 1 + ex;
        u64 k = KEY_BG;
        if (x >= 0 && x < W && y >= 0 && y < H) k = src[base + (int64_t)y * W + x];
        t[i] = k;
    }
    __syncthreads();
    // a thread owns 16 consecutive rows of one column: a pass down and a pass up carry a label along a whole run per
    // round; a wave reads 64 consecutive keys of a row
    const int lx = tid & (RG - 1), r0 = (tid >> 6) * RPT;
    const int col = lx + 1;
    int any = 0;
    // the region is stable after at most one round per pixel of the longest path inside it, plus the round that sees no change
    for (int round = 0; round <= RG * RG; ++round) {
        int ch = 0;
        for (int k = 0; k < RPT; ++k) ch |= relax(t, (r0 + k + 1) * GE + col);
        for (int k = RPT - 2; k >= 0; --k) ch |= relax(t, (r0 + k + 1) * GE + col);
        if (!__syncthreads_or(ch)) break;
        any = 1;
    }
    if (tid == 0) {
        flags_now[fi] = any;
        if (any && pending) atomicOr(pending, 1);
    }
    if (!any && !before) return;   // both buffers already agree on this region
    const int x = x0 + lx;
    if (x >= W) return;
    for (int k = 0; k < RPT; ++k) {
        const int y = y0 + r0 + k;
        if (y >= H) break;
        dst[base + (int64_t)y * W + x] = t[(r0 + k + 1) * GE + col];
    }
}

__device__ __forceinline__ uint32_t label_of(u64 k) { return k < KEY_INF ? (uint32_t)k : 0u; }

// the cut: a labelled pixel with a smaller non-zero label among its 4-neighbours becomes background
__global__ void __launch_bounds__(256) sp_finish_kernel(const uint8_t* __restrict__ mask, const u64* __restrict__ keys,
                                                        int H, int W, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ labels) {
    const int64_t hw = (int64_t)H * W, base = (int64_t)blockIdx.y * hw;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const u64* k = keys + base;
    const uint32_t l = label_of(k[p]);
    bool cut = false;
    if (l) {
        const uint32_t a = x > 0 ? label_of(k[p - 1]) : 0u, c = x + 1 < W ? label_of(k[p + 1]) : 0u;
        const uint32_t d = y > 0 ? label_of(k[p - W]) : 0u, e = y + 1 < H ? label_of(k[p + W]) : 0u;
        cut = (a && a < l) || (c && c < l) || (d && d < l) || (e && e < l);
    }
    out[base + p] = cut ? (uint8_t)0 : mask[base + p];
    if (labels) labels[base + p] = (int32_t)l;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535 && (H + RG - 1) / RG <= 65535;
}

int cap_of(int r2) {   // floor(sqrt(r2)) + 1
    int s = 0;
    while ((s + 1) * (s + 1) <= r2) ++s;
    return s + 1;
}

size_t edt_lds(int cap) {
    const size_t E = RG + 2 * (size_t)(cap - 1);
    return E * E + RG * E;   // 48260 bytes at cap = 64
}

int64_t regions_of(int H, int W) { return (int64_t)((H + RG - 1) / RG) * ((W + RG - 1) / RG); }

struct Layout {
    u64 *a, *b;
    int32_t* flags[2];  // read / written by the first sweep of a call, swapped every sweep
    uint8_t* seed;      // inside a, dead once the seeds are labelled
    int32_t* labels;    // inside b, dead once the keys are initialised
    int64_t regions;    // per tile
};

Layout layout(void* workspace, int B, int H, int W) {
    const size_t n = (size_t)B * H * W;
    char* ws = static_cast<char*>(workspace);
    Layout l;
    l.a = reinterpret_cast<u64*>(ws);
    l.b = reinterpret_cast<u64*>(ws + align256(8 * n));
    l.regions = regions_of(H, W);
    l.flags[0] = reinterpret_cast<int32_t*>(ws + 2 * align256(8 * n));
    l.flags[1] = l.flags[0] + (size_t)B * l.regions;
    l.seed = reinterpret_cast<uint8_t*>(l.a);
    l.labels = reinterpret_cast<int32_t*>(l.b);
    return l;
}

}  // namespace

static int sp_kid(int k) {
    static const int ids[] = {xv2::prof_register("sp_edt_kernel"), xv2::prof_register("sp_init_kernel"),
                              xv2::prof_register("sp_grow_kernel"), xv2::prof_register("sp_finish_kernel")};
    return ids[k];
}

static int sp_check(const char* what, int B, int H, int W) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B=%d H=%d W=%d must be positive", what, B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "%s: H*W=%lld exceeds 2^30 pixels per tile", what, (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + RG - 1) / RG <= 65535, "%s: B=%d or H=%d too large for one launch", what, B, H);
    return XV2_OK;
}

static int sp_check_ws(const char* what, const void* workspace) {
    XV2_CHECK_ARG(workspace, "%s: workspace required", what);
    XV2_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace must be 16-byte aligned", what);
    return XV2_OK;
}

extern "C" int xv2_edt_sq(const uint8_t* mask, int B, int H, int W, int cap, uint16_t* d2, void* stream) {
    if (int rc = sp_check("edt_sq", B, H, W)) return rc;
    XV2_CHECK_ARG(cap >= 1 && cap <= MAX_CAP, "edt_sq: cap=%d must lie in 1..%d", cap, MAX_CAP);
    XV2_CHECK_ARG(mask && d2, "edt_sq: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    XV2_LAUNCH(sp_kid(0), 3.0 * B * H * W, sp_edt_kernel<false>, grid, dim3(256), edt_lds(cap), st, mask, H, W, cap, 0, d2,
               nullptr);
    return XV2_OK;
}

extern "C" size_t xv2_split_workspace(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return 0;
    const size_t n = (size_t)B * H * W;
    // keys A | keys B (uint64 per pixel each) | two int32 flags per region
    return 2 * align256(8 * n) + align256(8 * (size_t)B * (size_t)regions_of(H, W));
}

extern "C" int xv2_split_seed(const uint8_t* mask, int B, int H, int W, int r2, void* workspace, void* stream) {
    if (int rc = sp_check("split_seed", B, H, W)) return rc;
    XV2_CHECK_ARG(r2 >= 1 && r2 <= 4095, "split_seed: r2=%d must lie in 1..4095", r2);
    XV2_CHECK_ARG(mask, "split_seed: null tensor");
    if (int rc = sp_check_ws("split_seed", workspace)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(workspace, B, H, W);
    const int64_t n = (int64_t)B * H * W;
    const int cap = cap_of(r2);
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    XV2_LAUNCH(sp_kid(0), 2.0 * n, sp_edt_kernel<true>, grid, dim3(256), edt_lds(cap), st, mask, H, W, cap, r2, nullptr,
               l.seed);
    if (int rc = xv2_label_components(l.seed, B, H, W, nullptr, l.labels, stream)) return rc;
    const int64_t hw = (int64_t)H * W;
    XV2_LAUNCH(sp_kid(1), 13.0 * n, sp_init_kernel, dim3((unsigned)xv2::cdiv(hw, 256), B), dim3(256), 0, st, mask, l.labels, hw,
               l.a, l.flags[0], l.regions);
    return XV2_OK;
}

extern "C" int xv2_split_grow(const uint8_t* mask, int B, int H, int W, int sweeps, void* workspace, int32_t* pending,
                              void* stream) {
    if (int rc = sp_check("split_grow", B, H, W)) return rc;
    XV2_CHECK_ARG(sweeps >= 1, "split_grow: sweeps=%d must be at least 1", sweeps);
    XV2_CHECK_ARG(mask && pending, "split_grow: null tensor");
    if (int rc = sp_check_ws("split_grow", workspace)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(workspace, B, H, W);
    const size_t n = (size_t)B * H * W;
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    XV2_CHECK_HIP(hipMemsetAsync(pending, 0, sizeof(int32_t), st));
    u64 *src = l.a, *dst = l.b;
    for (int s = 0; s < sweeps; ++s) {
        XV2_LAUNCH(sp_kid(2), 16.0 * n, sp_grow_kernel, grid, dim3(256), 0, st, src, dst, H, W, l.flags[s & 1],
                   l.flags[(s + 1) & 1], s == sweeps - 1 ? pending : nullptr);
        u64* t = src;
        src = dst;
        dst = t;
    }
    // the state lives in A between calls: an odd number of sweeps ends with a copy back (an even one costs nothing)
    if (src != l.a) {
        XV2_CHECK_HIP(hipMemcpyAsync(l.a, l.b, 8 * n, hipMemcpyDeviceToDevice, st));
        XV2_CHECK_HIP(hipMemcpyAsync(l.flags[0], l.flags[1], 4 * (size_t)B * l.regions, hipMemcpyDeviceToDevice, st));
    }
    return XV2_OK;
}

extern "C" int xv2_split_finish(const uint8_t* mask, int B, int H, int W, void* workspace, uint8_t* out, int32_t* labels,
                                void* stream) {
    if (int rc = sp_check("split_finish", B, H, W)) return rc;
    XV2_CHECK_ARG(mask && out, "split_finish: null tensor");
    if (int rc = sp_check_ws("split_finish", workspace)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Layout l = layout(workspace, B, H, W);
    const int64_t hw = (int64_t)H * W;
    XV2_LAUNCH(sp_kid(3), (labels ? 14.0 : 10.0) * B * hw, sp_finish_kernel, dim3((unsigned)xv2::cdiv(hw, 256), B), dim3(256), 0, st,
               mask, l.a, H, W, out, labels);
    return XV2_OK;
}
