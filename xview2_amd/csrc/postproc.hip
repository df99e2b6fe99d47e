// Offline post-processing and xView2 scoring (reference utils/post_process.py:27-47, utils/xview2_metrics.py):
// prediction fusion, 4-connected component labelling with a per-component majority vote, square dilation, and the
// per-tile TP / FN / FP rows of the scorer.
//
// Layout: a batch of B tiles of H x W, one 64 x 64 pixel region per 256-thread block, grid (regions_x, regions_y, B).
// A thread owns one column of its region (lx = tid & 63) and 16 rows (ly = tid >> 6, +4, ...), so every wave reads 64
// consecutive pixels of a row.
//
// Labels: a foreground pixel's label is 1 + the smallest in-tile linear index (y * W + x) of its component, 0 is
// background.  Unions always link the larger root below the smaller one, so a root IS the smallest index of its set
// and the labelling does not depend on the order in which atomics land.  While the merge runs a label is a parent
// pointer (1 + parent index); parents only ever decrease, so a stale read still names an ancestor.
//
// Launch sequence of xv2_postprocess with components (launch boundaries are the only cross-block synchronisation):
//   pp_fuse_kernel      pre / post from loc and dmg, union-find inside the region in LDS, provisional labels,
//                       histogram slots zeroed
//   pp_merge_kernel     unions across region borders in global memory (agent-scope atomicMin)
//   pp_compress_kernel  every label -> its root; per-block (root, class) tallies in LDS, one global add per tally
//   pp_vote_kernel      majority class per root, max over the clamped rate x rate window, uint8 outputs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "xv2_common.h"
#include "fuse_px.h"

namespace {

constexpr int RG = 64;             // region edge (pixels)
constexpr int RPT = RG * RG / 256; // rows per thread
constexpr int MAX_HALO = 32;       // dilation rate <= 65
constexpr int HT = 4096;           // LDS tally slots of pp_compress_kernel (>= pixels of a region)
constexpr unsigned EMPTY = 0xffffffffu;

using xv2::K_4CH;
using xv2::K_5CH;
using xv2::K_LABEL;
using xv2::K_MASK;

__device__ __forceinline__ int ld_label(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- union-find in LDS (one region) --------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* par, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void lds_union(int* par, int a, int b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;   // par[a] already pointed lower: join old and b instead
    }
}

// ---- union-find in global memory (one tile: labels are 1 + parent index) ---------------------------------------
__device__ __forceinline__ int g_find(const int32_t* lab, int x) {
    for (;;) {
        const int p = ld_label(&lab[x]) - 1;
        if (p == x) return x;
        x = p;
    }
}

__device__ __forceinline__ void g_union(int32_t* lab, int a, int b) {
    for (;;) {
        a = g_find(lab, a);
        b = g_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        // termination rests on the stored values strictly decreasing, never on seeing another block's plain stores
        const int old = __hip_atomic_fetch_min(&lab[a], b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (old == a) return;
        a = old;
    }
}

// Fuse + local labelling.  KIND: K_4CH / K_5CH (fp32 [B,C,H,W]), K_LABEL (int32 [B,H,W] label map), K_MASK
// (uint8 [B,H,W], connected components only: fg = mask != 0, no pre / post).  comp != 0: labels + zeroed counts.
// A label-map value that survives the fusion (pre set) but cannot be represented - outside 0..255 for a uint8 PNG, or
// outside 0..4 when voting (4 histogram slots per root) - becomes background and is counted in *status.
// t_loc, t_dmg and cs are the fusion's two thresholds and class scales (fuse_px.h; unused by K_MASK).
template <int KIND>
__global__ void __launch_bounds__(256) pp_fuse_kernel(const float* __restrict__ loc, const void* __restrict__ dmg, int H,
                                                      int W, int comp, int32_t* __restrict__ labels,
                                                      uint4* __restrict__ counts, uint8_t* __restrict__ pre_o,
                                                      uint8_t* __restrict__ post_o, int* __restrict__ status,
                                                      float t_loc, float t_dmg, xv2::ClassScale cs) {
    __shared__ int par[RG * RG];
    const int tid = threadIdx.x, lx = tid & (RG - 1), ly0 = tid >> 6;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t hw = (int64_t)H * W, base = (int64_t)b * hw;
    const int x = x0 + lx;
    uint8_t pv[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly;
        int post = 0, bad = 0;
        if (x < W && y < H) {
            const int64_t p = base + (int64_t)y * W + x;
            if (KIND == K_MASK) {
                post = reinterpret_cast<const uint8_t*>(dmg)[p] != 0;
            } else {
                const int raw = xv2::decode_raw<KIND == K_MASK ? K_LABEL : KIND>(dmg, b, hw, p - base, cs);
                const int pre = xv2::fuse_pre(loc[p], raw, t_loc, t_dmg);
                post = pre ? raw : 0;
                if (KIND == K_LABEL && (post < 0 || post > (comp ? 4 : 255))) {
                    bad = 1;
                    post = 0;
                }
                pre_o[p] = (uint8_t)pre;
                post_o[p] = (uint8_t)post;
            }
        }
        if (KIND == K_LABEL) {   // one atomic per wave that met an unrepresentable value
            const unsigned long long m = __ballot(bad);
            if (m && (tid & 63) == 0) atomicAdd(status, (int)__popcll(m));
        }
        pv[k] = (uint8_t)post;
        if (comp) par[ly * RG + lx] = post > 0 ? ly * RG + lx : -1;
    }
    if (!comp) return;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int i = (ly0 + 4 * k) * RG + lx;
        if (!pv[k]) continue;
        if (lx > 0 && par[i - 1] >= 0) lds_union(par, i, i - 1);
        if (i >= RG && par[i - RG] >= 0) lds_union(par, i, i - RG);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int64_t p = base + (int64_t)y * W + x;
        int lab = 0;
        if (pv[k]) {
            const int r = lds_find(par, ly * RG + lx);
            lab = 1 + (y0 + r / RG) * W + x0 + (r & (RG - 1));
        }
        labels[p] = lab;
        if (KIND != K_MASK) counts[p] = make_uint4(0, 0, 0, 0);
    }
}

// Border merge: a pixel on its region's top or left edge joins its foreground neighbour across the edge.
__global__ void __launch_bounds__(128) pp_merge_kernel(int32_t* __restrict__ labels, int H, int W) {
    const int t = threadIdx.x, b = blockIdx.z;
    int x = blockIdx.x * RG, y = blockIdx.y * RG, nx, ny;
    if (t < RG) {          // top edge: neighbour above
        x += t;
        nx = x;
        ny = y - 1;
    } else {               // left edge: neighbour to the left
        y += t - RG;
        nx = x - 1;
        ny = y;
    }
    if (x >= W || y >= H || nx < 0 || ny < 0) return;
    int32_t* lab = labels + (int64_t)b * H * W;
    const int p = y * W + x, q = ny * W + nx;
    if (ld_label(&lab[p]) == 0 || ld_label(&lab[q]) == 0) return;
    g_union(lab, p, q);
}

// Compress + count: every label becomes 1 + its root; COUNT adds 1 to counts[root][post - 1], tallied per block in
// an LDS table first (a building spans many regions but few roots per region: one global add per (root, class)).
template <bool COUNT>
__global__ void __launch_bounds__(256) pp_compress_kernel(int32_t* __restrict__ labels, const uint8_t* __restrict__ post,
                                                          int H, int W, unsigned* __restrict__ counts) {
    __shared__ unsigned keys[COUNT ? HT : 1], tally[COUNT ? HT : 1];
    const int tid = threadIdx.x, lx = tid & (RG - 1), ly0 = tid >> 6;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    int32_t* lab = labels + base;
    if (COUNT) {
        for (int i = tid; i < HT; i += 256) {
            keys[i] = EMPTY;
            tally[i] = 0;
        }
        __syncthreads();
    }
    const int x = x0 + lx;
#pragma unroll 4
    for (int k = 0; k < RPT; ++k) {
        const int y = y0 + ly0 + 4 * k;
        if (x >= W || y >= H) continue;
        const int p = y * W + x;
        const int l = ld_label(&lab[p]);
        if (l == 0) continue;
        const int r = g_find(lab, l - 1);
        if (r + 1 != l) __hip_atomic_store(&lab[p], r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (COUNT) {
            const unsigned key = (unsigned)r * 4u + (unsigned)(post[base + p] - 1);
            unsigned h = (key * 2654435761u) >> 20;   // 12-bit slot
            for (;;) {
                const unsigned old = atomicCAS(&keys[h], EMPTY, key);
                if (old == EMPTY || old == key) {
                    atomicAdd(&tally[h], 1u);
                    break;
                }
                h = (h + 1) & (HT - 1);
            }
        }
    }
    if (!COUNT) return;
    __syncthreads();
    unsigned* cnt = counts + base * 4;
    for (int i = tid; i < HT; i += 256)
        if (keys[i] != EMPTY) atomicAdd(&cnt[keys[i]], tally[i]);
}

// Vote + dilate: over the region plus a halo of h = rate / 2, a foreground pixel's post becomes its root's most
// frequent class (ties: the smaller class); then the max over the (2h+1)^2 window clamped to the image (separable:
// rows into LDS, then columns), uint8 out for pre and post.
template <bool VOTE>
__global__ void __launch_bounds__(256) pp_vote_kernel(const uint8_t* __restrict__ pre_i, const uint8_t* __restrict__ post_i,
                                                      const int32_t* __restrict__ labels, const uint4* __restrict__ counts,
                                                      int H, int W, int h, uint8_t* __restrict__ pre_o,
                                                      uint8_t* __restrict__ post_o) {
    constexpr int EMAX = RG + 2 * MAX_HALO;
    __shared__ uint8_t epre[EMAX * EMAX], epost[EMAX * EMAX];
    __shared__ uint8_t rpre[EMAX * RG], rpost[EMAX * RG];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    const int E = RG + 2 * h;
    for (int i = tid; i < E * E; i += 256) {
        const int ey = i / E, ex = i - ey * E, y = y0 - h + ey, x = x0 - h + ex;
        uint8_t pr = 0, po = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const int64_t p = base + (int64_t)y * W + x;
            pr = pre_i[p];
            po = post_i[p];
            if (VOTE && po) {
                const uint4 c = counts[base + labels[p] - 1];
                unsigned m = c.x;
                po = 1;
                if (c.y > m) { m = c.y; po = 2; }
                if (c.z > m) { m = c.z; po = 3; }
                if (c.w > m) po = 4;
            }
        }
        epre[i] = pr;
        epost[i] = po;
    }
    __syncthreads();
    for (int i = tid; i < E * RG; i += 256) {
        const int ey = i / RG, ox = i - ey * RG;
        uint8_t a = 0, c = 0;
        for (int d = 0; d <= 2 * h; ++d) {
            a = max(a, epre[ey * E + ox + d]);
            c = max(c, epost[ey * E + ox + d]);
        }
        rpre[i] = a;
        rpost[i] = c;
    }
    __syncthreads();
    for (int i = tid; i < RG * RG; i += 256) {
        const int oy = i / RG, ox = i - oy * RG, y = y0 + oy, x = x0 + ox;
        if (x >= W || y >= H) continue;
        uint8_t a = 0, c = 0;
        for (int d = 0; d <= 2 * h; ++d) {
            a = max(a, rpre[(oy + d) * RG + ox]);
            c = max(c, rpost[(oy + d) * RG + ox]);
        }
        const int64_t p = base + (int64_t)y * W + x;
        pre_o[p] = a;
        post_o[p] = c;
    }
}

// Scorer rows (utils/xview2_metrics.py RowPairCalculator.get_row_pair) of one tile per blockIdx.y:
// [lTP, lFN, lFP] of the building masks, [TP, FN, FP] x damage classes 1..4 where the damage target is a building
// (damage prediction masked by the localization prediction), slot 15: pixels > 4 in any input.
__device__ __forceinline__ void score_px(unsigned lp, unsigned dp, unsigned lt, unsigned dt, unsigned* c) {
    const unsigned lb = lp > 0, tb = lt > 0;
    c[0] += lb & tb;
    c[1] += (lb ^ 1u) & tb;
    c[2] += lb & (tb ^ 1u);
    c[15] += (lp > 4) | (dp > 4) | (lt > 4) | (dt > 4);
    if (dt > 0) {
        const unsigned d = lb ? dp : 0u;
#pragma unroll
        for (int k = 1; k <= 4; ++k) {
            c[3 * k + 0] += (d == (unsigned)k) & (dt == (unsigned)k);
            c[3 * k + 1] += (d != (unsigned)k) & (dt == (unsigned)k);
            c[3 * k + 2] += (d == (unsigned)k) & (dt != (unsigned)k);
        }
    }
}

__global__ void __launch_bounds__(256) xview2_counts_kernel(const uint8_t* __restrict__ lp, const uint8_t* __restrict__ dp,
                                                            const uint8_t* __restrict__ lt, const uint8_t* __restrict__ dt,
                                                            int64_t hw, unsigned long long* __restrict__ counts) {
    __shared__ unsigned sh[16];
    if (threadIdx.x < 16) sh[threadIdx.x] = 0;
    __syncthreads();
    unsigned c[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = 0;
    const int64_t base = (int64_t)blockIdx.y * hw;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t start = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if ((hw & 3) == 0) {   // four pixels per 32-bit load (torch allocations are 4-byte aligned)
        const uint32_t* a = reinterpret_cast<const uint32_t*>(lp + base);
        const uint32_t* bb = reinterpret_cast<const uint32_t*>(dp + base);
        const uint32_t* e = reinterpret_cast<const uint32_t*>(lt + base);
        const uint32_t* f = reinterpret_cast<const uint32_t*>(dt + base);
        for (int64_t i = start; i < hw / 4; i += stride) {
            const uint32_t va = a[i], vb = bb[i], ve = e[i], vf = f[i];
#pragma unroll
            for (int s = 0; s < 32; s += 8)
                score_px((va >> s) & 255u, (vb >> s) & 255u, (ve >> s) & 255u, (vf >> s) & 255u, c);
        }
    } else {
        for (int64_t i = start; i < hw; i += stride)
            score_px(lp[base + i], dp[base + i], lt[base + i], dt[base + i], c);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        unsigned v = c[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 16 && sh[threadIdx.x])
        atomicAdd(&counts[blockIdx.y * 16 + threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

static int pp_kid(int k) {
    static const int ids[] = {xv2::prof_register("pp_fuse_kernel"), xv2::prof_register("pp_merge_kernel"),
                              xv2::prof_register("pp_compress_kernel"), xv2::prof_register("pp_vote_kernel"),
                              xv2::prof_register("xview2_counts_kernel")};
    return ids[k];
}

extern "C" size_t xv2_postprocess_workspace(int B, int H, int W, int components) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)B * H * W;
    // counts (4 x uint32) | labels (int32) | pre, post (uint8): 22 bytes per pixel with components, 2 without
    return components ? align256(16 * n) + align256(4 * n) + 2 * align256(n) : 2 * align256(n);
}

static int check_sizes(const char* what, int B, int H, int W) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B=%d H=%d W=%d must be positive", what, B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "%s: H*W=%lld exceeds 2^30 pixels per tile", what, (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + RG - 1) / RG <= 65535, "%s: B=%d or H=%d too large for one launch", what, B, H);
    return XV2_OK;
}

extern "C" int xv2_postprocess_ex(const float* loc, const void* dmg, int dmg_kind, int B, int H, int W, int components,
                                  int rate, void* workspace, uint8_t* pre, uint8_t* post, int32_t* status, float t_loc,
                                  float t_dmg, const float* class_scale, void* stream) {
    if (int rc = check_sizes("postprocess", B, H, W)) return rc;
    XV2_CHECK_ARG(std::isfinite(t_loc) && std::isfinite(t_dmg), "postprocess: thresholds %g and %g must be finite",
                  (double)t_loc, (double)t_dmg);
    XV2_CHECK_ARG(t_dmg <= t_loc, "postprocess: the damage-gated threshold %g must not exceed the localization threshold %g",
                  (double)t_dmg, (double)t_loc);
    XV2_CHECK_ARG(!class_scale || dmg_kind != XV2_DMG_LABEL,
                  "postprocess: class scales need damage probabilities, a label map has none to scale");
    xv2::ClassScale cs = {{1.f, 1.f, 1.f, 1.f}, class_scale ? 1 : 0};
    for (int c = 0; class_scale && c < 4; ++c) {
        XV2_CHECK_ARG(std::isfinite(class_scale[c]) && class_scale[c] > 0.f,
                      "postprocess: class scale %d is %g, must be finite and > 0", c + 1, (double)class_scale[c]);
        cs.s[c] = class_scale[c];
    }
    XV2_CHECK_ARG(dmg_kind == XV2_DMG_4CH || dmg_kind == XV2_DMG_5CH || dmg_kind == XV2_DMG_LABEL,
                  "postprocess: dmg_kind=%d unsupported (4- or 5-channel probabilities, or an int32 label map)", dmg_kind);
    XV2_CHECK_ARG(rate == 0 || (rate >= 1 && rate % 2 == 1 && rate <= 2 * MAX_HALO + 1),
                  "postprocess: dilation rate %d must be 0 (off) or odd in 1..%d", rate, 2 * MAX_HALO + 1);
    XV2_CHECK_ARG(loc && dmg && pre && post, "postprocess: null tensor");
    XV2_CHECK_ARG(status || dmg_kind != XV2_DMG_LABEL, "postprocess: a label map needs the status counter");
    XV2_CHECK_ARG(workspace || (!components && rate == 0), "postprocess: workspace required");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W;
    char* ws = static_cast<char*>(workspace);
    uint4* counts = nullptr;
    int32_t* labels = nullptr;
    uint8_t *ipre = pre, *ipost = post;
    if (components) {
        counts = reinterpret_cast<uint4*>(ws);
        labels = reinterpret_cast<int32_t*>(ws + align256(16 * n));
        ws += align256(16 * n) + align256(4 * n);
    }
    if (components || rate) {
        ipre = reinterpret_cast<uint8_t*>(ws);
        ipost = ipre + align256(n);
    }
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    const int comp = components ? 1 : 0;
    const double px = (double)n, cin = dmg_kind == XV2_DMG_4CH ? 16 : dmg_kind == XV2_DMG_5CH ? 20 : 4;
    const double fuse_bytes = px * (4 + cin + 2 + (components ? 20 : 0));
    if (dmg_kind == XV2_DMG_4CH)
        XV2_LAUNCH(pp_kid(0), fuse_bytes, pp_fuse_kernel<K_4CH>, grid, dim3(256), 0, st, loc, dmg, H, W, comp, labels, counts,
                   ipre, ipost, status, t_loc, t_dmg, cs);
    else if (dmg_kind == XV2_DMG_5CH)
        XV2_LAUNCH(pp_kid(0), fuse_bytes, pp_fuse_kernel<K_5CH>, grid, dim3(256), 0, st, loc, dmg, H, W, comp, labels, counts,
                   ipre, ipost, status, t_loc, t_dmg, cs);
    else
        XV2_LAUNCH(pp_kid(0), fuse_bytes, pp_fuse_kernel<K_LABEL>, grid, dim3(256), 0, st, loc, dmg, H, W, comp, labels,
                   counts, ipre, ipost, status, t_loc, t_dmg, cs);
    if (components) {
        XV2_LAUNCH(pp_kid(1), 8.0 * 128 * grid.x * grid.y * B, pp_merge_kernel, grid, dim3(128), 0, st, labels, H, W);
        XV2_LAUNCH(pp_kid(2), px * 9, pp_compress_kernel<true>, grid, dim3(256), 0, st, labels, ipost, H, W,
                   reinterpret_cast<unsigned*>(counts));
        XV2_LAUNCH(pp_kid(3), px * 8, pp_vote_kernel<true>, grid, dim3(256), 0, st, ipre, ipost, labels, counts, H, W,
                   rate ? rate / 2 : 0, pre, post);
    } else if (rate) {
        XV2_LAUNCH(pp_kid(3), px * 4, pp_vote_kernel<false>, grid, dim3(256), 0, st, ipre, ipost, labels, counts, H, W,
                   rate / 2, pre, post);
    }
    return XV2_OK;
}

extern "C" int xv2_postprocess(const float* loc, const void* dmg, int dmg_kind, int B, int H, int W, int components,
                               int rate, void* workspace, uint8_t* pre, uint8_t* post, int32_t* status, void* stream) {
    return xv2_postprocess_ex(loc, dmg, dmg_kind, B, H, W, components, rate, workspace, pre, post, status, 0.3f, 0.1f, nullptr,
                              stream);
}

extern "C" int xv2_label_components(const uint8_t* mask, int B, int H, int W, void* workspace, int32_t* labels,
                                    void* stream) {
    (void)workspace;
    if (int rc = check_sizes("label_components", B, H, W)) return rc;
    XV2_CHECK_ARG(mask && labels, "label_components: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    const double px = (double)B * H * W;
    XV2_LAUNCH(pp_kid(0), px * 5, pp_fuse_kernel<K_MASK>, grid, dim3(256), 0, st, nullptr, mask, H, W, 1, labels, nullptr,
               nullptr, nullptr, nullptr, 0.f, 0.f, xv2::ClassScale{{1.f, 1.f, 1.f, 1.f}, 0});
    XV2_LAUNCH(pp_kid(1), 8.0 * 128 * grid.x * grid.y * B, pp_merge_kernel, grid, dim3(128), 0, st, labels, H, W);
    XV2_LAUNCH(pp_kid(2), px * 8, pp_compress_kernel<false>, grid, dim3(256), 0, st, labels, nullptr, H, W, nullptr);
    return XV2_OK;
}

extern "C" int xv2_xview2_counts(const uint8_t* lp, const uint8_t* dp, const uint8_t* lt, const uint8_t* dt, int B,
                                 int64_t hw, int64_t* counts, void* stream) {
    XV2_CHECK_ARG(B > 0 && B <= 65535 && hw > 0, "xview2_counts: B=%d hw=%lld must be positive", B, (long long)hw);
    XV2_CHECK_ARG(lp && dp && lt && dt && counts, "xview2_counts: null tensor");
    const int gx = (int)std::max<int64_t>(1, std::min<int64_t>(xv2::cdiv(hw, 256 * 16), 256));
    hipStream_t st = (hipStream_t)stream;
    XV2_LAUNCH(pp_kid(4), 4.0 * B * hw, xview2_counts_kernel, dim3(gx, B), dim3(256), 0, st, lp, dp, lt, dt, hw,
               reinterpret_cast<unsigned long long*>(counts));
    return XV2_OK;
}
