// Drop small buildings and fill small holes (include/xv2.h, "clean buildings"; xview2_amd/utils/clean.py).
//
// Layout as postproc.hip: a batch of B tiles of H x W, one 64 x 64 pixel region per 256-thread block, grid
// (regions_x, regions_y, B); a thread owns one column of its region and 16 rows, so a wave reads 64 consecutive pixels.
//
// Stage 1 labels BOTH kinds of pixel in one int32 map: a building pixel joins its building neighbours to W and N
// (4-connectivity), a background pixel its background neighbours to W, N, NW and NE (8-connectivity, the dual).  The two
// kinds never share a set, so one parent array serves both and a root's own pixel tells which kind its set is.
// (A row's runs of one kind start out linked, and a union is made only where runs meet: see the kernels.)  A label is
// 1 + the smallest in-tile linear index of the set: unions always link the larger root below the smaller one, so the
// labelling does not depend on the order in which atomics land (postproc.hip's argument, and its find / union loops).
// The root of a hole is therefore its first pixel in raster order, and the owner's pixel is the one at root - 1.
//
// Per-root words (uint32 x 4 per pixel, zeroed by the first launch): a building root's four class counts; a background
// root's area in word 0 and its number of pixels on the tile's outer frame in word 1.  Blocks tally in LDS first and add
// once per (root, word).  Stage 2 labels the filled map (buildings only) and keeps one area word per root.
//
// Launches of xv2_clean_buildings (launch boundaries are the only cross-block synchronisation; nothing is read back):
//   max_hole > 0:  cl_label<true>, cl_merge<true>, cl_tally<1>, cl_fill       (else two device copies of the inputs)
//   min_area > 1:  cl_label<false>, cl_merge<false>, cl_tally<2>, cl_drop
// Which launches run depends on the two arguments alone, never on the maps.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "xv2_common.h"

namespace {

constexpr int RG = 64;             // region edge (pixels)
constexpr int RPT = RG * RG / 256; // rows per thread
constexpr int HT = 4096;           // LDS tally slots (>= pixels of a region: a pixel adds to exactly one key)
constexpr unsigned EMPTY = 0xffffffffu;
constexpr int FLAT_BLOCKS = 1024;  // blocks per tile of the two per-pixel passes

enum { T_OUT = 0, T_BG = 1, T_FG = 2 };   // pixel kinds inside a region: outside the tile, background, building

__device__ __forceinline__ int ld_label(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- union-find in LDS (one region) and in global memory (one tile): postproc.hip's loops ---------------------------------
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

// Local labelling.  BOTH: buildings (4-connected) and background (8-connected) in one map, every pixel labelled, the four
// per-root words zeroed.  !BOTH: buildings only, background 0, one per-root word zeroed.
template <bool BOTH>
__global__ void __launch_bounds__(256) cl_label_kernel(const uint8_t* __restrict__ pre, int H, int W,
                                                       int32_t* __restrict__ labels, unsigned* __restrict__ words) {
    __shared__ int par[RG * RG];
    __shared__ uint8_t kind[RG * RG];
    const int tid = threadIdx.x, lx = tid & (RG - 1), ly0 = tid >> 6;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    const int x = x0 + lx;
    int kd[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly, i = ly * RG + lx;
        int t = T_OUT;
        if (x < W && y < H) t = pre[base + (int64_t)y * W + x] != 0 ? T_FG : T_BG;
        if (!BOTH && t == T_BG) t = T_OUT;
        kd[k] = t;
        kind[i] = (uint8_t)t;
        // a wave holds one row of the region: a pixel starts out linked to the first pixel of its run of one kind
        const unsigned long long fgm = __ballot(t == T_FG), bgm = __ballot(t == T_BG);
        const unsigned long long other = ~(t == T_FG ? fgm : bgm) & ((1ull << lx) - 1);
        par[i] = t != T_OUT ? ly * RG + (other ? 64 - __clzll(other) : 0) : -1;
    }
    __syncthreads();
    // A pixel joins the pixel above only where its row's run first meets that pixel's run (its W and NW neighbours are
    // not both of its kind), and a diagonal neighbour only where no straight neighbour already makes the link.
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, i = ly * RG + lx, t = kd[k];
        if (t == T_OUT || ly == 0) continue;
        const bool w = lx > 0 && kind[i - 1] == t, n = kind[i - RG] == t;
        if (n && !(w && kind[i - RG - 1] == t)) lds_union(par, i, i - RG);
        if (BOTH && t == T_BG && !n) {
            if (!w && lx > 0 && kind[i - RG - 1] == T_BG) lds_union(par, i, i - RG - 1);
            if (lx < RG - 1 && kind[i + 1] != T_BG && kind[i - RG + 1] == T_BG) lds_union(par, i, i - RG + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int64_t p = base + (int64_t)y * W + x;
        int lab = 0;
        if (kd[k] != T_OUT) {
            const int r = lds_find(par, ly * RG + lx);
            lab = 1 + (y0 + r / RG) * W + x0 + (r & (RG - 1));
        }
        labels[p] = lab;
        if (BOTH)
            reinterpret_cast<uint4*>(words)[p] = make_uint4(0, 0, 0, 0);
        else
            words[p] = 0;
    }
}

// whether (qx, qy) lies inside the tile and is of the kind `fg`; !BOTH: only buildings are labelled, and only they ask
template <bool BOTH>
__device__ __forceinline__ bool same(const uint8_t* pre, const int32_t* lab, int H, int W, int fg, int qx, int qy) {
    if (qx < 0 || qy < 0 || qx >= W || qy >= H) return false;
    const int q = qy * W + qx;
    return BOTH ? (pre[q] != 0) == fg : ld_label(&lab[q]) != 0;
}

// Border merge: a pixel on its region's top edge joins its neighbour above, a pixel on the left edge its neighbour to the
// left.  A background pixel also joins its diagonal neighbours across that edge: above-left and above-right for the top
// edge, above-left and below-left for the left edge; the ends of the two edges thereby reach across the region's corners
// into the diagonally adjacent regions.  A union is left out where the other unions of this launch and the local labelling
// make the same link: the straight one where the pixel before it on the edge and that pixel's partner across the edge are
// both of its kind (never for the top edge's first pixel, on which the left edge's first pixel relies), a diagonal one
// where either straight neighbour that touches both pixels is background.  A run of pixels along an edge so costs one
// union, not one per pixel.
template <bool BOTH>
__global__ void __launch_bounds__(128) cl_merge_kernel(const uint8_t* __restrict__ pre, int32_t* __restrict__ labels, int H,
                                                       int W) {
    const int t = threadIdx.x, b = blockIdx.z;
    int x = blockIdx.x * RG, y = blockIdx.y * RG;
    const bool top = t < RG;
    if (top) x += t; else y += t - RG;
    if (x >= W || y >= H || (top ? y == 0 : x == 0)) return;
    const int64_t base = (int64_t)b * H * W;
    int32_t* lab = labels + base;
    const uint8_t* pr = pre + base;
    const int p = y * W + x;
    int fg = 1;
    if (BOTH)
        fg = pr[p] != 0;
    else if (ld_label(&lab[p]) == 0)
        return;
    const bool n = same<BOTH>(pr, lab, H, W, fg, x, y - 1), w = same<BOTH>(pr, lab, H, W, fg, x - 1, y);
    const bool nw = same<BOTH>(pr, lab, H, W, fg, x - 1, y - 1);
    const bool diag = BOTH && !fg;
    if (top) {
        if (n && !(t > 0 && w && nw)) g_union(lab, p, p - W);
        if (diag && !n) {
            if (!w && nw) g_union(lab, p, p - W - 1);
            if (!same<BOTH>(pr, lab, H, W, fg, x + 1, y) && same<BOTH>(pr, lab, H, W, fg, x + 1, y - 1)) g_union(lab, p, p - W + 1);
        }
    } else {
        if (w && !(n && nw)) g_union(lab, p, p - 1);
        if (diag && !w) {
            if (!n && nw) g_union(lab, p, p - W - 1);
            if (!same<BOTH>(pr, lab, H, W, fg, x, y + 1) && same<BOTH>(pr, lab, H, W, fg, x - 1, y + 1)) g_union(lab, p, p + W - 1);
        }
    }
}

// adds `add` to the LDS tally of `key` (open addressing; a block holds at most HT keys)
__device__ __forceinline__ void tally_add(unsigned* keys, unsigned* tally, unsigned key, unsigned add) {
    unsigned h = (key * 2654435761u) >> 20;   // 12-bit slot
    for (;;) {
        const unsigned old = atomicCAS(&keys[h], EMPTY, key);
        if (old == EMPTY || old == key) {
            atomicAdd(&tally[h], add);
            return;
        }
        h = (h + 1) & (HT - 1);
    }
}

// Compress + tally: every label becomes 1 + its root.  STAGE 1: a building pixel with post in 1..4 adds 1 to word
// post - 1 of its root; a background pixel adds 1 to word 0 of its root and, on the outer frame, 1 to word 1.
// STAGE 2: a building pixel adds 1 to its root's single word.  A wave holds one row of the region: the first lane of a
// run of equal labels walks to the root for the whole run, and the first lane of a run of equal keys adds the run's
// length.  A block tallies in an LDS table first (low half: the count, at most 4096; high half: the frame count of a
// background root), one global add per key and half.
template <int STAGE>
__global__ void __launch_bounds__(256) cl_tally_kernel(int32_t* __restrict__ labels, const uint8_t* __restrict__ pre,
                                                       const uint8_t* __restrict__ post, int H, int W,
                                                       unsigned* __restrict__ words) {
    __shared__ unsigned keys[HT], tally[HT];
    const int tid = threadIdx.x, lx = tid & (RG - 1), ly0 = tid >> 6;
    const int x0 = blockIdx.x * RG, y0 = blockIdx.y * RG, b = blockIdx.z;
    const int64_t base = (int64_t)b * H * W;
    int32_t* lab = labels + base;
    for (int i = tid; i < HT; i += 256) {
        keys[i] = EMPTY;
        tally[i] = 0;
    }
    __syncthreads();
    const int x = x0 + lx;
    const unsigned long long upto = (2ull << lx) - 1;   // lanes 0 .. lx
    for (int k = 0; k < RPT; ++k) {                      // (every lane runs every round: the shuffles need the whole wave)
        const int y = y0 + ly0 + 4 * k;
        const bool in = x < W && y < H;
        const int p = y * W + x;
        const int l = in ? ld_label(&lab[p]) : 0;
        const int lprev = __shfl_up(l, 1);                 // (shuffles outside every condition: all lanes take part)
        const bool head = l != 0 && (lx == 0 || lprev != l);
        int r = -1;
        if (head) r = g_find(lab, l - 1);
        const unsigned long long heads = __ballot(head) & upto;
        r = __shfl(r, l != 0 ? 63 - __clzll(heads) : lx);
        if (l != 0 && r + 1 != l) __hip_atomic_store(&lab[p], r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned key = EMPTY;
        bool frame = false;
        if (l != 0) {
            key = (unsigned)r;
            if (STAGE == 1) {
                key *= 4u;
                if (pre[base + p] != 0) {
                    const unsigned c = post ? post[base + p] : 0u;
                    key = (c < 1 || c > 4) ? EMPTY : key + c - 1;
                } else {
                    frame = x == 0 || y == 0 || x == W - 1 || y == H - 1;
                }
            }
        }
        const bool active = key != EMPTY;
        const unsigned kprev = __shfl_up(key, 1);
        const bool first = active && (lx == 0 || kprev != key);
        const unsigned long long stop = (__ballot(first) | ~__ballot(active)) & ~upto;   // where the run of this key ends
        if (first) tally_add(keys, tally, key, (unsigned)((stop ? __ffsll((long long)stop) - 1 : 64) - lx));
        if (frame) tally_add(keys, tally, key, 1u << 16);
    }
    __syncthreads();
    unsigned* w = words + base * (STAGE == 1 ? 4 : 1);
    for (int i = tid; i < HT; i += 256) {
        if (keys[i] == EMPTY) continue;
        if (tally[i] & 0xffffu) atomicAdd(&w[keys[i]], tally[i] & 0xffffu);
        if (STAGE == 1 && (tally[i] >> 16)) atomicAdd(&w[keys[i] + 1], tally[i] >> 16);
    }
}

// per-block totals -> stats[b][slot], slot + 1: one global add per block and word (all blocks of a tile add to the same
// two words, so fill and drop run as at most FLAT_BLOCKS blocks per tile that walk the tile with a stride)
__device__ __forceinline__ void stats_flush(unsigned* s_n, unsigned long long* s_px, int64_t* stats, int slot) {
    __syncthreads();
    if (threadIdx.x == 0 && *s_n) {
        unsigned long long* st = reinterpret_cast<unsigned long long*>(stats) + (size_t)blockIdx.z * 4 + slot;
        atomicAdd(&st[0], (unsigned long long)*s_n);
        atomicAdd(&st[1], *s_px);
    }
}

// Fill: a background pixel whose root has no pixel on the frame and an area of at most max_hole becomes building, with
// the owner's voted class; the owner is the building of the pixel left of the hole's root.  Every other pixel is copied.
__global__ void __launch_bounds__(256) cl_fill_kernel(const uint8_t* __restrict__ pre, const uint8_t* __restrict__ post,
                                                      const int32_t* __restrict__ labels, const uint4* __restrict__ words,
                                                      int64_t hw, int64_t max_hole, uint8_t* __restrict__ pre_o,
                                                      uint8_t* __restrict__ post_o, int64_t* __restrict__ stats) {
    __shared__ unsigned s_n;
    __shared__ unsigned long long s_px;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_px = 0;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.z * hw;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
        uint8_t a = pre[base + p], c = post ? post[base + p] : (uint8_t)0;
        if (a == 0) {
            const int r = labels[base + p] - 1;
            const uint4 hole = words[base + r];
            if (hole.y == 0 && (int64_t)hole.x <= max_hole) {
                a = 1;
                if (post) {
                    const uint4 n = words[base + labels[base + r - 1] - 1];
                    unsigned m = n.x;
                    c = m ? 1 : 0;
                    if (n.y > m) { m = n.y; c = 2; }
                    if (n.z > m) { m = n.z; c = 3; }
                    if (n.w > m) c = 4;
                }
                if (r == p) {
                    atomicAdd(&s_n, 1u);
                    atomicAdd(&s_px, (unsigned long long)hole.x);
                }
            }
        }
        pre_o[base + p] = a;
        if (post) post_o[base + p] = c;
    }
    stats_flush(&s_n, &s_px, stats, 0);
}

// Drop: a building pixel of the filled map whose root's area is below min_area becomes background in both outputs.
__global__ void __launch_bounds__(256) cl_drop_kernel(const int32_t* __restrict__ labels, const unsigned* __restrict__ area,
                                                      int64_t hw, int64_t min_area, uint8_t* __restrict__ pre_o,
                                                      uint8_t* __restrict__ post_o, int64_t* __restrict__ stats) {
    __shared__ unsigned s_n;
    __shared__ unsigned long long s_px;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_px = 0;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.z * hw;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (int64_t)gridDim.x * 256) {
        const int l = labels[base + p];
        if (l != 0) {
            const unsigned n = area[base + l - 1];
            if ((int64_t)n < min_area) {
                pre_o[base + p] = 0;
                if (post_o) post_o[base + p] = 0;
                if (l - 1 == p) {
                    atomicAdd(&s_n, 1u);
                    atomicAdd(&s_px, (unsigned long long)n);
                }
            }
        }
    }
    stats_flush(&s_n, &s_px, stats, 2);
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535 && (H + RG - 1) / RG <= 65535;
}

}  // namespace

static int cl_kid(int k) {
    static const int ids[] = {xv2::prof_register("cl_label_kernel"), xv2::prof_register("cl_merge_kernel"),
                              xv2::prof_register("cl_tally_kernel"), xv2::prof_register("cl_fill_kernel"),
                              xv2::prof_register("cl_drop_kernel")};
    return ids[k];
}

extern "C" size_t xv2_clean_workspace(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return 0;
    const size_t n = (size_t)B * H * W;
    // per-root words (4 x uint32) | labels (int32): 20 bytes per pixel
    return align256(16 * n) + align256(4 * n);
}

extern "C" int xv2_clean_buildings(const uint8_t* pre, const uint8_t* post, int B, int H, int W, int64_t min_area,
                                   int64_t max_hole, void* workspace, uint8_t* pre_out, uint8_t* post_out, int64_t* stats,
                                   void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "clean_buildings: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "clean_buildings: H*W=%lld exceeds 2^30 pixels per tile", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + RG - 1) / RG <= 65535, "clean_buildings: B=%d or H=%d too large for one launch", B, H);
    XV2_CHECK_ARG(min_area >= 0 && max_hole >= 0, "clean_buildings: min_area=%lld and max_hole=%lld must not be negative",
                  (long long)min_area, (long long)max_hole);
    XV2_CHECK_ARG(pre && pre_out && stats, "clean_buildings: null tensor");
    XV2_CHECK_ARG((post == nullptr) == (post_out == nullptr), "clean_buildings: post and post_out must both be given or both be NULL");
    XV2_CHECK_ARG(pre != pre_out && (!post || (post != post_out && post != pre_out && pre != post_out)),
                  "clean_buildings: outputs must not alias inputs");
    const bool fill = max_hole > 0, drop = min_area > 1;   // an area is at least 1: min_area <= 1 drops nothing
    XV2_CHECK_ARG(workspace || !(fill || drop), "clean_buildings: workspace required");
    XV2_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "clean_buildings: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W;
    const int64_t hw = (int64_t)H * W;
    char* ws = static_cast<char*>(workspace);
    unsigned* words = reinterpret_cast<unsigned*>(ws);
    int32_t* labels = reinterpret_cast<int32_t*>(ws + align256(16 * n));
    const dim3 grid((W + RG - 1) / RG, (H + RG - 1) / RG, B);
    const dim3 flat((unsigned)std::min<int64_t>(xv2::cdiv(hw, 256), FLAT_BLOCKS), 1, B);
    const double px = (double)n, edges = 8.0 * 128 * grid.x * grid.y * B;
    XV2_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)B * 4 * sizeof(int64_t), st));
    if (fill) {
        XV2_LAUNCH(cl_kid(0), px * 21, cl_label_kernel<true>, grid, dim3(256), 0, st, pre, H, W, labels, words);
        XV2_LAUNCH(cl_kid(1), edges, cl_merge_kernel<true>, grid, dim3(128), 0, st, pre, labels, H, W);
        XV2_LAUNCH(cl_kid(2), px * 10, cl_tally_kernel<1>, grid, dim3(256), 0, st, labels, pre, post, H, W, words);
        XV2_LAUNCH(cl_kid(3), px * (post ? 8 : 6), cl_fill_kernel, flat, dim3(256), 0, st, pre, post, labels,
                   reinterpret_cast<const uint4*>(words), hw, max_hole, pre_out, post_out, stats);
    } else {
        XV2_CHECK_HIP(hipMemcpyAsync(pre_out, pre, n, hipMemcpyDeviceToDevice, st));
        if (post) XV2_CHECK_HIP(hipMemcpyAsync(post_out, post, n, hipMemcpyDeviceToDevice, st));
    }
    if (drop) {
        XV2_LAUNCH(cl_kid(0), px * 9, cl_label_kernel<false>, grid, dim3(256), 0, st, pre_out, H, W, labels, words);
        XV2_LAUNCH(cl_kid(1), edges, cl_merge_kernel<false>, grid, dim3(128), 0, st, pre_out, labels, H, W);
        XV2_LAUNCH(cl_kid(2), px * 8, cl_tally_kernel<2>, grid, dim3(256), 0, st, labels, nullptr, nullptr, H, W, words);
        XV2_LAUNCH(cl_kid(3 + 1), px * 6, cl_drop_kernel, flat, dim3(256), 0, st, labels, words, hw, min_area, pre_out,
                   post_out, stats);
    }
    return XV2_OK;
}
