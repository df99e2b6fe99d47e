// Tolerance simplification of traced outlines (include/xv2.h xv2_polygon_simplify): Douglas-Peucker on every ring of a ring
// table, in integers, with the unique result the header's rule defines.  The header states the rule (anchors, key, split,
// collapse, flags); this file is one method for it: the level-synchronous form, in which every open segment of a ring picks
// its farthest vertex in the same round.  It keeps the vertices the recursive form keeps, because a segment's decision
// depends on the segment alone.
//
// Three launches, nothing read back between them:
//   sp_simplify_kernel  one block of 256 threads per RC = 64 consecutive rings, all rounds of a ring inside the launch.  Ring
//                       sizes are very skewed (on a 4096 x 4096 scene the median ring has 4 vertices, one in a hundred more
//                       than 80), so a ring is taken by one of six paths, by its vertex count n:
//                         n <= 8, 16, 32, 64     8, 16, 32 or 64 lanes of a wave, one vertex per lane, everything in
//                                                registers, 8, 4, 2 or 1 rings per wave at a time: the kept vertices are a
//                                                bit mask, a lane's segment ends are the set bits on either side of it, the
//                                                farthest vertex is a segmented max-scan over the lanes
//                         n <= LDS_MAX = 1024    the whole block, after its waves are done with the small rings: vertices,
//                                                segment ends and the per-segment maxima in LDS (36 KiB of the block's
//                                                37.5 KiB, so four blocks share a CU's 160 KiB)
//                         n >  LDS_MAX           the whole block, the same code with that state in the workspace, striding
//                                                over global memory
//                       The ring's kept vertices go, compacted, to a staging array at the ring's own input offset, with the
//                       ring's kept count, flag and 2A; the block ends with the scan of its rings' kept counts.
//   sp_offsets_kernel   one block: exclusive scan of the blocks' kept counts, out_total
//   sp_write_kernel     flat: the ring rows with columns 2, 3, 4, 7 rewritten; every staged vertex to its new place
//
// The two block paths, per round: every vertex of an open segment takes the max of its key on the segment's word (a 64-bit
// integer max, ds_max_u64 in LDS), the vertices that hold the max take the min of their index, and then every vertex reads
// the winner: it is kept, or it moves its own left or right end to the winner, or - no split - it is dropped for good.  A
// vertex whose segment did not split never looks again, and the loop ends with the first round in which nothing split, at
// most n rounds.  The words are double-buffered by the round's parity: a winner clears the next round's words of the two
// segments it opens while this round's are still being read.  Three block barriers per round, no grid-wide synchronisation.
//
// Every value is an integer.  The atomics are integer max, min and add: no result depends on the order in which threads,
// waves or blocks run, and the same bits come out of every run.  Ring rows whose vertex range does not lie inside
// [0, total_vertices) are not simplified and write nothing (the binding refuses such tables before the call).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>
#include "xv2_common.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int RC = 64;                 // rings per block, at most 64 (one lane of the first wave each); 32 and 16
                                       // measured the same on a scene of 85 000 rings
constexpr int T = 256;                 // threads per block
constexpr int WAVE_MAX = 64;           // largest ring of the register path: 8, 16, 32 or 64 lanes per ring
constexpr int LDS_MAX = 1024;          // largest ring of the LDS path
constexpr int SCAN_T = 1024;
constexpr int COLS = XV2_POLYGON_RING_COLS;
constexpr int KEPT = -2, DEAD = -1;    // a vertex's left end once it is decided
constexpr i64 EXT_MAX = 32767;

struct Work {                          // the workspace, carved by carve()
    int2* tmpv;                        // [V] staged vertices: ring r's kept ones at its input offset
    int* tmpr;                         // [V] the ring of a staged vertex, -1 behind a ring's kept ones
    int* sa;                           // [V] left segment end (rings above LDS_MAX only, as the next three)
    int* sb;                           // [V] right segment end
    u64* best[2];                      // [V] a segment's largest key, at its left end, per round parity
    int* bidx[2];                      // [V] the lowest index that holds it
    int* kept;                         // [R]
    int* flag;                         // [R]
    i64* area;                         // [R]
    i64* newoff;                       // [R] the new offset within the ring's block of RC rings
    i64* bsum;                         // [ceil(R / RC)] kept vertices per block, then the blocks' exclusive scan
    size_t bytes;
};

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

Work carve(void* workspace, int64_t n_rings, int64_t V) {
    Work w;
    const uintptr_t p = reinterpret_cast<uintptr_t>(workspace);
    size_t o = 0;
    auto take = [&](size_t n) { void* q = reinterpret_cast<void*>(p + o); o += align256(n); return q; };
    const size_t v = (size_t)V, r = (size_t)n_rings;
    w.tmpv = reinterpret_cast<int2*>(take(8 * v));
    w.tmpr = reinterpret_cast<int*>(take(4 * v));
    w.sa = reinterpret_cast<int*>(take(4 * v));
    w.sb = reinterpret_cast<int*>(take(4 * v));
    w.best[0] = reinterpret_cast<u64*>(take(8 * v));
    w.best[1] = reinterpret_cast<u64*>(take(8 * v));
    w.bidx[0] = reinterpret_cast<int*>(take(4 * v));
    w.bidx[1] = reinterpret_cast<int*>(take(4 * v));
    w.kept = reinterpret_cast<int*>(take(4 * r));
    w.flag = reinterpret_cast<int*>(take(4 * r));
    w.area = reinterpret_cast<i64*>(take(8 * r));
    w.newoff = reinterpret_cast<i64*>(take(8 * r));
    w.bsum = reinterpret_cast<i64*>(take(8 * ((r + RC - 1) / RC)));
    w.bytes = o + 256;                 // never 0 inside the limits
    return w;
}

struct Sh {                            // 36 KiB for the LDS path and 1.5 KiB for the block's ring list
    int2 v[LDS_MAX];
    short sa[LDS_MAX], sb[LDS_MAX];
    u64 best[2][LDS_MAX];
    int bidx[2][LDS_MAX];
    u64 wsum[16];
    u64 red, area, mask[3];
    i64 roff[RC];                      // the block's rings: offset, vertex count (0 for a row outside the vertex array),
    int rn[RC];
    int ext[4], cnt, count[4];         // rings per group width,
    unsigned char list[4][RC];         // and which they are
};

// ---- the rule's key ------------------------------------------------------------------------------------------------------
// squared distance of P to the segment A B, times scale; the differences are at most 32767, so every product is < 2^62
__device__ __forceinline__ u64 seg_scale(int2 a, int2 b) {
    const i64 dx = (i64)b.x - a.x, dy = (i64)b.y - a.y;
    const i64 L2 = dx * dx + dy * dy;
    return L2 == 0 ? 1ull : (u64)L2;
}

__device__ __forceinline__ u64 seg_key(int2 a, int2 b, int2 p) {
    const i64 dx = (i64)b.x - a.x, dy = (i64)b.y - a.y, vx = (i64)p.x - a.x, vy = (i64)p.y - a.y;
    const i64 L2 = dx * dx + dy * dy;
    if (L2 == 0) return (u64)(vx * vx + vy * vy);
    const i64 t = vx * dx + vy * dy;
    if (t <= 0) return (u64)(vx * vx + vy * vy) * (u64)L2;
    if (t >= L2) {
        const i64 wx = (i64)p.x - b.x, wy = (i64)p.y - b.y;
        return (u64)(wx * wx + wy * wy) * (u64)L2;
    }
    const i64 c = vx * dy - vy * dx;
    return (u64)(c * c);
}

// ---- helpers ---------------------------------------------------------------------------------------------------------------
// exclusive scan over the block (a multiple of 64 threads, at most 1024); wsum: 16 LDS words; total: the block's sum
__device__ __forceinline__ u64 block_scan(u64 v, u64* wsum, u64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u64 before = 0;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const u64 s = wsum[w];
        before += w < wave ? s : 0ull;
        total += s;
    }
    __syncthreads();
    return before + inc - v;
}

// the lowest set bit of m above position i, or `none`
__device__ __forceinline__ int next_bit(u64 m, int i, int none) {
    const u64 above = i < 63 ? m >> (i + 1) : 0ull;
    return above ? i + 1 + __builtin_ctzll(above) : none;
}

// ---- n <= 64: G lanes per ring, one vertex per lane, 64 / G rings per wave ------------------------------------------------
// ring `slot * (64 / G) + group` of the block's list of rings of this size class; a group without a ring idles with n = 0.
// Nothing here is uniform over the wave: the groups' rings differ in size and in rounds, so every step is predicated and the
// round loop runs while any group has an open segment.
template <int G>
__device__ __forceinline__ void group_rings(const Sh& sh, const int2* __restrict__ verts, u64 q2, i64 r0, int cls, int slot,
                                            const Work& w) {
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const u64 gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
    const int at = slot * (64 / G) + lane / G;
    const bool have = at < sh.count[cls];
    const int j = have ? sh.list[cls][at] : 0;
    const int n = have ? sh.rn[j] : 0;
    const i64 off = sh.roff[j];
    const int r = (int)(r0 + j);
    const bool in = gl < n;
    int2 p = make_int2(0, 0);
    if (in) p = verts[off + gl];
    const int2 p0 = make_int2(__shfl(p.x, gbase, 64), __shfl(p.y, gbase, 64));
    if (!in) p = p0;
    int x0 = p.x, x1 = p.x, y0 = p.y, y1 = p.y;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)), x1 = max(x1, __shfl_xor(x1, o, 64));
        y0 = min(y0, __shfl_xor(y0, o, 64)), y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    const u64 all = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    const u64 lt = (1ull << gl) - 1ull;
    // anchor m: the largest squared distance from v[0], the lowest index among equals (the products wrap harmlessly in a ring
    // over the extent limit, whose result is not used)
    const u64 rx = (u64)((i64)p.x - p0.x), ry = (u64)((i64)p.y - p0.y);
    u64 mx = in ? ((rx * rx + ry * ry) << 32) | (u64)(63 - gl) : 0ull;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(mx, o, 64);
        mx = t > mx ? t : mx;
    }
    int flag = 0;
    if ((i64)x1 - x0 > EXT_MAX || (i64)y1 - y0 > EXT_MAX) flag = 2;
    else if (n < 3 || (mx >> 32) == 0) flag = 1;
    u64 keep = flag ? all : 1ull | (1ull << (63 - (int)(mx & 0xffffffffull)));
    u64 act = all & ~keep;                                              // the vertices of the ring's open segments
    for (int round = 0; round < G && __ballot(act != 0) != 0; ++round) {
        const bool me = (act >> gl) & 1ull;
        const int A = me ? 63 - __builtin_clzll(keep & lt) : 0;          // (vertex 0 is kept, so the mask is not 0)
        const int B = me ? next_bit(keep, gl, n) : 1;
        const int bsrc = B == n ? 0 : B;                                // v[n] is v[0]
        const int2 a = make_int2(__shfl(p.x, gbase + A, 64), __shfl(p.y, gbase + A, 64));
        const int2 b = make_int2(__shfl(p.x, gbase + bsrc, 64), __shfl(p.y, gbase + bsrc, 64));
        u64 bk = me ? seg_key(a, b, p) : 0ull;
        int bi = gl;
        // inclusive max-scan inside the segment's lanes A + 1 .. B - 1: the larger key, the lower index among equals
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const u64 ok = __shfl_up(bk, o, 64);
            const int oi = __shfl_up(bi, o, 64);
            if (me && gl - o > A && (ok > bk || (ok == bk && oi < bi))) {
                bk = ok;
                bi = oi;
            }
        }
        const u64 fk = __shfl(bk, gbase + B - 1, 64);                   // the segment's last lane holds its result
        const int fi = __shfl(bi, gbase + B - 1, 64);
        const bool split = me && fk > ((q2 * seg_scale(a, b)) >> 8);
        const u64 win = (__ballot(split && fi == gl) >> gbase) & gmask;
        act = ((__ballot(split) >> gbase) & gmask) & ~win;
        keep |= win;
    }
    if (flag == 0 && __popcll(keep) < 3) flag = 1;
    if (flag) keep = all;
    const int kept = __popcll(keep);
    const bool mine = (keep >> gl) & 1ull;
    const int nl = next_bit(keep, gl, 0);
    const int2 nx = make_int2(__shfl(p.x, gbase + nl, 64), __shfl(p.y, gbase + nl, 64));
    u64 area = mine ? (u64)((i64)p.x * nx.y - (i64)nx.x * p.y) : 0ull;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) area += __shfl_xor(area, o, 64);
    if (in) {
        if (mine) w.tmpv[off + __popcll(keep & lt)] = p;
        w.tmpr[off + gl] = gl < kept ? r : -1;
    }
    if (have && gl == 0) {
        w.kept[r] = kept;
        w.flag[r] = flag;
        w.area[r] = (i64)area;
    }
}

// ---- n > 64: the block, its state in LDS or in the workspace --------------------------------------------------------------
// what other threads wrote with an atomic is read past the vector cache when it lives in global memory
template <bool LDS> __device__ __forceinline__ u64 ld_u64(const u64* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ int ld_int(const int* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void st_u64(u64* p, u64 v) {
    if (LDS) *p = v;
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS> __device__ __forceinline__ void st_int(int* p, int v) {
    if (LDS) *p = v;
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ void block_ring(Sh& sh, const int2* __restrict__ verts, i64 off, int n, u64 q2, int r,
                                           const Work& w) {
    const int t = threadIdx.x;
    const int2* gv = verts + off;
    const int2* vv = LDS ? sh.v : gv;
    typedef typename std::conditional<LDS, short, int>::type End;       // (n <= 1024 in LDS)
    End* sa = nullptr;
    End* sb = nullptr;
    if constexpr (LDS) sa = sh.sa, sb = sh.sb;
    else sa = w.sa + off, sb = w.sb + off;
    u64* best[2] = {LDS ? sh.best[0] : w.best[0] + off, LDS ? sh.best[1] : w.best[1] + off};
    int* bidx[2] = {LDS ? sh.bidx[0] : w.bidx[0] + off, LDS ? sh.bidx[1] : w.bidx[1] + off};
    if (t == 0) {
        sh.red = 0;
        sh.area = 0;
        sh.cnt = 0;
        sh.ext[0] = sh.ext[2] = INT_MAX;
        sh.ext[1] = sh.ext[3] = INT_MIN;
    }
    __syncthreads();
    {
        int x0 = INT_MAX, x1 = INT_MIN, y0 = INT_MAX, y1 = INT_MIN;
        for (int i = t; i < n; i += T) {
            const int2 p = gv[i];
            if (LDS) sh.v[i] = p;
            x0 = min(x0, p.x), x1 = max(x1, p.x), y0 = min(y0, p.y), y1 = max(y1, p.y);
        }
        if (t < n) {
            atomicMin(&sh.ext[0], x0);
            atomicMax(&sh.ext[1], x1);
            atomicMin(&sh.ext[2], y0);
            atomicMax(&sh.ext[3], y1);
        }
    }
    __syncthreads();
    int flag = 0;                                                       // (every branch below is uniform over the block)
    if ((i64)sh.ext[1] - sh.ext[0] > EXT_MAX || (i64)sh.ext[3] - sh.ext[2] > EXT_MAX) {
        flag = 2;
    } else if (n < 3) {
        flag = 1;
    } else {
        const int2 p0 = vv[0];
        u64 pk = 0;
        for (int i = t; i < n; i += T) {
            const int2 p = vv[i];
            const i64 rx = (i64)p.x - p0.x, ry = (i64)p.y - p0.y;
            const u64 c = ((u64)(rx * rx + ry * ry) << 32) | (u64)(0xffffffffu - (unsigned)i);
            pk = c > pk ? c : pk;
        }
        atomicMax(&sh.red, pk);
        __syncthreads();
        const u64 mx = sh.red;
        if ((mx >> 32) == 0) {
            flag = 1;
        } else {
            const int m = (int)(0xffffffffu - (unsigned)(mx & 0xffffffffull));
            for (int i = t; i < n; i += T) {
                if (i == 0 || i == m) {
                    sa[i] = KEPT;
                    st_u64<LDS>(best[0] + i, 0ull);
                    st_int<LDS>(bidx[0] + i, INT_MAX);
                } else {
                    sa[i] = (End)(i < m ? 0 : m);
                    sb[i] = (End)(i < m ? m : n);
                }
            }
            __syncthreads();
            int par = 0;
            for (int round = 0; round < n; ++round) {
                u64* bw = best[par];
                int* iw = bidx[par];
                for (int i = t; i < n; i += T) {
                    const int a = sa[i];
                    if (a < 0) continue;
                    const int b = sb[i];
                    atomicMax(bw + a, seg_key(vv[a], vv[b == n ? 0 : b], vv[i]));
                }
                __syncthreads();
                for (int i = t; i < n; i += T) {
                    const int a = sa[i];
                    if (a < 0) continue;
                    const int b = sb[i];
                    if (seg_key(vv[a], vv[b == n ? 0 : b], vv[i]) == ld_u64<LDS>(bw + a)) atomicMin(iw + a, i);
                }
                __syncthreads();
                int any = 0;
                for (int i = t; i < n; i += T) {
                    const int a = sa[i];
                    if (a < 0) continue;
                    const int b = sb[i];
                    if (ld_u64<LDS>(bw + a) > ((q2 * seg_scale(vv[a], vv[b == n ? 0 : b])) >> 8)) {
                        const int win = ld_int<LDS>(iw + a);
                        any = 1;
                        if (i == win) {                                 // kept: it opens (a, i) and (i, b) for the next round
                            sa[i] = KEPT;
                            st_u64<LDS>(best[par ^ 1] + a, 0ull);
                            st_int<LDS>(bidx[par ^ 1] + a, INT_MAX);
                            st_u64<LDS>(best[par ^ 1] + i, 0ull);
                            st_int<LDS>(bidx[par ^ 1] + i, INT_MAX);
                        } else if (i < win) {
                            sb[i] = (End)win;
                        } else {
                            sa[i] = (End)win;
                        }
                    } else {
                        sa[i] = DEAD;
                    }
                }
                if (!__syncthreads_or(any)) break;
                par ^= 1;
            }
            int c = 0;
            for (int i = t; i < n; i += T) c += sa[i] == KEPT;
            atomicAdd(&sh.cnt, c);
            __syncthreads();
            if (sh.cnt < 3) flag = 1;
        }
    }
    const int kept = flag ? n : sh.cnt;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += T) {
        const int i = i0 + t;
        const bool k = i < n && (flag != 0 || sa[i] == KEPT);
        u64 total;
        const int ex = (int)block_scan(k ? 1ull : 0ull, sh.wsum, total);
        if (k) w.tmpv[off + carry + ex] = vv[i];
        if (i < n) w.tmpr[off + i] = i < kept ? r : -1;
        carry += (int)total;
    }
    __syncthreads();
    u64 s = 0;
    for (int k = t; k < kept; k += T) {
        const int2 a = w.tmpv[off + k], b = w.tmpv[off + (k + 1 == kept ? 0 : k + 1)];
        s += (u64)((i64)a.x * b.y - (i64)b.x * a.y);
    }
    atomicAdd(&sh.area, s);
    __syncthreads();
    if (t == 0) {
        w.kept[r] = kept;
        w.flag[r] = flag;
        w.area[r] = (i64)sh.area;
    }
    __syncthreads();
}

__device__ __forceinline__ bool ring_range(const int64_t* __restrict__ rings, i64 r, i64 V, i64& off, int& n) {
    const i64 nn = rings[r * COLS + 2];
    off = rings[r * COLS + 3];
    n = (int)nn;
    return nn >= 0 && off >= 0 && nn <= V && off <= V - nn;
}

template <int G>
__device__ __forceinline__ void group_class(const Sh& sh, const int2* __restrict__ verts, u64 q2, i64 r0, int cls,
                                            const Work& w) {
    for (int slot = threadIdx.x >> 6; slot * (64 / G) < sh.count[cls]; slot += T / 64) group_rings<G>(sh, verts, q2, r0, cls, slot, w);
}

__global__ void __launch_bounds__(T) sp_simplify_kernel(const int64_t* __restrict__ rings, const int2* __restrict__ verts,
                                                        i64 n_rings, i64 V, u64 q2, Work w) {
    __shared__ Sh sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 r0 = (i64)blockIdx.x * RC;
    if (wave == 0) {                                                    // the block's rings by path
        int cls = 7;
        i64 off = 0;
        int n = 0;
        if (lane < RC && r0 + lane < n_rings) {
            if (!ring_range(rings, r0 + lane, V, off, n)) cls = 6, n = 0, off = 0;
            else cls = n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= WAVE_MAX ? 3 : n <= LDS_MAX ? 4 : 5;
        }
        if (lane < RC) sh.rn[lane] = n, sh.roff[lane] = off;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u64 m = __ballot(cls == c);
            if (cls == c) sh.list[c][__popcll(m & ((1ull << lane) - 1ull))] = (unsigned char)lane;
            if (lane == 0) sh.count[c] = __popcll(m);
        }
        const u64 m4 = __ballot(cls == 4), m5 = __ballot(cls == 5), m6 = __ballot(cls == 6);
        if (lane == 0) sh.mask[0] = m4, sh.mask[1] = m5, sh.mask[2] = m6;
    }
    __syncthreads();
    group_class<8>(sh, verts, q2, r0, 0, w);
    group_class<16>(sh, verts, q2, r0, 1, w);
    group_class<32>(sh, verts, q2, r0, 2, w);
    group_class<64>(sh, verts, q2, r0, 3, w);
    if (threadIdx.x < RC && ((sh.mask[2] >> threadIdx.x) & 1ull)) {     // a row that points outside the vertex array
        w.kept[r0 + threadIdx.x] = 0;
        w.flag[r0 + threadIdx.x] = 0;
        w.area[r0 + threadIdx.x] = 0;
    }
    const u64 lds = sh.mask[0];
    u64 todo = lds | sh.mask[1];
    while (todo) {                                                      // (block_ring begins and ends with a barrier)
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        if ((lds >> j) & 1ull) block_ring<true>(sh, verts, sh.roff[j], sh.rn[j], q2, (int)(r0 + j), w);
        else block_ring<false>(sh, verts, sh.roff[j], sh.rn[j], q2, (int)(r0 + j), w);
    }
    __syncthreads();
    if (wave == 0) {                                                    // the kept counts of the block's rings, scanned
        const bool live = lane < RC && r0 + lane < n_rings;
        const u64 k = live ? (u64)w.kept[r0 + lane] : 0ull;
        u64 inc = k;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (live) w.newoff[r0 + lane] = (i64)(inc - k);
        if (lane == 63) w.bsum[blockIdx.x] = (i64)inc;
    }
}

// exclusive scan of the blocks' kept counts in place, their total -> out_total
__global__ void __launch_bounds__(SCAN_T) sp_offsets_kernel(i64* __restrict__ bsum, i64 n_blocks, int64_t* __restrict__ out_total) {
    __shared__ u64 wsum[16];
    u64 carry = 0;
    for (i64 i0 = 0; i0 < n_blocks; i0 += SCAN_T) {
        const i64 i = i0 + threadIdx.x;
        u64 total;
        const u64 ex = block_scan(i < n_blocks ? (u64)bsum[i] : 0ull, wsum, total);
        if (i < n_blocks) bsum[i] = (i64)(carry + ex);
        carry += total;
    }
    if (threadIdx.x == 0) *out_total = (int64_t)carry;
}

__global__ void __launch_bounds__(256) sp_write_kernel(const int64_t* __restrict__ rings, i64 n_rings, i64 V, Work w,
                                                       int64_t* __restrict__ out_rings, int2* __restrict__ out_verts) {
    const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
    if (g < n_rings * COLS) {
        const i64 r = g / COLS;
        const int c = (int)(g % COLS);
        out_rings[g] = c == 2 ? (int64_t)w.kept[r] : c == 3 ? w.bsum[r / RC] + w.newoff[r] : c == 4 ? w.area[r]
                       : c == 7 ? (int64_t)w.flag[r] : rings[g];
    }
    if (g < V) {
        const int r = w.tmpr[g];
        if (r >= 0 && (i64)r < n_rings) {
            const i64 k = g - rings[(i64)r * COLS + 3], dst = w.bsum[r / RC] + w.newoff[r] + k;
            if (k >= 0 && k < (i64)w.kept[r] && dst >= 0 && dst < V) out_verts[dst] = w.tmpv[g];
        }
    }
}

bool sizes_ok(int64_t n_rings, int64_t V) {
    return n_rings >= 0 && V >= 0 && n_rings < (1ll << 31) && V < (1ll << 31);
}

}  // namespace

static int sp_kid(int k) {
    static const int ids[] = {xv2::prof_register("sp_simplify_kernel"), xv2::prof_register("sp_offsets_kernel"),
                              xv2::prof_register("sp_write_kernel")};
    return ids[k];
}

extern "C" size_t xv2_polygon_simplify_workspace(int64_t n_rings, int64_t total_vertices) {
    if (!sizes_ok(n_rings, total_vertices)) return 0;
    return carve(nullptr, n_rings, total_vertices).bytes;
}

extern "C" int xv2_polygon_simplify(const int64_t* rings, const int32_t* verts, int64_t n_rings, int64_t total_vertices, int q,
                                    void* workspace, int64_t* out_rings, int32_t* out_verts, int64_t* out_total,
                                    void* stream) {
    XV2_CHECK_ARG(sizes_ok(n_rings, total_vertices), "polygon_simplify: n_rings=%lld total_vertices=%lld outside 0 .. 2^31 - 1",
                  (long long)n_rings, (long long)total_vertices);
    XV2_CHECK_ARG(q >= 0 && q <= 65535, "polygon_simplify: q=%d outside 0 .. 65535", q);
    XV2_CHECK_ARG(workspace && out_total, "polygon_simplify: null workspace or out_total");
    XV2_CHECK_ARG((n_rings == 0 || (rings && out_rings)) && (total_vertices == 0 || (verts && out_verts)),
                  "polygon_simplify: null tensor with n_rings=%lld total_vertices=%lld", (long long)n_rings,
                  (long long)total_vertices);
    XV2_CHECK_ARG(((reinterpret_cast<uintptr_t>(verts) | reinterpret_cast<uintptr_t>(out_verts) |
                    reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                  "polygon_simplify: verts, out_verts and the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Work w = carve(workspace, n_rings, total_vertices);
    const double rb = 64.0 * (double)n_rings, vb = 8.0 * (double)total_vertices;
    const int2* v2 = reinterpret_cast<const int2*>(verts);
    const int64_t n_blocks = (n_rings + RC - 1) / RC;
    if (n_rings > 0)
        XV2_LAUNCH(sp_kid(0), rb + 2.5 * vb, sp_simplify_kernel, dim3((unsigned)n_blocks), dim3(T), 0, st, rings,
                   v2, (i64)n_rings, (i64)total_vertices, (u64)q * (u64)q, w);
    XV2_LAUNCH(sp_kid(1), 16.0 * (double)n_blocks, sp_offsets_kernel, dim3(1), dim3(SCAN_T), 0, st, w.bsum, (i64)n_blocks,
               out_total);
    const int64_t flat = n_rings * COLS > total_vertices ? n_rings * COLS : total_vertices;
    if (flat > 0)
        XV2_LAUNCH(sp_kid(2), 2.0 * rb + 2.5 * vb, sp_write_kernel, dim3((unsigned)((flat + 255) / 256)), dim3(256), 0, st, rings,
                   (i64)n_rings, (i64)total_vertices, w, out_rings, reinterpret_cast<int2*>(out_verts));
    return XV2_OK;
}
