// Building outlines of a label map (include/xv2.h xv2_polygon_count / xv2_polygon_trace): the boundary edges of every
// 4-connected component, ordered into closed rings with their corner vertices, in parallel and with the same bits on
// every run.  The contract (edges, successor rule, leaders, vertices, 2A) is the header's; this file is one method for it.
//
// Every value is an integer.  The only atomics are integer adds of ring numbers into ring_count[b]; everything else is a gather or
// a scan, so no result depends on the order in which blocks run.  Launch boundaries are the only cross-block
// synchronisation, and nothing is read back between the launches of a call.
//
// xv2_polygon_count (two launches):
//   pg_count_kernel   boundary and turning edges per chunk of PC consecutive pixels of the flattened tile; the 3 x 3
//                     neighbourhoods come from LDS flags of the chunk and of the rows above and below it
//   pg_scan_kernel    exclusive scan of a tile's chunk counts in place, the tile's totals -> counts[b]
// xv2_polygon_trace (10 + 2 R launches, R = ceil(log2(total_edges))):
//   the two above into its own workspace, then
//   pg_tiles_kernel   scan of the tile totals -> first dense edge index per tile; totals != the caller's -> status, and
//                     every later kernel returns at once (the arrays are sized by the caller's totals)
//   pg_index_kernel   dense index (raster order, tile-major) of every pixel's first edge; edge -> 4 * pixel + side
//   pg_succ_kernel    successor of every edge by the three-pixel rule, in dense indices, bit 31 = the edge turns
//   pg_min_kernel     R rounds of pointer doubling over {next, minimum of the window}: the ring's leader at every edge
//   pg_cut_kernel     cuts each ring before its leader, starts the sums {edges, turning edges, shoelace} at every edge
//   pg_rank_kernel    R rounds of pointer doubling: suffix sums to the ring's end; at the leader these are the ring's
//                     totals, and leader - own is what lies before an edge
//   pg_lcount_kernel, pg_lscan_kernel   rings and their vertices per chunk of EC edges, scanned
//   pg_rings_kernel   one ring-table row per leader, in ascending leader; ring_count
//   pg_verts_kernel   every turning edge writes its end corner at offset[ring] + ordinal
// A doubling round that changed nothing raises no flag, and the rounds after it see that and return: the number of
// rounds that work follows the longest ring, not the edge total, with no host decision.  (A round of window minima
// that changes nothing has m[e] <= m[e + 2^k] all around every ring, so m is constant on each stride orbit; the windows
// of an orbit cover the ring, so m is already the ring's minimum.)
//
// The shoelace sum is carried in 32 bits: only a ring's total is used, |2A| <= 2 H W < 2^31, and unsigned wrap-around
// of the partial sums cancels in the total.  That keeps the per-edge record of the ranking rounds at 16 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

constexpr int PC = 1024;               // pixels per chunk: 256 threads x 4 consecutive pixels
constexpr int EC = 1024;               // edges per chunk of the ring passes
constexpr int SCAN_T = 1024;
constexpr int MAX_ROUNDS = 32;
constexpr unsigned NIL = 0xffffffffu;
constexpr unsigned TURN = 0x80000000u;

typedef unsigned long long u64;

// head of the trace workspace; chg[phase][r] != 0: round r of that phase changed something
struct Hdr {
    long long found[2];
    int ok;
    int rounds[2];
    int pad;
    int chg[2][MAX_ROUNDS];
};

struct Trace {                         // the trace workspace, carved by carve()
    Hdr* hdr;
    long long* tile_tot;               // [B][2]
    long long* tile_eoff;              // [B + 1]
    u64* pchunk;                       // [B][npc]: turning edges << 32 | edges
    unsigned* pix_off;                 // [B][H * W]: dense index of the pixel's first edge
    unsigned char* pix_em;             // [B][H * W]: the pixel's boundary sides
    unsigned* einfo;                   // [E]: 4 * pixel + side
    unsigned* succ;                    // [E]: dense successor | TURN
    unsigned* lead;                    // [E]
    unsigned* voff;                    // [E], written at leaders only
    uint2* recA[2];                    // [E] {next, window minimum}
    uint4* recB[2];                    // [E] {next, edges, turning edges, shoelace}
    u64* lchunk;                       // [nec]: rings << 32 | vertices
    size_t bytes;
};

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
int64_t pchunks_of(int H, int W) { return ((int64_t)H * W + PC - 1) / PC; }
int64_t echunks_of(int64_t E) { return (E + EC - 1) / EC; }

Trace carve(void* workspace, int B, int H, int W, int64_t E) {
    Trace t;
    const uintptr_t p = reinterpret_cast<uintptr_t>(workspace);
    size_t o = 0;
    auto take = [&](size_t n) { void* q = reinterpret_cast<void*>(p + o); o += align256(n); return q; };
    const size_t px = (size_t)B * H * W, e = (size_t)E;
    t.hdr = reinterpret_cast<Hdr*>(take(sizeof(Hdr)));
    t.tile_tot = reinterpret_cast<long long*>(take(16 * (size_t)B));
    t.tile_eoff = reinterpret_cast<long long*>(take(8 * ((size_t)B + 1)));
    t.pchunk = reinterpret_cast<u64*>(take(8 * (size_t)B * pchunks_of(H, W)));
    t.pix_off = reinterpret_cast<unsigned*>(take(4 * px));
    t.pix_em = reinterpret_cast<unsigned char*>(take(px));
    t.einfo = reinterpret_cast<unsigned*>(take(4 * e));
    t.succ = reinterpret_cast<unsigned*>(take(4 * e));
    t.lead = reinterpret_cast<unsigned*>(take(4 * e));
    t.voff = reinterpret_cast<unsigned*>(take(4 * e));
    t.recA[0] = reinterpret_cast<uint2*>(take(8 * e));
    t.recA[1] = reinterpret_cast<uint2*>(take(8 * e));
    t.recB[0] = reinterpret_cast<uint4*>(take(16 * e));
    t.recB[1] = reinterpret_cast<uint4*>(take(16 * e));
    t.lchunk = reinterpret_cast<u64*>(take(8 * (size_t)echunks_of(E)));
    t.bytes = o;
    return t;
}

// ---- the contract's local rules -------------------------------------------------------------------------------------------
// directions 0 E, 1 S, 2 W, 3 N on screen; side s heads in direction s, and left(d) = (d + 3) % 4
__device__ __forceinline__ int dxs(int d) { return (d == 0) - (d == 2); }
__device__ __forceinline__ int dys(int d) { return (d == 1) - (d == 3); }

// fg flags of a chunk's pixels and of the rows above and below them, from three coalesced ranges of the flattened tile:
// F[r][i] is the pixel at flattened index c0 - 1 + i + (r - 1) W, background outside the tile.  A neighbour across the
// left or right border of the image has a flattened index of the next or previous row, so x decides there.
typedef unsigned char Flags[3][PC + 2];

__device__ __forceinline__ void load_flags(const int32_t* __restrict__ lab, int W, int hw, int c0, Flags& F) {
    for (int i = threadIdx.x; i < PC + 2; i += 256) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int64_t idx = (int64_t)c0 - 1 + i + (int64_t)(r - 1) * W;
            F[r][i] = idx >= 0 && idx < hw && lab[idx] != 0;
        }
    }
    __syncthreads();
}

// bit (dy + 1) * 3 + (dx + 1): the neighbour at (y + dy, x + dx) of the chunk's k-th pixel is foreground
__device__ __forceinline__ unsigned nb9(const Flags& F, int W, int k, int x) {
    unsigned n = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if ((unsigned)(x + d - 1) < (unsigned)W && F[r][k + d]) n |= 1u << (3 * r + d);
    return n;
}
__device__ __forceinline__ bool at(unsigned n, int dy, int dx) { return (n >> ((dy + 1) * 3 + dx + 1)) & 1u; }

// boundary sides (em) and turning boundary sides (tm) of a foreground pixel from its neighbourhood
__device__ __forceinline__ void side_masks(unsigned n, unsigned& em, unsigned& tm) {
    em = tm = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int l = (s + 3) & 3;
        if (at(n, dys(l), dxs(l))) continue;              // the pixel across side s is p + left(direction s)
        em |= 1u << s;
        const bool a = at(n, dys(s), dxs(s)), ll = at(n, dys(s) + dys(l), dxs(s) + dxs(l));
        if (!(a && !ll)) tm |= 1u << s;
    }
}

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

// the neighbourhoods and masks of the four pixels of a thread (k0 = 4 * threadIdx.x within the chunk at c0); returns
// turning edges << 32 | edges
__device__ __forceinline__ u64 four_pixels(const Flags& F, int W, int c0, unsigned (&nb)[4], unsigned (&em)[4],
                                           unsigned (&tm)[4]) {
    const int k0 = threadIdx.x * 4;
    int x = (c0 + k0) % W;
    u64 v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        nb[j] = em[j] = tm[j] = 0;
        if (F[1][k0 + j + 1]) {
            nb[j] = nb9(F, W, k0 + j, x);
            side_masks(nb[j], em[j], tm[j]);
            v += (u64)__popc(em[j]) | ((u64)__popc(tm[j]) << 32);
        }
        if (++x == W) x = 0;
    }
    return v;
}

__global__ void __launch_bounds__(256) pg_count_kernel(const int32_t* __restrict__ labels, int H, int W, int npc,
                                                       u64* __restrict__ pchunk) {
    __shared__ u64 wsum[16];
    __shared__ Flags F;
    const int b = blockIdx.y, hw = H * W, c0 = blockIdx.x * PC;
    load_flags(labels + (int64_t)b * hw, W, hw, c0, F);
    unsigned nb[4], em[4], tm[4];
    u64 total;
    block_scan(four_pixels(F, W, c0, nb, em, tm), wsum, total);
    if (threadIdx.x == 0) pchunk[(int64_t)b * npc + blockIdx.x] = total;
}

// exclusive scan of a tile's chunk counts in place (both halves stay below 2^32 within a tile: at most 2 H W + H + W edges)
__global__ void __launch_bounds__(SCAN_T) pg_scan_kernel(u64* __restrict__ pchunk, int npc, int64_t* __restrict__ tot) {
    __shared__ u64 wsum[16];
    const int b = blockIdx.x;
    u64* c = pchunk + (int64_t)b * npc;
    u64 carry = 0;
    for (int i0 = 0; i0 < npc; i0 += SCAN_T) {
        const int i = i0 + threadIdx.x;
        u64 total;
        const u64 ex = block_scan(i < npc ? c[i] : 0ull, wsum, total);
        if (i < npc) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        tot[2 * b] = (int64_t)(carry & 0xffffffffull);
        tot[2 * b + 1] = (int64_t)(carry >> 32);
    }
}

__global__ void __launch_bounds__(256) pg_tiles_kernel(const long long* __restrict__ tot, int B, long long E, long long V,
                                                       long long* __restrict__ tile_eoff, Hdr* __restrict__ hdr,
                                                       int32_t* __restrict__ ring_count, int32_t* __restrict__ status) {
    __shared__ u64 wsum[16];
    u64 ce = 0, cv = 0;
    for (int i0 = 0; i0 < B; i0 += 256) {
        const int i = i0 + threadIdx.x;
        u64 te, tv;
        const u64 ex = block_scan(i < B ? (u64)tot[2 * i] : 0ull, wsum, te);
        block_scan(i < B ? (u64)tot[2 * i + 1] : 0ull, wsum, tv);
        if (i < B) {
            tile_eoff[i] = (long long)(ce + ex);
            ring_count[i] = 0;
        }
        ce += te;
        cv += tv;
    }
    if (threadIdx.x < 2 * MAX_ROUNDS) hdr->chg[threadIdx.x / MAX_ROUNDS][threadIdx.x % MAX_ROUNDS] = 0;
    if (threadIdx.x == 0) {
        tile_eoff[B] = (long long)ce;
        hdr->found[0] = (long long)ce;
        hdr->found[1] = (long long)cv;
        const int ok = (long long)ce == E && (long long)cv == V;
        hdr->ok = ok;
        hdr->rounds[0] = hdr->rounds[1] = 0;
        hdr->pad = 0;
        if (!ok) *status = *status | 1;
    }
}

__global__ void __launch_bounds__(256) pg_index_kernel(const int32_t* __restrict__ labels, int H, int W, int npc,
                                                       const Hdr* __restrict__ hdr, const long long* __restrict__ tile_eoff,
                                                       const u64* __restrict__ pchunk, unsigned E,
                                                       unsigned* __restrict__ pix_off, unsigned char* __restrict__ pix_em,
                                                       unsigned* __restrict__ einfo) {
    __shared__ u64 wsum[16];
    __shared__ Flags F;
    if (!hdr->ok) return;
    const int b = blockIdx.y, hw = H * W, c0 = blockIdx.x * PC, p0 = c0 + threadIdx.x * 4;
    load_flags(labels + (int64_t)b * hw, W, hw, c0, F);
    unsigned nb[4], em[4], tm[4];
    u64 total;
    const u64 v = four_pixels(F, W, c0, nb, em, tm);
    const u64 ex = block_scan(v & 0xffffffffull, wsum, total);
    unsigned e = (unsigned)(tile_eoff[b] + (long long)(pchunk[(int64_t)b * npc + blockIdx.x] & 0xffffffffull) + (long long)ex);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= hw) break;
        pix_off[(int64_t)b * hw + p] = e;
        pix_em[(int64_t)b * hw + p] = (unsigned char)em[j];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if ((em[j] >> s) & 1u) {
                if (e < E) einfo[e] = 4u * (unsigned)p + (unsigned)s;
                ++e;
            }
    }
}

__global__ void __launch_bounds__(256) pg_succ_kernel(const int32_t* __restrict__ labels, int H, int W,
                                                      const Hdr* __restrict__ hdr, const unsigned* __restrict__ pix_off,
                                                      const unsigned char* __restrict__ pix_em, unsigned E,
                                                      unsigned* __restrict__ succ, uint2* __restrict__ recA) {
    __shared__ Flags F;
    if (!hdr->ok) return;
    const int b = blockIdx.y, hw = H * W, c0 = blockIdx.x * PC, p0 = c0 + threadIdx.x * 4;
    load_flags(labels + (int64_t)b * hw, W, hw, c0, F);
    const unsigned* off = pix_off + (int64_t)b * hw;
    const unsigned char* pem = pix_em + (int64_t)b * hw;
    unsigned nb[4], em[4], tm[4];
    four_pixels(F, W, c0, nb, em, tm);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (em[j] == 0) continue;                                  // background, outside the tile, or an interior pixel
        const int p = p0 + j;
        const unsigned n = nb[j], e0 = off[p];
        unsigned k = 0;
        for (int s = 0; s < 4; ++s) {
            if (!((em[j] >> s) & 1u)) continue;
            const unsigned e = e0 + k++;
            const int l = (s + 3) & 3;
            int q = p, qs;                                         // the successor's pixel (a neighbour inside the tile) and side
            if (!at(n, dys(s), dxs(s))) {
                qs = (s + 1) & 3;                                  // right turn: the next side of p
            } else if (!at(n, dys(s) + dys(l), dxs(s) + dxs(l))) {
                q += dys(s) * W + dxs(s), qs = s;                  // straight: the same side of a
            } else {
                q += (dys(s) + dys(l)) * W + dxs(s) + dxs(l), qs = l;   // left turn: side (s + 3) % 4 of l
            }
            const unsigned qem = q == p ? em[j] : (unsigned)pem[q];
            unsigned idx = (q == p ? e0 : off[q]) + (unsigned)__popc(qem & ((1u << qs) - 1u));
            if (e >= E) continue;
            if (idx >= E) idx = e;                                 // only for labels that changed under the call
            succ[e] = idx | (((tm[j] >> s) & 1u) ? TURN : 0u);
            recA[e] = make_uint2(idx, e);
        }
    }
}

// rounds 0 .. n - 1 of a phase ran; the result is in buffer n & 1
__device__ __forceinline__ int rounds_run(const Hdr* __restrict__ hdr, int phase, int R) {
    int n = 1;
    for (int r = 0; r + 1 < R; ++r) n += hdr->chg[phase][r] != 0;
    return n;
}

__global__ void __launch_bounds__(256) pg_min_kernel(Hdr* __restrict__ hdr, int r, unsigned E, uint2* __restrict__ a0,
                                                     uint2* __restrict__ a1) {
    if (!hdr->ok || (r > 0 && hdr->chg[0][r - 1] == 0)) return;
    const uint2* src = (r & 1) ? a1 : a0;
    uint2* dst = (r & 1) ? a0 : a1;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    bool ch = false;
    if (e < E) {
        const uint2 a = src[e];
        const uint2 n = src[a.x];
        const unsigned m = min(a.y, n.y);
        ch = m != a.y;
        dst[e] = make_uint2(n.x, m);
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) hdr->chg[0][r] = 1;
}

__global__ void __launch_bounds__(256) pg_cut_kernel(Hdr* __restrict__ hdr, int R, unsigned E, int W,
                                                     const uint2* __restrict__ a0, const uint2* __restrict__ a1,
                                                     const unsigned* __restrict__ succ, const unsigned* __restrict__ einfo,
                                                     unsigned* __restrict__ lead, uint4* __restrict__ recB) {
    if (!hdr->ok) return;
    const int n = rounds_run(hdr, 0, R);
    const uint2* res = (n & 1) ? a1 : a0;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e == 0) hdr->rounds[0] = n;
    if (e >= E) return;
    const unsigned ld = res[e].y, s = succ[e], nx = s & ~TURN, info = einfo[e];
    const unsigned p = info >> 2, x = p % (unsigned)W, y = p / (unsigned)W;
    // x0 y1 - x1 y0 of the unit edge: -y heading east, x + 1 south, y + 1 west, -x north
    const unsigned side = info & 3u;
    const unsigned term = side == 0 ? 0u - y : side == 1 ? x + 1u : side == 2 ? y + 1u : 0u - x;
    lead[e] = ld;
    recB[e] = make_uint4(nx == ld ? NIL : nx, 1u, s >> 31, term);
}

__global__ void __launch_bounds__(256) pg_rank_kernel(Hdr* __restrict__ hdr, int r, unsigned E, uint4* __restrict__ b0,
                                                      uint4* __restrict__ b1) {
    if (!hdr->ok || (r > 0 && hdr->chg[1][r - 1] == 0)) return;
    const uint4* src = (r & 1) ? b1 : b0;
    uint4* dst = (r & 1) ? b0 : b1;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    bool ch = false;
    if (e < E) {
        uint4 a = src[e];
        if (a.x != NIL) {
            const uint4 n = src[a.x];
            a = make_uint4(n.x, a.y + n.y, a.z + n.z, a.w + n.w);
            ch = true;
        }
        dst[e] = a;
    }
    if (__any(ch) && (threadIdx.x & 63) == 0) hdr->chg[1][r] = 1;
}

// rings << 32 | vertices of the four edges of a thread
__device__ __forceinline__ u64 four_edges(const unsigned* __restrict__ lead, const uint4* __restrict__ res, unsigned E,
                                          unsigned e0, u64 (&v)[4]) {
    u64 s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned e = e0 + j;
        v[j] = (e < E && lead[e] == e) ? (1ull << 32) | (u64)res[e].z : 0ull;
        s += v[j];
    }
    return s;
}

__global__ void __launch_bounds__(256) pg_lcount_kernel(const Hdr* __restrict__ hdr, int R, unsigned E,
                                                        const unsigned* __restrict__ lead, const uint4* __restrict__ b0,
                                                        const uint4* __restrict__ b1, u64* __restrict__ lchunk) {
    __shared__ u64 wsum[16];
    if (!hdr->ok) return;
    const uint4* res = (rounds_run(hdr, 1, R) & 1) ? b1 : b0;
    u64 v[4], total;
    block_scan(four_edges(lead, res, E, blockIdx.x * (unsigned)EC + threadIdx.x * 4u, v), wsum, total);
    if (threadIdx.x == 0) lchunk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_T) pg_lscan_kernel(const Hdr* __restrict__ hdr, u64* __restrict__ lchunk, int nec) {
    __shared__ u64 wsum[16];
    if (!hdr->ok) return;
    u64 carry = 0;
    for (int i0 = 0; i0 < nec; i0 += SCAN_T) {
        const int i = i0 + threadIdx.x;
        u64 total;
        const u64 ex = block_scan(i < nec ? lchunk[i] : 0ull, wsum, total);
        if (i < nec) lchunk[i] = carry + ex;
        carry += total;
    }
}

// the tile whose edges hold dense index e: the last b with tile_eoff[b] <= e (empty tiles share their successor's start)
__device__ __forceinline__ int tile_holding(const long long* __restrict__ tile_eoff, int B, unsigned e) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_eoff[mid] <= (long long)e) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) pg_rings_kernel(const int32_t* __restrict__ labels, int B, int H, int W,
                                                       Hdr* __restrict__ hdr, int R, unsigned E, long long rcap,
                                                       const long long* __restrict__ tile_eoff,
                                                       const unsigned* __restrict__ lead, const unsigned* __restrict__ einfo,
                                                       const uint4* __restrict__ b0, const uint4* __restrict__ b1,
                                                       const u64* __restrict__ lchunk, unsigned* __restrict__ voff,
                                                       int64_t* __restrict__ rings, int32_t* __restrict__ ring_count) {
    __shared__ u64 wsum[16];
    __shared__ int tile_of[2];
    if (!hdr->ok) return;
    const int n = rounds_run(hdr, 1, R);
    const uint4* res = (n & 1) ? b1 : b0;
    const unsigned e0 = blockIdx.x * (unsigned)EC + threadIdx.x * 4u;
    if (e0 == 0) hdr->rounds[1] = n;
    // the tiles of the block's first and last edge: nearly every block lies in one tile, and then the block adds its rings
    // to ring_count once (85 000 single adds to one word took 0.9 ms on a 4096 x 4096 scene)
    if (threadIdx.x < 2) {
        const unsigned last = min(blockIdx.x * (unsigned)EC + (unsigned)EC, E) - 1u;
        tile_of[threadIdx.x] = tile_holding(tile_eoff, B, threadIdx.x == 0 ? blockIdx.x * (unsigned)EC : last);
    }
    u64 v[4], total;
    const u64 s = four_edges(lead, res, E, e0, v);
    u64 base = lchunk[blockIdx.x] + block_scan(s, wsum, total);       // (its barriers also publish tile_of)
    const int t0 = tile_of[0];
    const bool one_tile = t0 == tile_of[1];
    if (one_tile && threadIdx.x == 0 && (total >> 32) != 0) atomicAdd(ring_count + t0, (int)(total >> 32));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (v[j] == 0) continue;
        const unsigned e = e0 + j;
        const long long ridx = (long long)(base >> 32);
        const unsigned vo = (unsigned)(base & 0xffffffffull);
        base += v[j];
        const int b = one_tile ? t0 : tile_holding(tile_eoff, B, e);
        voff[e] = vo;
        if (!one_tile) atomicAdd(ring_count + b, 1);
        if (ridx >= rcap) continue;
        const uint4 t = res[e];
        const unsigned info = einfo[e];
        int64_t* row = rings + ridx * XV2_POLYGON_RING_COLS;
        row[0] = (int64_t)labels[(int64_t)b * H * W + (info >> 2)] - 1;
        row[1] = (int64_t)info;
        row[2] = (int64_t)t.z;
        row[3] = (int64_t)vo;
        row[4] = (int64_t)(int32_t)t.w;
        row[5] = (int64_t)t.y;
        row[6] = b;
        row[7] = 0;
    }
}

__global__ void __launch_bounds__(256) pg_verts_kernel(const Hdr* __restrict__ hdr, int R, unsigned E, long long V, int W,
                                                       const unsigned* __restrict__ succ, const unsigned* __restrict__ lead,
                                                       const unsigned* __restrict__ einfo, const unsigned* __restrict__ voff,
                                                       const uint4* __restrict__ b0, const uint4* __restrict__ b1,
                                                       int32_t* __restrict__ verts) {
    if (!hdr->ok) return;
    const uint4* res = (rounds_run(hdr, 1, R) & 1) ? b1 : b0;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= E || !(succ[e] & TURN)) return;
    const unsigned ld = lead[e];
    // turning edges from e to the ring's end, e included, taken from those of the whole ring: the ones before e
    const long long i = (long long)voff[ld] + (long long)(res[ld].z - res[e].z);
    if (i >= V) return;
    const unsigned info = einfo[e], p = info >> 2, s = info & 3u;
    const int x = (int)(p % (unsigned)W), y = (int)(p / (unsigned)W);
    // end corner: (x + 1, y) heading east, (x + 1, y + 1) south, (x, y + 1) west, (x, y) north
    verts[2 * i] = x + (s < 2);
    verts[2 * i + 1] = y + (s == 1 || s == 2);
}

bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535;
}

int rounds_for(int64_t E) {
    int R = 1;
    while (((int64_t)1 << R) < E) ++R;
    return R;
}

}  // namespace

enum { K_COUNT = 0, K_SCAN, K_TILES, K_INDEX, K_SUCC, K_MIN, K_CUT, K_RANK, K_LCOUNT, K_LSCAN, K_RINGS, K_VERTS };

static int pg_kid(int k) {
    static const int ids[] = {xv2::prof_register("pg_count_kernel"), xv2::prof_register("pg_scan_kernel"),
                              xv2::prof_register("pg_tiles_kernel"), xv2::prof_register("pg_index_kernel"),
                              xv2::prof_register("pg_succ_kernel"), xv2::prof_register("pg_min_kernel"),
                              xv2::prof_register("pg_cut_kernel"), xv2::prof_register("pg_rank_kernel"),
                              xv2::prof_register("pg_lcount_kernel"), xv2::prof_register("pg_lscan_kernel"),
                              xv2::prof_register("pg_rings_kernel"), xv2::prof_register("pg_verts_kernel")};
    return ids[k];
}

static int check_sizes(const char* what, int B, int H, int W) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B=%d H=%d W=%d must be positive", what, B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "%s: H*W=%lld exceeds 2^30 pixels per tile", what, (long long)H * W);
    XV2_CHECK_ARG(B <= 65535, "%s: B=%d too large for one launch", what, B);
    return XV2_OK;
}

extern "C" size_t xv2_polygon_count_workspace(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return 0;
    return align256(8 * (size_t)B * pchunks_of(H, W));
}

extern "C" size_t xv2_polygon_trace_workspace(int B, int H, int W, int64_t total_edges) {
    if (!sizes_ok(B, H, W) || total_edges < 0 || total_edges >= (1ll << 31)) return 0;
    return carve(nullptr, B, H, W, total_edges).bytes;
}

extern "C" int xv2_polygon_count(const int32_t* labels, int B, int H, int W, void* workspace, int64_t* counts,
                                 void* stream) {
    if (int rc = check_sizes("polygon_count", B, H, W)) return rc;
    XV2_CHECK_ARG(labels && workspace && counts, "polygon_count: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int npc = (int)pchunks_of(H, W);
    const double px = (double)B * H * W;
    u64* pchunk = static_cast<u64*>(workspace);
    XV2_LAUNCH(pg_kid(K_COUNT), px * 4, pg_count_kernel, dim3(npc, B), dim3(256), 0, st, labels, H, W, npc, pchunk);
    XV2_LAUNCH(pg_kid(K_SCAN), 16.0 * B * npc, pg_scan_kernel, dim3(B), dim3(SCAN_T), 0, st, pchunk, npc, counts);
    return XV2_OK;
}

extern "C" int xv2_polygon_trace(const int32_t* labels, int B, int H, int W, int64_t total_edges, int64_t total_vertices,
                                 void* workspace, int64_t* rings, int32_t* verts, int32_t* ring_count, int32_t* status,
                                 void* stream) {
    if (int rc = check_sizes("polygon_trace", B, H, W)) return rc;
    XV2_CHECK_ARG(total_edges >= 0 && total_edges < (1ll << 31), "polygon_trace: total_edges=%lld outside 0 .. 2^31 - 1",
                  (long long)total_edges);
    XV2_CHECK_ARG(total_vertices >= 0 && total_vertices <= total_edges,
                  "polygon_trace: total_vertices=%lld outside 0 .. total_edges=%lld", (long long)total_vertices,
                  (long long)total_edges);
    XV2_CHECK_ARG(labels && workspace && ring_count && status, "polygon_trace: null tensor");
    XV2_CHECK_ARG((total_vertices < 4 || rings) && (total_vertices == 0 || verts),
                  "polygon_trace: null rings or verts with total_vertices=%lld",
                  (long long)total_vertices);
    hipStream_t st = (hipStream_t)stream;
    const Trace t = carve(workspace, B, H, W, total_edges);
    const int npc = (int)pchunks_of(H, W);
    const double px = (double)B * H * W, ed = (double)total_edges;
    const unsigned E = (unsigned)total_edges;
    XV2_LAUNCH(pg_kid(K_COUNT), px * 4, pg_count_kernel, dim3(npc, B), dim3(256), 0, st, labels, H, W, npc, t.pchunk);
    XV2_LAUNCH(pg_kid(K_SCAN), 16.0 * B * npc, pg_scan_kernel, dim3(B), dim3(SCAN_T), 0, st, t.pchunk, npc,
               reinterpret_cast<int64_t*>(t.tile_tot));
    XV2_LAUNCH(pg_kid(K_TILES), 28.0 * B, pg_tiles_kernel, dim3(1), dim3(256), 0, st, t.tile_tot, B, (long long)total_edges,
               (long long)total_vertices, t.tile_eoff, t.hdr, ring_count, status);
    if (total_edges == 0) return XV2_OK;
    const int R = rounds_for(total_edges), nec = (int)echunks_of(total_edges);
    const unsigned eb = (E + 255u) / 256u;
    XV2_LAUNCH(pg_kid(K_INDEX), px * 9 + ed * 4, pg_index_kernel, dim3(npc, B), dim3(256), 0, st, labels, H, W, npc, t.hdr,
               t.tile_eoff, t.pchunk, E, t.pix_off, t.pix_em, t.einfo);
    XV2_LAUNCH(pg_kid(K_SUCC), px * 8 + ed * 12, pg_succ_kernel, dim3(npc, B), dim3(256), 0, st, labels, H, W, t.hdr,
               t.pix_off, t.pix_em, E, t.succ, t.recA[0]);
    for (int r = 0; r < R; ++r)
        XV2_LAUNCH(pg_kid(K_MIN), ed * 24, pg_min_kernel, dim3(eb), dim3(256), 0, st, t.hdr, r, E, t.recA[0], t.recA[1]);
    XV2_LAUNCH(pg_kid(K_CUT), ed * 36, pg_cut_kernel, dim3(eb), dim3(256), 0, st, t.hdr, R, E, W, t.recA[0], t.recA[1], t.succ,
               t.einfo, t.lead, t.recB[0]);
    for (int r = 0; r < R; ++r)
        XV2_LAUNCH(pg_kid(K_RANK), ed * 48, pg_rank_kernel, dim3(eb), dim3(256), 0, st, t.hdr, r, E, t.recB[0], t.recB[1]);
    XV2_LAUNCH(pg_kid(K_LCOUNT), ed * 8, pg_lcount_kernel, dim3(nec), dim3(256), 0, st, t.hdr, R, E, t.lead, t.recB[0],
               t.recB[1], t.lchunk);
    XV2_LAUNCH(pg_kid(K_LSCAN), 16.0 * nec, pg_lscan_kernel, dim3(1), dim3(SCAN_T), 0, st, t.hdr, t.lchunk, nec);
    XV2_LAUNCH(pg_kid(K_RINGS), ed * 8, pg_rings_kernel, dim3(nec), dim3(256), 0, st, labels, B, H, W, t.hdr, R, E,
               (long long)(total_vertices / 4), t.tile_eoff, t.lead, t.einfo, t.recB[0], t.recB[1], t.lchunk, t.voff, rings,
               ring_count);
    XV2_LAUNCH(pg_kid(K_VERTS), ed * 28, pg_verts_kernel, dim3(eb), dim3(256), 0, st, t.hdr, R, E, (long long)total_vertices, W,
               t.succ, t.lead, t.einfo, t.voff, t.recB[0], t.recB[1], verts);
    return XV2_OK;
}
