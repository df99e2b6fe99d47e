// Per-building table of a labelled prediction (include/xv2.h xv2_building_table): one 16-column int64 row per
// 4-connected component of a label map as xv2_label_components writes it (label = 1 + the smallest in-tile linear index
// of the component), rows in ascending order of that index, which is scipy.ndimage.label's numbering.
//
// Every column is an integer and every reduction an integer add, min or max, so the table has the same bits on every
// run and in any launch order.  Launch boundaries are the only cross-block synchronisation; nothing is read back.
//
// Launch sequence (five launches whatever B, H, W):
//   bt_count_kernel   roots (labels[p] == p + 1) per chunk of CHUNK consecutive pixels of the flattened tile
//   bt_scan_kernel    exclusive scan of a tile's chunk counts in place (one block per tile, looping), total -> count[b]
//   bt_rank_kernel    every root takes its rank (chunk offset + roots before it in the chunk), writes it at its own
//                     position of the rank map and, when rank < max_rows, initialises its row
//   bt_accum_kernel   one RW x RH region per block: per-root tallies in an LDS hash table, then one global integer
//                     atomic per non-zero field of every root the block met
//   bt_finish_kernel  column 13 (the voted class) of every written row
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

constexpr int CHUNK = 4096;            // pixels per chunk of the rank passes: 4 waves x 16 steps x 64 lanes
constexpr int STEPS = CHUNK / 256;
constexpr int RW = 64, RH = 32;        // region of bt_accum_kernel: a wave reads 64 consecutive pixels of a row
constexpr int RPT = RW * RH / 256;     // rows per thread
// Pixels of different components are never 4-adjacent, so the roots that meet a region form an independent set of its
// grid graph: at most RW * RH / 2 (a checkerboard).  The table holds exactly that many; 13 words per slot = 52 KB.
constexpr int HT = RW * RH / 2;
constexpr unsigned EMPTY = 0xffffffffu;
constexpr int SCAN_T = 1024;
constexpr int RG = 64;                 // region edge of postproc.hip (its size limits are kept)

typedef long long i64;

__device__ __forceinline__ void g_add(int64_t* p, i64 v) {
    __hip_atomic_fetch_add(reinterpret_cast<i64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_min(int64_t* p, i64 v) {
    __hip_atomic_fetch_min(reinterpret_cast<i64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void g_max(int64_t* p, i64 v) {
    __hip_atomic_fetch_max(reinterpret_cast<i64*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// q(v): clamp (NaN -> 0), ONE multiplication, round to nearest even; no a * b + c for the compiler to contract
__device__ __forceinline__ int quant(float v) {
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    return __float2int_rn(c * 65535.f);
}

// root flags of the 64 pixels a wave looks at in step k of its chunk (flat order: chunk, wave, step, lane)
__device__ __forceinline__ unsigned long long root_mask(const int32_t* __restrict__ lab, int64_t hw, int64_t p) {
    return __ballot(p < hw && lab[p] == (int32_t)(p + 1));
}

__global__ void __launch_bounds__(256) bt_count_kernel(const int32_t* __restrict__ labels, int64_t hw, int nchunks,
                                                       unsigned* __restrict__ chunk_cnt) {
    __shared__ unsigned wt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int32_t* lab = labels + (int64_t)b * hw;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK + wave * (CHUNK / 4) + lane;
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) n += (unsigned)__popcll(root_mask(lab, hw, p0 + k * 64));
    if (lane == 0) wt[wave] = n;
    __syncthreads();
    if (tid == 0) chunk_cnt[(int64_t)b * nchunks + blockIdx.x] = wt[0] + wt[1] + wt[2] + wt[3];
}

// exclusive scan in place, SCAN_T chunk counts per round with a running carry (a tile of 2^30 pixels has 2^18 chunks)
__global__ void __launch_bounds__(SCAN_T) bt_scan_kernel(unsigned* __restrict__ chunk_cnt, int nchunks,
                                                         int32_t* __restrict__ count) {
    __shared__ unsigned wsum[SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    unsigned* c = chunk_cnt + (int64_t)b * nchunks;
    unsigned carry = 0;
    for (int i0 = 0; i0 < nchunks; i0 += SCAN_T) {
        const int i = i0 + tid;
        const unsigned v = i < nchunks ? c[i] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCAN_T / 64; ++w) {
            const unsigned s = wsum[w];
            before += w < wave ? s : 0u;
            total += s;
        }
        if (i < nchunks) c[i] = carry + before + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) count[b] = (int32_t)carry;
}

__global__ void __launch_bounds__(256) bt_rank_kernel(const int32_t* __restrict__ labels, int64_t hw, int nchunks,
                                                      const unsigned* __restrict__ chunk_off, int max_rows,
                                                      unsigned* __restrict__ rank_map, int64_t* __restrict__ rows) {
    __shared__ unsigned wt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const int32_t* lab = labels + (int64_t)b * hw;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK + wave * (CHUNK / 4) + lane;
    unsigned long long m[STEPS];
    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        m[k] = root_mask(lab, hw, p0 + k * 64);
        n += (unsigned)__popcll(m[k]);
    }
    if (lane == 0) wt[wave] = n;
    __syncthreads();
    unsigned off = chunk_off[(int64_t)b * nchunks + blockIdx.x];
    for (int w = 0; w < wave; ++w) off += wt[w];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        if ((m[k] >> lane) & 1ull) {
            const int64_t p = p0 + k * 64;
            const unsigned rank = off + (unsigned)__popcll(m[k] & below);
            rank_map[(int64_t)b * hw + p] = rank;
            if (rank < (unsigned)max_rows) {
                // col 0 and the identities of min / max; the sums start at 0
                int64_t* row = rows + ((int64_t)b * max_rows + rank) * XV2_BUILDING_COLS;
#pragma unroll
                for (int j = 0; j < XV2_BUILDING_COLS; ++j)
                    row[j] = j == 0 ? p : (j == 2 || j == 3) ? (int64_t)1 << 40 : (j == 4 || j == 5) ? -1 : 0;
            }
        }
        off += (unsigned)__popcll(m[k]);
    }
}

// LDS tally of one root within a region, region-local coordinates (sums stay below 2^32: sy <= 31 * 2048,
// sx <= 63 * 2048, q <= 65535 * 2048)
enum { F_YMIN = 0, F_XMIN, F_YMAX, F_XMAX, F_SY, F_SX, F_N1, F_N2, F_N3, F_N4, F_NO, F_Q, NF };

__global__ void __launch_bounds__(256) bt_accum_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ dmg,
                                                       const float* __restrict__ loc, int H, int W, int rx, int max_rows,
                                                       const unsigned* __restrict__ rank_map, int64_t* __restrict__ rows) {
    __shared__ unsigned keys[HT];
    __shared__ unsigned f[NF][HT];
    const int tid = threadIdx.x, lx = tid & (RW - 1), ly0 = tid >> 6;
    const int bx = blockIdx.x % rx, by = blockIdx.x / rx, b = blockIdx.y;
    const int x0 = bx * RW, y0 = by * RH;
    const int64_t hw = (int64_t)H * W, base = (int64_t)b * hw;
    for (int i = tid; i < HT; i += 256) {
        keys[i] = EMPTY;
#pragma unroll
        for (int j = 0; j < NF; ++j) f[j][i] = (j == F_YMIN || j == F_XMIN) ? 0xffffu : 0u;
    }
    __syncthreads();
    const int x = x0 + lx;
#pragma unroll 2
    for (int k = 0; k < RPT; ++k) {
        const int ly = ly0 + 4 * k, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int64_t p = base + (int64_t)y * W + x;
        const int l = labels[p];
        if (l == 0) continue;
        const unsigned key = (unsigned)(l - 1);
        const unsigned d = dmg[p];
        const unsigned qv = loc ? (unsigned)quant(loc[p]) : 0u;
        unsigned h = (key * 2654435761u) >> 22;   // 10-bit slot
        // the table has a slot for every root that can meet the region, so a probe sequence of HT slots always ends
        // on the key or on a free slot; the bound only matters for a label map that is no labelling at all
        for (int probe = 0; probe < HT; ++probe) {
            const unsigned old = atomicCAS(&keys[h], EMPTY, key);
            if (old == EMPTY || old == key) {
                atomicMin(&f[F_YMIN][h], (unsigned)ly);
                atomicMin(&f[F_XMIN][h], (unsigned)lx);
                atomicMax(&f[F_YMAX][h], (unsigned)ly);
                atomicMax(&f[F_XMAX][h], (unsigned)lx);
                atomicAdd(&f[F_SY][h], (unsigned)ly);
                atomicAdd(&f[F_SX][h], (unsigned)lx);
                atomicAdd(&f[(d >= 1 && d <= 4) ? F_N1 + (int)d - 1 : F_NO][h], 1u);
                if (qv) atomicAdd(&f[F_Q][h], qv);
                break;
            }
            h = (h + 1) & (HT - 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < HT; i += 256) {
        const unsigned root = keys[i];
        if (root == EMPTY) continue;
        // only a root's position of the rank map was ever written: a label that names no root is dropped
        if ((int64_t)root >= hw || labels[base + root] != (int32_t)(root + 1)) continue;
        const unsigned rank = rank_map[base + root];
        if (rank >= (unsigned)max_rows) continue;
        int64_t* row = rows + ((int64_t)b * max_rows + rank) * XV2_BUILDING_COLS;
        const i64 n1 = f[F_N1][i], n2 = f[F_N2][i], n3 = f[F_N3][i], n4 = f[F_N4][i], no = f[F_NO][i];
        const i64 area = n1 + n2 + n3 + n4 + no;
        g_add(row + 1, area);
        g_min(row + 2, (i64)y0 + f[F_YMIN][i]);
        g_min(row + 3, (i64)x0 + f[F_XMIN][i]);
        g_max(row + 4, (i64)y0 + f[F_YMAX][i]);
        g_max(row + 5, (i64)x0 + f[F_XMAX][i]);
        // 64 bits from here: the sum of y over one component passes 2^32 from about 2100 x 2100 pixels
        const i64 sy = (i64)f[F_SY][i] + area * y0, sx = (i64)f[F_SX][i] + area * x0;
        if (sy) g_add(row + 6, sy);
        if (sx) g_add(row + 7, sx);
        if (n1) g_add(row + 8, n1);
        if (n2) g_add(row + 9, n2);
        if (n3) g_add(row + 10, n3);
        if (n4) g_add(row + 11, n4);
        if (no) g_add(row + 12, no);
        if (f[F_Q][i]) g_add(row + 14, (i64)f[F_Q][i]);
    }
}

// the vote of pp_vote_kernel: the class with the most pixels, ties to the smaller class, 0 without any class pixel
__global__ void __launch_bounds__(256) bt_finish_kernel(int64_t* __restrict__ rows, const int32_t* __restrict__ count,
                                                        int max_rows) {
    const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    if (r >= max_rows || r >= count[b]) return;
    int64_t* row = rows + ((int64_t)b * max_rows + r) * XV2_BUILDING_COLS;
    int64_t m = 0, cls = 0;
#pragma unroll
    for (int c = 1; c <= 4; ++c)
        if (row[7 + c] > m) { m = row[7 + c]; cls = c; }
    row[13] = cls;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
int64_t chunks_of(int H, int W) { return ((int64_t)H * W + CHUNK - 1) / CHUNK; }

}  // namespace

static int bt_kid(int k) {
    static const int ids[] = {xv2::prof_register("bt_count_kernel"), xv2::prof_register("bt_scan_kernel"),
                              xv2::prof_register("bt_rank_kernel"), xv2::prof_register("bt_accum_kernel"),
                              xv2::prof_register("bt_finish_kernel")};
    return ids[k];
}

static bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535 && (H + RG - 1) / RG <= 65535;
}

extern "C" size_t xv2_building_table_workspace(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return 0;
    // rank map (uint32 per pixel, root positions only) | chunk counts / offsets (uint32 per chunk)
    return align256(4 * (size_t)B * H * W) + align256(4 * (size_t)B * chunks_of(H, W));
}

extern "C" int xv2_building_table(const int32_t* labels, const uint8_t* dmg, const float* loc, int B, int H, int W,
                                  int max_rows, void* workspace, int64_t* rows, int32_t* count, void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "building_table: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "building_table: H*W=%lld exceeds 2^30 pixels per tile", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + RG - 1) / RG <= 65535, "building_table: B=%d or H=%d too large for one launch", B, H);
    XV2_CHECK_ARG(max_rows >= 1, "building_table: max_rows=%d must be at least 1", max_rows);
    XV2_CHECK_ARG(labels && dmg && workspace && rows && count, "building_table: null tensor (only loc may be NULL)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const int nchunks = (int)chunks_of(H, W);
    char* ws = static_cast<char*>(workspace);
    unsigned* rank_map = reinterpret_cast<unsigned*>(ws);
    unsigned* chunk_cnt = reinterpret_cast<unsigned*>(ws + align256(4 * (size_t)B * hw));
    const int rx = (W + RW - 1) / RW, ry = (H + RH - 1) / RH;
    const double px = (double)B * hw;
    XV2_LAUNCH(bt_kid(0), px * 4, bt_count_kernel, dim3(nchunks, B), dim3(256), 0, st, labels, hw, nchunks, chunk_cnt);
    XV2_LAUNCH(bt_kid(1), 8.0 * B * nchunks, bt_scan_kernel, dim3(B), dim3(SCAN_T), 0, st, chunk_cnt, nchunks, count);
    XV2_LAUNCH(bt_kid(2), px * 4, bt_rank_kernel, dim3(nchunks, B), dim3(256), 0, st, labels, hw, nchunks, chunk_cnt,
               max_rows, rank_map, rows);
    XV2_LAUNCH(bt_kid(3), px * (loc ? 9 : 5), bt_accum_kernel, dim3((unsigned)rx * ry, B), dim3(256), 0, st, labels, dmg, loc,
               H, W, rx, max_rows, rank_map, rows);
    XV2_LAUNCH(bt_kid(4), 48.0 * B * max_rows, bt_finish_kernel, dim3((max_rows + 255) / 256, B), dim3(256), 0, st, rows, count,
               max_rows);
    return XV2_OK;
}
