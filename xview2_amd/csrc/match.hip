// Match predicted buildings to labelled buildings by intersection over union (include/xv2.h xv2_building_match): one
// 8-column int64 row per building of either table with its best partner, I, U, the matched flag and the partner count.
//
// The observation the design rests on.  Two 4-adjacent pixels that are both foreground in the prediction lie in the same
// predicted component, and likewise in the target.  So along any 4-connected path inside the overlap mask
// (labels_p != 0) & (labels_t != 0) neither label changes: every 4-connected component of the overlap mask, a PIECE,
// belongs to exactly one (predicted building, labelled building) pair.  One pair may own several pieces (a U-shaped
// prediction over a bar has two), so |a n b| is the sum of the areas of the pair's pieces, and the number of distinct pairs
// is at most the number of pieces.  Labelling the overlap mask and tabulating it are the two existing entry points
// (xv2_label_components, xv2_building_table: root and area per piece, the true piece count); what is new here is grouping
// the pieces by pair and the reduction per building.
//
// Why 2 * iou_num >= iou_den.  With a threshold of at least 1/2 a pair that passes has I >= U / 2 >= max(|a|, |b|) / 2,
// and more than half of both areas as soon as I / U > 1/2.  The partners of one building are disjoint, so no building has
// two partners above 1/2 and each such pair is the best of both its members: the matched set is the same under every
// matching rule in use (greedy by score, Hungarian, mutual best), and no ordering of the predictions enters.  (Two passing
// partners at I / U = 1/2 exactly would each be half of the building, lie inside it and tile it, so they would touch and be
// one component: with tables that are the labels' own, a pair that passes is always mutual.  The mutual test decides only
// when a table comes from another map, and then the root tie rule picks one.)  Below 1/2 the rules differ, and none is
// made up here.
//
// What was built (fourteen launches whatever B, H, W and content; nothing is read back):
//   mt_overlap_kernel       the overlap mask, uint8, into the workspace
//   xv2_label_components    (3 launches) the pieces' labels
//   xv2_building_table      (5 launches) piece_count and one row (root, area) per piece of rank < max_pieces
//   mt_init_kernel          pair table: keys empty, sums 0; every match row that will be written: partner -1, best-partner
//                           word empty (column 5 while the entry runs)
//   mt_insert_kernel        one thread per piece: the two labels at the piece's root -> the two table ranks -> the key
//                           (rank_p << 32 | rank_t) into the tile's open-addressing table with a 64-bit CAS, the area added
//                           to the slot's sum; the thread that created the slot adds 1 to both buildings' partner counts
//   mt_offer_kernel         one thread per slot, a launch later so the sums are final: (I << 32 | partner rank) offered to
//                           both buildings' best-partner words; a CAS replaces the holder only when the exact comparison
//                           I1 * U2 vs I2 * U1 (int64), then the smaller partner root, says "better"
//   mt_resolve_kernel       one thread per building: mutuality, the threshold, columns 0..3
//   mt_tidy_kernel          column 5 back to 0 (its own launch: mt_resolve_kernel reads the words of OTHER buildings, so
//                           no thread of it may overwrite its own)
// A label's rank is found by bisection over column 0 of its table (ascending, as xv2_building_table writes it) instead of
// through a per-pixel rank map: it runs once per piece, needs no 4-byte-per-pixel maps and reads no uninitialised word.
// The per-building scratch (partner count, best-partner word) lives in the building's own output row, so the workspace
// does not depend on max_rows.
//
// Atomic traffic.  The per-pixel work is aggregated on chip before it gets here (the piece table's LDS tallies), so the
// global atomics of this file are per PIECE (a compare-and-swap, an add, and two more adds for a pair's first piece) and per
// PAIR (two offers): thousands per scene, not millions.  Only a building with thousands of partners (the checkerboard
// tests) makes many of them meet on one word.
//
// Determinism.  Slot positions depend on arrival order, nothing read from a slot does: a slot's sum is an integer add, a
// partner count an integer add, and a best-partner word ends as the maximum of a total order over the offers, whichever
// order the compare-and-swaps land in.  All global atomics are agent-scope relaxed integer atomics; launch boundaries are
// the only cross-block synchronisation.
//
// Bounds.  A label whose root is outside the tile or is no column 0 of a row 0 .. min(count, max_rows) - 1, or whose row
// has an area outside 1 .. H * W, is dropped.  Pieces of rank >= max_pieces are not inserted, so the pair table (a power
// of two >= 2 * max_pieces slots per tile) is at most half full and a probe sequence always ends; it is bounded by the
// table size all the same, as is the number of compare-and-swap retries (every failure is another offer's success, and
// there are no more offers than slots).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

constexpr int RG = 64;   // region edge of postproc.hip (its size limits are kept)
constexpr unsigned long long EMPTY = ~0ull;

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ u64 ld64(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// true when *p went from expect to want; expect takes the value found otherwise
__device__ __forceinline__ bool cas64(u64* p, u64& expect, u64 want) {
    return __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add64(u64* p, u64 v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int rows_of(const int32_t* __restrict__ count, int b, int max_rows) {
    const int c = count[b];
    return c < 0 ? 0 : c < max_rows ? c : max_rows;
}

__global__ void __launch_bounds__(256)
mt_overlap_kernel(const int32_t* __restrict__ lp, const int32_t* __restrict__ lt, int64_t hw,
                  uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, p = (int64_t)blockIdx.y * hw + i;
    if (i < hw) mask[p] = (uint8_t)(lp[p] != 0 && lt[p] != 0);
}

// blockIdx.z: 0 the prediction's rows, 1 the target's, 2 the pair table
__global__ void __launch_bounds__(256)
mt_init_kernel(const int32_t* __restrict__ count_p, int max_rows_p, int64_t* __restrict__ match_p,
               const int32_t* __restrict__ count_t, int max_rows_t, int64_t* __restrict__ match_t,
               u64* __restrict__ keys, u64* __restrict__ sums, int64_t slots) {
    const int side = blockIdx.z, b = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (side == 2) {
        if (r < slots) {
            keys[(int64_t)b * slots + r] = EMPTY;
            sums[(int64_t)b * slots + r] = 0;
        }
        return;
    }
    const int max_rows = side ? max_rows_t : max_rows_p;
    if (r >= rows_of(side ? count_t : count_p, b, max_rows)) return;
    int64_t* m = (side ? match_t : match_p) + ((int64_t)b * max_rows + r) * XV2_MATCH_COLS;
#pragma unroll
    for (int j = 0; j < XV2_MATCH_COLS; ++j) m[j] = (j == 0 || j == 5) ? -1 : 0;
}

// rank of the row whose column 0 is label - 1 among the n rows of a tile's table (ascending column 0), or -1
__device__ __forceinline__ int rank_of(const int64_t* __restrict__ rows, int n, int label, int64_t hw) {
    const int64_t root = (int64_t)label - 1;
    if (root < 0 || root >= hw) return -1;
    int lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rows[(int64_t)mid * XV2_BUILDING_COLS] < root) lo = mid + 1; else hi = mid;
    }
    if (lo >= n || rows[(int64_t)lo * XV2_BUILDING_COLS] != root) return -1;
    const int64_t area = rows[(int64_t)lo * XV2_BUILDING_COLS + 1];
    return (area >= 1 && area <= hw) ? lo : -1;
}

__global__ void __launch_bounds__(256)
mt_insert_kernel(const int32_t* __restrict__ labels_p, const int64_t* __restrict__ rows_p,
                 const int32_t* __restrict__ count_p, int max_rows_p,
                 const int32_t* __restrict__ labels_t, const int64_t* __restrict__ rows_t,
                 const int32_t* __restrict__ count_t, int max_rows_t, int64_t hw,
                 const int64_t* __restrict__ pieces, const int32_t* __restrict__ piece_count,
                 int cap, int log2s, u64* __restrict__ keys, u64* __restrict__ sums,
                 int64_t* __restrict__ match_p, int64_t* __restrict__ match_t) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_of(piece_count, b, cap)) return;
    const int64_t* piece = pieces + ((int64_t)b * cap + i) * XV2_BUILDING_COLS;
    const int64_t root = piece[0], area = piece[1];
    if (root < 0 || root >= hw || area < 1 || area > hw) return;
    const int64_t* tp = rows_p + (int64_t)b * max_rows_p * XV2_BUILDING_COLS;
    const int64_t* tt = rows_t + (int64_t)b * max_rows_t * XV2_BUILDING_COLS;
    const int rp = rank_of(tp, rows_of(count_p, b, max_rows_p), labels_p[(int64_t)b * hw + root], hw);
    const int rt = rank_of(tt, rows_of(count_t, b, max_rows_t), labels_t[(int64_t)b * hw + root], hw);
    if (rp < 0 || rt < 0) return;
    const u64 key = ((u64)(unsigned)rp << 32) | (unsigned)rt;
    const int64_t slots = (int64_t)1 << log2s;
    u64* k = keys + (int64_t)b * slots;
    u64* s = sums + (int64_t)b * slots;
    int64_t h = (int64_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2s));
    for (int64_t probe = 0; probe < slots; ++probe) {
        u64 found = EMPTY;
        const bool created = cas64(&k[h], found, key);
        if (created || found == key) {
            add64(&s[h], (u64)area);
            if (created) {
                add64(reinterpret_cast<u64*>(match_p + ((int64_t)b * max_rows_p + rp) * XV2_MATCH_COLS + 4), 1);
                add64(reinterpret_cast<u64*>(match_t + ((int64_t)b * max_rows_t + rt) * XV2_MATCH_COLS + 4), 1);
            }
            return;
        }
        h = (h + 1) & (slots - 1);
    }
}

// Offer partner `rank` (root `root`, area `area`) with intersection I to the building of area `own` whose best-partner word
// is *word.  The order: larger I / U first (exact cross products; |I * U| < 2^61), then the smaller partner root, then the
// smaller rank (only a table with repeated roots gets that far).
__device__ __forceinline__ void offer(u64* word, i64 own, const int64_t* __restrict__ other, i64 I, int rank,
                                      int64_t retries) {
    const i64 root = other[(int64_t)rank * XV2_BUILDING_COLS], U = own + other[(int64_t)rank * XV2_BUILDING_COLS + 1] - I;
    const u64 mine = ((u64)I << 32) | (unsigned)rank;
    u64 cur = ld64(word);
    for (int64_t it = 0; it <= retries; ++it) {
        if (cur != EMPTY) {
            const int crank = (int)(unsigned)cur;
            const i64 cI = (i64)(cur >> 32), croot = other[(int64_t)crank * XV2_BUILDING_COLS];
            const i64 cU = own + other[(int64_t)crank * XV2_BUILDING_COLS + 1] - cI;
            const i64 l = I * cU, r = cI * U;
            const bool better = l != r ? l > r : root != croot ? root < croot : rank < crank;
            if (!better) return;
        }
        if (cas64(word, cur, mine)) return;
    }
}

__global__ void __launch_bounds__(256)
mt_offer_kernel(const int64_t* __restrict__ rows_p, int max_rows_p,
                const int64_t* __restrict__ rows_t, int max_rows_t, int log2s,
                const u64* __restrict__ keys, const u64* __restrict__ sums,
                int64_t* __restrict__ match_p, int64_t* __restrict__ match_t) {
    const int b = blockIdx.y;
    const int64_t slots = (int64_t)1 << log2s, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const u64 key = keys[(int64_t)b * slots + i];
    if (key == EMPTY) return;
    const int rp = (int)(key >> 32), rt = (int)(unsigned)key;
    const i64 I = (i64)sums[(int64_t)b * slots + i];
    const int64_t* tp = rows_p + (int64_t)b * max_rows_p * XV2_BUILDING_COLS;
    const int64_t* tt = rows_t + (int64_t)b * max_rows_t * XV2_BUILDING_COLS;
    int64_t* mp = match_p + ((int64_t)b * max_rows_p + rp) * XV2_MATCH_COLS;
    int64_t* mt = match_t + ((int64_t)b * max_rows_t + rt) * XV2_MATCH_COLS;
    offer(reinterpret_cast<u64*>(mp + 5), tp[(int64_t)rp * XV2_BUILDING_COLS + 1], tt, I, rt, slots);
    offer(reinterpret_cast<u64*>(mt + 5), tt[(int64_t)rt * XV2_BUILDING_COLS + 1], tp, I, rp, slots);
}

// columns 0..3 of every written row; column 5 (everybody's best-partner word) is only read here
__global__ void __launch_bounds__(256)
mt_resolve_kernel(const int64_t* __restrict__ rows_p, const int32_t* __restrict__ count_p,
                  int max_rows_p, const int64_t* __restrict__ rows_t,
                  const int32_t* __restrict__ count_t, int max_rows_t, int iou_num, int iou_den,
                  int64_t* __restrict__ match_p, int64_t* __restrict__ match_t) {
    const int side = blockIdx.z, b = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int max_rows = side ? max_rows_t : max_rows_p, max_other = side ? max_rows_p : max_rows_t;
    if (r >= rows_of(side ? count_t : count_p, b, max_rows)) return;
    const int64_t* own = (side ? rows_t : rows_p) + ((int64_t)b * max_rows + r) * XV2_BUILDING_COLS;
    const int64_t* other = (side ? rows_p : rows_t) + (int64_t)b * max_other * XV2_BUILDING_COLS;
    int64_t* m = (side ? match_t : match_p) + ((int64_t)b * max_rows + r) * XV2_MATCH_COLS;
    const int64_t* mo = (side ? match_p : match_t) + (int64_t)b * max_other * XV2_MATCH_COLS;
    const u64 w = (u64)m[5];
    if (w == EMPTY) {
        m[2] = own[1];   // columns 0, 1, 3 are as mt_init_kernel left them: -1, 0, 0
        return;
    }
    const int partner = (int)(unsigned)w;
    const i64 I = (i64)(w >> 32), U = own[1] + other[(int64_t)partner * XV2_BUILDING_COLS + 1] - I;
    const u64 wo = (u64)mo[(int64_t)partner * XV2_MATCH_COLS + 5];
    const bool mutual = wo != EMPTY && (int64_t)(unsigned)wo == r;
    m[0] = partner;
    m[1] = I;
    m[2] = U;
    m[3] = (mutual && I * iou_den >= (i64)iou_num * U) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
mt_tidy_kernel(const int32_t* __restrict__ count_p, int max_rows_p, int64_t* __restrict__ match_p,
               const int32_t* __restrict__ count_t, int max_rows_t, int64_t* __restrict__ match_t) {
    const int side = blockIdx.z, b = blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int max_rows = side ? max_rows_t : max_rows_p;
    if (r >= rows_of(side ? count_t : count_p, b, max_rows)) return;
    (side ? match_t : match_p)[((int64_t)b * max_rows + r) * XV2_MATCH_COLS + 5] = 0;
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool sizes_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 30) && B <= 65535 && (H + RG - 1) / RG <= 65535;
}

// a tile has at most ceil(H * W / 2) pieces (no two are 4-adjacent), so a larger max_pieces buys nothing
int piece_cap(int H, int W, int max_pieces) {
    const int64_t most = ((int64_t)H * W + 1) / 2;
    return (int)(max_pieces < most ? max_pieces : most);
}

int log2_slots(int cap) {
    int l = 1;
    while (((int64_t)1 << l) < 2 * (int64_t)cap) ++l;
    return l;
}

}  // namespace

static int mt_kid(int k) {
    static const int ids[] = {xv2::prof_register("mt_overlap_kernel"), xv2::prof_register("mt_init_kernel"),
                              xv2::prof_register("mt_insert_kernel"),  xv2::prof_register("mt_offer_kernel"),
                              xv2::prof_register("mt_resolve_kernel"), xv2::prof_register("mt_tidy_kernel")};
    return ids[k];
}

extern "C" size_t xv2_building_match_workspace(int B, int H, int W, int max_pieces) {
    if (!sizes_ok(B, H, W) || max_pieces < 1) return 0;
    const size_t n = (size_t)B * H * W, cap = (size_t)piece_cap(H, W, max_pieces), slots = (size_t)1 << log2_slots((int)cap);
    // overlap mask (uint8 per pixel) | piece labels (int32 per pixel) | the piece table's own workspace | piece rows
    // (int64 [B][cap][16]) | pair keys, pair sums (uint64 [B][slots] each)
    return align256(n) + align256(4 * n) + align256(xv2_building_table_workspace(B, H, W)) +
           align256(8 * (size_t)B * cap * XV2_BUILDING_COLS) + 2 * align256(8 * (size_t)B * slots);
}

extern "C" int xv2_building_match(const int32_t* labels_p, const int64_t* rows_p, const int32_t* count_p, int max_rows_p,
                                  const int32_t* labels_t, const int64_t* rows_t, const int32_t* count_t, int max_rows_t,
                                  int B, int H, int W, int iou_num, int iou_den, int max_pieces, void* workspace,
                                  int64_t* match_p, int64_t* match_t, int32_t* piece_count, void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "building_match: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "building_match: H*W=%lld exceeds 2^30 pixels per tile", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535 && (H + RG - 1) / RG <= 65535, "building_match: B=%d or H=%d too large for one launch", B, H);
    XV2_CHECK_ARG(max_rows_p >= 1 && max_rows_t >= 1, "building_match: max_rows_p=%d and max_rows_t=%d must be at least 1",
                  max_rows_p, max_rows_t);
    XV2_CHECK_ARG(max_pieces >= 1, "building_match: max_pieces=%d must be at least 1", max_pieces);
    XV2_CHECK_ARG(1 <= iou_num && iou_num <= iou_den && iou_den <= 65536,
                  "building_match: threshold %d/%d must satisfy 1 <= iou_num <= iou_den <= 65536", iou_num, iou_den);
    XV2_CHECK_ARG(2 * (int64_t)iou_num >= iou_den,
                  "building_match: threshold %d/%d is below 1/2, where the matching rules in use disagree", iou_num, iou_den);
    XV2_CHECK_ARG(labels_p && rows_p && count_p && labels_t && rows_t && count_t && workspace && match_p && match_t &&
                      piece_count, "building_match: null tensor");
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const size_t n = (size_t)B * hw;
    const int cap = piece_cap(H, W, max_pieces), log2s = log2_slots(cap);
    const int64_t slots = (int64_t)1 << log2s;
    char* ws = static_cast<char*>(workspace);
    uint8_t* mask = reinterpret_cast<uint8_t*>(ws);
    ws += align256(n);
    int32_t* plabels = reinterpret_cast<int32_t*>(ws);
    ws += align256(4 * n);
    void* table_ws = ws;
    ws += align256(xv2_building_table_workspace(B, H, W));
    int64_t* pieces = reinterpret_cast<int64_t*>(ws);
    ws += align256(8 * (size_t)B * cap * XV2_BUILDING_COLS);
    u64* keys = reinterpret_cast<u64*>(ws);
    u64* sums = reinterpret_cast<u64*>(ws + align256(8 * (size_t)B * slots));

    const dim3 blk(256), per_pixel((unsigned)xv2::cdiv(hw, 256), B), per_slot((unsigned)xv2::cdiv(slots, 256), B);
    XV2_LAUNCH(mt_kid(0), 9.0 * n, mt_overlap_kernel, per_pixel, blk, 0, st, labels_p, labels_t, hw, mask);
    if (int rc = xv2_label_components(mask, B, H, W, nullptr, plabels, stream)) return rc;
    // the mask doubles as the damage map (every piece pixel is class 1); only columns 0 and 1 of a piece's row are used
    if (int rc = xv2_building_table(plabels, mask, nullptr, B, H, W, cap, table_ws, pieces, piece_count, stream)) return rc;
    // max_rows has no upper bound: the block count of the per-row launches is formed in 64 bits (at most 2^23 blocks)
    const int64_t row_blocks = xv2::cdiv((int64_t)(max_rows_p > max_rows_t ? max_rows_p : max_rows_t), 256);
    const int64_t slot_blocks = xv2::cdiv(slots, 256);
    const dim3 per_row((unsigned)row_blocks, B, 2);
    const dim3 init((unsigned)(row_blocks > slot_blocks ? row_blocks : slot_blocks), B, 3);
    const double row_bytes = 64.0 * B * ((double)max_rows_p + max_rows_t);
    XV2_LAUNCH(mt_kid(1), row_bytes + 16.0 * B * slots, mt_init_kernel, init, blk, 0, st, count_p, max_rows_p, match_p, count_t,
               max_rows_t, match_t, keys, sums, slots);
    XV2_LAUNCH(mt_kid(2), 64.0 * B * cap, mt_insert_kernel, dim3((cap + 255) / 256, B), blk, 0, st, labels_p, rows_p, count_p,
               max_rows_p, labels_t, rows_t, count_t, max_rows_t, hw, pieces, piece_count, cap, log2s, keys, sums, match_p,
               match_t);
    XV2_LAUNCH(mt_kid(3), 16.0 * B * slots, mt_offer_kernel, per_slot, blk, 0, st, rows_p, max_rows_p, rows_t, max_rows_t,
               log2s, keys, sums, match_p, match_t);
    XV2_LAUNCH(mt_kid(4), row_bytes, mt_resolve_kernel, per_row, blk, 0, st, rows_p, count_p, max_rows_p, rows_t, count_t,
               max_rows_t, iou_num, iou_den, match_p, match_t);
    XV2_LAUNCH(mt_kid(5), row_bytes / 8, mt_tidy_kernel, per_row, blk, 0, st, count_p, max_rows_p, match_p, count_t, max_rows_t,
               match_t);
    return XV2_OK;
}
