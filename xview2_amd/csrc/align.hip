// Registering the post scene to the pre scene by an integer translation (include/xv2.h, "register the post image"):
// luma, a table of sums of absolute differences over every shift of a square search window, the best shift of every
// tile and of the whole scene, and the reflecting resampler that applies a shift.  All integer work with a unique result.
//
// al_sad_kernel, one 256-thread block per tile (by, bx) of image b, grid (nby * nbx, B).  The block converts its pre tile
// (T x T) and its post halo ((T + 2R)^2) to luma once, four pixels per thread and store, into LDS as packed bytes: pre rows
// of T + 16 bytes (16-byte aligned for ds_read_b128), post rows of PSW words, at least (T + 2R) / 4 + 2.  Positions outside
// the tile (partial edge tiles) and past the halo hold 0.  The halo's column 0 is the tile's column 0 at dx = -R, so a word
// of pre at tile word j meets, for the four shifts dx + R = 4q .. 4q + 3, the eight post bytes of the words j + q and
// j + q + 1: always word-aligned.
// Work units are (band, dy, quad q of dx) with q fastest: a thread walks the rows band, band + nb, ... of the tile, and along
// a row the words of pre (one ds_read_b128 per four words, the same address in every lane of a band: a broadcast) against the
// words of post; it keeps the previous post word and reads the next one - one LDS word per four pixels and four shifts - and
// v_qsad_pk_u16_u8 adds the four sums of absolute differences to four packed 16-bit lanes.  A lane takes at most 4 * 255 per
// instruction, so after 64 instructions (256 / T rows of T / 4 words) the lanes are widened into four 32-bit sums and cleared;
// the instructions alternate between two such accumulators, so that one does not wait for the result of the one before it.
// Lanes of a wave with neighbouring q read neighbouring words, lanes with neighbouring dy words PSW apart: the host pads PSW
// by up to 8 words where that takes bank conflicts out of the read (bank_cost) and 64 KiB of LDS allow it.
// The ragged right edge of a partial tile is the last group of four words of a row.  There the quad's four shifts are taken
// one by one: v_alignbyte_b32 of the two post words by 0..3 bytes, ANDed with a byte mask of the valid columns (the masks are
// wave-uniform; pre holds 0 there, so those bytes add |0 - 0|), and v_sad_u8 into the 32-bit sums.  Rows past the tile's
// last are not visited.  D is odd, so the last quad of a row of shifts is not full: its surplus sums are dropped.
// nb > 1 (small D, to give every thread work): the band sums meet in LDS and the thread that owns shift d adds them in
// band order and stores S_b(d); nb = 1: the thread that walked the tile stores it.  Every S_b(d) has one plain store.  The
// tile's best shift is a block-wide minimum of the 64-bit key S << 26 | (dy^2 + dx^2) << 14 | (dy + R) << 7 | (dx + R).
//
// al_chunk_kernel adds S_b(d) over chunks of 32 tiles into the workspace (int64), al_total_kernel adds the chunks in order,
// stores S(d) and takes the minimum of the same key (S < 2^38).  Integer sums: the same bytes on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xv2_common.h"

namespace {

typedef unsigned long long u64;
constexpr int MAX_R = 32;
constexpr int CHUNK = 32;          // tiles per partial sum of al_chunk_kernel
constexpr int UNIT_TARGET = 1024;  // bands are added while bands * D * ceil(D / 4) units stay below this (4 per thread)
constexpr size_t LDS_BUDGET = 65536 - 2048;   // dynamic LDS of al_sad_kernel: 64 KiB less its static reduction array

__device__ __forceinline__ uint32_t luma_of(const uint8_t* p) {
    return (29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8;
}

// four horizontally neighbouring pixels from (y, x) as packed luma bytes, pixels at x + k >= x_end as 0
__device__ __forceinline__ uint32_t luma4(const uint8_t* img, int W, int y, int x, int x_end) {
    uint32_t w = 0;
    const uint8_t* p = img + ((int64_t)y * W + x) * 3;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (x + k < x_end) w |= luma_of(p + 3 * k) << (8 * k);
    return w;
}

__device__ __forceinline__ u64 shift_key(u64 s, int dyi, int dxi, int R) {
    const int dy = dyi - R, dx = dxi - R;
    return (s << 26) | (u64)((dy * dy + dx * dx) << 14 | dyi << 7 | dxi);
}

// the minimum of one key per thread over a block of a power of two of threads (every thread gets it)
__device__ __forceinline__ u64 block_min(u64 key, u64* red) {
    const int tid = threadIdx.x;
    red[tid] = key;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const u64 o = red[tid + s];
            if (o < red[tid]) red[tid] = o;
        }
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ uint32_t byte_mask(int valid) {   // the low `valid` bytes of a word, valid clamped to 0..4
    return valid >= 4 ? 0xffffffffu : valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
}

// the ragged group's word: the four shifts of a quad one by one, post bytes past the tile's last column masked away
__device__ __forceinline__ void ragged_word(uint32_t lo, uint32_t hi, uint32_t p, uint32_t m, uint32_t (&a)[4]) {
    a[0] = __builtin_amdgcn_sad_u8(lo & m, p, a[0]);
    a[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 1) & m, p, a[1]);
    a[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 2) & m, p, a[2]);
    a[3] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(hi, lo, 3) & m, p, a[3]);
}

__device__ __forceinline__ void widen(u64 pk, uint32_t (&a)[4]) {   // the four packed 16-bit sums into the 32-bit ones
    a[0] += (uint32_t)pk & 0xffffu;
    a[1] += (uint32_t)pk >> 16;
    a[2] += (uint32_t)(pk >> 32) & 0xffffu;
    a[3] += (uint32_t)(pk >> 48);
}

__device__ __forceinline__ u64 pair64(uint32_t hi, uint32_t lo) { return ((u64)hi << 32) | lo; }

template <int T>
__global__ void __launch_bounds__(256) al_sad_kernel(const uint8_t* __restrict__ pre, const uint8_t* __restrict__ post, int H,
                                                     int W, int R, int nbx, int nb, int PSW, uint32_t* __restrict__ block_sad,
                                                     int32_t* __restrict__ block_shift) {
    extern __shared__ __attribute__((aligned(16))) uint32_t al_lds[];
    __shared__ u64 red[256];
    constexpr int PRW = (T + 16) / 4;              // words per pre row
    constexpr int WIDEN = 256 / T;                 // rows of T / 4 words: at most 64 accumulations of at most 4 * 255 fit 16 bits
    const int D = 2 * R + 1, DD = D * D, Q = (D + 3) / 4;
    uint32_t* pre_l = al_lds;                      // [T][PRW]
    uint32_t* post_l = al_lds + T * PRW;           // [T + 2R][PSW]
    uint32_t* part = post_l + (T + 2 * R) * PSW;   // [nb][DD], nb > 1 only
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, by = tile / nbx, bx = tile - by * nbx, b = blockIdx.y;
    const int y0 = R + by * T, x0 = R + bx * T;
    const int th = min(T, H - R - y0), tw = min(T, W - R - x0);
    const uint8_t* pre_b = pre + (int64_t)b * H * W * 3;
    const uint8_t* post_b = post + (int64_t)b * H * W * 3;

    for (int i = tid; i < T * (T / 4); i += 256) {
        const int y = i / (T / 4), xw = i - y * (T / 4);
        uint32_t w = 0;
        if (y < th && 4 * xw < tw) w = luma4(pre_b, W, y0 + y, x0 + 4 * xw, x0 + tw);
        pre_l[y * PRW + xw] = w;
    }
    const int hh = th + 2 * R, hw = tw + 2 * R;    // the halo that exists: rows / columns y0 - R + [0, hh), x0 - R + [0, hw)
    for (int i = tid; i < hh * PSW; i += 256) {
        const int y = i / PSW, xw = i - y * PSW;
        uint32_t w = 0;
        if (4 * xw < hw) w = luma4(post_b, W, y0 - R + y, x0 - R + 4 * xw, x0 - R + hw);
        post_l[i] = w;
    }
    __syncthreads();

    const int gf = tw >> 4;                        // groups of four words without a ragged edge
    const int c = tw - 16 * gf;                    // valid columns of the last, ragged group (0: there is none)
    const uint32_t m0 = byte_mask(c), m1 = byte_mask(c - 4), m2 = byte_mask(c - 8), m3 = byte_mask(c - 12);
    const int64_t out0 = ((int64_t)b * gridDim.x + tile) * DD;
    u64 best = ~0ull;
    for (int u = tid; u < nb * D * Q; u += 256) {
        const int band = u / (D * Q), r = u - band * (D * Q), dyi = r / Q, q = r - dyi * Q;
        uint32_t a[4] = {0, 0, 0, 0};
        u64 pk = 0, pk2 = 0;   // two chains: a quad SAD does not wait for the one before it
        int rows = 0;
        for (int y = band; y < th; y += nb) {
            const uint4* prow = reinterpret_cast<const uint4*>(pre_l + y * PRW);
            const uint32_t* qrow = post_l + (y + dyi) * PSW + q;
            uint32_t lo = qrow[0], hi;
            for (int g = 0; g < gf; ++g) {
                const uint4 p = prow[g];
                hi = qrow[4 * g + 1];
                pk = __builtin_amdgcn_qsad_pk_u16_u8(pair64(hi, lo), p.x, pk);
                lo = qrow[4 * g + 2];
                pk2 = __builtin_amdgcn_qsad_pk_u16_u8(pair64(lo, hi), p.y, pk2);
                hi = qrow[4 * g + 3];
                pk = __builtin_amdgcn_qsad_pk_u16_u8(pair64(hi, lo), p.z, pk);
                lo = qrow[4 * g + 4];
                pk2 = __builtin_amdgcn_qsad_pk_u16_u8(pair64(lo, hi), p.w, pk2);
            }
            if (c) {
                const uint4 p = prow[gf];
                hi = qrow[4 * gf + 1];
                ragged_word(lo, hi, p.x, m0, a);
                lo = qrow[4 * gf + 2];
                ragged_word(hi, lo, p.y, m1, a);
                hi = qrow[4 * gf + 3];
                ragged_word(lo, hi, p.z, m2, a);
                lo = qrow[4 * gf + 4];
                ragged_word(hi, lo, p.w, m3, a);
            }
            if (++rows == WIDEN) {
                widen(pk, a);
                widen(pk2, a);
                pk = pk2 = 0;
                rows = 0;
            }
        }
        widen(pk, a);
        widen(pk2, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dxi = 4 * q + k;
            if (dxi >= D) break;                   // the last quad of a row of shifts is not full: D is odd
            if (nb == 1) {
                block_sad[out0 + dyi * D + dxi] = a[k];
                best = min(best, shift_key(a[k], dyi, dxi, R));
            } else {
                part[band * DD + dyi * D + dxi] = a[k];
            }
        }
    }
    if (nb > 1) {
        __syncthreads();
        for (int d = tid; d < DD; d += 256) {
            uint32_t s = 0;
            for (int k = 0; k < nb; ++k) s += part[k * DD + d];
            block_sad[out0 + d] = s;
            const int dyi = d / D;
            best = min(best, shift_key(s, dyi, d - dyi * D, R));
        }
    }
    best = block_min(best, red);
    if (tid == 0) {
        int32_t* o = block_shift + ((int64_t)b * gridDim.x + tile) * 2;
        o[0] = (int)((best >> 7) & 127) - R;
        o[1] = (int)(best & 127) - R;
    }
}

// chunk[b][c][d] = the sum of S_t(d) over the tiles t of chunk c; grid (ceil(DD / 256), chunks, B)
__global__ void __launch_bounds__(256) al_chunk_kernel(const uint32_t* __restrict__ block_sad, int tiles, int DD,
                                                       int64_t* __restrict__ chunk) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= DD) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const int t1 = min(tiles, (c + 1) * CHUNK);
    int64_t s = 0;
    for (int t = c * CHUNK; t < t1; ++t) s += block_sad[((int64_t)b * tiles + t) * DD + d];
    chunk[((int64_t)b * gridDim.y + c) * DD + d] = s;
}

// S(d) = the sum of the chunks in order, and the best shift of image b; grid (B)
__global__ void __launch_bounds__(1024) al_total_kernel(const int64_t* __restrict__ chunk, int chunks, int R,
                                                       int64_t* __restrict__ sad, int32_t* __restrict__ shift) {
    __shared__ u64 red[1024];
    const int D = 2 * R + 1, DD = D * D, b = blockIdx.x;
    u64 best = ~0ull;
    for (int d = threadIdx.x; d < DD; d += 1024) {
        int64_t s = 0;
        for (int c = 0; c < chunks; ++c) s += chunk[((int64_t)b * chunks + c) * DD + d];
        sad[(int64_t)b * DD + d] = s;
        const int dyi = d / D;
        best = min(best, shift_key((u64)s, dyi, d - dyi * D, R));
    }
    best = block_min(best, red);
    if (threadIdx.x == 0) {
        shift[2 * b] = (int)((best >> 7) & 127) - R;
        shift[2 * b + 1] = (int)(best & 127) - R;
    }
}

// reflection without repeating the edge, for every int64 index: period 2 (L - 1), floor modulo
__device__ __forceinline__ int tri_of(int64_t i, int L) {
    if (L == 1) return 0;
    const int64_t p = 2 * ((int64_t)L - 1);
    int64_t m = i % p;
    if (m < 0) m += p;
    return (int)(m < L ? m : p - m);
}

__global__ void __launch_bounds__(256) al_translate_kernel(const uint8_t* __restrict__ src, int H, int W, int C,
                                                           const int32_t* __restrict__ shift, uint8_t* __restrict__ out) {
    const int64_t hw = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int sy = tri_of((int64_t)y + shift[2 * b], H), sx = tri_of((int64_t)x + shift[2 * b + 1], W);
    const uint8_t* s = src + ((int64_t)b * hw + (int64_t)sy * W + sx) * C;
    uint8_t* o = out + ((int64_t)b * hw + p) * C;
    for (int k = 0; k < C; ++k) o[k] = s[k];
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool sizes_ok(int B, int H, int W, int R, int T) {
    return B > 0 && B <= 65535 && R >= 1 && R <= MAX_R && (T == 32 || T == 64 || T == 128) && H > 2 * R && W > 2 * R &&
           (int64_t)H * W < (1ll << 30);
}

struct Plan {
    int nby, nbx, tiles, chunks, D, DD, nb, psw;
    size_t lds;
};

// LDS cycles of one post read of the first wave: per half-wave the largest number of different words on one bank, with the
// lanes on (dy, quad) units, quad fastest, and one word per lane
int bank_cost(int psw, int D, int Q) {
    int cost = 0;
    for (int half = 0; half < 2; ++half) {
        int words[32][32], n[32] = {0}, worst = 0;
        for (int l = 32 * half; l < 32 * half + 32 && l < D * Q; ++l) {
            const int w = (l / Q) * psw + l % Q, bank = w & 31;
            bool seen = false;
            for (int k = 0; k < n[bank]; ++k) seen = seen || words[bank][k] == w;
            if (!seen) words[bank][n[bank]++] = w;
            if (n[bank] > worst) worst = n[bank];
        }
        cost += worst;
    }
    return cost;
}

Plan plan(int H, int W, int R, int T) {
    Plan p;
    p.nby = (H - 2 * R + T - 1) / T;
    p.nbx = (W - 2 * R + T - 1) / T;
    p.tiles = p.nby * p.nbx;   // below 2^20: H * W < 2^30 and T >= 32
    p.chunks = (p.tiles + CHUNK - 1) / CHUNK;
    p.D = 2 * R + 1;
    p.DD = p.D * p.D;
    const int Q = (p.D + 3) / 4;
    p.nb = UNIT_TARGET / (p.D * Q);
    if (p.nb < 1) p.nb = 1;
    if (p.nb > T) p.nb = T;
    const size_t rows = T + 2 * R, pre_bytes = 4 * (size_t)T * ((T + 16) / 4);
    const int psw0 = (T + 2 * R) / 4 + 2;
    // pre 18432 and post 38400 bytes at T = 128, R = 32 (no bands there); bands hold at most 4 UNIT_TARGET * 4 bytes
    auto bytes = [&](int psw) { return pre_bytes + 4 * rows * psw + (p.nb > 1 ? 4 * (size_t)p.nb * p.DD : 0); };
    while (p.nb > 1 && bytes(psw0) > LDS_BUDGET) --p.nb;
    // a few words of padding per post row where they take bank conflicts out of the first wave's reads and LDS allows
    p.psw = psw0;
    for (int pad = 1, cost = bank_cost(psw0, p.D, Q); pad <= 8 && bytes(psw0 + pad) <= LDS_BUDGET; ++pad) {
        const int c = bank_cost(psw0 + pad, p.D, Q);
        if (c < cost) {
            cost = c;
            p.psw = psw0 + pad;
        }
    }
    p.lds = bytes(p.psw);
    return p;
}

}  // namespace

static int al_kid(int k) {
    static const int ids[] = {xv2::prof_register("al_sad_kernel"), xv2::prof_register("al_chunk_kernel"),
                              xv2::prof_register("al_total_kernel"), xv2::prof_register("al_translate_kernel")};
    return ids[k];
}

extern "C" size_t xv2_align_workspace(int B, int H, int W, int R, int T) {
    if (!sizes_ok(B, H, W, R, T)) return 0;
    const Plan p = plan(H, W, R, T);
    return align256(8 * (size_t)B * p.chunks * p.DD);   // int64 [B][chunks][D][D]
}

extern "C" int xv2_align_estimate(const uint8_t* pre, const uint8_t* post, int B, int H, int W, int R, int T, void* workspace,
                                  uint32_t* block_sad, int64_t* sad, int32_t* block_shift, int32_t* shift, void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "align_estimate: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG(R >= 1 && R <= MAX_R, "align_estimate: radius R=%d must lie in 1..%d", R, MAX_R);
    XV2_CHECK_ARG(T == 32 || T == 64 || T == 128, "align_estimate: tile T=%d must be 32, 64 or 128", T);
    XV2_CHECK_ARG(H > 2 * R && W > 2 * R, "align_estimate: H=%d W=%d leave no interior at radius R=%d (H, W > 2R)", H, W, R);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "align_estimate: H*W=%lld exceeds 2^30 pixels per image", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535, "align_estimate: B=%d too large for one launch", B);
    XV2_CHECK_ARG(pre && post && block_sad && sad && block_shift && shift, "align_estimate: null tensor");
    XV2_CHECK_ARG(workspace, "align_estimate: workspace required");
    XV2_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "align_estimate: the workspace must be 16-byte aligned");
    XV2_CHECK_ARG(reinterpret_cast<uintptr_t>(block_sad) % 4 == 0 && reinterpret_cast<uintptr_t>(sad) % 8 == 0 &&
                      reinterpret_cast<uintptr_t>(block_shift) % 4 == 0 && reinterpret_cast<uintptr_t>(shift) % 4 == 0,
                  "align_estimate: an output is not aligned to its element size");
    hipStream_t st = (hipStream_t)stream;
    const Plan p = plan(H, W, R, T);
    int64_t* chunk = static_cast<int64_t*>(workspace);
    const double px = (double)B * H * W;
    const dim3 grid(p.tiles, B), blk(256);
    if (T == 32)
        XV2_LAUNCH(al_kid(0), 6.0 * px, al_sad_kernel<32>, grid, blk, p.lds, st, pre, post, H, W, R, p.nbx, p.nb, p.psw, block_sad,
                   block_shift);
    else if (T == 64)
        XV2_LAUNCH(al_kid(0), 6.0 * px, al_sad_kernel<64>, grid, blk, p.lds, st, pre, post, H, W, R, p.nbx, p.nb, p.psw, block_sad,
                   block_shift);
    else
        XV2_LAUNCH(al_kid(0), 6.0 * px, al_sad_kernel<128>, grid, blk, p.lds, st, pre, post, H, W, R, p.nbx, p.nb, p.psw, block_sad,
                   block_shift);
    XV2_LAUNCH(al_kid(1), 4.0 * B * p.tiles * p.DD, al_chunk_kernel, dim3((p.DD + 255) / 256, p.chunks, B), blk, 0, st,
               block_sad, p.tiles, p.DD, chunk);
    XV2_LAUNCH(al_kid(2), 8.0 * B * p.chunks * p.DD, al_total_kernel, dim3(B), dim3(1024), 0, st, chunk, p.chunks, R, sad, shift);
    return XV2_OK;
}

extern "C" int xv2_translate_u8(const uint8_t* src, int B, int H, int W, int C, const int32_t* shift, uint8_t* out,
                                void* stream) {
    XV2_CHECK_ARG(B > 0 && H > 0 && W > 0, "translate_u8: B=%d H=%d W=%d must be positive", B, H, W);
    XV2_CHECK_ARG(C >= 1 && C <= 8, "translate_u8: C=%d channels must lie in 1..8", C);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "translate_u8: H*W=%lld exceeds 2^30 pixels per image", (long long)H * W);
    XV2_CHECK_ARG(B <= 65535, "translate_u8: B=%d too large for one launch", B);
    XV2_CHECK_ARG(src && shift && out, "translate_u8: null tensor");
    XV2_CHECK_ARG(reinterpret_cast<uintptr_t>(shift) % 4 == 0, "translate_u8: shift is not aligned to its element size");
    const uintptr_t n = (uintptr_t)B * H * W * C, s0 = reinterpret_cast<uintptr_t>(src), o0 = reinterpret_cast<uintptr_t>(out);
    XV2_CHECK_ARG(s0 + n <= o0 || o0 + n <= s0, "translate_u8: out must not overlap src");
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    XV2_LAUNCH(al_kid(3), 2.0 * n, al_translate_kernel, dim3((unsigned)xv2::cdiv(hw, 256), B), dim3(256), 0, st, src, H, W, C,
               shift, out);
    return XV2_OK;
}
