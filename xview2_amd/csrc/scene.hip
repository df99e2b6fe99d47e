// Scene inference: a scene of any size, resident in HBM, is cut into overlapping windows, the model runs on batches of them,
// and the per-window probabilities are blended back into scene-sized maps - all on the device (call site:
// xview2_amd/scene.py ScenePredictor.predict; the geometry is specified there in integer arithmetic: window_origins, tri,
// ramp, axis_normaliser).  Three launches:
//   xv2_scene_windows_u8   the gather: uint8 windows in the [K][h][w][3 | 6] layout ops.DeviceImage normalises
//   xv2_scene_blend        acc += ramp weight * decode(logits) for the K windows of one model batch
//   xv2_scene_finalize     acc /= the weight sum, which is a product of two per-axis tables (the window grid is a product)
//
// The blend is SCENE-PIXEL-MAJOR: one thread owns one scene pixel, walks the call's window table in index order and chains
// acc = fmaf(weight, p, acc) over the windows that hold the pixel, then stores once.  No atomics and no race, and since acc is
// carried between calls as the fp32 it is, the chain - and so every bit of the result - is the same however the windows of a
// scene are split over calls, as long as calls and windows arrive in the same order.
//
// Launching only over what the windows cover, with the table on the device: the grid is K x (the scene-aligned 64 x 4 pixel
// tiles one window can touch).  Block (k, tile) works iff no window j < k of the table touches that tile - the first window
// touching a tile owns it, the others' blocks retire after one scan of the table in LDS.  Every covered tile has exactly one
// owner for any table, and no block is launched for an uncovered part of the scene.
//
// All three are HBM-streaming: x on the lanes, so a wave reads 256 contiguous bytes of each NCHW logit plane and of each acc
// plane; the gather packs four output bytes per lane (w * C is a multiple of 4) so a wave stores 256 contiguous bytes, and
// its loads are contiguous wherever a window row is not reflected.  The window table sits in LDS (blend) or in scalar
// registers (gather: one origin per block).  Offsets are 64-bit throughout.
#include "xv2_common.h"

namespace xv2 {

constexpr int SC_BW = 64, SC_BH = 4;        // scene tile of one blend block: x on the lanes, one wave per row
constexpr int SC_MAXC = 5;

// reflection without repeating the edge, iterated (np.pad mode="reflect"); i >= 0
__device__ __forceinline__ int tri(int i, int L) {
    if (i < L) return i;
    if (L == 1) return 0;
    const int p = 2 * (L - 1), m = i % p;
    return m < L ? m : p - m;
}
// four bytes at any alignment (gfx950 global loads need none)
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ int clamp_origin(int o, int L) { return min(max(o, 0), L - 1); }
__device__ __forceinline__ int ramp(int i, int n, int overlap) { return min(min(i + 1, n - i), overlap + 1); }

template <int CC>
__global__ void __launch_bounds__(256) scene_windows_kernel(const uint8_t* __restrict__ pre, const uint8_t* __restrict__ post,
                                                             int H, int W, const int32_t* __restrict__ origins, int h, int w,
                                                             uint32_t* __restrict__ out) {
    const int k = blockIdx.z, iy = blockIdx.y;
    const int words = w * CC / 4, q4 = blockIdx.x * 256 + threadIdx.x;
    if (q4 >= words) return;
    const int y0 = clamp_origin(origins[2 * k], H), x0 = clamp_origin(origins[2 * k + 1], W);
    const size_t row = (size_t)tri(y0 + iy, H) * W;
    uint32_t v = 0;
    if (CC == 3 && x0 + (q4 * 4 + 3) / 3 < W) {
        // no reflection under this word: the window row is the scene row's bytes from x0 on
        v = ld_u32(pre + (row + x0) * 3 + q4 * 4);
    } else if (CC == 6 && x0 + 2 * (q4 / 3) + 1 < W) {
        // three words hold two pixels, a0 a1 a2 b0 | b1 b2 a3 a4 | a5 b3 b4 b5 (a: pre, b: post, six bytes each): every word is
        // one word of each scene, taken from inside the pair's six bytes
        const int pair = q4 / 3, j = q4 - 3 * pair;
        const size_t s = (row + x0 + 2 * pair) * 3;
        const uint32_t A = ld_u32(pre + s + (j ? 2 : 0)), B = ld_u32(post + s + (j == 2 ? 2 : 0));
        v = j == 0 ? (A & 0x00ffffffu) | (B << 24) : j == 1 ? ((B >> 8) & 0xffffu) | ((A << 8) & 0xffff0000u)
                                                            : (A >> 24) | (B & 0xffffff00u);
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int q = q4 * 4 + b, ix = q / CC, c = q - ix * CC;
            const int xs = tri(x0 + ix, W);
            const uint8_t* src = (CC == 6 && c >= 3) ? post : pre;
            v |= (uint32_t)src[(row + xs) * 3 + (c >= 3 ? c - 3 : c)] << (8 * b);
        }
    }
    out[((size_t)k * h + iy) * words + q4] = v;
}

template <int KIND>
__device__ __forceinline__ void decode_px(const float* __restrict__ p, size_t plane, int C, float (&v)[SC_MAXC]) {
    if (KIND == XV2_SCENE_SIGMOID1) {
        v[0] = 1.f / (1.f + expf(-p[plane]));
        return;
    }
    float l[SC_MAXC];
#pragma unroll
    for (int c = 0; c < SC_MAXC; ++c) l[c] = c < C ? p[c * plane] : 0.f;
    if (KIND == XV2_SCENE_SOFTMAX) {
        float m = l[0];
#pragma unroll
        for (int c = 1; c < SC_MAXC; ++c)
            if (c < C) m = fmaxf(m, l[c]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c)
            if (c < C) {
                l[c] = expf(l[c] - m);
                s += l[c];
            }
        const float inv = 1.f / s;
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c) v[c] = l[c] * inv;
    } else if (KIND == XV2_SCENE_SIGMOID) {
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c) v[c] = 1.f / (1.f + expf(-l[c]));
    } else {      // relu; a NaN stays a NaN, as torch.relu keeps it
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c) v[c] = l[c] < 0.f ? 0.f : l[c];
    }
}

template <int KIND>
__global__ void __launch_bounds__(SC_BW* SC_BH) scene_blend_kernel(const float* __restrict__ logits, int C,
                                                                    const int32_t* __restrict__ origins, int K, int h, int w,
                                                                    int overlap, int H, int W, float* __restrict__ acc) {
    __shared__ int sy[XV2_SCENE_MAX_WINDOWS], sx[XV2_SCENE_MAX_WINDOWS];
    const int tid = threadIdx.y * SC_BW + threadIdx.x;
    for (int i = tid; i < K; i += SC_BW * SC_BH) {
        sy[i] = clamp_origin(origins[2 * i], H);
        sx[i] = clamp_origin(origins[2 * i + 1], W);
    }
    __syncthreads();
    // the tile of this block: the blockIdx-th scene-aligned tile that window k touches
    const int k = blockIdx.z;
    const int TY = sy[k] / SC_BH + blockIdx.y, TX = sx[k] / SC_BW + blockIdx.x;
    if (TY > (min(sy[k] + h, H) - 1) / SC_BH || TX > (min(sx[k] + w, W) - 1) / SC_BW) return;
    const int ty0 = TY * SC_BH, tx0 = TX * SC_BW;
    for (int j = 0; j < k; ++j)      // an earlier window touches the tile: its block owns it
        if (sy[j] < ty0 + SC_BH && sy[j] + h > ty0 && sx[j] < tx0 + SC_BW && sx[j] + w > tx0) return;
    const int y = ty0 + threadIdx.y, x = tx0 + threadIdx.x;
    if (y >= H || x >= W) return;
    const int Cout = KIND == XV2_SCENE_SIGMOID1 ? 1 : C;
    const size_t scene = (size_t)H * W, plane = (size_t)h * w;
    float* a = acc + (size_t)y * W + x;
    float s[SC_MAXC];
#pragma unroll
    for (int c = 0; c < SC_MAXC; ++c) s[c] = c < Cout ? a[c * scene] : 0.f;
    for (int j = 0; j < K; ++j) {
        const int iy = y - sy[j], ix = x - sx[j];
        if ((unsigned)iy >= (unsigned)h || (unsigned)ix >= (unsigned)w) continue;
        const float wt = (float)(ramp(iy, h, overlap) * ramp(ix, w, overlap));
        float v[SC_MAXC];
        // SIGMOID1 reads channel 1 of the window's two
        const float* p = logits + ((size_t)j * C + (KIND == XV2_SCENE_SIGMOID1 ? 1 : 0)) * plane + (size_t)iy * w + ix;
        decode_px<KIND>(p, KIND == XV2_SCENE_SIGMOID1 ? 0 : plane, C, v);
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c)
            if (c < Cout) s[c] = fmaf(wt, v[c], s[c]);
    }
#pragma unroll
    for (int c = 0; c < SC_MAXC; ++c)
        if (c < Cout) a[c * scene] = s[c];
}

__global__ void __launch_bounds__(256) scene_finalize_kernel(float* __restrict__ acc, int Cout, int H, int W,
                                                              const int32_t* __restrict__ wy, const int32_t* __restrict__ wx) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int nx = wx[x];
    const size_t scene = (size_t)H * W;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {      // (rows past the grid's limit of 65535: a second sweep)
        const float d = (float)(wy[y] * nx);
        float* a = acc + (size_t)y * W + x;
        float v[SC_MAXC];      // all planes' loads in flight before the first division
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c)
            if (c < Cout) v[c] = a[c * scene];
#pragma unroll
        for (int c = 0; c < SC_MAXC; ++c)
            if (c < Cout) a[c * scene] = v[c] / d;
    }
}

static int check_scene(const char* what, int H, int W) {
    XV2_CHECK_ARG(H > 0 && W > 0, "%s: H=%d W=%d must be positive", what, H, W);
    XV2_CHECK_ARG((int64_t)H * W < (1ll << 30), "%s: H*W=%lld exceeds 2^30 pixels per scene", what, (long long)H * W);
    return XV2_OK;
}

static int check_window(const char* what, int K, int h, int w) {
    XV2_CHECK_ARG(K > 0 && K <= XV2_SCENE_MAX_WINDOWS, "%s: K=%d windows per call must be in 1..%d", what, K,
                  XV2_SCENE_MAX_WINDOWS);
    XV2_CHECK_ARG(h >= 32 && h <= 2048 && h % 32 == 0 && w >= 32 && w <= 2048 && w % 32 == 0,
                  "%s: window %d x %d: sides must be multiples of 32 in 32..2048", what, h, w);
    return XV2_OK;
}

}  // namespace xv2

using namespace xv2;

// ScenePredictor.predict, per model batch: the K windows the model is about to see
extern "C" int xv2_scene_windows_u8(const uint8_t* pre, const uint8_t* post, int H, int W, const int32_t* origins, int K, int h,
                                    int w, uint8_t* out, void* stream) {
    if (int rc = check_scene("scene_windows_u8", H, W)) return rc;
    if (int rc = check_window("scene_windows_u8", K, h, w)) return rc;
    XV2_CHECK_ARG(pre && origins && out, "scene_windows_u8: null tensor");
    XV2_CHECK_ARG(((uintptr_t)out & 3) == 0, "scene_windows_u8: out must be 4-byte aligned");
    const int C = post ? 6 : 3;
    const dim3 grid((unsigned)cdiv(w * C / 4, 256), (unsigned)h, (unsigned)K);
    if (post)
        hipLaunchKernelGGL(scene_windows_kernel<6>, grid, dim3(256), 0, (hipStream_t)stream, pre, post, H, W, origins, h, w,
                           (uint32_t*)out);
    else
        hipLaunchKernelGGL(scene_windows_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, pre, post, H, W, origins, h, w,
                           (uint32_t*)out);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// ScenePredictor.predict, per model batch: the batch's logits onto the scene's accumulators
extern "C" int xv2_scene_blend(const float* logits, int kind, int C, const int32_t* origins, int K, int h, int w, int overlap,
                               int H, int W, float* acc, void* stream) {
    if (int rc = check_scene("scene_blend", H, W)) return rc;
    if (int rc = check_window("scene_blend", K, h, w)) return rc;
    XV2_CHECK_ARG(kind == XV2_SCENE_SIGMOID1 || kind == XV2_SCENE_SOFTMAX || kind == XV2_SCENE_SIGMOID || kind == XV2_SCENE_RELU,
                  "scene_blend: unknown kind %d (sigmoid1 0, softmax 1, sigmoid 2, relu 3)", kind);
    XV2_CHECK_ARG(kind == XV2_SCENE_SIGMOID1 ? C == 2 : (C >= (kind == XV2_SCENE_SOFTMAX ? 2 : 1) && C <= SC_MAXC),
                  "scene_blend: C=%d does not fit kind %d (sigmoid1: 2, softmax: 2..5, sigmoid and relu: 1..5)", C, kind);
    XV2_CHECK_ARG(overlap >= 0 && overlap <= min(h, w) / 2, "scene_blend: overlap=%d must be in 0..%d (half the window)",
                  overlap, min(h, w) / 2);
    XV2_CHECK_ARG(logits && origins && acc, "scene_blend: null tensor");
    const dim3 grid((unsigned)((w - 1) / SC_BW + 2), (unsigned)((h - 1) / SC_BH + 2), (unsigned)K), block(SC_BW, SC_BH);
    hipStream_t st = (hipStream_t)stream;
    if (kind == XV2_SCENE_SIGMOID1)
        hipLaunchKernelGGL(scene_blend_kernel<XV2_SCENE_SIGMOID1>, grid, block, 0, st, logits, C, origins, K, h, w, overlap, H, W, acc);
    else if (kind == XV2_SCENE_SOFTMAX)
        hipLaunchKernelGGL(scene_blend_kernel<XV2_SCENE_SOFTMAX>, grid, block, 0, st, logits, C, origins, K, h, w, overlap, H, W, acc);
    else if (kind == XV2_SCENE_SIGMOID)
        hipLaunchKernelGGL(scene_blend_kernel<XV2_SCENE_SIGMOID>, grid, block, 0, st, logits, C, origins, K, h, w, overlap, H, W, acc);
    else
        hipLaunchKernelGGL(scene_blend_kernel<XV2_SCENE_RELU>, grid, block, 0, st, logits, C, origins, K, h, w, overlap, H, W, acc);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}

// ScenePredictor.predict, once per scene after the last batch
extern "C" int xv2_scene_finalize(float* acc, int Cout, int H, int W, const int32_t* wy, const int32_t* wx, void* stream) {
    if (int rc = check_scene("scene_finalize", H, W)) return rc;
    XV2_CHECK_ARG(Cout >= 1 && Cout <= SC_MAXC, "scene_finalize: Cout=%d must be in 1..%d", Cout, SC_MAXC);
    XV2_CHECK_ARG(acc && wy && wx, "scene_finalize: null tensor");
    hipLaunchKernelGGL(scene_finalize_kernel, dim3((unsigned)cdiv(W, 256), (unsigned)min(H, 65535)), dim3(256), 0,
                       (hipStream_t)stream, acc, Cout, H, W, wy, wx);
    XV2_CHECK_LAUNCH();
    return XV2_OK;
}
