/*
 * xv2.h — C ABI of the MI355X (gfx950) U-Net training hot path.
 *
 * The reference (michal2409/xView2) has no FFI layer: its hot path is the set of torch
 * operators dispatched by model/unet.py, model/layers.py and model/loss.py.  Every entry
 * point below therefore names the torch operator call-site it replaces (reference file:line).
 * Conventions
 *   - all tensors are caller-owned DEVICE buffers, fp32 unless stated, activations are NHWC
 *     ("pixel-major, channel-minor"); `ld*` arguments are the pixel stride in floats so that a
 *     channel slice of a wider tensor can be passed without a copy (virtual concat / groups);
 *   - every call enqueues work on `stream` (a hipStream_t) and returns without synchronising;
 *   - return value 0 = success, otherwise an XV2_E* code; xv2_last_error() gives the message
 *     (thread-local), no C++ exception crosses this boundary;
 *   - no allocation happens inside any call: workspaces are sized by the *_workspace() helpers.
 */
#ifndef XV2_H_
#define XV2_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XV2_OK 0
#define XV2_EINVAL 1   /* bad argument / unsupported shape */
#define XV2_EHIP 2     /* a HIP runtime call failed */

#define XV2_ACT_NONE 0
#define XV2_ACT_RELU 1      /* encoders: model/unet.py:80 and the un-vendored ResNet/ResNeSt blocks */
#define XV2_ACT_LEAKY 2     /* LeakyReLU(0.01): model/layers.py:17,37,94 */
#define XV2_ACT_SIGMOID 3   /* attention gate: model/layers.py:147,165 */

const char* xv2_last_error(void);
int xv2_version(void);

/* ---- convolution ------------------------------------------------------------------------
 * Geometry of one nn.Conv2d (model/layers.py:35,71,92,139,180; torchvision/resnest blocks),
 * groups handled by the caller through channel-offset views.  The input may be the virtual
 * concatenation of two tensors (torch.cat at model/layers.py:114,167): channels [0,C0) come
 * from x0, [C0,C0+C1) from x1.  C0 and C1 must be multiples of 32, except the RGB stems which
 * are passed as a single 4-channel (zero padded) source (C0=4, C1=0).
 */
typedef struct xv2_conv_desc {
    int32_t N, IH, IW;          /* input batch / height / width */
    int32_t C0, C1;             /* input channels taken from source 0 / source 1 */
    int32_t Cout;               /* output channels, multiple of 32 */
    int32_t KH, KW, stride, pad, dil;
    int32_t OH, OW;             /* output height / width */
    int32_t math;               /* XV2_MATH_F32 (exact fp32 MFMA) or XV2_MATH_BF16 (operands rounded to bf16 in
                                   LDS, bf16 MFMA, fp32 accumulate: the reference's --precision 16 autocast) */
} xv2_conv_desc;
#define XV2_MATH_F32 0
#define XV2_MATH_BF16 1
/* bf16 STORAGE (the --precision 16 path proper, reference main.py:36,99): activations, their gradients and the packed
 * weight layouts are bf16 in HBM (every `void*` activation / packed-weight argument below then points to bf16),
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, BatchNorm statistics / coefficients, biases, weight gradients and the
 * master weights stay fp32.  The 4-channel RGB source of the stems stays an fp32 image with fp32 packed weights. */
#define XV2_MATH_BF16_STORE 2

/* fp32 tensors, fp32-grade arithmetic on the bf16 matrix pipe: each fp32 operand is split into three bf16 terms
 * (x = hi + mid + lo, exact to 24 bits) while it is staged in LDS and the product is formed from the six significant
 * cross terms hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid with v_mfma_f32_32x32x16_bf16 (fp32 accumulate; the dropped
 * terms are below 2^-24 relative).  6 bf16 MFMAs of 16 k each replace 8 exact-fp32 MFMAs of 2 k each: 0.375x the
 * matrix-pipe time for fp32-level accuracy.  Covers the implicit-GEMM kernel (forward, backward-data, transposed
 * convolution) and the two main weight-gradient kernels (all-taps 3x3, transpose-read 1x1 / strided); the direct 3x3
 * kernel, the RGB stem and odd-shaped weight-gradient layers run their exact-fp32 forms under this mode.  This is the
 * mode the host layer uses for fp32 tensors by default (XV2_F32X3=0 in the environment selects XV2_MATH_F32).
 * NON-FINITE OPERANDS: the split of +-Inf is h = Inf, m = bf16(Inf - Inf) = NaN, so an operand element that is +-Inf (or NaN)
 * makes every output it contributes to NaN, where the exact-fp32 MFMA (and torch) would propagate +-Inf through products
 * with non-zero finite values.  Both are already-diverged training states; finite inputs are unaffected: bf16 has fp32's exponent
 * range, so a finite fp32 rounds to a finite h (to Inf only above 0x7f7f8000 ~ 3.39e38, where h = Inf again yields NaN), and
 * the three terms add up to x exactly whenever x is a multiple of 2^-133, the smallest bf16 denormal - every x with
 * |x| >= 2^-110, and the smaller ones whose low bits are zero; the rest (denormals, the smallest normals) lose what lies
 * below 2^-133, at most 2^-134 (tests/test_weights_ref_cpu.py).  Callers that must keep Inf semantics select XV2_MATH_F32. */
#define XV2_MATH_F32X3 3

/* element type of activation tensors for the non-convolution entry points (`dtype` arguments) */
#define XV2_F32 0
#define XV2_BF16 1

/* weight repacking: w_oihw[Cout][Cin][KH][KW] (the reference's state_dict layout)
 *   -> w_ohwi[Cout][KH*KW][CinP]  (forward operand; CinP = Cin padded to `cin_pad`)
 *   -> w_ihwo[CinP][KH*KW][Cout]  (backward-data operand)                                  */
int xv2_pack_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, int cin_pad,
                    void* w_ohwi, void* w_ihwo, int dtype, void* stream);
/* the same for MANY weights in one launch (all packed layouts go stale together at the optimizer step):
 * table[n][8] int64 in device memory = {w_oihw, w_ohwi or 0, w_ihwo or 0 (pointers), Cout, Cin,
 * KH*KW | (dtype of the packed layouts << 16), cin_pad, first tile}; an entry owns xv2_pack_weights_tiles() consecutive tiles (one workgroup each), total_tiles = their sum */
int64_t xv2_pack_weights_tiles(int Cout, int KH, int KW, int cin_pad);
int xv2_pack_weights_table(const int64_t* table, int n, int64_t total_tiles, void* stream);

/* Packed fp32 weight operands PRE-SPLIT into three bf16 planes (XV2_MATH_F32X3: every fp32 value = hi + mid + lo exactly,
 * xv2_common.h split3x4) for the halo form of the implicit-GEMM kernel: the 3x3 / stride-1 forward and backward-data
 * launches of nn.Conv2d (model/layers.py:92, ConvLayer) then stream their weight operand global -> LDS with direct-to-LDS
 * loads - no registers, no split, no LDS store instructions for it.
 * `b_fp32` = a packed layout [nrows][T][ctot] as xv2_pack_weight writes it (w_ohwi: nrows = Cout, ctot = cin_pad; w_ihwo:
 * nrows = cin_pad, ctot = Cout); `x3` = xv2_presplit_bytes() bytes, 16-byte aligned, laid out
 * [nrows/64][T][ctot/16][3 planes][64 rows][16] bf16 (the LDS image of a weight stage).  xv2_presplit_weights() fills x3
 * AND remembers the pair: convolutions handed `b_fp32` afterwards read the planes, so the caller must refresh them on the
 * same stream whenever the packed weights change (xv2_presplit_table: all pairs of a device table [n][6] int64 =
 * {b_fp32, x3 (pointers), nrows, T, ctot, first block} in one launch, an entry owns xv2_presplit_blocks() blocks) and call
 * xv2_presplit_forget(b_fp32) before releasing either buffer (NULL: forget every pair). */
/* RGB stem (model/unet.py:45 enc_l1: the 7x7 / stride-2 convolution over the image) as a "band" convolution: a KH x KW
 * (KW <= 8) kernel over the 4-channel image equals a KH x 1 kernel over 32 "channels" = the floats of eight consecutive
 * pixels of a row.  xv2_pad_band copies the NHWC4 image into a zero-padded frame [N][IHp][IWp][4] (fp32 or bf16, image at
 * (pad_top, pad_left)); xv2_pack_stem_band lays the weights out as [Cout][KH][8][4]; xv2_conv2d_forward* then runs the
 * layer on the 32-channel kernels with the descriptor {IH = IHp, IW = IWp, C0 = 32, KH, KW = 1, stride, pad = 0, OH, OW}
 * and ldx0 = 4 (IWp even, IWp >= stride * (OW - 1) + 8, IHp >= stride * (OH - 1) + KH). */
int xv2_pad_band(const float* x4, int N, int H, int W, int pad_top, int pad_left, int IHp, int IWp, void* out,
                 int dtype, void* stream);
int xv2_pack_stem_band(const float* w_oihw, int Cout, int Cin, int KH, int KW, void* w_band, int dtype, void* stream);
int xv2_presplit_supported(int nrows, int T, int ctot);
size_t xv2_presplit_bytes(int nrows, int T, int ctot);
int64_t xv2_presplit_blocks(int nrows, int T, int ctot);
int xv2_presplit_weights(const float* b_fp32, int nrows, int T, int ctot, void* x3, void* stream);
int xv2_presplit_table(const int64_t* table, int n, int64_t total_blocks, void* stream);
int xv2_presplit_forget(const void* b_fp32);

/* F16X2 - the two-plane form of XV2_MATH_F32X3 (same tensors, same accumulation, half the matrix instructions): an operand x is
 * scaled by a power of two s taken from the tensor's max |x| (|x * s| < 2^15) and split as x * s = h + m, h = fp16(x * s),
 * m = fp16(x * s - h): 22 significant bits for every element within 2^18 of the maximum, an absolute error of 2^-39 of the maximum
 * below that; each product is three v_mfma_f32_32x32x16_f16 (h*h, h*m, m*h; the dropped m*m <= 2^-22) with fp32 accumulation and
 * the epilogue multiplies by 1 / (s_a * s_b) - exact.  Measured against an fp64 convolution it is as close as an fp32 one
 * (scripts/chk_f16x2.py); F.conv2d on the reference's GPU path defaults to TF32, 2^-11.  The mode needs the operands' maxima:
 *   - a tensor's maximum lives in 64 uint32 "slots" (bit patterns of |x|; the maximum of the 64 is the tensor's), written with
 *     atomicMax by the kernel that PRODUCES the tensor (the BatchNorm apply passes, below) or by xv2_tensor_amax (zeroes the
 *     slots first, then one pass over x); one slot per 128-byte line, i.e. 64 x 32 uint32 = 8 KB per tensor (the atomics of
 *     a few thousand blocks on one or two lines cost the producer more than the mode returns); a producer that cannot know the
 *     maximum leaves the consumer on the three-plane bf16 form;
 *   - xv2_amax_ctx(a0, a1, dy, out) names, for the NEXT convolution / BatchNorm-apply / layer call of THIS host thread only
 *     (every such entry point clears the context when it returns - also the convolutions' plan queries, so set it right
 *     before the call), the slots of the activation sources x0 / x1 (forward, weight gradient), of the output gradient dy (backward-data,
 *     weight gradient) and the slots `out` into which the call's BatchNorm apply pass records the maximum of the tensor it writes
 *     (xv2_bn_act_forward* / xv2_conv_bn_act_forward: z; xv2_bn_act_backward_apply* / xv2_bn_act_backward: dy).  `out` must be
 *     zero (or hold a lower bound) beforehand; NULL = unknown / not wanted;
 *   - a weight operand's maximum: xv2_tensor_amax over one of its packed fp32 layouts, then xv2_weight_amax_register(layout, slots)
 *     for every layout of that weight (the per-tap kernels split the weights themselves and only need the maximum);
 *     xv2_presplit_weights_f16 writes the two scaled fp16 planes of a 3x3 layout ([nrows/64][T][ctot/16][2][64][16],
 *     xv2_presplit_f16_bytes) FROM the maximum already in `amax_slots` and remembers the pair like xv2_presplit_weights.  After
 *     an optimizer step: xv2_weight_amax_table (table [n][4] int64 = {layout, float4 count, slots, first block}, an entry owns
 *     ceil(count / 1024) blocks; zeroes amax_base .. + amax_bytes first) and then xv2_presplit_f16_table (table [n][7] =
 *     {b_fp32, x2, nrows, T, ctot, first block, slots}, xv2_presplit_blocks() blocks per entry), both on the stream of the step;
 *     xv2_presplit_forget drops all three kinds of registration.
 * A convolution whose operand maxima are all known runs as F16X2 (halo form with planes, per-tap form, the split weight-gradient
 * kernels), every other one as F32X3; a value above the recorded maximum (a slot that is stale) overflows to Inf / NaN - loud,
 * never a silently wrong finite result.  XV2_F16X2=0 in the environment keeps every launch on the three-plane form. */
int xv2_amax_ctx(const void* amax_a0, const void* amax_a1, const void* amax_dy, void* amax_out);
int xv2_tensor_amax(const float* x, int64_t n, void* slots, void* stream);
int xv2_presplit_f16_supported(int nrows, int T, int ctot);   /* 3x3 layouts as xv2_presplit_supported; 1x1 layouts with nrows % 64 == 0, ctot % 16 == 0 */
size_t xv2_presplit_f16_bytes(int nrows, int T, int ctot);
int xv2_presplit_weights_f16(const float* b_fp32, int nrows, int T, int ctot, void* x2, void* amax_slots, void* stream);
int xv2_presplit_f16_table(const int64_t* table, int n, int64_t total_blocks, void* stream);
int xv2_weight_amax_register(const void* b_fp32, const void* amax_slots);
int xv2_weight_amax_table(const int64_t* table, int n, int64_t total_blocks, void* amax_base, int64_t amax_bytes, void* stream);

/* y = conv2d(cat(x0,x1), w) [+ bias]; replaces F.conv2d.  If `stats` != NULL the kernel also
 * writes per-channel partial sums of y and y*y per row tile: stats[tile][Cout][2]
 * (tile count = xv2_conv2d_forward_stats_tiles(d)), consumed by xv2_bn_reduce_stats. */
int64_t xv2_conv2d_forward_stats_tiles(const xv2_conv_desc* d);
/* rows (output pixels) per statistics tile of that plan: 64 or 128.  A caller that reduces tile RANGES separately
 * (several BatchNorm batches back to back in one launch: the Siamese pre/post passes) needs every range to end on a
 * tile boundary */
int64_t xv2_conv2d_forward_stats_tile_rows(const xv2_conv_desc* d);
/* Convolution + training-mode BatchNorm statistics behind one call (model/layers.py:92-93 conv -> norm; the encoder blocks):
 * xv2_conv2d_forward with the per-tile partials, then per part the reduction of the partials (a fixed summation order:
 * bit-reproducible) to sums[parts][part_stride][2] (fp64 sum and sum of squares per channel) and - when `mean` != NULL - mean /
 * invstd / scale / shift [parts][part_stride] and the running-statistics update, part after part (xv2_bn_reduce_stats /
 * xv2_bn_reduce_finalize).  parts > 1: the batch holds that many independent BatchNorm batches back to back (the Siamese pre /
 * post passes); every part must end on a statistics-tile boundary ((N*OH*OW / parts) % xv2_conv2d_forward_stats_tile_rows(d)
 * == 0).  SyncBatchNorm: pass mean = NULL, all-reduce `sums`, then xv2_bn_finalize.  stats_partials:
 * xv2_conv2d_forward_stats_tiles(d) * Cout * 2 floats; scratch: XV2_BN_SCRATCH_ROWS * Cout * 2 doubles; workspace as for
 * xv2_conv2d_forward.
 * (Rounds 3 - 5 carried three opt-in variants of this layer that all measured as losses on MI355X and were removed in round 6:
 * the statistics reduction folded into the convolution launch behind device-scope tickets (+0.65 ms per cfg2 step once fenced
 * correctly), the BatchNorm apply behind a gate in that same launch (cfg3 18.3 -> 20.3 ms), and the producing layer's BatchNorm
 * applied in this convolution's operand load (cfg2 27.39 -> 27.63 ms); numbers in DESIGN.md section 4.) */
int xv2_conv2d_forward_bn(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                          const void* w_ohwi, void* y, int ldy, float* stats_partials, float* workspace,
                          int parts, int part_stride, double* sums, double* scratch, double count,
                          const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                          float* shift, void* stream);
/* split-K scratch (bytes, may be 0): layers with few output pixels and a deep reduction keep the large
 * tile and fill the chip by splitting K; `workspace` may be NULL, which disables split-K */
size_t xv2_conv2d_forward_workspace(const xv2_conv_desc* d);
int xv2_conv2d_forward(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1,
                       int ldx1, const void* w_ohwi, const float* bias, void* y, int ldy,
                       float* stats, float* workspace, void* stream);
/* inference form of conv + nn.BatchNorm2d (eval) [+ residual] + activation in ONE launch: the running statistics are
 * folded to per-channel scale/shift (xv2_bn_eval_coeffs) and applied in the convolution epilogue,
 * z = act(conv(x) * scale + shift [+ residual]); the raw convolution output is never written.  Same arithmetic, bit
 * for bit, as xv2_conv2d_forward followed by xv2_bn_act_forward.  act = XV2_ACT_*. */
int xv2_conv2d_forward_fused(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1,
                             int ldx1, const void* w_ohwi, const float* scale, const float* shift,
                             const void* residual, int ldres, int act, void* z, int ldz,
                             float* workspace, void* stream);
/* dx = conv2d_backward_input(dy, w); dx0/dx1 receive the channel ranges of the two sources */
size_t xv2_conv2d_backward_data_workspace(const xv2_conv_desc* d);
int xv2_conv2d_backward_data(const xv2_conv_desc* d, const void* dy, int lddy,
                             const void* w_ihwo, void* dx0, int lddx0, void* dx1, int lddx1,
                             float* workspace, void* stream);
/* the same, ADDING into dx0 (accumulate bit 0) and/or dx1 (bit 1) instead of overwriting them: the gradient of a
 * tensor with two consumers (residual shortcut, encoder skip) is summed in the kernel epilogue, not by a separate
 * elementwise pass */
int xv2_conv2d_backward_data_acc(const xv2_conv_desc* d, const void* dy, int lddy,
                                 const void* w_ihwo, void* dx0, int lddx0, void* dx1, int lddx1,
                                 int accumulate, float* workspace, void* stream);
/* dw_oihw (reference layout, Cin = real channel count `cin_real` <= C0+C1) */
size_t xv2_conv2d_backward_weight_workspace(const xv2_conv_desc* d);
int xv2_conv2d_backward_weight(const xv2_conv_desc* d, const void* x0, int ldx0,
                               const void* x1, int ldx1, const void* dy, int lddy,
                               float* dw_oihw, int cin_real, float* workspace, void* stream);
/* xv2_conv2d_backward_weight launched on `side_stream`, ordered behind the work enqueued so far on `stream` (event
 * record / wait inside the call).  The weight gradient is consumed only by the optimizer / gradient all-reduce, so it
 * can overlap the rest of the backward pass; the caller joins `side_stream` before reading dw_oihw and keeps the
 * operands and the workspace alive until then. */
int xv2_conv2d_backward_weight_async(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                                     const void* dy, int lddy, float* dw_oihw, int cin_real, float* workspace,
                                     void* side_stream, void* stream);

/* nn.ConvTranspose2d(k=2, s=2, bias=False) (model/layers.py:83).  `d` describes the
 * EQUIVALENT convolution (input = the large 2H x 2W tensor with C0 = conv-transpose output
 * channels, Cout = conv-transpose input channels): forward of the transposed conv is the
 * backward-data of `d`, and vice versa; weights are the torch tensor [Cin_T][Cout_T][2][2]
 * viewed as OIHW of `d`. */
int xv2_conv_transpose2d_forward(const xv2_conv_desc* d, const void* x, int ldx,
                                 const void* w_ihwo, void* y, int ldy, void* stream);
int xv2_conv_transpose2d_backward_data(const xv2_conv_desc* d, const void* dy, int lddy,
                                       const void* w_ohwi, void* dx, int lddx, void* stream);
/* the same with accumulate != 0: the gradient is ADDED onto what dx holds (the transposed convolution's input also feeds a
 * deep-supervision head, model/unet.py:193-197: no elementwise sum of the two gradients); workspace as for xv2_conv2d_forward
 * of the same descriptor (may be NULL: no split-K plan then) */
int xv2_conv_transpose2d_backward_data_acc(const xv2_conv_desc* d, const void* dy, int lddy, const void* w_ohwi,
                                           void* dx, int lddx, int accumulate, float* workspace, void* stream);
int xv2_conv_transpose2d_backward_weight(const xv2_conv_desc* d, const void* x, int ldx,
                                         const void* dy, int lddy, float* dw, float* workspace,
                                         void* stream);

/* 1x1 convolution with a handful of output channels (segmentation heads n_class<=4,
 * model/layers.py:177,180; attention psi conv model/layers.py:145).  NHWC in; output either
 * NHWC (nchw_out=0) or NCHW (nchw_out=1, the layout model/unet.py:191-197 returns). */
int xv2_head_conv_forward(const void* x, int ldx, int64_t npix, int64_t hw, int Cin, int Cout,
                          const float* w, const float* bias, float* y, int nchw_out, int dtype, void* stream);
int xv2_head_conv_backward(const void* x, int ldx, const float* dy, int64_t npix, int64_t hw,
                           int Cin, int Cout, const float* w, int nchw_dy, void* dx, int lddx,
                           float* dw, float* dbias, float* workspace, int dtype, void* stream);
size_t xv2_head_conv_backward_workspace(int64_t npix, int Cin, int Cout);

/* ---- batch norm + activation (nn.BatchNorm2d + ReLU/LeakyReLU, everywhere) -------------- */
/* partial sums [tiles][C][2] -> sums[C][2] (double), fixed-order (deterministic) reduction;
 * scratch: XV2_BN_SCRATCH_ROWS*C*2 doubles */
#define XV2_BN_SCRATCH_ROWS 64
int xv2_bn_reduce_stats(const float* partial, int64_t tiles, int C, double* sums, double* scratch,
                        void* stream);
/* xv2_bn_reduce_stats + xv2_bn_finalize in ONE launch (single-process nn.BatchNorm2d in training mode; SyncBatchNorm
 * keeps the two calls with the all-reduce of `sums` between them).  Same outputs as the pair, bit for bit. */
int xv2_bn_reduce_finalize(const float* partial, int64_t tiles, int C, double* sums, double* scratch,
                           double count, const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, float* mean, float* invstd,
                           float* scale, float* shift, void* stream);
/* direct statistics of an NHWC tensor (when no conv epilogue produced them):
 * workspace = xv2_bn_tensor_stats_workspace() bytes (partials followed by the double scratch) */
int xv2_bn_tensor_stats(const float* x, int ldx, int64_t npix, int C, double* sums,
                        float* workspace, void* stream);
size_t xv2_bn_tensor_stats_workspace(int64_t npix, int C);
/* sums (+count, possibly all-reduced across ranks) -> mean, invstd, scale, shift; updates the
 * running statistics exactly like torch (momentum, unbiased running_var). */
int xv2_bn_finalize(const double* sums, double count, const float* gamma, const float* beta,
                    float eps, float momentum, float* running_mean, float* running_var,
                    float* mean, float* invstd, float* scale, float* shift, int C, void* stream);
/* eval mode: scale/shift from the running statistics */
int xv2_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, int C,
                       void* stream);
/* z = act(y*scale[c] + shift[c] (+ residual)) */
int xv2_bn_act_forward(const void* y, int ldy, const float* scale, const float* shift,
                       const void* residual, int ldr, int act, void* z, int ldz,
                       int64_t npix, int C, int dtype, void* stream);
/* backward: pass 1 -> sums2[C][2] = (sum g, sum g*xhat), g = dz*act'; the activation mask comes from the saved
 * output z, or - when z is NULL (no residual) - is recomputed from y*scale+shift, which saves a third of the
 * HBM traffic.  dgamma/dbeta (optional) receive the fp32 copies of the LOCAL sums. */
int xv2_bn_act_backward_reduce(const void* dz, int lddz, const void* z, int ldz,
                               const void* y, int ldy, const float* mean, const float* invstd,
                               const float* scale, const float* shift, int act, int64_t npix, int C,
                               double* sums2, float* dgamma, float* dbeta, float* workspace,
                               int dtype, void* stream);
size_t xv2_bn_backward_workspace(int64_t npix, int C);
/* pass 2 -> dy (and dresidual = g if requested).  dgamma = sums2[:,1], dbeta = sums2[:,0] of
 * the LOCAL rank (torch SyncBatchNorm semantics); sums2 passed here may be all-reduced.
 * `count` is the (global) number of elements per channel; eval-mode BN passes train=0. */
int xv2_bn_act_backward_apply(const void* dz, int lddz, const void* z, int ldz, const void* y,
                              int ldy, const float* mean, const float* invstd,
                              const float* gamma, const float* scale, const float* shift,
                              const double* sums2, double count, int act,
                              int train, void* dy, int lddy, void* dres, int lddres,
                              int64_t npix, int C, int dtype, void* stream);
/* Mask forms for layers whose activation follows a residual add (z = act(BN(y) + residual), the bottleneck tail):
 * the forward also writes one byte per 4 channels, bit k = (z[4j + k] > 0), and the backward passes read that byte
 * instead of re-reading z (0.25 instead of 4 bytes per element in each pass).  C % 4 == 0, dense rows (ld == C for
 * the mask indexing), ReLU / LeakyReLU only.  Results are bit-identical to the z forms. */
int xv2_bn_act_forward_mask(const void* y, int ldy, const float* scale, const float* shift,
                            const void* residual, int ldr, int act, void* z, int ldz, int64_t npix, int C,
                            uint8_t* zmask, int dtype, void* stream);
int xv2_bn_act_backward_reduce_mask(const void* dz, int lddz, const uint8_t* zmask, const void* y, int ldy,
                                    const float* mean, const float* invstd, int act, int64_t npix, int C,
                                    double* sums2, float* dgamma, float* dbeta, float* workspace, int dtype,
                                    void* stream);
int xv2_bn_act_backward_apply_mask(const void* dz, int lddz, const uint8_t* zmask, const void* y, int ldy,
                                   const float* mean, const float* invstd, const float* gamma,
                                   const double* sums2, double count, int act, int train, void* dy,
                                   int lddy, void* dres, int lddres, int64_t npix, int C, int dtype, void* stream);

/* BatchNorm over a handful of rows: y [parts * rows][C] fp32, rows <= 64 (ResNeSt split attention's bn1 on the pooled
 * [N, inter] vector, model/unet.py:52 -> resnest SplAtConv2d).  ONE launch each way: batch statistics (two-pass fp64 per
 * channel), running-statistics update (part after part), coefficients [parts][C] and z = act(bn(y)) forward;
 * dy, dgamma, dbeta (summed over the parts) backward, the activation derivative taken from z.  Same arithmetic as the
 * general path (xv2_bn_tensor_stats + xv2_bn_finalize + xv2_bn_act_forward / xv2_bn_act_backward_*) to fp32 rounding. */
int xv2_bn_rows_forward(const float* y, int rows, int C, int parts, const float* gamma, const float* beta, float eps,
                        float momentum, float* running_mean, float* running_var, int train, int act,
                        float* mean, float* invstd, float* scale, float* shift, float* z, void* stream);
int xv2_bn_rows_backward(const float* dz, const float* z, const float* y, const float* mean, const float* invstd,
                         const float* gamma, int rows, int C, int parts, int act, int train, float* dy,
                         float* dgamma, float* dbeta, void* stream);

/* ---- layer-level entry points ---------------------------------------------------------------
 * One call = the launch sequence of one reference layer (model/layers.py:89-100 ConvLayer: conv -> norm -> activation;
 * the bottleneck convolutions of the encoders), issued in the same order on the same stream as the op-level calls
 * they replace - results are bit-identical.  They exist because a --precision 16 step is bound by the host's call
 * rate: every ABI call costs the binding ~9 us of marshalling on top of its launches.
 * xv2_conv_bn_act_forward = xv2_conv2d_forward (with statistics partials; `tiles` = xv2_conv2d_forward_stats_tiles)
 *   + xv2_bn_reduce_finalize + xv2_bn_act_forward[_mask] (zmask != NULL selects the mask form).  Single-process
 *   training-mode BatchNorm only (SyncBatchNorm keeps the op-level calls around its all-reduce).
 * xv2_bn_act_backward = xv2_bn_act_backward_reduce[_mask] + xv2_bn_act_backward_apply[_mask] (training mode). */
int xv2_conv_bn_act_forward(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                            const void* w_ohwi, void* y, int ldy, float* stats_partials, int64_t tiles,
                            float* workspace, double* sums, double* scratch, double count,
                            const float* gamma, const float* beta, float eps, float momentum,
                            float* running_mean, float* running_var, float* mean, float* invstd,
                            float* scale, float* shift, const void* residual, int ldr, int act, void* z,
                            int ldz, uint8_t* zmask, int dtype, void* stream);
/* xv2_splat_tail_forward / _backward = the op-level sequence of split attention's tail (xv2_splat_gap_forward, xv2_linear_forward,
 *   xv2_bn_rows_forward, xv2_linear_forward, xv2_rsoftmax_forward, xv2_splat_apply_forward; backward: their twins in reverse) behind
 *   one call: 10 calls less per ResNeSt block and direction (cfg5 runs 132 blocks per pass and is bound by the host's call
 *   rate).  parts = BatchNorm batches back to back in the N rows (N / parts <= 64 rows each); every intermediate vector is
 *   passed explicitly (the caller owns what the backward pass needs); workspace: xv2_splat_gap_workspace(N, hw, C). */
int xv2_splat_tail_forward(const void* x, int N, int64_t hw, int C, int inter, const float* w1, const float* b1,
                           const float* gamma1, const float* beta1, float eps, float momentum,
                           float* running_mean, float* running_var, int train, int parts, const float* w2,
                           const float* b2, float* gap, float* h1, float* a1, float* mean1, float* invstd1,
                           float* scale1, float* shift1, float* logits, float* att, void* out, float* workspace,
                           int gap_ready, int dtype, void* stream);
int xv2_splat_tail_backward(const void* x, const void* dout, int N, int64_t hw, int C, int inter,
                            const float* gap, const float* h1, const float* a1, const float* mean1,
                            const float* invstd1, const float* gamma1, const float* w1, const float* w2,
                            const float* att, int train, int parts, float* datt, float* dlogits, float* da1,
                            float* dh1, float* dgap, float* dw2, float* db2, float* dgamma1, float* dbeta1,
                            float* dw1, float* db1, void* dx, float* workspace, int dtype, void* stream);
/* ---- head fusion: the <= 4-channel head of the last decoder layer inside that layer's BatchNorm passes ----
 * The reference's last decoder ConvLayer (model/layers.py:89-100: conv -> norm -> LeakyReLU) feeds OutputBlock's 1x1 convolution
 * (model/layers.py:171-189; model/unet.py:191-197 hands it dec5) and nothing else.  Its activated output z (the largest tensor of
 * the net: N x H x W x 32) and the head's input gradient dz are therefore never stored:
 *   xv2_bn_act_head_forward  (replaces xv2_bn_act_forward + xv2_head_conv_forward, call sites layers.py ConvLayer + unet.py
 *     OutputBlock): logits = head(act(y * scale + shift)) in one pass over y; z stays in registers.
 *   xv2_bn_act_head_backward (replaces xv2_head_conv_backward + xv2_bn_act_backward): both BatchNorm backward passes rebuild
 *     dz[p][c] = sum_o dlogits[p][o] * w[o][c] per element; the second one (dy is elementwise: it walks the tensor in the head
 *     kernel's pixel partition) also leaves the head's dw / db partials (z recomputed from y), folded in fp64 like
 *     xv2_head_conv_backward's.  dy, dgamma, dbeta, sums2, the recorded maximum of dy, the head's dw / db and the logits are
 *     bit-identical to the unfused calls.  workspace: xv2_bn_act_head_backward_workspace(npix, C, Cout) bytes.
 *   xv2_conv_bn_act_head_forward = xv2_conv2d_forward_bn + xv2_bn_act_head_forward behind one call (layer-level, like
 *     xv2_conv_bn_act_forward).
 * Shapes: xv2_bn_act_head_supported(npix, C, Cout) - C a power of two in 4 .. 256 (C / 4 lanes per pixel), Cout 1 .. 4; dense or
 * strided rows (ld % 4 == 0); single-process training-mode BatchNorm without a residual input.  dlogits / logits: fp32, NCHW
 * ([N][Cout][hw]) or NHWC.  The Python layer takes this path for a head that reads one ConvLayer output with no other consumer
 * (networks._decode); XV2_HEAD_FUSE=0 in the environment restores the unfused calls (A/B runs). */
int xv2_bn_act_head_supported(int64_t npix, int C, int Cout);
int xv2_bn_act_head_forward(const void* y, int ldy, const float* scale, const float* shift, int act, int64_t npix,
                            int64_t hw, int C, int Cout, const float* w, const float* bias, float* logits,
                            int nchw_out, int dtype, void* stream);
size_t xv2_bn_act_head_backward_workspace(int64_t npix, int C, int Cout);
int xv2_bn_act_head_backward(const float* dlogits, int nchw_dl, int64_t hw, const float* w, int Cout, const void* y, int ldy,
                             const float* mean, const float* invstd, const float* gamma, const float* scale,
                             const float* shift, int act, double count, void* dy, int lddy, int64_t npix, int C,
                             double* sums2, float* dgamma, float* dbeta, float* dw, float* dbias, float* workspace,
                             int dtype, void* stream);
int xv2_conv_bn_act_head_forward(const xv2_conv_desc* d, const void* x0, int ldx0, const void* x1, int ldx1,
                                 const void* w_ohwi, void* y, int ldy, float* stats_partials,
                                 float* workspace, double* sums, double* scratch, double count, const float* gamma,
                                 const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                 float* mean, float* invstd, float* scale, float* shift, int act, int head_cout,
                                 const float* head_w, const float* head_bias, float* logits, int nchw_out, int dtype,
                                 void* stream);
int xv2_bn_act_backward(const void* dz, int lddz, const void* z, int ldz, const uint8_t* zmask, const void* y,
                        int ldy, const float* mean, const float* invstd, const float* gamma,
                        const float* scale, const float* shift, int act, double count, void* dy, int lddy,
                        void* dres, int lddres, int64_t npix, int C, double* sums2, float* dgamma,
                        float* dbeta, float* workspace, int dtype, void* stream);
/* ---- shortcut fusion: the projection shortcut's BatchNorm inside the bottleneck block's last BatchNorm passes ----
 * A bottleneck block with a projection shortcut (torchvision Bottleneck / ResNeSt Bottleneck with `downsample`: layer1.0 ..
 * layer4.0) ends in z = act(BN3(conv3(a)) + BN_ds(conv_ds(x))).  The shortcut's normalised output idt = BN_ds(y_ds) has one
 * consumer, BN3's apply pass, and the residual gradient dres that pass sends back has one consumer, BN_ds's backward - both are
 * elementwise functions of what the neighbouring pass holds in registers, so neither tensor is stored (five tensor passes and four
 * launches less per block and step):
 *   xv2_bn_act_shortcut_forward  (replaces xv2_bn_act_forward of the shortcut + xv2_bn_act_forward_mask of conv3's layer): one
 *     pass over y3 and y_ds writes z, the byte mask of z and records max |z| (xv2_amax_ctx `out`); idt is rounded to the storage
 *     type the way the unfused pass stores it.
 *   xv2_bn_act_shortcut_backward (replaces xv2_bn_act_backward of both layers): one column pass takes both layers' (sum g,
 *     sum g * xhat) - g = dz * act'(mask) for BN3, g rounded to the storage type (the stored dres) for the shortcut - in the row
 *     chunks of the unfused passes; ONE statistics fold over 2C channels (sums2: [2C][2] doubles, BN3's channels first); one apply
 *     pass writes dy3 and dy_ds, the four parameter-gradient vectors (the fp64 sums rounded to fp32) and records max |dy3|
 *     (xv2_amax_ctx `out`) and max |dy_ds| (amax_dy_ds: 64 slots like `out`, zero beforehand, or NULL).
 *     workspace: xv2_bn_act_shortcut_backward_workspace(npix, C) bytes.
 *   z, the mask, dy3, dy_ds, both layers' sums, dgamma, dbeta and the recorded maxima are bit-identical to the unfused calls.
 * Shapes: xv2_bn_act_shortcut_supported(npix, C, dtype) - the vector path of the column sums (C % 4 == 0 and C / 4 divides 256, or
 * C a multiple of 256); both tensors dense [npix][C] in the same storage type, 16-byte aligned; ReLU / LeakyReLU; single-process
 * training-mode BatchNorm of one batch.  The Python layer takes this path for the tail of Bottleneck / StBottleneck
 * (nn.bottleneck_tail); XV2_SHORTCUT_FUSE=0 in the environment restores the unfused calls (A/B runs). */
int xv2_bn_act_shortcut_supported(int64_t npix, int C, int dtype);
int xv2_bn_act_shortcut_forward(const void* y3, const void* y_ds, const float* scale3, const float* shift3,
                                const float* scale_ds, const float* shift_ds, int act, void* z, uint8_t* zmask,
                                int64_t npix, int C, int dtype, void* stream);
size_t xv2_bn_act_shortcut_backward_workspace(int64_t npix, int C);
int xv2_bn_act_shortcut_backward(const void* dz, const uint8_t* zmask, const void* y3, const void* y_ds,
                                 const float* mean3, const float* invstd3, const float* gamma3, const float* mean_ds,
                                 const float* invstd_ds, const float* gamma_ds, int act, double count, void* dy3,
                                 void* dy_ds, int64_t npix, int C, double* sums2, float* dgamma3, float* dbeta3,
                                 float* dgamma_ds, float* dbeta_ds, void* amax_dy_ds, float* workspace, int dtype,
                                 void* stream);

/* ---- pooling / resampling ----------------------------------------------------------------- */
/* nn.MaxPool2d(3,2,1) (model/unet.py:81); idx = argmax tap (first maximum in scan order).  Backward passes of the pooling
 * layers: accumulate != 0 ADDS the gradient onto what dx already holds - the gradient of the input's other consumer (the
 * decoder's skip connection, model/unet.py:150-170) - instead of a separate elementwise sum. */
int xv2_maxpool3x3s2_forward(const void* x, int N, int H, int W, int C, void* y, uint8_t* idx,
                             int dtype, void* stream);
int xv2_maxpool3x3s2_backward(const void* dy, const uint8_t* idx, int N, int H, int W, int C,
                              void* dx, int accumulate, int dtype, void* stream);
/* nn.AvgPool2d(k, s, pad, count_include_pad) (ResNeSt avd / avg_down shortcuts) */
int xv2_avgpool_forward(const void* x, int N, int H, int W, int C, int k, int s, int pad,
                        int count_include_pad, int OH, int OW, void* y, int dtype, void* stream);
int xv2_avgpool_backward(const void* dy, int N, int H, int W, int C, int k, int s, int pad,
                         int count_include_pad, int OH, int OW, void* dx, int accumulate, int dtype, void* stream);
/* F.adaptive_avg_pool2d(x, bins) (model/layers.py:14; bins=1 is the split-attention GAP) */
int xv2_adaptive_avgpool_forward(const float* x, int ldx, int N, int H, int W, int C, int bins,
                                 float* y, void* stream);
int xv2_adaptive_avgpool_backward(const float* dy, int N, int H, int W, int C, int bins,
                                  float* dx, int lddx, int accumulate, void* stream);
/* F.interpolate(mode="bilinear", align_corners=True) (model/layers.py:27,154,188) */
int xv2_bilinear_forward(const float* x, int N, int IH, int IW, int C, int OH, int OW, float* y,
                         int ldy, void* stream);
int xv2_bilinear_backward(const float* dy, int lddy, int N, int IH, int IW, int C, int OH, int OW,
                          float* dx, void* stream);

/* ---- split attention (ResNeSt SplAtConv2d, radix 2) --------------------------------------- */
/* gap[n][c] = mean_{hw}(x[n,hw,c] + x[n,hw,C+c]) for x NHWC with 2C channels */
int xv2_splat_gap_forward(const void* x, int N, int64_t hw, int C, float* gap, float* workspace,
                          int dtype, void* stream);
size_t xv2_splat_gap_workspace(int N, int64_t hw, int C);
/* small dense layers on [N][Cin] vectors (fc1/fc2 are 1x1 convs on 1x1 maps) */
int xv2_linear_forward(const float* x, const float* w, const float* b, float* y, int N, int Cin,
                       int Cout, void* stream);
int xv2_linear_backward(const float* x, const float* w, const float* dy, float* dx, float* dw,
                        float* db, int N, int Cin, int Cout, void* stream);
/* rSoftMax over the radix axis: logits[n][r*C + c] -> att[n][r*C + c] */
int xv2_rsoftmax_forward(const float* logits, float* att, int N, int C, void* stream);
int xv2_rsoftmax_backward(const float* att, const float* datt, float* dlogits, int N, int C,
                          void* stream);
/* bn0's apply pass that also takes the global average pool's column sums (ResNeSt SplAtConv2d, oracle/backbones.py:115-171;
 * reference call site model/unet.py:52): z = act(y * scale + shift) over [N][hw][2C] (the arithmetic of xv2_bn_act_forward) AND the
 * column-sum partials that xv2_splat_gap_forward would take from z, written to `workspace` (xv2_splat_gap_workspace bytes) -
 * bit-identical partials, no second pass over z, one launch per block less; xv2_splat_gap_finish folds them into gap.
 * xv2_conv_bn_act_forward_grouped(gap_part != NULL) runs it as the layer's apply pass; xv2_splat_tail_forward(gap_ready = 1) then
 * skips the column-sum launch. */
int xv2_bn_act_gap_supported(int C);
int xv2_bn_act_gap_forward(const void* y, const float* scale, const float* shift, int act, void* z, int N, int64_t hw,
                           int C, float* workspace, int dtype, void* stream);
int xv2_splat_gap_finish(int N, int64_t hw, int C, float* gap, const float* workspace, void* stream);
/* out[n,hw,c] = att[n][c]*x[n,hw,c] + att[n][C+c]*x[n,hw,C+c] */
int xv2_splat_apply_forward(const void* x, const float* att, int N, int64_t hw, int C,
                            void* out, int dtype, void* stream);
/* dx (2C channels) += / = ; datt[n][2C] (reduction over hw); dgap adds the GAP branch */
int xv2_splat_apply_backward(const void* x, const float* att, const void* dout,
                             const float* dgap, int N, int64_t hw, int C, void* dx, float* datt,
                             float* workspace, int dtype, void* stream);

/* ---- attention gate glue (model/layers.py:161-166) ---------------------------------------- */
/* r = relu(a + b) */
int xv2_add_relu_forward(const void* a, const void* b, void* r, int64_t n, int dtype, void* stream);
int xv2_add_relu_backward(const void* r, const void* dr, void* dab, int64_t n, int dtype, void* stream);
/* out[p][c] = skip[p][c] * gate[p] */
int xv2_gate_mul_forward(const void* skip, int lds, const float* gate, void* out, int64_t npix,
                         int C, int dtype, void* stream);
int xv2_gate_mul_backward(const void* skip, int lds, const float* gate, const void* dout,
                          void* dskip, float* dgate, int64_t npix, int C, int dtype, void* stream);
/* generic elementwise helpers */
int xv2_add(const float* a, const float* b, float* out, int64_t n, void* stream);
int xv2_axpby(float alpha, const float* a, float beta, const float* b, float* out, int64_t n,
              void* stream);

/* ---- layout --------------------------------------------------------------------------------- */
/* NCHW image [N][C][H][W] (model/plt.py:51 batch["image"]) -> NHWC with Cp >= C (zero padded) */
int xv2_nchw_to_nhwc(const float* x, int64_t x_batch_stride, int N, int C, int H, int W,
                     float* y, int Cp, void* stream);
int xv2_nhwc_to_nchw(const float* x, int ldx, int N, int C, int H, int W, float* y, void* stream);
/* Input hand-over on the device: uint8 HWC tiles [N][H][W][csrc] exactly as cv2.imread /
 * np.concatenate produce them (data_loading/pytorch_loader.py:38,113; csrc = 3, or 6 for the pre|post pair) ->
 * A.Normalize() (pytorch_loader.py:63,90,145: (v - mean*255) * (1 / (std*255)), fp32, statistics applied in STORED
 * channel order) -> fp32 NHWC [N][H][W][4] (channel 3 = 0) of channels c0 .. c0+2, with an optional horizontal /
 * vertical flip (pytorch_loader.py:59-60; model/plt.py:42-48 TTA).  Replaces the host-side normalise + the
 * HWC->CHW transpose (pytorch_loader.py:91,147,170) + xv2_nchw_to_nhwc: the kernels are NHWC. */
int xv2_normalize_u8_to_nhwc(const uint8_t* img_hwc, int csrc, int c0, int N, int H, int W, int hflip,
                             int vflip, const float* mean3, const float* std3, float* out_nhwc4,
                             void* stream);
/* strided channel copy: dst[p][doff + c] = src[p][soff + c] (materialised concat) */
int xv2_copy_channels(const void* src, int lds, void* dst, int ldd, int64_t npix, int C,
                      int dtype, void* stream);

/* ---- losses (model/loss.py:78-101 + monai 0.4.0 DiceLoss/FocalLoss, Ohem == mean CE) ------- */
#define XV2_LOSS_DICE 1
#define XV2_LOSS_FOCAL 2
#define XV2_LOSS_CE 4      /* "ce" and "ohem" (model/loss.py:24-51 is numerically mean CE) */
#define XV2_LOSS_MSE 8     /* "mse" (model/loss.py:92-94), C = 1, exclusive */
#define XV2_LOSS_CORAL 16  /* "coral" (model/loss.py:54-65), C = 3, exclusive */
/* logits NCHW [N][C][H][W]; labels uint8 [N][LH][LW] sampled with stride `lstride`
 * (deep supervision nearest down-sampling, model/plt.py:73).  post != 0 applies the building
 * mask of model/loss.py:86-90 (pixels with label 0 are dropped, label-1 is the class).
 * `terms` is a bit-or of XV2_LOSS_*.  acc[XV2_LOSS_ACC_DOUBLES] doubles of device scratch.    */
#define XV2_LOSS_ACC_DOUBLES 32
int xv2_loss_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W,
                     int lstride, int post, int terms, double* acc, float* loss, float* workspace,
                     void* stream);
size_t xv2_loss_workspace(int N, int C, int H, int W);
/* dlogits = gscale[0] * weight * dLoss/dlogits, uses acc[] written by the forward call */
int xv2_loss_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W,
                      int lstride, int post, int terms, const double* acc, const float* gscale,
                      float weight, float* dlogits, void* stream);
/* ---- "ohem_hard": hard-negative mining with the selection the reference's Ohem intends (ohem.hip) --------
 * Per image i of fp32 NCHW logits (C = 2 or 4) and uint8 labels sampled with `lstride` as above, with
 * l = logsumexp(x) - x[y] per pixel: every positive (y > 0) is kept, of the Cn negatives (y == 0) the
 * k = min(Cn, max(Cn / 4, 5, 2 Cp)) with the largest l.
 *   loss = sum_i (sum of l over positives + sum of the k largest negative l) / sum_i (Cp + k).
 * "ohem" is NOT this: it stays XV2_LOSS_CE, the mean CE the reference computes.  There is no `post` argument: behind
 * the building mask every pixel is its own row with k >= 1, i.e. mean CE over building pixels (criterion.Loss sends
 * that to XV2_LOSS_CE).
 * Outputs, owned by the caller until the backward call has run:
 *   px_loss[N*H*W]  l per pixel; positives hold the sentinel -1; zero is always +0 and NaN always 0x7fc00000, so
 *                   the unsigned bit pattern of a negative's entry orders like its value, NaN above +Inf
 *   records[N][8]   int32: Cp, Cn, k, bits(t), c_gt, c_eq, r, 0 with t the k-th largest negative loss, c_gt / c_eq
 *                   the number of negatives with l > t / l == t and r = k - c_gt (all zero behind Cn when k == 0)
 *   sums[3]         doubles: sum over positives, sum over selected negatives, number of samples sum_i (Cp + k)
 *   loss[1]
 * Tie rule: the loss does not depend on which r of the c_eq tied negatives are taken; the gradient gives each of
 * them the weight r / c_eq (the mean over every valid choice), negatives above t the weight 1, below t 0:
 *   dlogits = gscale[0] * w * (softmax - onehot) / sums[2].
 * This differs from autograd through sort() only on exact ties.  A NaN loss among an image's negatives is its
 * largest, is selected and makes the loss NaN.  The backward pass takes "above / at / below t" from px_loss and the
 * record; it never evaluates l again.  Sums are fp32 inside a thread, fp64 across, in a fixed order; the selection
 * is an exact radix select on integer counts: every output is bitwise reproducible.  9 launches forward, 1 backward,
 * whatever N; nothing is read back.  M = H * W < 2^30, N <= 65535.                                              */
size_t xv2_ohem_workspace(int N, int64_t M);
int xv2_ohem_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W,
                     int lstride, float* px_loss, int* records, double* sums, float* loss,
                     void* workspace, void* stream);
int xv2_ohem_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W,
                      int lstride, const float* px_loss, const int* records, const double* sums,
                      const float* gscale, float* dlogits, void* stream);
/* The select stage alone: per row n of values[N][M], the k[n]-th largest (k device int32, clamped to 0..Cn) among
 * the entries whose sign bit is clear (-0.0 counts as +0; every other entry with the sign bit set is skipped),
 * ordered by bit pattern.  records as above with Cp = 0 and Cn = the number of candidates.  Workspace:
 * xv2_ohem_workspace(N, M).                                                                                      */
int xv2_topk_select(const float* values, int N, int64_t M, const int* k, int* records,
                    void* workspace, void* stream);
/* ---- key sort (sort.hip) ------------------------------------------------------------------------------------------
 * R independent rows of M uint32 keys, ascending: out[r][.] = sort(keys[r][.]).  A stable least-significant-digit radix
 * sort, 8-bit digits, 4 passes of 3 launches (12 launches whatever R and M, rows on gridDim.y), nothing is read back.
 * The sorted order of a key-only sort is unique, so every call gives the same bits.  out may be keys (in place);
 * keys is otherwise left untouched.  1 <= R <= 65535, 1 <= M < 2^30; xv2_sort_workspace is 0 outside that.        */
size_t xv2_sort_workspace(int R, int64_t M);
int xv2_sort_u32(const uint32_t* keys, uint32_t* out, int R, int64_t M, void* workspace, void* stream);
/* ---- "lovasz": the Lovasz-softmax loss (Berman et al., CVPR 2018, Algorithm 1; lovasz.hip) -----------------------
 * classes = "present", per_image = False: the whole batch is one set per class.  fp32 NCHW logits (C = 2 or 4), uint8
 * labels sampled with `lstride` as above, M = N * H * W < 2^30.  post == 0: a pixel's class is its label.  post != 0:
 * pixels with label 0 are SKIPPED (in no class's set), the class is label - 1.  class_mask: bit c set = class c takes
 * part in the mean (criterion.Loss: 0b10 for --type pre, the building class; 0b1111 for --type post).
 * For class c: fg = (class == c), error e = 1 - p(c) if fg else p(c), p the channel softmax; G foreground and Nb
 * background pixels.  With B_>(v) / b the background errors > v / == v and F_>=(v) the foreground errors >= v:
 *   foreground weight  w = 1 / (G + B_>(e))
 *   background weight  w = (G - F_>=(e)) / ((G + B_>(e)) (G + B_>(e) + b))
 *   loss_c = sum e w,  loss = mean of loss_c over the classes of class_mask with G > 0 (0 when there is none)
 * which is the sum of e_(j) (J_j - J_(j-1)) over the errors in descending order.  Tie rule: among equal errors the
 * foreground comes first and the b tied background entries share their telescoped Jaccard increment equally, the mean
 * over every order of the tied group: a valid subgradient that depends on no order.
 * Outputs, owned by the caller until the backward call has run:
 *   keys[C][M]     bits(e) | fg << 31; e is canonical (zero is +0, NaN the one pattern 0x7fc00000, above 1.0, which makes
 *                  the loss NaN); skipped pixels hold 0xFFFFFFFF.  Written for every class.
 *   sorted[C][M]   each row of keys ascending: background ascending, foreground ascending, skipped.  Written for the
 *                  classes from the lowest to the highest one in class_mask; the other rows are not touched.
 *   records[C][4]  int32: G, Nb, skipped, 1 if the class is in class_mask and G > 0 else 0
 *   sums[5]        doubles: loss_c for c < C (0 for a class that is not included and present, and for c >= C), then
 *                  sums[4] = n_present
 *   loss[1]
 * Backward: dlogit_k = gscale[0] * p_k (g_k - sum_c g_c p_c) with g_c = -w / n_present (foreground), +w / n_present
 * (background), 0 for skipped pixels and classes that are not included and present.  It takes every comparison from the
 * saved keys and the sorted rows, never from an error evaluated again.  Counts are integers, products and sums fp64 in a
 * fixed order: every output is bitwise reproducible.  16 launches forward, 1 backward; nothing is read back.         */
size_t xv2_lovasz_workspace(int N, int C, int H, int W);
int xv2_lovasz_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W,
                       int lstride, int post, unsigned class_mask, uint32_t* keys, uint32_t* sorted,
                       int* records, double* sums, float* loss, void* workspace, void* stream);
int xv2_lovasz_backward(const float* logits, int N, int C, int H, int W, const uint32_t* keys,
                        const uint32_t* sorted, const int* records, const double* sums,
                        const float* gscale, float* dlogits, void* stream);
/* ---- "wce": cross-entropy with a per-pixel weight, class weights + border map (wce.hip, wce_px.h) ------------------------
 * fp32 NCHW logits (C = 2 or 4), uint8 labels [N][LH][LW] sampled with `lstride` exactly as xv2_loss_forward samples them.
 * post == 0: a pixel's class is its label.  post != 0: pixels with label 0 are dropped, the class is label - 1 (as
 * XV2_LOSS_CE).  A pixel whose class is >= C is dropped as well.  With l(p) = logsumexp(x_p) - x_p[class] and
 * w(p) = class_w[class(p)] + b(p) over the pixels that are not dropped:
 *   loss    = sum_p w(p) l(p) / sum_p w(p)
 *   dlogits = gscale[0] * w(p) * (softmax - onehot) / sum_p w(p)
 * With b == 0 this is torch.nn.functional.cross_entropy(weight = class_w, reduction = "mean").  The weight is a constant of the
 * labels: it gets no gradient.  sum w == 0 (no pixel left, or every present class weighted 0): loss is exactly +0 and dlogits
 * exact zeros.  A NaN logit gives a NaN loss and the call returns.  class_w: C floats ON THE DEVICE, finite and >= 0 (the
 * caller's duty: nothing is read back).  Sums are fp32 inside a thread and fp64 across threads in a fixed order: two calls give
 * the same bits.  sums[2]: sum w l, sum w, owned by the caller until the backward call has run.  2 launches forward, 1 backward.
 *
 * Border term b(p), post == 0 only (Ronneberger et al., U-Net, 2015: w0 exp(-(d1 + d2)^2 / (2 sigma^2))).  Components are the
 * 4-connected components of label > 0 in the FULL-RESOLUTION label map, as xv2_label_components numbers them.  For a
 * background pixel p and a component k, delta_k(p) is the smallest squared pixel-centre distance dy^2 + dx^2 <= R^2 from p to
 * a pixel of k inside the image (no padding: a pixel outside the image is no building).  D1(p) is the smallest delta_k, D2(p)
 * the second smallest over the components (they may be equal); 0xFFFF stands for "none within R", and building pixels hold
 * 0xFFFF in both.  D1 and D2 are integers in 1..1024 that depend on no scan order.
 *   b(p) = w0 * exp(-(sqrt(D1) + sqrt(D2))^2 / (2 sigma^2)) where D2 != 0xFFFF, else 0,
 * evaluated in fp32 as w0 * expf(-(D1 + D2 + 2 sqrtf(D1 D2)) / (2 sigma sigma)), each operation rounded once (D1 + D2 and
 * D1 D2 <= 2^20 are exact), by ONE device function (wce_px.h) that the map entry, the forward and the backward pass share:
 * their weights hold identical bits, and the backward pass never reads a stored float.  With lstride > 1 the distances stay
 * those of the full-resolution labels, read at (y lstride, x lstride) like the labels: the geometry is in full-resolution
 * pixels for every deep-supervision head.  Labelled buildings that touch in the raster are ONE component with no border
 * between them: the map weights gaps that exist in the label, up to 2R wide.
 *
 * xv2_border_distances: labels uint8 [B][H][W] -> d1, d2 uint16 [B][H][W].  xv2_label_components into the workspace (int32
 * per pixel), then one block per 32 x 32 tile with its (32 + 2R)^2 labels in LDS; nothing is read back, the launches do not
 * depend on the content.  1 <= R <= 32, H W < 2^30, B <= 65535.
 * xv2_border_weights: the fp32 map b alone over n entries (tests, utils/border_map.py).  w0 >= 0, sigma > 0, both finite.
 * xv2_wce_forward / backward: d1 and d2 both NULL = no border term (w0 and sigma are then ignored), else [N][LH][LW] as above;
 * post != 0 with distance maps is XV2_EINVAL.  N <= 65535.                                                                  */
size_t xv2_border_workspace(int B, int H, int W);
int xv2_border_distances(const uint8_t* labels, int B, int H, int W, int R, void* workspace, uint16_t* d1,
                         uint16_t* d2, void* stream);
int xv2_border_weights(const uint16_t* d1, const uint16_t* d2, int64_t n, float w0, float sigma, float* out,
                       void* stream);
size_t xv2_wce_workspace(int N, int C, int H, int W);
int xv2_wce_forward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                    int post, const float* class_w, const uint16_t* d1, const uint16_t* d2, float w0,
                    float sigma, double* sums, float* loss, void* workspace, void* stream);
int xv2_wce_backward(const float* logits, const uint8_t* labels, int N, int C, int H, int W, int lstride,
                     int post, const float* class_w, const uint16_t* d1, const uint16_t* d2, float w0,
                     float sigma, const double* sums, const float* gscale, float* dlogits, void* stream);
/* argmax over channels of NCHW logits (utils/f1.py:14,36), equal to torch.argmax: the first maximum wins, a NaN is the
 * maximum and the first NaN wins */
int xv2_argmax_nchw(const float* logits, int N, int C, int64_t hw, int add, uint8_t* labels,
                    void* stream);
/* F1 bookkeeping (utils/f1.py:27-47): counts[(c-1)*3 + {tp, fn, fp}] += ... for classes c = 1..n_class-1 over two
 * uint8 label maps; masked != 0 counts only pixels whose target is > 0 (damage task).  `counts` (int64, device) is
 * accumulated into, never cleared. */
int xv2_f1_counts(const uint8_t* pred, const uint8_t* target, int64_t total, int n_class, int masked,
                  int64_t* counts, void* stream);

/* ---- grouped layers behind one call (ResNeSt's radix-2 3x3 convolution: reference call site model/unet.py:52 via the
 * resnest encoders, oracle/backbones.py:115-171 Conv2d(groups = 2) -> bn0 -> ReLU).  `d` describes ONE group (C0 and Cout are
 * channels per group), the ld* arguments are the channel strides of the whole tensors, w[g] are the packed weights of group g.
 * Each function issues exactly the per-group calls named in its comment, group after group: bit-identical to them. */
/* groups x xv2_conv2d_forward_bn (statistics + coefficients of the group's channels), then ONE xv2_bn_act_forward[_mask] over
 * all groups * Cout channels */
int xv2_conv_bn_act_forward_grouped(const xv2_conv_desc* d, int groups, const void* x0, int ldx0,
                                    const void* const* w_ohwi, void* y, int ldy, float* stats_partials, int64_t tiles,
                                    float* workspace, double* sums, double* scratch, double count,
                                    const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var, float* mean, float* invstd,
                                    float* scale, float* shift, const void* residual, int ldr, int act, void* z,
                                    int ldz, uint8_t* zmask, float* gap_part, int dtype, void* stream);
/* groups x xv2_conv2d_backward_data_acc */
int xv2_conv2d_backward_data_grouped(const xv2_conv_desc* d, int groups, const void* dy, int lddy,
                                     const void* const* w_ihwo, void* dx0, int lddx0, int accumulate,
                                     float* workspace, int dtype, void* stream);
/* xv2_conv2d_backward_weight_async for the first group (the hop to side_stream), xv2_conv2d_backward_weight on side_stream for
 * the others; dw_oihw holds the groups' gradients back to back ([groups * Cout][cin_real][KH][KW]) */
int xv2_conv2d_backward_weight_async_grouped(const xv2_conv_desc* d, int groups, const void* x0, int ldx0,
                                             const void* dy, int lddy, float* dw_oihw, int cin_real,
                                             float* workspace, int dtype, void* side_stream, void* stream);

/* ---- optimizer (model/plt.py:154 torch.optim.AdamW) ---------------------------------------- */
int xv2_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   float grad_scale, void* stream);

/* hipGraph-capturable variant: learning rate and step counter are read from device memory (the step counter is
 * incremented by the call), so a captured training step can be replayed while the schedule advances */
int xv2_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                       int* step_dev, float grad_scale, void* stream);

/* The other --optimizer rules (model/plt.py:150-161) on the same flat buffers, graph-capturable like
 * xv2_adamw_step_dev: lr and the step counter live in device memory, the call increments the counter.
 * xv2_flat_step_dev: one elementwise launch (+ the counter increment); `rule`
 *   0 sgd without momentum     model/plt.py:152  apex FusedSGD(lr, momentum=0)             (state0, state1 unused)
 *   1 sgd with momentum        model/plt.py:152  apex FusedSGD(lr, momentum)                (state0 = momentum buffer)
 *   2 radam                    model/plt.py:155  torch_optimizer RAdam(lr, weight_decay)    (state0/1 = exp_avg / exp_avg_sq)
 *   3 adabelief                model/plt.py:156  torch_optimizer AdaBelief(lr, weight_decay) (state0/1 = exp_avg / exp_avg_var)
 *   4 adabound                 model/plt.py:157  torch_optimizer AdaBound(lr, weight_decay) (state0/1 = exp_avg / exp_avg_sq;
 *                                                base_lr = lr at construction, final_lr / gamma the package's)
 * momentum is rule 1's, base_lr / final_lr / gamma rule 4's; the others ignore them.  The betas travel as double so
 * that 1 - beta is formed before the rounding to fp32 (1 - 0.999f is 1.3e-5 away from 0.001). */
int xv2_flat_step_dev(int rule, float* param, const float* grad, float* state0, float* state1, int64_t n,
                      const float* lr_dev, int* step_dev, double beta1, double beta2, float eps, float weight_decay,
                      float momentum, float base_lr, float final_lr, float gamma, float grad_scale, void* stream);

/* Segmented rules: rows = int64 [rows_total][3] {first element, length, tensor} (one row per dim-0 slice of a tensor
 * with >= 2 dims, one row per other tensor), tensors = int64 [ntensors][4] {first row, rows, numel, dims >= 2},
 * partials = float [rows_total][4] scratch.  Three launches (row sums, per-tensor fold, apply) + the counter increment;
 * fixed reduction order, no atomics.
 * xv2_adamp_step_dev replaces model/plt.py:158 torch_optimizer AdamP(lr, weight_decay) (delta, wd_ratio the
 * package's defaults); decision = int [ntensors] (0 no projection, 1 channel view, 2 layer view of the step),
 * aux = float [ntensors][2] scratch. */
int xv2_adamp_step_dev(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors,
                       float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* partials,
                       int* decision, float* aux, const float* lr_dev, int* step_dev, double beta1, double beta2,
                       float eps, float weight_decay, float delta, float wd_ratio, float grad_scale, void* stream);

/* replaces model/plt.py:159 apex FusedNovoGrad(lr, weight_decay): norm_avg = float [ntensors], the blended per-tensor
 * gradient norm (the step-1 launch sets it to the first norm) */
int xv2_novograd_step_dev(const int64_t* rows, int64_t rows_total, const int64_t* tensors, int ntensors,
                          float* param, const float* grad, float* exp_avg, float* norm_avg, float* partials,
                          const float* lr_dev, int* step_dev, double beta1, double beta2, float eps,
                          float weight_decay, float grad_scale, void* stream);

/* Gradient guard: global-norm clipping (torch.nn.utils.clip_grad_norm_, PL's Trainer(gradient_clip_val)) and the skipping of a
 * step whose gradient holds an Inf or NaN (what the reference's --precision 16 GradScaler does, main.py:99), decided on the
 * device between the backward pass and any of the device-state rules above.
 * xv2_grad_guard: two launches over grad[0 .. n) - the sum of squares in double (16-byte loads where `grad` is 16-byte
 *   aligned, one double per block in `workspace` = xv2_grad_guard_workspace(n) bytes, a grid that depends on n alone, fixed
 *   lane order and butterfly, no atomics: bitwise reproducible), then a one-block fold that adds the partials in index order
 *   and writes `guard`, a 64-byte, 8-byte aligned record the caller zeroes ONCE and keeps for the run:
 *     byte  0  float   norm              grad_scale * sqrt(sum), of this call (grad_scale: the reducer's 1 / world)
 *     byte  4  float   coef              min(max_norm / (norm + 1e-6), 1), computed in double; 1 when max_norm == 0 (no clipping)
 *     byte  8  int32   skip              1: skip_nonfinite != 0 and the norm is not finite
 *     byte 12  int32   skipped_in_a_row  consecutive skipped calls up to and including this one
 *     byte 16  int64   steps             calls so far          (these three accumulate)
 *     byte 24  int64   clipped           calls with coef < 1 that were not skipped
 *     byte 32  int64   skipped           calls with skip = 1
 *     byte 40  float   norm_max          the largest finite norm so far
 *     bytes 44 .. 63   reserved
 *   With skip_nonfinite == 0 the formula is applied as it stands: an Inf norm gives coef 0, a NaN norm gives NaN, as in torch.
 *   A finite fp32 squared cannot overflow a double, so the one reduction answers both questions.
 * xv2_optim_guard_ctx(guard) names the record for the NEXT optimizer entry point of THIS host thread (xv2_adamw_step_dev,
 *   xv2_flat_step_dev, xv2_adamp_step_dev, xv2_novograd_step_dev); it is cleared when that call returns, whatever it returns
 *   (the lifetime of xv2_amax_ctx).  The call then runs the guarded instantiation of its kernels: the effective gradient scale
 *   is grad_scale * coef, read from the device, and with skip = 1 every kernel returns before touching anything - parameters,
 *   state arrays, decision / norm_avg and the step counter stay bit for bit (scaling the gradient to zero would not be a skip:
 *   moments and weight decay would still move).  NULL, or no call: the kernels without a guard.  xv2_adamw_step takes its
 *   step from the host and refuses a guard (XV2_EINVAL). */
size_t xv2_grad_guard_workspace(int64_t n);
int xv2_grad_guard(const float* grad, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, void* workspace,
                   void* guard, void* stream);
int xv2_optim_guard_ctx(const void* guard);

/* Exponential moving average of the weights, taken right after any of the optimizer entry points above on the same flat buffer
 * (a launch of its own: the rule kernels are not touched).  t = *count_dev, the updates applied so far, is read on the device;
 *   d  = warmup ? min(decay, (1 + t) / (10 + t)) : decay        in double
 *   om = (float)(1.0 - d)                                       the complement formed before the one rounding, like the betas
 *   ema[i] = fmaf(om, param[i] - ema[i], ema[i])                one rounded subtraction, one fused multiply-add
 * so param[i] == ema[i] leaves ema[i] bit for bit (but for the sign of a zero: an average of -0 comes back as +0, since
 * (-0) - (-0) = +0 and +0 + -0 = +0) and a non-finite parameter reaches only its own element.  16-byte loads and
 * stores when both pointers are 16-byte aligned, the same operations in a scalar loop for the tail and otherwise; the call's
 * last launch increments *count_dev.  `guard` is NULL or the 64-byte record of xv2_grad_guard, passed explicitly (NOT through
 * xv2_optim_guard_ctx): with its skip word set every kernel returns before touching anything - ema and *count_dev stay bit for
 * bit, a skipped optimizer step neither pulls the average towards unchanged weights nor advances the warm-up; coef is ignored.
 * decay and warmup are the only host values that enter, so a captured step that contains the call stays valid.
 * n == 0: OK without a launch.  decay outside [0, 1) or NaN, n < 0, or n > 0 with a NULL pointer: XV2_EINVAL. */
int xv2_ema_update_dev(float* ema, const float* param, int64_t n, double decay, int warmup, int* count_dev,
                       const void* guard, void* stream);

/* Gradient accumulation over micro-batches (--accumulate_grad_batches): the HIP backward kernels overwrite their slice of the
 * flat gradient buffer, so the sum over a group of micro-batches is kept in a second flat buffer `acc` of the same layout.  One
 * launch over acc[0 .. n) and grad[0 .. n), any slice of the two buffers (the pointers need not be their bases):
 *   mode 0  open    acc[i]  = grad[i]                     8 bytes per element    after the group's first micro-batch
 *   mode 1  add     acc[i]  = acc[i] + grad[i]           12 bytes per element    after every further one but the last
 *   mode 2  close   grad[i] = acc[i] + grad[i]           12 bytes per element    after the last: `acc` is only read
 * Each element gets exactly one IEEE fp32 addition, round to nearest even: no fma, no scaling, no reordering.  The gradient of a
 * group of m micro-batches g1 .. gm is therefore ((g1 + g2) + g3 ... ) + gm bit for bit, summed in micro-batch order, a function
 * of the inputs alone - what torch's own .grad accumulation computes.  A non-finite element reaches only its own element.  The
 * division by m is NOT done here: it rides in the rule's grad_scale, as the reducer's 1 / world does.  16-byte loads and stores
 * when both pointers are 16-byte aligned, the same operation in a scalar loop for the tail and otherwise.
 * n == 0: OK without a launch.  n < 0, n > 0 with a NULL pointer, a mode outside 0 .. 2, or acc[0 .. n) and grad[0 .. n)
 * overlapping: XV2_EINVAL before any launch. */
int xv2_grad_accumulate(float* acc, float* grad, int64_t n, int mode, void* stream);

/* ---- in-library kernel timing (bench.py roofline leg) --------------------------------------
 * When enabled, every launch of an MFMA kernel (implicit-GEMM conv / weight-gradient) is bracketed
 * by hipEvents on its own stream and tagged with its algorithmic FLOP count (2*M*N*K of the
 * convolution it computes, real channel counts) and its algorithmic byte count (each operand read
 * once, the result written once).  xv2_prof_summary synchronises the recorded
 * events and returns the totals per kernel id.
 * xv2_prof_enable: 0 = off, 1 = every MFMA launch, 2 + kid = only launches of kernel id `kid` (the timed region
 * of bench.py brackets just the dominant kernel: 400 event records per step cost 1.3 ms, 160 cost a third). */
int xv2_prof_enable(int on);
/* bracket only every n-th eligible launch (n coprime with the launches per step rotates through the layers): the
 * event records themselves cost ~3 us each on the stream */
int xv2_prof_stride(int n);
int xv2_prof_num_kernels(void);
const char* xv2_prof_kernel_name(int kid);
int xv2_prof_summary(int kid, double* total_ms, double* total_flops, double* total_algorithmic_bytes,
                     int64_t* launches);
int xv2_prof_num_records(void);
int xv2_prof_record(int i, int* kid, double* ms, double* flops, double* algorithmic_bytes);

/* ---- training-time augmentation of the uint8 tiles on the device ---------------------------------------
 * The albumentations recipe the reference's datasets apply to the uint8 tile before A.Normalize()
 * (data_loading/pytorch_loader.py:57-63,77-91): CropNonEmptyMaskIfExists(512, 512), HorizontalFlip, VerticalFlip, GaussNoise,
 * RandomBrightnessContrast.  The random DECISIONS are drawn on the host; this launch moves the bytes - crop origin + flips as a
 * gather, the Gaussian field from a counter-based generator (splitmix64 of seed and element index, Box-Muller in fp64; the
 * same field on host and device), brightness / contrast as a 256-entry table per image - for image and mask together.
 * params: [N][16] int32 in device memory = {src, H, W, y0, x0, hflip, vflip, noise[2], sigma[2] (float bits), seed_lo[2],
 * seed_hi[2], lut bits}; src_img / src_mask: device arrays of device pointers to the source tiles (uint8 [H][W][C] /
 * [H][W]; src_mask may be NULL), row `src` of them belongs to the sample; luts [N][2][256]; outputs img [N][h][w][C] and
 * mask [N][h][w].  C = 3 (pre) or 6 (pre | post: the two images draw their own noise and table).  Bit-exact against
 * xview2_amd.data_loading.device_aug.apply_params_numpy (tests/test_augment_gpu.py). */
int xv2_augment_u8(const void* params, const void* src_img, const void* src_mask, const uint8_t* luts, int N, int C,
                   int h, int w, uint8_t* img, uint8_t* mask, void* stream);

/* A.RandomScale(p=0.2, scale_limit=(0, 0.3), interpolation=INTER_CUBIC) of the same recipe (data_loading/pytorch_loader.py:57-63;
 * this project's worker path resizes with Pillow: pytorch_loader.apply_scale) for the Z zoomed samples of a batch in ONE launch:
 * the [y0:y0+h, x0:x0+w] window of the bicubic-resized tile and of the nearest-resized mask, the one-off sources of the
 * xv2_augment_u8 call that follows.  The twin is of PILLOW's uint8 resampler: integer arithmetic on 22-bit fixed-point
 * coefficients, horizontal pass -> round, clip to uint8 -> vertical pass -> round, clip; only the coefficient tables are
 * floating point (fp64) and the host builds them (xview2_amd.data_loading.device_aug.resample_tables / nearest_table).
 * params: [Z][8] int32 in device memory = {src, H, W, xoff, yoff, nxoff, nyoff, 0}: row of the pointer tables, source tile
 * size and the offsets (in int32 elements) of the sample's tables in `tables`: at xoff [w][7] = {start, count, k[5]} of the
 * window's columns, at yoff [h][7] of its rows (source index of the first tap, number of taps <= 5, coefficients * 2^22),
 * at nxoff [w] / nyoff [h] the mask's nearest source column / row.  Up-scaling only (count <= 4 unclamped, a 32-row tile
 * reads <= 36 source rows).  src_img / src_mask as in xv2_augment_u8; outputs img [Z][h][w][C], mask [Z][h][w]; C = 3 or 6.
 * Bit-exact against device_aug.zoom_crop_numpy and Pillow (tests/test_zoom_cpu.py, tests/test_zoom_gpu.py). */
int xv2_zoom_crop_u8(const void* params, const int32_t* tables, const void* src_img, const void* src_mask, int Z, int C,
                     int h, int w, uint8_t* img, uint8_t* mask, void* stream);

/* `--autoaugment` (data_loading/autoaugment.py ImageNetPolicy; this project's worker path runs it through Pillow:
 * xview2_amd/data_loading/autoaugment.py) for the N cropped samples of a batch, IN PLACE on img [N][h][w][C] and mask [N][h][w] -
 * the outputs of an xv2_augment_u8 call without flips, noise or tables.  Every sample runs the 0 .. 2 operations the host drew
 * for it (autoaugment.draw_policy), stage 2 on stage 1's output; the twin is of PILLOW's bytes for the ten operations of the
 * POLICY table: posterize / solarize / invert (host-built 256-byte tables), autocontrast / equalize (tables built on the device
 * from per-channel histograms: integer counts, equalize in integers, autocontrast one fp64 multiply and add per entry), color /
 * contrast / sharpness (Image.blend in float32 against L, the rounded mean of L, ImageFilter.SMOOTH), rotate (NEAREST gather
 * in 16.16 fixed point, zero fill, image and mask) and shearX (BICUBIC in fp64, zero fill, image AND mask: the reference
 * interpolates labels).  The same operation runs on each 3-channel part in STORED channel order, on the mask only if geometric.
 * params: [N][2][8] int32 in device memory, per sample and stage {op, a[6], 0}: op 0 none, 1 host-built table, 2 autocontrast,
 * 3 equalize, 4 color, 5 contrast, 6 sharpness (a[0] = bits of the float32 factor 1 + magnitude * sign), 7 rotate (a[0..5] =
 * the fixed-point coefficients a0 .. a5 of Geometry.c affine_fixed), 8 shearX (a[1], a[2] = low and high word of the fp64
 * coefficient); host_params: the same table in HOST memory - it is validated (unknown ids are rejected) and decides which
 * launches a stage needs, the device never reports back; luts: [N][2][256] uint8 in device memory, the table of (sample, stage)
 * where op = 1 (NULL if no sample has one).  Per stage at most a statistics, a table and an apply launch, ordered by `stream`
 * alone; nothing is enqueued when no sample has an operation.  workspace: xv2_autoaugment_workspace(N, C, h, w) bytes (histograms,
 * sums, tables and one copy of the batch: a gather cannot run in place), 0 for arguments the entry point rejects.  C = 3 or 6,
 * h * w <= 2^24.  Bit-exact against device_autoaug.autoaug_numpy and Pillow (tests/test_autoaug_cpu.py, tests/test_autoaug_gpu.py). */
size_t xv2_autoaugment_workspace(int N, int C, int h, int w);
int xv2_autoaugment_u8(const int32_t* host_params, const void* params, const uint8_t* luts, int N, int C, int h, int w,
                       uint8_t* img, uint8_t* mask, void* workspace, void* stream);

/* ---- SyncBatchNorm statistics exchange without a collective library call ------------------------------------------
 * (reference: Trainer(sync_batchnorm=gpus > 1), main.py:106 - torch.nn.SyncBatchNorm exchanges <= 32 KB per BatchNorm
 * layer and direction, 126 ... 606 times per step).  Every rank allocates one exchange buffer (xv2_xchg_alloc returns
 * its 64-byte hipIpc handle), the ranks of the node swap handles through their process group and map each other's
 * buffers (xv2_xchg_open).  xv2_xchg_allreduce then sums `n` doubles over the ranks IN PLACE with one single-block launch:
 * each rank stores its vector straight into every peer's buffer over xGMI (write-through 8-byte stores + a sequence-number
 * flag), waits for the `world` flags of its own buffer and adds the rows in RANK order (identical bits on every rank).
 * `seq` counts the exchanges of the job (same value on every rank); `peers_dev` = device array of the `world` mapped base
 * pointers (own buffer at index `rank`); `timeout_flag` (device int) becomes non-zero if a peer never arrived within the
 * spin limit (xv2_xchg_set_spin_limit polls, default 2^26 ~ seconds) - from then on every exchange writes NaN instead of a
 * sum of stale rows (a failed exchange must be loud: NaN statistics -> NaN loss; the collective library would have waited).
 * xv2_xchg_alloc: *finegrained = 1 if the runtime granted fine-grained device memory (coherent across GPUs while kernels
 * run), 0 if it fell back to ordinary device memory - usable only when all ranks share ONE device; a caller on a multi-GPU
 * node must then stay with the collective library (xview2_amd.dist.stats_all_reduce_ does). */
size_t xv2_xchg_bytes(int world, size_t row_doubles);
int xv2_xchg_alloc(int world, size_t row_doubles, void** base_out, unsigned char* handle64, int* finegrained);
int xv2_xchg_set_spin_limit(unsigned polls);
int xv2_xchg_open(const unsigned char* handle64, void** peer_base);
int xv2_xchg_close(void* peer_base);
int xv2_xchg_free(void* base);
int xv2_xchg_allreduce(double* vals, int n, const void* peers_dev, int world, int rank, size_t row_doubles,
                       uint64_t seq, int* timeout_flag, void* stream);

/* ---- offline post-processing and scoring (utils/post_process.py, utils/xview2_metrics.py) ---------------------------
 * Batches of B tiles of H x W, row-major.  Connected-component labels: 1 + the smallest in-tile linear index
 * (y * W + x) of the pixel's 4-connected component, 0 = background (np.unique(labels, return_inverse=True) gives
 * scipy.ndimage.label's numbering). */
#define XV2_DMG_4CH 0    /* fp32 [B,4,H,W] damage probabilities: post = argmax + 1 (post_process.py:31-32) */
#define XV2_DMG_5CH 1    /* fp32 [B,5,H,W] background + 4 damage channels: argmax over channels 1..4, + 1 */
#define XV2_DMG_LABEL 2  /* int32 [B,H,W] decoded label map (coral / mse: post_process.py:33-34) */
/* Workspace bytes of xv2_postprocess: 22 per pixel with components (counts, labels, pre / post intermediates), 2
 * without (used only when dilating).  Nothing in it needs clearing by the caller. */
size_t xv2_postprocess_workspace(int B, int H, int W, int components);
/* post_process.py:28-44: pre = (loc > 0.3f) | ((loc > 0.1f) & (post > 1)) in float32, post *= pre; components != 0:
 * every pixel of a 4-connected component of post > 0 takes the component's most frequent post value (ties: the smaller,
 * post_process.py:40-43); rate > 0 (odd, <= 65): both maps dilated by a rate x rate square clamped to the image
 * (post_process.py:44-45); uint8 [B,H,W] pre and post out.  An even rate, another dmg_kind or a non-positive size is
 * XV2_EINVAL.  workspace may be NULL when components == 0 and rate == 0.
 * Label maps: any int32 value is read; only the values that survive the fusion (pre set) must be representable:
 * 0..255 (the uint8 PNG), or 0..4 with components (the vote keeps four classes per component).  A surviving value outside
 * that range is written as background and counted into *status (device int32, accumulated, never cleared; required for
 * XV2_DMG_LABEL, may be NULL otherwise), so the caller can reject the result. */
int xv2_postprocess(const float* loc, const void* dmg, int dmg_kind, int B, int H, int W, int components, int rate,
                    void* workspace, uint8_t* pre, uint8_t* post, int32_t* status, void* stream);
/* xv2_postprocess with the fusion's constants as arguments: pre = (loc > t_loc) | ((loc > t_dmg) & (post > 1)), both
 * compared in float32, and with class_scale (a HOST pointer to 4 floats, or NULL) post = 1 + the first maximum of the
 * float32 products class_scale[c] * dmg[c] (each rounded once); NULL: no multiplication.  Everything after the fusion is
 * xv2_postprocess's.  xv2_postprocess is this call with (0.3f, 0.1f, NULL).  A non-finite threshold, t_dmg > t_loc, a scale
 * that is not finite and > 0, or scales with XV2_DMG_LABEL (a label map has no channels to scale) are XV2_EINVAL. */
int xv2_postprocess_ex(const float* loc, const void* dmg, int dmg_kind, int B, int H, int W, int components, int rate,
                       void* workspace, uint8_t* pre, uint8_t* post, int32_t* status, float t_loc, float t_dmg,
                       const float* class_scale, void* stream);
/* The joint histogram from which every point of a threshold / class-scale grid of xv2_postprocess_ex can be scored
 * (calibrate.hip, xview2_amd/utils/calibrate.py).  loc, dmg, dmg_kind as xv2_postprocess reads them; lt, dt: uint8 [B,H,W],
 * the localization and damage targets.  thresholds: DEVICE fp32 [n], 1 <= n <= 128, finite and strictly ascending (device
 * memory is not read back: ops.calibrate_hist checks the host copy it uploads; a table out of order gives a histogram that
 * means nothing, never a fault).  scales: DEVICE fp32 [S][4], finite and > 0 (checked by ops.calibrate_hist likewise),
 * 1 <= S <= 64, or NULL for S = 1 and no multiplication; must be NULL for XV2_DMG_LABEL.  Per pixel and scale vector s:
 *   k = #{ j : loc > thresholds[j] } in float32 (0..n; NaN gives 0; monotone, so loc > thresholds[j] <=> k > j),
 *   r = post - 1 (0..3), post decoded as xv2_postprocess_ex decodes it with class_scale = scales[s],
 *   t = lt > 0,  d = dt (0..4),
 * and hist[s][k][r][t][d] += 1, hist int64 [S][n+1][4][2][5].  A pixel with lt > 4 or dt > 4, or for XV2_DMG_LABEL a value
 * outside 1..4, adds to bad[0] (int64, once per pixel, not once per scale vector) and to no bin.  hist and bad are
 * accumulated into, never cleared (as xv2_xview2_counts), so one histogram covers a dataset over many calls; integer adds
 * make the result independent of the schedule.  Size limits as xv2_postprocess. */
int xv2_calibrate_hist(const float* loc, const void* dmg, int dmg_kind, const uint8_t* lt, const uint8_t* dt, int B, int H,
                       int W, const float* thresholds, int n, const float* scales, int S, int64_t* hist, int64_t* bad,
                       void* stream);
/* Measurement switch of scripts/bench_calibrate.py: how many rounds of per-wave combining of equal keys later
 * xv2_calibrate_hist calls of the process make before every lane left adds its own one; 0: one LDS atomic per pixel (the
 * naive form), negative: the built-in default.  Same histogram whatever the value; no product code sets it. */
int xv2_calibrate_hist_rounds(int rounds);
/* scipy.ndimage.label of mask != 0 (post_process.py:39) with the labels above, int32 [B,H,W] out.  workspace is
 * unused (may be NULL); labels is the union-find's own storage. */
int xv2_label_components(const uint8_t* mask, int B, int H, int W, void* workspace, int32_t* labels, void* stream);
/* xview2_metrics.py RowPairCalculator.get_row_pair over four uint8 [B,hw] maps: counts[b*16 + ...] += [lTP, lFN, lFP],
 * [TP, FN, FP] x damage classes 1..4, then the number of pixels holding a value > 4 in any map.  `counts` (int64,
 * device) is accumulated into, never cleared. */
int xv2_xview2_counts(const uint8_t* lp, const uint8_t* dp, const uint8_t* lt, const uint8_t* dt, int B, int64_t hw,
                      int64_t* counts, void* stream);

/* ---- per-building table of a prediction (buildings.hip, xview2_amd/utils/buildings.py) -------------------------------
 * labels: int32 [B,H,W] as xv2_label_components writes them; dmg: uint8 [B,H,W]; loc: fp32 [B,H,W] or NULL.
 * count[b] (int32 [B]) = the number of components of tile b, the true number even above max_rows.  rows: int64
 * [B][max_rows][16]; rows 0 .. min(count[b], max_rows) - 1 are written, in ascending order of column 0 (scipy.ndimage.label's
 * numbering for 4-connectivity); nothing else of rows is touched.  count is overwritten by every call; neither it nor the
 * workspace needs clearing.  Columns:
 *   0        root: label - 1, the linear index y * W + x of the component's first pixel in raster order
 *   1        area in pixels
 *   2..5     ymin, xmin, ymax, xmax (inclusive)
 *   6, 7     sum of y, sum of x over the component's pixels
 *   8..11    pixels whose dmg is 1, 2, 3, 4
 *   12       pixels whose dmg is anything else (0, or > 4)
 *   13       the class 1..4 with the largest of columns 8..11, ties to the smaller class (pp_vote_kernel's rule); 0 when all
 *            four are 0
 *   14       sum of q(loc), q(v) = __float2int_rn(fminf(fmaxf(v, 0.f), 1.f) * 65535.f) in fp32 (NaN -> 0); 0 when loc is NULL
 *   15       0
 * Every column is an integer and every reduction an integer add, min or max: the same bits on every run.  Five launches,
 * nothing is read back.  Size limits as xv2_postprocess (H * W < 2^30, B <= 65535), max_rows >= 1; the workspace query is 0
 * outside them.  A label that names no root of its tile is dropped (it adds to no row). */
#define XV2_BUILDING_COLS 16
size_t xv2_building_table_workspace(int B, int H, int W);
int xv2_building_table(const int32_t* labels, const uint8_t* dmg, const float* loc, int B, int H, int W, int max_rows,
                       void* workspace, int64_t* rows, int32_t* count, void* stream);

/* ---- predicted buildings matched to labelled buildings by IoU (match.hip, xview2_amd/utils/building_metrics.py) -------
 * labels_*: int32 [B,H,W] as xv2_label_components writes them; rows_*: int64 [B][max_rows_*][16] and count_*: int32 [B] as
 * xv2_building_table wrote them for those labels.  p is the prediction, t the target; the entry is symmetric in them.
 * match_p: int64 [B][max_rows_p][8], match_t likewise with max_rows_t; rows 0 .. min(count[b], max_rows) - 1 of a tile are
 * written, in the table's row order; nothing else of the buffers is touched.  Columns of the row of building a, where b
 * ranges over the buildings of the other map that share at least one pixel with it, I(a,b) = |a n b| and
 * U(a,b) = |a| + |b| - I (areas: column 1 of the tables):
 *   0        row index of the best partner in the other table, -1 if there is none: the largest I / U, fractions compared
 *            exactly (I1 * U2 vs I2 * U1 in int64), ties to the partner with the smaller column-0 root
 *   1        I with that partner (0 if none)
 *   2        U with that partner (the building's own area if none)
 *   3        1 if matched, else 0: the partner's best partner is this building (mutual best) AND I * iou_den >= iou_num * U
 *   4        the number of distinct partners: 0 is a missed or spurious building, more than 1 a merge or a split
 *   5..7     0
 * Threshold.  1 <= iou_num <= iou_den <= 65536 and 2 * iou_num >= iou_den, anything else is XV2_EINVAL.  With a threshold of
 * at least 1/2 a pair that passes has I >= U / 2 and U >= max(|a|, |b|), so it holds at least half of both areas and more
 * than half of both as soon as I / U > 1/2; partners of one building are disjoint, so no building has two partners above
 * 1/2: the matched set is the same under every matching rule in use (greedy by score, Hungarian, mutual best) and no
 * ordering of the predictions enters.  (Two passing partners at I / U = 1/2 exactly would each be half of the building, lie
 * inside it and tile it, so they would touch and be one component: with tables that are the labels' own, a pair that passes
 * is always mutual.  The mutual test decides only when a table comes from another map; the tie rule of column 0 then picks
 * one.)  Thresholds below 1/2 are rejected rather than given a made-up rule.
 * Pieces.  The 4-connected components of the overlap mask (labels_p != 0) & (labels_t != 0) each lie inside one pair (two
 * 4-adjacent foreground pixels of a map share its component), a pair may own several, and I is the sum of their areas.
 * piece_count[b] (int32 [B], overwritten by every call) is the true number of pieces of tile b, even above max_pieces.  A
 * tile's match rows are valid when piece_count[b] <= max_pieces, count_p[b] <= max_rows_p and count_t[b] <= max_rows_t;
 * otherwise that tile's rows hold unspecified values inside their own storage, and the other tiles are unaffected.
 * No input that passes the host-side argument checks makes a kernel address outside its buffers: a label that names no row
 * of its table is dropped (its root label - 1 must be column 0 of a row below min(count, max_rows), found by bisection over
 * the ascending column 0, so no per-pixel rank map and no uninitialised word is read); a row whose column 0 is outside
 * 0 .. H*W-1 or whose area is outside 1 .. H*W is dropped; pieces of rank >= max_pieces are not inserted, so the pair
 * table, sized for max_pieces entries at load factor at most 1/2, can never fill; every probe and retry loop has a bound.
 * Built as: overlap mask, xv2_label_components and xv2_building_table on it (piece_count; root and area per piece), pair
 * table cleared and match rows initialised in one launch, one thread per piece inserting (rank_p, rank_t) with a 64-bit compare-and-swap and
 * adding its area, one thread per pair offering (I, partner) to both buildings' best-partner words, one thread per building
 * resolving, one pass returning the scratch column to 0: fourteen launches whatever B, H, W and content, nothing read back.
 * Every reduction is an integer add or an exact compare-and-swap towards the maximum of a total order: the same input gives
 * the same bytes on every run.  Size limits as xv2_postprocess (H * W < 2^30, B <= 65535), max_rows_* >= 1, max_pieces >= 1;
 * the workspace query is 0 outside them; the workspace needs no clearing. */
#define XV2_MATCH_COLS 8
size_t xv2_building_match_workspace(int B, int H, int W, int max_pieces);
int xv2_building_match(const int32_t* labels_p, const int64_t* rows_p, const int32_t* count_p, int max_rows_p,
                       const int32_t* labels_t, const int64_t* rows_t, const int32_t* count_t, int max_rows_t,
                       int B, int H, int W, int iou_num, int iou_den, int max_pieces, void* workspace,
                       int64_t* match_p, int64_t* match_t, int32_t* piece_count, void* stream);

/* ---- building outlines of a label map (polygons.hip, xview2_amd/utils/polygons.py) ------------------------------------
 * Input and grid.  labels: int32 [B,H,W] as xv2_label_components writes them.  A pixel is foreground if it is inside the
 * tile and its label is not 0.  Pixel (y,x) covers the square [x,x+1] x [y,y+1]; corners are the lattice points (x,y) with
 * 0 <= x <= W and 0 <= y <= H.
 * Boundary edges.  Side s of a foreground pixel p is a boundary edge if p's neighbour across that side is not foreground.
 * Sides: 0 top, 1 right, 2 bottom, 3 left.  An edge is directed so that p is on its right: 0 heads east, 1 south, 2 west,
 * 3 north (on screen, y down).  Its id is 4 (y W + x) + s.
 * Successor.  With d the edge's direction, left(d) the direction a quarter turn to its left (left(E) = N), a = p + d and
 * l = p + d + left(d): if a is not foreground the successor is side (s+1)%4 of p (a right turn); otherwise, if l is not
 * foreground, side s of a (straight); otherwise side (s+3)%4 of l (a left turn).  Right-turn-first is 4-connectivity: two
 * buildings touching at a corner stay two rings, two hole pixels touching at a corner form one ring that passes that
 * corner twice.  The successor map is a permutation of the boundary edges; its cycles are the rings; all pixels on a
 * ring's right belong to one component.
 * Rings.  A ring's leader is its smallest edge id.  Its vertices are the end corners of those edges whose successor has a
 * different side (collinear points are dropped, nothing else is simplified), in ring order starting at the leader edge.
 * 2A = sum of x_i y_{i+1} - x_{i+1} y_i is positive for exterior rings and negative for holes.  A component's exterior
 * ring is the one whose leader is 4 root + 0; the 2A of all rings of a component sum to twice its pixel area.
 * Outputs.  xv2_polygon_count: counts int64 [B][2] = the numbers of boundary edges and of vertices per tile (both local
 * properties: one launch and a scan); the host reads them once and sizes everything after them exactly.
 * xv2_polygon_trace, with total_edges / total_vertices the sums of counts over the tiles:
 *   verts       int32 [total_vertices][2] as (x,y): tiles in order, rings within a tile in ring-table order, each ring's
 *               vertices contiguous
 *   rings       int64 [total_vertices / 4][8]; rows ordered by tile, then ascending leader:
 *               0 root (label - 1), 1 leader edge id, 2 number of vertices, 3 offset of the first vertex in verts,
 *               4 2A (signed), 5 number of edges (the perimeter in pixels), 6 tile index, 7 0
 *   ring_count  int32 [B]: the rings of every tile (every ring has at least 4 vertices, so the rows always suffice)
 *   status      device int32, accumulated, never cleared: bit 0 is raised when the totals disagree with what the kernels
 *               find; then ring_count is zeroed and nothing else is written
 * Nothing beyond the counted rows and vertices is written; nothing is read back between the launches; every value is an
 * integer and the same bits come out of every run.  Size limits as xv2_postprocess (H * W < 2^30, B <= 65535), and
 * total_edges < 2^31; the workspace queries are 0 outside them.  Neither workspace needs clearing.  After a trace the first
 * 32 bytes of its workspace hold, for diagnosis: int64 edges and vertices found, int32 ok, int32 pointer-doubling rounds
 * that did work in the leader pass and in the ranking pass (each at most ceil(log2(total_edges))). */
#define XV2_POLYGON_RING_COLS 8
size_t xv2_polygon_count_workspace(int B, int H, int W);
size_t xv2_polygon_trace_workspace(int B, int H, int W, int64_t total_edges);
int xv2_polygon_count(const int32_t* labels, int B, int H, int W, void* workspace, int64_t* counts, void* stream);
int xv2_polygon_trace(const int32_t* labels, int B, int H, int W, int64_t total_edges, int64_t total_vertices,
                      void* workspace, int64_t* rings, int32_t* verts, int32_t* ring_count, int32_t* status, void* stream);

/* ---- tolerance simplification of the outlines (simplify.hip, xview2_amd/utils/polygons.py --simplify T) ---------------------
 * Douglas-Peucker on every ring of a ring table, exterior or hole, each on its own, in integers: the result is unique and
 * compared with ==.
 * Tolerance.  T is in pixels and is quantised once on the host to q = round(16 T), 0 <= q <= 65535.  The rule is stated in q.
 * Extent.  Only differences of coordinates enter.  A ring whose extent (max - min) exceeds 32767 in x or in y is copied
 * unchanged with flag 2 (this is looked at first, whatever n is).  Within that limit every quantity below fits an unsigned 64-bit word: every product is < 2^62 and
 * q^2 L2 < 2^63.
 * Anchors.  A ring's vertices are v[0..n-1], and v[n] means v[0].  Anchor 0 is the ring's first vertex (the trace starts every
 * ring at its leader edge, so this is canonical).  Anchor m is the vertex with the largest squared distance from v[0], the
 * lowest index winning ties.  If that distance is 0, or n < 3, the ring is copied unchanged with flag 1.  Otherwise the ring
 * is the two open chains [0..m] and [m..n].
 * Key of an interior vertex P of a chain segment with ends A, B.  With d = B - A, L2 = d.d, v = P - A and t = v.d:
 *   L2 == 0 (a hole ring can pass one corner twice):  key = v.v,                     scale = 1
 *   t <= 0:                                           key = (v.v) L2,                scale = L2
 *   t >= L2:                                          key = ((P - B).(P - B)) L2,    scale = L2
 *   otherwise:                                        key = (v.x d.y - v.y d.x)^2,   scale = L2
 * That is the squared distance to the segment, not to the line, times scale.
 * Split.  A segment's farthest vertex is the one with the largest key, the lowest index winning ties.  It is kept, and the
 * segment splits there, iff key > (q^2 scale) >> 8, which is exactly dist > T because key is an integer.  Otherwise every
 * interior vertex of the segment is dropped.  A segment's decision depends on the segment alone, so the order in which
 * segments are looked at (recursive, or all open segments of a ring at once) does not enter the result.
 * Collapse.  If fewer than 3 vertices of a ring survive, the ring is copied unchanged with flag 1: no building and no hole
 * is ever lost, and the ring count never changes.
 * Order.  The kept vertices stay in ring order and start at v[0].
 * Not promised.  Rings are simplified independently: the outlines of neighbouring buildings may cross afterwards, so may a
 * hole and its exterior, and a simplified ring may intersect itself.  The sign of 2A is recomputed, not guaranteed.
 * Inputs.  rings int64 [n_rings][8] and verts int32 [total_vertices][2] as xv2_polygon_trace writes them; columns 2 (vertices)
 * and 3 (offset) are read; the offsets must be contiguous in row order and start at 0 (column 3 of row r is the sum of column
 * 2 over the rows before it, and the columns 2 sum to total_vertices).  A row whose vertex range does not lie inside the
 * vertex array is not simplified, gets 0 vertices and writes none.
 * Outputs.  out_rings int64 [n_rings][8]: the same rows with column 2 = kept vertices, 3 = new offset, 4 = 2A of the kept
 * vertices (64-bit wrap-around arithmetic: exact whenever it fits), 7 = the flag: 0 simplified or left unchanged by the rule,
 * 1 would collapse and was copied, 2 extent over 32767 and was copied.  out_verts int32 [total_vertices][2], compacted in the
 * same ring order: only its first out_total rows are written.  out_total: device int64, the sum of column 2.
 * Three launches; nothing is read back between them; no float operation; the atomics are integer max, min and add, so the
 * same bits come out of every run and on every stream.  0 <= n_rings, total_vertices < 2^31; the workspace query (44 bytes
 * per vertex and 24 per ring) is 0 outside that; the workspace needs no clearing.  verts, out_verts and the workspace must be
 * 8-byte aligned; outputs must not overlap inputs.  A bad argument is XV2_EINVAL before anything is enqueued. */
size_t xv2_polygon_simplify_workspace(int64_t n_rings, int64_t total_vertices);
int xv2_polygon_simplify(const int64_t* rings, const int32_t* verts, int64_t n_rings, int64_t total_vertices, int q,
                         void* workspace, int64_t* out_rings, int32_t* out_verts, int64_t* out_total, void* stream);

/* ---- polygons -> masks (rasterize.hip, xview2_amd/utils/rasterize.py): the inverse of the outlines above ----------------------
 * Coordinates.  Vertices are int32 in units of 2^-k pixel, k = frac_bits in 0..8.  Pixel (y,x) is sampled at the point
 * s = ((x << k) + off, (y << k) + off).  off = 0 samples the lattice point (a vertex is a pixel index, the convention of the
 * reference's label conversion); off = 2^(k-1), k >= 1, samples the pixel centre (the convention of the outlines, where pixel
 * (y,x) covers [x,x+1] x [y,y+1]).  |coordinate| <= 2^24 and max(H, W) << k <= 2^24, so every cross product fits int64 with
 * room to spare.
 * Coverage of one feature.  A feature is a set of rings, flattened by the host into directed edges a -> b.  With
 * cr = (bx - ax)(sy - ay) - (by - ay)(sx - ax) in int64: s is ON the edge if cr == 0 and s lies in the edge's closed box; the
 * edge is CROSSED if min(ay, by) <= sy < max(ay, by) and the edge's x at height sy is greater than sx, that is cr > 0 when
 * by > ay and cr < 0 otherwise (horizontal edges never cross).  The pixel is covered iff it is on some edge or an odd number
 * of edges cross: even-odd over all rings with a closed boundary.  Holes are rings like any other, orientation does not
 * matter, and a zero-area feature covers exactly the sample points on its edges.
 * Painting.  Features of a tile are painted in table order and the last one wins: out[b][y][x] (uint8 [B,H,W]) is the value
 * of the last covering feature, or 0 if none.
 * Tables.  One int32 buffer, uploaded once; the call takes its device copy and its host copy (as xv2_autoaugment_u8 takes its
 * decisions).  Its parts, in order:
 *   edges     [n_edges][4]     ax, ay, bx, by
 *   features  [n_features][8]  tile, value 0..255, first edge, edge count, clipped pixel box x0, y0, x1, y1 (inclusive);
 *                              sorted by tile, file order inside a tile
 *   work      [n_work][4]      feature, window x0, window y0, 0: one 32 x 32 window of the feature's box; pixels of a window
 *                              beyond the box are not painted, pixels of the box that no window holds stay unpainted
 * The host copy is validated before anything is enqueued: index ranges, boxes inside the tile, window origins inside their
 * boxes, tile order, value range, coordinate bounds, frac_bits and off.  A failure returns XV2_EINVAL and nothing is written.
 * n_features == 0 or n_work == 0 is valid and gives an all-zero out (the tables may then be NULL when all three counts are 0).
 * The device tables and the workspace must be 16-byte aligned, out 4-byte aligned.  Size limits as xv2_postprocess
 * (H * W < 2^30, B <= 65535); the workspace query (4 bytes per pixel, cleared by the call itself) is 0 outside them.  Three
 * launches (clear, cover, resolve), nothing is read back, every value is an integer and the only atomic is an integer max:
 * the same bits come out of every run. */
size_t xv2_rasterize_workspace(int B, int H, int W);
int xv2_rasterize_polygons(const int32_t* dev_tables, const int32_t* host_tables, int64_t n_edges, int n_features,
                           int64_t n_work, int frac_bits, int off, int B, int H, int W, void* workspace, uint8_t* out,
                           void* stream);

/* ---- split touching buildings (split.hip, xview2_amd/utils/split.py) -------------------------------------------------------
 * Per tile, mask is uint8 [H,W], M = mask != 0, and r2 >= 1 is an integer squared radius.  Neighbours are 4-neighbours inside
 * the tile.
 * Distance.  cap = floor(sqrt(r2)) + 1 and d2(p) = min(cap^2, min over q in the tile with !M(q) of |p - q|^2).  Pixels
 * outside the tile are not background: a building cut by the tile edge is not eroded from that edge, and an all-ones tile has
 * d2 = cap^2 everywhere.  d2 is exact wherever it is below cap^2.
 * Seeds.  S = M & (d2 > r2); a seed's label is the one xv2_label_components(S) gives it: 1 + the smallest linear index of its
 * 4-connected component.
 * Growth.  For a pixel p of M, g_l(p) is the 4-connected geodesic distance inside M from p to the seed labelled l,
 * g(p) = min over l of g_l(p), and L(p) = min{ l : g_l(p) = g(p) }; L(p) = 0 for background and for pixels of components of M
 * that hold no seed.  Equivalently L is the fixed point of synchronous rounds in which every unlabelled pixel of M with a
 * labelled neighbour takes the smallest label among those neighbours, and the unique fixed point of relaxing the key (g, l),
 * ordered lexicographically, with key(p) <- min(key(p), key(q) + (1, 0)) over the neighbours q in M, in any order of
 * relaxations: the kernel's schedule does not enter the result.
 * Cut.  p is cut iff L(p) > 0 and some neighbour q has 0 < L(q) < L(p).  out = M & !cut as uint8 with the input's own values
 * kept: out(p) = mask(p) or 0.
 * So out <= mask; every component of out lies inside one component of mask and carries one value of L; two pixels with
 * different non-zero L are never adjacent in out; a component of mask with at most one seed is returned untouched (thin or
 * small buildings that the erosion removes entirely stay as they are); a straight neck of width n between two wide bodies is
 * cut iff ceil(n / 2)^2 <= r2.
 * xv2_edt_sq: d2 as uint16 [B,H,W] for 1 <= cap <= 64, one launch.
 * xv2_split_seed: the distance, the threshold, xv2_label_components on the seeds and the growth state: seeds (0, label), other
 * mask pixels (inf, 0); five launches.
 * xv2_split_grow: sweeps >= 1 sweeps, one launch each.  In a sweep every block loads its 64 x 64 region of keys plus a 1-pixel
 * ring from one buffer, relaxes inside LDS until the region is stable against that ring (a bounded loop), and writes the region
 * to the other buffer; the buffers swap every sweep, so no block reads what another writes and the state after s sweeps is a
 * function of the input alone.  A region that changed neither in this sweep nor in the one before is read and not written,
 * and a region that rested in the previous sweep together with its four neighbouring regions is not even read.
 * The state is left in the first buffer: an odd number of sweeps ends with a copy, an even one does not.  *pending (device
 * int32, overwritten by the call) is non-zero iff the last sweep changed anything: the host reads it once per call and stops
 * at 0, the only read-back.
 * xv2_split_finish: the cut; out uint8 [B,H,W], and L as int32 [B,H,W] into labels unless it is NULL.  L carries seed labels;
 * it is no component labelling of out.
 * The three calls take the same mask, sizes and workspace.  Size limits as xv2_postprocess (H * W < 2^30, B <= 65535), r2 in
 * 1..4095; the workspace query (16 bytes per pixel and 8 per region) is 0 outside the limits.  The workspace must be 16-byte
 * aligned and needs no clearing.  No input is written, nothing is written outside out, labels, d2, pending and the workspace,
 * and a bad argument is XV2_EINVAL before anything is enqueued. */
int xv2_edt_sq(const uint8_t* mask, int B, int H, int W, int cap, uint16_t* d2, void* stream);
size_t xv2_split_workspace(int B, int H, int W);
int xv2_split_seed(const uint8_t* mask, int B, int H, int W, int r2, void* workspace, void* stream);
int xv2_split_grow(const uint8_t* mask, int B, int H, int W, int sweeps, void* workspace, int32_t* pending, void* stream);
int xv2_split_finish(const uint8_t* mask, int B, int H, int W, void* workspace, uint8_t* out, int32_t* labels, void* stream);

/* ---- clean buildings: fill small holes, drop small buildings (clean.hip, xview2_amd/utils/clean.py) ------------------------
 * Per tile, pre is uint8 [H,W] and a pixel is building iff its value != 0; post is an optional uint8 [H,W];
 * min_area = A >= 0 and max_hole = M >= 0 are integers.
 * Stage 1, fill.  A hole is an 8-connected component of background pixels none of which lies on the tile's outer frame
 * (y == 0, y == H - 1, x == 0, x == W - 1).  Its area is its number of pixels; islands of building inside it do not count.
 * A hole is filled iff 1 <= area <= M.  A filled pixel gets pre = 1.  The hole's owner is the 4-connected building, in the
 * unfilled map, that holds the pixel immediately left of the hole's first pixel in raster order: that pixel is always
 * building, and it belongs to the enclosing building, never to an island.  A filled pixel gets post = the owner's voted class:
 * the class 1..4 with the most pixels among the owner's pixels in the unfilled post, ties to the smaller class (the rule of
 * xv2_postprocess with components), and 0 if the owner has no pixel in 1..4.
 * Stage 2, drop.  The 4-connected components of the FILLED pre map are labelled: an island inside a filled hole has thereby
 * merged with its owner, and filled pixels count towards area.  A component with area < A is dropped: pre = 0 and post = 0
 * on its pixels.  Every other pixel keeps its input bytes.
 * stats: device int64 [B][4], overwritten by every call: holes filled, pixels filled, buildings dropped, pixels dropped.
 * A = 0 and M = 0 together are the identity (two device copies).  Any value above H * W is legal and means "all".
 * Background goes by 8-connectivity, the dual of 4-connected buildings and the notion of hole that xv2_polygon_trace rings:
 * a courtyard joined to the outside only through a diagonal step is no hole, and a hole that touches the frame is never
 * filled.
 * post and post_out are both NULL or both set.  Outputs must not alias inputs; no input is written, and nothing is written
 * outside pre_out, post_out, stats and the workspace.  The workspace (xv2_clean_workspace: 20 bytes per pixel, four uint32
 * words per root and an int32 label; 0 outside the limits) must be 16-byte aligned and needs no clearing; it may be NULL when
 * M == 0 and A <= 1.  Size limits as xv2_postprocess (H * W < 2^30, B <= 65535).  A negative A or M, a post without a
 * post_out or the reverse, or a size outside the limits is XV2_EINVAL before anything is enqueued.
 * Launches: four when M > 0 (label both kinds, merge region borders including the diagonal neighbours across edges and
 * corners, compress + tally, fill), four when A > 1 (label, merge, compress + tally, drop); which of them run depends on A
 * and M alone, never on the maps.  Nothing is read back, and every reduction is an integer add or min, so the bytes are the
 * same on every run. */
size_t xv2_clean_workspace(int B, int H, int W);
int xv2_clean_buildings(const uint8_t* pre, const uint8_t* post, int B, int H, int W, int64_t min_area, int64_t max_hole,
                        void* workspace, uint8_t* pre_out, uint8_t* post_out, int64_t* stats, void* stream);

/* ---- register the post image to the pre image (align.hip, xview2_amd/utils/align.py) ---------------------------------------
 * An integer translation found by block matching.  All quantities are integers.
 * Luma.  Scenes are uint8 [B][H][W][3] in stored channel order (B, G, R).  Y = (29 c0 + 150 c1 + 77 c2 + 128) >> 8, in 0..255.
 * Search.  R is the radius, 1 <= R <= 32, D = 2R + 1.  H > 2R, W > 2R, H * W < 2^30 and B <= 65535 are required.  The interior
 * is I = [R, H - R) x [R, W - R): for every p in I and every shift d = (dy, dx) with |dy|, |dx| <= R the pixel p + d lies inside
 * the image, so no padding rule enters the estimate and every shift is summed over the same pixels.
 * Tiles.  T in {32, 64, 128}.  Tile (by, bx) holds the rows R + by T ... min(R + (by + 1) T, H - R) - 1 and the columns
 * likewise; nby = ceil((H - 2R) / T), nbx = ceil((W - 2R) / T); edge tiles are partial.
 * Tables.  S_b(d) = the sum over p in tile b of |Ypre(p) - Ypost(p + d)|, at most 255 T^2 < 2^22 (uint32), and
 * S(d) = the sum of S_b(d) over the tiles, below 2^38 (int64).  Tables are indexed [dy + R][dx + R].
 * Best shift of a table.  The smallest S wins; ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx.
 * A table whose entries are all equal (no texture) therefore gives (0, 0).  The best shift d aligns post(p + d) with pre(p).
 * Resampling.  out[b][y][x][:] = src[b][tri(y + dy, H)][tri(x + dx, W)][:] with tri the reflection of the scene section below,
 * extended to negative indices by floor modulo (m = i mod 2 (L - 1); m < L ? m : 2 (L - 1) - m; tri(i, 1) = 0): every int32
 * shift is defined, and the near side reflects as np.pad(mode="reflect") does.
 * xv2_align_estimate: block_sad uint32 [B][nby][nbx][D][D], sad int64 [B][D][D], block_shift int32 [B][nby][nbx][2] and shift
 * int32 [B][2], both as (dy, dx).  Three launches; nothing is read back between them.  Every table entry is written once with
 * a plain store and every sum is an integer sum, so the same input gives the same bytes on every run and stream.  The
 * workspace (xv2_align_workspace bytes, 0 outside the limits above; 16-byte aligned; needs no clearing) holds int64 partial
 * sums over chunks of 32 tiles.  Outputs must be aligned to their element size; the scenes may have any alignment.
 * xv2_translate_u8: src, out uint8 [B][H][W][C], 1 <= C <= 8, H * W < 2^30, B <= 65535; shift is the DEVICE array int32 [B][2]
 * the estimate wrote (or any other), so estimate followed by translate needs no host round trip; out must not overlap src.
 * No input is written, nothing is written outside the outputs and the workspace, and a bad argument is XV2_EINVAL before
 * anything is enqueued. */
size_t xv2_align_workspace(int B, int H, int W, int R, int T);
int xv2_align_estimate(const uint8_t* pre, const uint8_t* post, int B, int H, int W, int R, int T, void* workspace,
                       uint32_t* block_sad, int64_t* sad, int32_t* block_shift, int32_t* shift, void* stream);
int xv2_translate_u8(const uint8_t* src, int B, int H, int W, int C, const int32_t* shift, uint8_t* out, void* stream);

/* ---- scene inference: windows of a scene of any size, blended on the device (xview2_amd/scene.py, scene.hip) ---------
 * A scene is H x W pixels, H * W < 2^30.  Windows are h x w (multiples of 32, 32..2048) with their origins (y0, x0) in a
 * device table; the table's order is the summation order.  tri(i, L) is reflection without repeating the edge, iterated:
 * period 2 (L - 1), tri(i, 1) = 0 (np.pad(mode="reflect")).  ramp r(i) = min(i + 1, n - i, overlap + 1) along an axis of
 * window side n; a window pixel weighs r(iy) * r(ix).  Origins are clamped into the scene on the device (a corrupt table
 * reads a wrong pixel, never another allocation). */
#define XV2_SCENE_SIGMOID1 0  /* C = 2: sigmoid(channel 1)      -> 1 map   (Model._decode, --type pre)   */
#define XV2_SCENE_SOFTMAX  1  /* softmax over C channels        -> C maps  (damage heads)                */
#define XV2_SCENE_SIGMOID  2  /* sigmoid per channel            -> C maps  (coral, C = 3)                */
#define XV2_SCENE_RELU     3  /* max(x, 0)                      -> C maps  (mse, C = 1)                  */
#define XV2_SCENE_MAX_WINDOWS 1024   /* windows per call (the table is held in LDS) */
/* out[k][iy][ix][:] = pre[tri(y0 + iy, H)][tri(x0 + ix, W)][0..2] (then post's three channels when post != NULL): uint8
 * [K][h][w][3 | 6], the layout ops.DeviceImage normalises.  pre / post: uint8 [H][W][3].  out must be 4-byte aligned. */
int xv2_scene_windows_u8(const uint8_t* pre, const uint8_t* post, int H, int W, const int32_t* origins, int K, int h, int w,
                         uint8_t* out, void* stream);
/* acc[c][y][x] = fmaf(r(iy) r(ix), p_c, acc[c][y][x]) for every window of the table that holds scene pixel (y, x), in table
 * order, p = the decode `kind` of that window's logits [K][C][h][w] at (y - y0, x - x0); window positions at or past H / W
 * (padding) are dropped.  One thread owns a scene pixel: no atomics, and the same bits however a scene's windows are split
 * over calls in the same order.  C: 2 (SIGMOID1), 2..5 (SOFTMAX), 1..5 (SIGMOID, RELU).  0 <= overlap <= min(h, w) / 2.
 * acc: fp32 [Cout][H][W], zeroed by the caller once per scene. */
int xv2_scene_blend(const float* logits, int kind, int C, const int32_t* origins, int K, int h, int w, int overlap, int H,
                    int W, float* acc, void* stream);
/* acc[c][y][x] /= (float)(wy[y] * wx[x]) in place (a division, no reciprocal): wy [H], wx [W] the per-axis sums of the ramps
 * (scene.axis_normaliser); their product is below 2^24. */
int xv2_scene_finalize(float* acc, int Cout, int H, int W, const int32_t* wy, const int32_t* wx, void* stream);

/* ---- resize a device scene and bring its maps back (resize.hip, xview2_amd/resize.py, scene.py predict(scales=...)) --------
 * The separable resampler of Pillow (libImaging/Resample.c).  Per axis in -> out: scale = in / out, filterscale =
 * max(scale, 1), support = base * filterscale with base 2 (bicubic, a = -0.5) or 1 (bilinear, the triangle); output i has
 * center = (i + 0.5) scale, start = max((int)(center - support + 0.5), 0), count = min((int)(center + support + 0.5), in) -
 * start, weights filter((start + j - center + 0.5) / filterscale) summed in index order and divided by that sum, all in fp64.
 * ceil(support) * 2 + 1 coefficient slots.  Limits: per axis out <= 4 in and in <= 4 out, so at most 17 (bicubic) / 9
 * (bilinear) slots; both images below 2^30 pixels.  The HOST builds the tables (xview2_amd/resize.py); xtab / ytab are device
 * arrays int32 [w | h][2 + slots] with rows {start, count, k[slots]}, unused slots zero.  An axis that keeps its size carries
 * the identity table {i, 1, one}: the same values as a skipped pass.  Horizontal pass first.  One launch each on `stream`, no
 * workspace, no intermediate in device memory.  Every table-derived index is clamped into the image.  No input is written,
 * nothing is written outside dst, dst must not overlap src, and a bad argument is XV2_EINVAL before anything is enqueued.
 * xv2_resize_u8: uint8 [H][W][C] -> [h][w][C], C = 1, 3 or 6, exactly Image.resize((w, h), Image.BICUBIC): k is the weight in
 * 22-bit fixed point, (int)(+-0.5 + weight * 2^22), and each pass ends in the uint8 round-and-clip
 * clip8((2^21 + sum_j s[start + j] k[j]) >> 22), int32 sums.
 * xv2_resize_f32: fp32 planar [C][Hs][Ws] -> [C][H][W], 1 <= C <= 8, bilinear (no negative weight: an average of
 * probabilities stays inside the range of its inputs up to rounding).  k holds the bits of the fp32 nearest the fp64 weight.
 * r = k[0] s[start]; r = r + k[j] s[start + j] for j = 1 .. count - 1: every product and every sum rounded to fp32 on its
 * own, in tap order, the intermediate between the passes fp32.  mode: WRITE dst = r; ACCUMULATE dst = dst + r; FINISH
 * dst = (dst + r) / (float)k, an fp32 division, k = 1..8 the number of maps in the average (read in that mode only). */
#define XV2_RESIZE_U8_TAPS  17
#define XV2_RESIZE_F32_TAPS 9
#define XV2_RESIZE_WRITE      0
#define XV2_RESIZE_ACCUMULATE 1
#define XV2_RESIZE_FINISH     2
int xv2_resize_u8(const uint8_t* src, int H, int W, int C, const int32_t* xtab, const int32_t* ytab, int h, int w, uint8_t* dst,
                  void* stream);
int xv2_resize_f32(const float* src, int C, int Hs, int Ws, const int32_t* xtab, const int32_t* ytab, int H, int W, int mode,
                   int k, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XV2_H_ */
