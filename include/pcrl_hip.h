/*
 * pcrl_hip.h -- C ABI of libpcrl_hip.so: the MI355X (gfx950) native operator layer of the
 * PCRLv2 3D pre-training hot path.
 *
 * The reference (RL4M/PCRLv2) has no FFI of its own: its operator boundary is torch.nn /
 * autograd.  Each entry point below replaces the ATen operator that the cited
 * reference line dispatches.  Paths are relative to the reference repository.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch types.  All pointers are DEVICE pointers.
 *   - Activations are NDHWC ("channels last 3d"): element (n,d,h,w,c) at (((n*D+d)*H+h)*W+w)*C+c.
 *     `dtype` selects the activation / packed-weight storage type: PCRL_F32 or PCRL_BF16.
 *     Accumulation, statistics, 1-channel maps, head tensors, gradients of parameters and the
 *     parameters themselves ("*_ref" pointers, reference layout) are always float32.
 *   - Every call is asynchronous on `stream`; nothing synchronises, allocates or frees.
 *     The caller owns all memory, including workspaces (sizes from the *_ws_bytes helpers).
 *   - Returns 0 on success, a negative PCRL_E* code on failure; pcrl_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.  Re-entrant: the entry points keep no mutable state of their own;
 *     the only process-wide state is the set of kernel-selection switches of the "Test hooks" section at the end of this
 *     header (std::atomic<int>, defaults = the product path; tests and probes flip them to A/B the kernels behind one entry point).
 *   - Reductions are deterministic (two-stage, fixed order; no floating-point atomics).
 */
#ifndef PCRL_HIP_H
#define PCRL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pcrl_stream_t; /* hipStream_t */

enum { PCRL_F32 = 0, PCRL_BF16 = 1 };
enum { PCRL_ACT_NONE = 0, PCRL_ACT_RELU = 1, PCRL_ACT_SIGMOID = 2, PCRL_ACT_SILU = 3 /* optional extra, not used by the reference path */,
       PCRL_ACT_ELU = 4 /* LUConv(act='elu'), models/pcrlv2_model_3d.py:24-25: a constructor variant train_3d.py never instantiates */ };
enum { PCRL_OK = 0, PCRL_EINVAL = -1, PCRL_ELAUNCH = -2, PCRL_EWORKSPACE = -3 };

#define PCRL_CONV_BM 128 /* rows (voxels) per conv tile == rows per BN-statistics partial */

const char* pcrl_version(void);
const char* pcrl_last_error(void);
/* zero-fill `bytes` bytes at p on `stream` (hipMemsetAsync; aten::zero_ on a freshly allocated gradient tensor) */
int pcrl_zero(void* p, size_t bytes, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Weight packing (once per optimizer step).  Reference layouts: Conv3d weight [Co][Ci][3][3][3]
 * (models/pcrlv2_model_3d.py:9), ConvTranspose3d weight [Ci][Co][2][2][2] (:52).
 *   conv3 : w_fwd[co][t][ci]           (t = kd*9+kh*3+kw)         -- B^T operand of the forward GEMM
 *           w_dgrad[ci][26-t][co]                                   -- B^T operand of the data-gradient GEMM
 *   convT : w_fwd[t][co][ci]           (t = i*4+j*2+k)
 *           w_dgrad[ci][t][co]
 * Either output pointer may be NULL. */
int pcrl_pack_conv3_weight(const float* w_ref, void* w_fwd, void* w_dgrad, int Co, int Ci, int dtype, pcrl_stream_t stream);
int pcrl_pack_convt_weight(const float* w_ref, void* w_fwd, void* w_dgrad, int Ci, int Co, int dtype, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3x3x3 convolution, pad 1, stride 1 -- aten::convolution at pcrlv2_model_3d.py:9,33 (LUConv.conv1).
 * Implicit GEMM on MFMA: M = N*D*H*W voxels, N = Co, K = 27*Ci.  Ci % 32 == 0, Co % 32 == 0.
 *   y[m][co] = bias[co] + sum_{t,ci} x[m+delta_t][ci] * wp[co][t][ci]      (zero outside the volume)
 * `stats_partial` (optional): [pcrl_conv3d_k3_stats_rows(...)][Co][2] float; row r receives (sum y, sum y^2) of
 * output tile r, taken from the fp32 accumulators, for the training-mode BatchNorm that follows (:12,33).
 * Three kernels sit behind this entry point: two LDS-halo "brick" kernels (bf16, D%4 == 0, H%8 == 0: 4x8x16-voxel tiles when
 * W%16 == 0, 4x8x8-voxel tiles when W%8 == 0) and a gather kernel (any shape, both dtypes: 128-voxel tiles); the helper tells
 * which tiling the given shape gets.
 * The data gradient (aten::convolution_backward, input half) is the same call with wp = w_dgrad,
 * Ci/Co exchanged, bias = NULL, stats_partial = NULL. */
int64_t pcrl_conv3d_k3_stats_rows(int N, int D, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_conv3d_k3_fwd_kernel(int N, int D, int H, int W, int Ci, int Co, int dtype);   /* informational: 2 wide-brick, 1 brick, 0 gather kernel */
int pcrl_conv3d_k3_fwd(const void* x, const void* wp, const float* bias, void* y, float* stats_partial,
                       int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);
/* Same operation with a caller-provided workspace: volumes too small to fill the chip with 128-voxel tiles (the 8x8x4 bottleneck
 * level at b=32; the 4^3 / 2^3 levels of the 16^3 local views, train_3d.py:118-121) are then split along K = 27 taps x Ci/32
 * into float partial sums in `ws`, combined in fixed order by a second pass that also adds the bias, rounds and emits
 * `stats_partial` (same layout and row count as the one-pass kernel).  `pcrl_conv3d_k3_fwd_ws_bytes` returns the size needed
 * (0: the shape is not split; `ws` may then be NULL). */
int64_t pcrl_conv3d_k3_fwd_ws_bytes(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_conv3d_k3_fwd_ws(const void* x, const void* wp, const float* bias, void* y, float* stats_partial, void* ws, int64_t ws_bytes,
                          int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);

/* Inference forward of a LUConv in .eval() (models/pcrlv2_model_3d.py:9,12,21,33: aten::convolution -> aten::native_batch_norm on the running
 * statistics -> aten::relu) as ONE pass: a[m][co] = act(scale[co] * (sum + bias[co]) + shift[co]) from the float32 accumulators, stored once in
 * `dtype`.  No pre-normalisation tensor, no statistics rows.  x, wp: as pcrl_conv3d_k3_fwd; scale, shift: Co floats (eval-mode BatchNorm:
 * gamma / sqrt(running_var + eps), beta - running_mean * scale); act: PCRL_ACT_RELU or PCRL_ACT_NONE (other codes are an error).
 * Kernels: the wide-brick kernel where pcrl_conv3d_k3_fwd would take it, otherwise the gather kernel in one pass -- every shape is computed.
 * `pcrl_conv3d_k3_fwd_affine_fused` (host only) -> 1 where this one pass replaces pcrl_conv3d_k3_fwd_ws + pcrl_bn_act_apply on the same kernel
 * family (wide-brick shapes; gather shapes that are not split along K), 0 where the unfused convolution runs on a family without this
 * epilogue (4x8x8 bricks, split-K, voxel-major rows) and the caller should keep the two passes.  `_ws_bytes` -> workspace size (0 today: every
 * fused form is one pass; `ws` may be NULL). */
int64_t pcrl_conv3d_k3_fwd_affine_fused(int N, int D, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_conv3d_k3_fwd_affine_ws_bytes(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_conv3d_k3_fwd_affine(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, void* a, void* ws,
                              int64_t ws_bytes, int N, int D, int H, int W, int Ci, int Co, int act, int dtype, pcrl_stream_t stream);

/* Data gradient of a 3x3x3 convolution (convolution_backward(input) of LUConv.conv1, models/pcrlv2_model_3d.py:9,33) WITH the first pass of the
 * BatchNorm backward of the layer BELOW in its epilogue -- for the case that layer's activation has this convolution as its only consumer
 * (ops.0 -> ops.1 inside nn.Sequential(LUConv, LUConv), :37-45): dx IS the gradient of a = relu(scale * bn_y + shift), and rows of
 * (sum dz, sum dz * xhat), dz = [scale * bn_y + shift > 0] * dx (as stored), xhat = (bn_y - mean) * rstd, come out of the convolution's tiles
 * instead of a separate pass over dx and bn_y (pcrl_bn_act_bwd_reduce; aten::threshold_backward + native_batch_norm_backward's reduction).
 * dy: [N][D][H][W][Ci]; wp_dgrad: the packed data-gradient weights of pcrl_conv3d_k3_fwd; dx, bn_y: [N][D][H][W][Co]; scale .. rstd: Co floats
 * (pcrl_bn_finalize's outputs for the layer below); partial: [rows][Co][2] float for pcrl_bn_bwd_finalize(partial, rows, Co, count = N D H W, ...).
 * `pcrl_conv3d_k3_dgrad_bnred_rows` returns the row count, or 0 when the shape / activation / dtype has no such kernel (wide-brick bf16 shapes
 * behind ReLU only): the caller then runs pcrl_conv3d_k3_fwd_ws and pcrl_bn_act_bwd_reduce as two passes. */
int64_t pcrl_conv3d_k3_dgrad_bnred_rows(int N, int D, int H, int W, int Ci, int Co, int act, int dtype);
int pcrl_conv3d_k3_dgrad_bnred(const void* dy, const void* wp_dgrad, void* dx, const void* bn_y, const float* scale, const float* shift,
                               const float* mean, const float* rstd, float* partial, int N, int D, int H, int W, int Ci, int Co, int act,
                               int dtype, pcrl_stream_t stream);

/* Weight gradient (aten::convolution_backward, weight half).  dw_ref[co][ci][27] float32, reference layout.
 * Split-K over voxels with a fixed-order second pass.  ws: pcrl_conv3d_k3_wgrad_ws_bytes(). */
size_t pcrl_conv3d_k3_wgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Co);
int pcrl_conv3d_k3_wgrad(const void* x, const void* dy, float* dw_ref, void* ws, size_t ws_bytes,
                         int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);

/* First layer, Ci == 1 (pcrlv2_model_3d.py:101 -> down_tr64.ops.0, K = 27: HBM-bound, no MFMA).
 * x: float32 scalar field [M]; w_ref [Co][1][27] float32; y: dtype [M][Co]; Co in {16, 32, 64}.
 * `stats_partial`: [pcrl_conv3d_k3_c1_stats_rows(...)][Co][2] (bf16 on D%4 == 0, H%8 == 0, W%8 == 0 volumes: an MFMA brick kernel, one
 * row per 4x8x8 brick, x and w enter the MFMA as bf16; otherwise one row per 128 voxels, float32 FMAs).
 * The weight gradient is an MFMA GEMM dy^T . im2col(x) (im2col built in LDS on brick volumes, else staged in the workspace). */
int64_t pcrl_conv3d_k3_c1_stats_rows(int N, int D, int H, int W, int Co, int dtype);
int pcrl_conv3d_k3_c1_fwd(const float* x, const float* w_ref, const float* bias, void* y, float* stats_partial,
                          int N, int D, int H, int W, int Co, int dtype, pcrl_stream_t stream);
/* The first layer in .eval() (pcrlv2_model_3d.py:101 -> down_tr64.ops.0: convolution -> BatchNorm on the running statistics -> relu) as one
 * pass, like pcrl_conv3d_k3_fwd_affine: a = act(scale[co] * (sum + bias[co]) + shift[co]), act = PCRL_ACT_RELU or PCRL_ACT_NONE; every shape
 * and dtype pcrl_conv3d_k3_c1_fwd takes, on the same kernels. */
int pcrl_conv3d_k3_c1_fwd_affine(const float* x, const float* w_ref, const float* bias, const float* scale, const float* shift, void* a,
                                 int N, int D, int H, int W, int Co, int act, int dtype, pcrl_stream_t stream);
size_t pcrl_conv3d_k3_c1_wgrad_ws_bytes(int N, int D, int H, int W, int Co);
int pcrl_conv3d_k3_c1_wgrad(const float* x, const void* dy, float* dw_ref, void* ws, size_t ws_bytes,
                            int N, int D, int H, int W, int Co, int dtype, pcrl_stream_t stream);

/* Convolutions with ONE output channel: deep-supervision head conv3x3x3 C->1 (pcrlv2_model_3d.py:60,71)
 * and OutputTransition.final_conv 1x1x1 64->1 (:78).  taps = 27 or 1.  y, dy: float32 [M].
 * C: a multiple of 8 (bf16) / 4 (float32), <= 1024, and taps * C * 4 <= 65536 bytes (27 taps: C <= 606) -- fwd and dgrad keep the weights in LDS.
 * w_ref: [1][C][taps] float32.  `stats_partial`: [pcrl_conv3d_to1_stats_rows(...)][1][2] or NULL.  fwd, 27 taps, three kernels:
 * an LDS-halo brick kernel (bf16, D%4 == 0, H%8 == 0, W%8 == 0, C%32 == 0: z = x.w for every halo voxel on MFMA, gathered per
 * output voxel inside the block; one statistics row per 4x8x8 brick); else a pointwise MFMA product z[t][m] = sum_c x[m][c] w[c][t]
 * (x read once) + a shifted sum of the 27 planes, staged in `ws` (pcrl_conv3d_to1_fwd_ws_bytes; one row per 1024 voxels);
 * ws = NULL falls back to the direct 27-tap gather kernel.
 * dgrad: dx[m][c] = add_src[m][c] + sum_t dy[m-delta_t] * w[c][t]; add_src may be NULL (zero), dx itself
 * (in-place accumulation) or another tensor of the same shape (an upstream gradient to fold in). */
int64_t pcrl_conv3d_to1_stats_rows(int N, int D, int H, int W, int C, int taps, int dtype);
size_t pcrl_conv3d_to1_fwd_ws_bytes(int N, int D, int H, int W, int C, int taps);
int pcrl_conv3d_to1_fwd(const void* x, const float* w_ref, const float* bias, float* y, float* stats_partial,
                        void* ws, size_t ws_bytes, int N, int D, int H, int W, int C, int taps, int dtype,
                        pcrl_stream_t stream);
int pcrl_conv3d_to1_dgrad(const float* dy, const float* w_ref, const void* add_src, void* dx,
                          int N, int D, int H, int W, int C, int taps, int dtype, pcrl_stream_t stream);
size_t pcrl_conv3d_to1_wgrad_ws_bytes(int N, int D, int H, int W, int C, int taps);
int pcrl_conv3d_to1_wgrad(const void* x, const float* dy, float* dw_ref, float* db, void* ws, size_t ws_bytes,
                          int N, int D, int H, int W, int C, int taps, int dtype, pcrl_stream_t stream);
int64_t pcrl_conv3d_to1_wgrad_route(int D, int H, int W, int C, int taps, int dtype);   /* informational: 0 im2col + plain GEMM, 1 scalar brick kernel, 2 weighted column sum (1 tap) */

/* ---------------------------------------------------------------------------------------
 * ConvTranspose3d kernel 2 stride 2 -- aten::convolution (transposed) at pcrlv2_model_3d.py:52,64.
 * N,D,H,W are the INPUT dims; the output is [N][2D][2H][2W][Co].  Eight independent GEMMs with a
 * scatter store (fwd) / one K = 8*Co gather GEMM (dgrad).  Ci % 32 == 0, Co % 32 == 0. */
int pcrl_convt3d_k2s2_fwd(const void* x, const void* wp_fwd, const float* bias, void* y,
                          int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);
int pcrl_convt3d_k2s2_dgrad(const void* dy, const void* wp_dgrad, void* dx,
                            int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);
size_t pcrl_convt3d_k2s2_wgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Co);
int pcrl_convt3d_k2s2_wgrad(const void* x, const void* dy, float* dw_ref, void* ws, size_t ws_bytes,
                            int N, int D, int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);
int64_t pcrl_convt3d_k2s2_fwd_kernel(int Ci, int Co, int dtype);    /* informational: 1 streaming kernel (conv_up2.hip), 0 implicit GEMM */
int64_t pcrl_convt3d_k2s2_wgrad_route(int Ci, int Co, int dtype);   /* informational: 1 all-taps kernel, 0 gather kernel */

/* Per-channel column sum of a [M][C] activation (bias gradients): out[c] = sum_m v[m][c].
 * ws: pcrl_colsum_ws_bytes(M, C). */
size_t pcrl_colsum_ws_bytes(int64_t M, int C);
int pcrl_colsum(const void* v, float* out, void* ws, size_t ws_bytes, int64_t M, int C, int dtype, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training-mode BatchNorm3d + activation -- aten::native_batch_norm(+_backward), relu_, sigmoid
 * at pcrlv2_model_3d.py:12,21,27,33.  Statistics arrive as per-tile partials from the conv epilogue.
 *   finalize : mean, biased var over `count` elements per channel (fp64 fixed-order reduction);
 *              running_mean/var updated in place (momentum, unbiased var), num_batches_tracked is the
 *              caller's; emits mean, rstd and the fused apply coefficients scale = gamma*rstd,
 *              shift = beta - mean*scale.
 *   apply    : a = act(scale[c]*y + shift[c])
 *   bwd      : dz = da*act'(z);  reduce -> partial (sum dz, sum dz*xhat) per 1024-row tile;
 *              bwd_finalize -> dgamma, dbeta and coefficients k1,kB,kA;  bwd_apply: dy = k1*dz + kB*y + kA. */
int pcrl_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps,
                     float* mean, float* rstd, float* scale, float* shift, pcrl_stream_t stream);
int pcrl_bn_act_apply(const void* y, void* a, const float* scale, const float* shift,
                      int64_t M, int C, int act, int dtype, pcrl_stream_t stream);
/* rows of `partial` for bwd_reduce: ceil(M / tile), tile = 1024 rows for M >= 2^20, halved down to 32 for smaller M */
int64_t pcrl_bn_bwd_partial_rows(int64_t M);
int pcrl_bn_act_bwd_reduce(const void* da, const void* y, const float* scale, const float* shift,
                           const float* mean, const float* rstd, float* partial,
                           int64_t M, int C, int act, int dtype, pcrl_stream_t stream);
/* The two passes for a LUConv whose activation is consumed through nn.MaxPool3d(2) ONLY (pcrlv2_model_3d.py:115-117: the second LUConv
 * of an encoder stage; the skip tensors are never used): max_pool3d_backward folded in.  dp: dtype [N][D/2][H/2][W/2][C] gradient of the
 * POOLED tensor; y: dtype [N][D][H][W][C] the layer's pre-normalisation output.  The activation is recomputed from y exactly as the
 * forward stored it; the first maximum of a window in scan order (d, h, w) receives the gradient, NaN wins (aten's rule).  The
 * full-resolution gradient of the activation is never materialised.  Available when pcrl_bn_act_bwd_pool_ok() != 0 (even D, H, W and
 * pcrl_bn_act_bwd_rowadd_ok(C, dtype)); partial: [pcrl_bn_act_bwd_pool_partial_rows(N, D, H, W)][C][2] -> pcrl_bn_bwd_finalize with
 * count = N*D*H*W. */
int64_t pcrl_bn_act_bwd_pool_ok(int D, int H, int W, int C, int dtype);   /* 1 / 0 */
/* forward of the same pair: a = act(scale*y + shift) and p = MaxPool3d(2)(a) in one pass (same availability).  a may be NULL: only p is stored --
   the encoder stages' unpooled outputs have no reader in a training step (models/pcrlv2_model_3d.py:114-117 stashes them as attributes, nothing
   consumes them), and the backward of the pair reads y, not a: 47 % of the pass's bytes */
int pcrl_bn_act_apply_pool(const void* y, void* a, void* p, const float* scale, const float* shift, int N, int D, int H, int W, int C,
                           int act, int dtype, pcrl_stream_t stream);
int64_t pcrl_bn_act_bwd_pool_partial_rows(int N, int D, int H, int W);
int pcrl_bn_act_bwd_reduce_pool(const void* dp, const void* y, const float* scale, const float* shift, const float* mean,
                                const float* rstd, float* partial, int N, int D, int H, int W, int C, int act, int dtype,
                                pcrl_stream_t stream);
int pcrl_bn_act_bwd_apply_pool(const void* dp, const void* y, void* dy, const float* scale, const float* shift, const float* k1,
                               const float* kB, const float* kA, int N, int D, int H, int W, int C, int act, int dtype,
                               pcrl_stream_t stream);
int pcrl_bn_bwd_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* mean,
                         const float* rstd, float* dgamma, float* dbeta, float* k1, float* kB, float* kA,
                         pcrl_stream_t stream);
int pcrl_bn_act_bwd_apply(const void* da, const void* y, void* dy, const float* scale, const float* shift,
                          const float* k1, const float* kB, const float* kA,
                          int64_t M, int C, int act, int dtype, pcrl_stream_t stream);
/* The same two passes with a per-(sample, channel) term folded into the incoming gradient: da_eff[n][s][c] = da[n][s][c] + row_g[n][c] / S
 * (M = N * S rows; da may be NULL: the term alone).  This is the global-average-pool branch of UpTransition.forward
 * (pcrlv2_model_3d.py:67; autograd: adaptive_avg_pool3d_backward + the add of the two gradients of x) without materialising the
 * broadcast (pcrl_gap_bwd).  Available when pcrl_bn_act_bwd_rowadd_ok(C, dtype) != 0 (C a multiple of the 16-byte vector that
 * divides 256 vectors). */
int64_t pcrl_bn_act_bwd_rowadd_ok(int C, int dtype);   /* 1 / 0 */
int pcrl_bn_act_bwd_reduce_rowadd(const void* da, const float* row_g, int N, int64_t S, const void* y, const float* scale,
                                  const float* shift, const float* mean, const float* rstd, float* partial,
                                  int64_t M, int C, int act, int dtype, pcrl_stream_t stream);
int pcrl_bn_act_bwd_apply_rowadd(const void* da, const float* row_g, int N, int64_t S, const void* y, void* dy, const float* scale,
                                 const float* shift, const float* k1, const float* kB, const float* kA,
                                 int64_t M, int C, int act, int dtype, pcrl_stream_t stream);

/* The same two passes when the incoming gradient is a SUM of up to three parts: da + da2 + row_g[n][c] / S (each may be NULL, at least
 * one given; N, S only read with row_g).  Replaces the aten::add launches autograd issues where one activation has several consumers:
 * a 2D decoder block's output feeds the next block, its own deep-supervision head and the pooled projection head
 * (models/pcrlv2_model.py:119-127), a BasicBlock's input feeds conv1 and the identity branch.  Same availability as the row term. */
int pcrl_bn_act_bwd_reduce_sum(const void* da, const void* da2, const float* row_g, int N, int64_t S, const void* y, const float* scale,
                               const float* shift, const float* mean, const float* rstd, float* partial,
                               int64_t M, int C, int act, int dtype, pcrl_stream_t stream);
int pcrl_bn_act_bwd_apply_sum(const void* da, const void* da2, const float* row_g, int N, int64_t S, const void* y, void* dy,
                              const float* scale, const float* shift, const float* k1, const float* kB, const float* kA,
                              int64_t M, int C, int act, int dtype, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * MaxPool3d(2) -- aten::max_pool3d_with_indices(+backward) at pcrlv2_model_3d.py:100,115-117.
 * N,D,H,W are the INPUT dims (even).  Backward recomputes the argmax from the saved input
 * (first maximum in d,h,w scan order takes the gradient, like ATen). */
int pcrl_maxpool3d_2_fwd(const void* x, void* y, int N, int D, int H, int W, int C, int dtype, pcrl_stream_t stream);
int pcrl_maxpool3d_2_bwd(const void* x, const void* dy, void* dx, int N, int D, int H, int W, int C, int dtype, pcrl_stream_t stream);

/* Global average pool -- aten::adaptive_avg_pool3d -> (1,1,1) at pcrlv2_model_3d.py:67.
 * fwd: g[n][c] = mean_s a[n][s][c] (float32 out).  bwd: da[n][s][c] = add_src[n][s][c] + dg[n][c]/S
 * (add_src: NULL, da itself, or another tensor, as for pcrl_conv3d_to1_dgrad). */
size_t pcrl_gap_ws_bytes(int N, int64_t S, int C);
int pcrl_gap_fwd(const void* a, float* g, void* ws, size_t ws_bytes, int N, int64_t S, int C, int dtype, pcrl_stream_t stream);
int pcrl_gap_bwd(const float* dg, const void* add_src, void* da, int N, int64_t S, int C, int dtype, pcrl_stream_t stream);
/* pcrl_bn_act_apply and pcrl_gap_fwd of its result in one pass over y (UpTransition: ops.1's activation feeds the pool, :64-67):
 * a = act(scale*y + shift) (dtype [N][S][C]), g[n][c] = mean_s a (the stored, rounded values).  ws: pcrl_gap_ws_bytes(N, S, C).
 * Available when pcrl_bn_act_bwd_rowadd_ok(C, dtype) != 0. */
int pcrl_bn_act_apply_gap(const void* y, void* a, float* g, const float* scale, const float* shift, void* ws, size_t ws_bytes,
                          int N, int64_t S, int C, int act, int dtype, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Projection / predictor heads on [rows][C] float32 -- BatchNorm1d, Linear, ReLU at
 * pcrlv2_model_3d.py:55-59,69-70.  Tiny (latency-bound) kernels. */
int pcrl_bn1d_fwd(const float* x, float* y, const float* gamma, const float* beta, float* running_mean, float* running_var,
                  float momentum, float eps, float* mean, float* rstd, int rows, int C, int relu, pcrl_stream_t stream);
int pcrl_bn1d_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* mean, const float* rstd,
                  float* dx, float* dgamma, float* dbeta, int rows, int C, int relu, pcrl_stream_t stream);
/* eval mode, any C: y = scale[c] * x + shift[c] (+ReLU) with the coefficients of the running statistics (C % 4 == 0 also runs on pcrl_bn_act_apply) */
int pcrl_bn1d_eval(const float* x, float* y, const float* scale, const float* shift, int rows, int C, int relu, pcrl_stream_t stream);
int pcrl_linear_fwd(const float* x, const float* w, const float* b, float* y, int rows, int Cin, int Cout, pcrl_stream_t stream);
int pcrl_linear_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db,
                    int rows, int Cin, int Cout, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Trilinear upsampling of 1-channel float32 maps, align_corners=False, integer scale --
 * aten::upsample_trilinear3d(+backward) at pcrlv2_model_3d.py:125-126.  N,D,H,W: INPUT dims. */
int pcrl_upsample_trilinear_fwd(const float* x, float* y, int N, int D, int H, int W, int scale, pcrl_stream_t stream);
int pcrl_upsample_trilinear_bwd(const float* dy, float* dx, int N, int D, int H, int W, int scale, pcrl_stream_t stream);

/* Elementwise sigmoid on float32 maps (OutputTransition, pcrlv2_model_3d.py:79,82) and its backward
 * dpre = dout * out * (1 - out). */
int pcrl_sigmoid_fwd(const float* x, float* y, int64_t n, pcrl_stream_t stream);
int pcrl_sigmoid_bwd(const float* dout, const float* out, float* dpre, int64_t n, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Losses -- aten::mse_loss (train_3d.py:56,135,137) and aten::cosine_similarity(dim=1, eps=1e-8).mean()
 * (train_3d.py:57,90-91).  ws: pcrl_reduce_ws_bytes(n).  The cosine is x.y / (max(|x|, eps) max(|y|, eps)) with an active clamp
 * treated as a constant in the backward; ATen applies its clamp under no-grad, so its gradient differs on rows with 0 < |x| <= eps. */
size_t pcrl_reduce_ws_bytes(int64_t n);
int pcrl_mse_fwd(const float* p, const float* gt, float* loss, void* ws, size_t ws_bytes, int64_t n, pcrl_stream_t stream);
int pcrl_mse_bwd(const float* p, const float* gt, const float* dloss, float* dp, int64_t n, pcrl_stream_t stream);
/* out[0] = mean_r cos(x_r, y_r); saved[r][3] = (dot, |x|, |y|).  bwd: gradient w.r.t. x only (y is detached). */
int pcrl_cosine_mean_fwd(const float* x, const float* y, float* out, float* saved, int rows, int C, float eps, pcrl_stream_t stream);
int pcrl_cosine_mean_bwd(const float* x, const float* y, const float* saved, const float* dout, float* dx,
                         int rows, int C, float eps, pcrl_stream_t stream);

/* Validation metrics of one batch (the loss terms of train_3d.py:119-138 -- aten::mse_loss at :135,137, cos_loss :86-92 -- at EVERY scale index
 * k = 0..2 instead of the drawn one), added to a device accumulator of 11 doubles as batch-size-weighted sums:
 *   acc[0] += B MSE(out1, gt);  acc[1 + k] += B MSE(mask_k, gt);
 *   acc[4 + k] += B * -(mean cos(pre1_k, pro2_k) + mean cos(pre2_k, pro1_k)) / 2                                     (cos_loss(.., view 1, view 2) at index k)
 *   acc[7 + k] += B * mean over local views i and global views v of -(mean cos(pre_v, proL_i) + mean cos(preL_i, pro_v)) / 2      (train_3d.py:127-134)
 *   acc[10] += B.
 * out1, mask_k, gt: float32 [B * S] (S voxels per sample; the masks already upsampled); pro / pre of view 1 and 2 at scale k: float32 [B][Ck];
 * proL / preL: [nlocal * B][Ck], local view i in rows i * B .. (train_3d.py:121's torch.cat).  Deterministic: two stages in fixed order,
 * float64 arithmetic throughout (exact differences and products of the float32 inputs); three launches, no host synchronisation.  ws: pcrl_val_metrics_ws_bytes(B * S, B, nlocal). */
size_t pcrl_val_metrics_ws_bytes(int64_t n, int B, int nlocal);
int pcrl_val_metrics(const float* out1, const float* mask0, const float* mask1, const float* mask2, const float* gt,
                     const float* pro1_0, const float* pre1_0, const float* pro2_0, const float* pre2_0, const float* proL_0, const float* preL_0,
                     const float* pro1_1, const float* pre1_1, const float* pro2_1, const float* pre2_1, const float* proL_1, const float* preL_1,
                     const float* pro1_2, const float* pre1_2, const float* pro2_2, const float* pre2_2, const float* proL_2, const float* preL_2,
                     double* acc, void* ws, size_t ws_bytes, int B, int64_t S, int nlocal, int C0, int C1, int C2, float eps, pcrl_stream_t stream);

/* Validation metrics of one 2D batch (the loss terms of train_2d.py:139-168 -- aten::mse_loss at :165,167, cos_loss :111-117 -- at EVERY scale index
 * k = 0..4 instead of the drawn one, with pcrlv2_model.py:190's aten::upsample_bilinear2d inside the reduction), added to 17 device doubles:
 *   acc[0] += B MSE(out1, gt);  acc[1 + k] += B MSE(bilinear_up(mask_k, 2^(4 - k)), gt)   (the upsampled map is never stored)
 *   acc[6 + k] += B * -(mean cos(pre1_k, pro2_k) + mean cos(pre2_k, pro1_k)) / 2                                    (train_2d.py:111-117 at index k)
 *   acc[11 + k] += B * mean over local views i and global views v of -(mean cos(pre_v, proL_i) + mean cos(preL_i, pro_v)) / 2     (train_2d.py:148-163)
 *   acc[16] += B.
 * out1: float32 NHWC [B][H][W][3]; masks: HOST array of 5 device pointers, mask_k float32 NHWC [B][H >> (4-k)][W >> (4-k)][3] at its own resolution
 * (index rule of pcrl_upsample2d_bilinear_fwd, align_corners=False); gt: float32 NCHW [B][3][H][W] as the loader delivers it (as pcrl_mse2d_fwd reads
 * it); feats: HOST array of 30 device pointers, scale-major: pro1, pre1, pro2, pre2 [B][C[k]], proL, preL [nlocal * B][C[k]] (local view i in rows
 * i * B ..); C: HOST array of the 5 channel counts.  H, W multiples of 16.  nlocal, eps, row layout: the rules of pcrl_val_metrics.  Deterministic: two
 * stages in fixed order, float64 arithmetic on the float32 inputs (dyadic interpolation weights: exact products), three launches, no atomics, no host
 * synchronisation.  ws: pcrl_val2d_metrics_ws_bytes(B, H, W, nlocal). */
size_t pcrl_val2d_metrics_ws_bytes(int B, int H, int W, int nlocal);
int pcrl_val2d_metrics(const float* out1, const float* const* masks, const float* gt, const float* const* feats, const int* C, double* acc,
                       void* ws, size_t ws_bytes, int B, int H, int W, int nlocal, float eps, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * OPTIONAL EXTRA, not part of the reference: NT-Xent (SimCLR) contrastive loss over z = [z1; z2], R = 2N
 * rows (row i's positive is row (i + N) mod R), temperature tau:
 *   zn = z / max(|z|, eps);  loss = mean_i ( logsumexp_{k != i} zn_i.zn_k / tau  -  zn_i.zn_pos(i) / tau ).
 * fwd leaves zn, the softmax and the norms in `ws` (pcrl_ntxent_ws_bytes) for bwd, which must get the same workspace. */
size_t pcrl_ntxent_ws_bytes(int R, int C);
int pcrl_ntxent_fwd(const float* z, float* loss, void* ws, size_t ws_bytes, int R, int C, float tau, float eps, pcrl_stream_t stream);
int pcrl_ntxent_bwd(const float* z, const float* dloss, float* dz, void* ws, size_t ws_bytes, int R, int C, float tau, float eps,
                    pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * OPTIONAL EXTRA, not part of the reference: GroupNorm(G) + activation on NDHWC activations, built from the
 * BatchNorm streaming kernels applied per sample with per-(sample, channel) coefficients:
 *   gn_stats:        partial[n][tile][c][2] = (sum, sum^2) of y over the tile's voxels        (tiles = pcrl_gn_stats_tiles(S))
 *   gn_finalize:     per (n, group): mean, rstd (biased variance, eps) -> mean_c, rstd_c, scale, shift as [N][C] arrays
 *   apply:           pcrl_bn_act_apply on sample n with scale + n*C, shift + n*C   (act = PCRL_ACT_SILU for GroupNorm+SiLU)
 *   backward:        pcrl_bn_act_bwd_reduce per sample (mean_c/rstd_c rows) -> gn_bwd_finalize (k1, kB, kA as [N][C]; per-sample
 *                    dgamma/dbeta parts [N][C]) -> pcrl_bn_act_bwd_apply per sample. */
int64_t pcrl_gn_stats_tiles(int64_t S);
int pcrl_gn_stats(const void* y, float* partial, int N, int64_t S, int C, int dtype, pcrl_stream_t stream);
int pcrl_gn_finalize(const float* partial, int tiles, int N, int64_t S, int C, int G, const float* gamma, const float* beta, float eps,
                     float* mean_c, float* rstd_c, float* scale, float* shift, pcrl_stream_t stream);
int pcrl_gn_bwd_finalize(const float* partial_b, int rows_b, int N, int64_t S, int C, int G, const float* gamma, const float* mean_c,
                         const float* rstd_c, float* k1, float* kB, float* kA, float* dgamma_n, float* dbeta_n, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LUConv constructor variants (models/pcrlv2_model_3d.py:15-16,22-25; accepted by the reference's constructor, never instantiated by
 * train_3d.py:45): act='elu' is PCRL_ACT_ELU of the fused BatchNorm kernels; norm='in' (InstanceNorm3d, affine) is the GroupNorm
 * machinery above with G == C; act='prelu' (nn.PReLU(out_chan), aten::prelu / prelu_backward) is a streaming pass behind the
 * normalisation, which then runs with PCRL_ACT_NONE:
 *   prelu_fwd:  a[m][c] = z > 0 ? z : w[c] * z                                   (z, a: [M][C] activations; w: float32 [C])
 *   prelu_bwd:  dz = da * (z > 0 ? 1 : w[c]);  partial[tile][c] = sum_m da * z * [z <= 0] over the tile's rows
 *               (pcrl_prelu_bwd_partial_rows(M) tiles; dw = column sums of `partial`, e.g. pcrl_colsum). */
int pcrl_prelu_fwd(const void* z, const float* w, void* a, int64_t M, int C, int dtype, pcrl_stream_t stream);
int64_t pcrl_prelu_bwd_partial_rows(int64_t M);
int pcrl_prelu_bwd(const void* da, const void* z, const float* w, void* dz, float* partial, int64_t M, int C, int dtype, pcrl_stream_t stream);

/* =======================================================================================
 * 2D path: the PCRLv2 ResNet-18 U-Net of models/pcrlv2_model.py:68-209 (decoder) and the smp/torchvision ResNet-18
 * encoder it wraps (pcrlv2_model.py:200).  Activations NHWC ([N][H][W][C], C-contiguous), float32 or bf16.
 *
 * Convolution KHxKW, stride 1|2, zero padding `pad`, optional fused nearest x2 upsample of the input (F.interpolate(scale_factor=2,
 * mode="nearest") at pcrlv2_model.py:114 followed by conv1): replaces aten::convolution / convolution_backward for nn.Conv2d.
 * Source channel counts must be powers of two >= 8: the caller zero-pads 3-channel tensors (image, 3-channel gradients) to 8.
 *   pack  : reference weight float32 [Co][Ci][KH][KW] -> K-contiguous rows in `dtype`; mode 0 = forward ([round32(Co)][Kpad],
 *           k = tap*CsP + ci), mode 1 = data gradient ([round32(Ci)][Kpad], k = tap*CsP + co); Kpad = round32(KH*KW*CsP);
 *           pcrl_conv2d_packed_elems(rows, taps, CsP) elements.
 *   fwd   : y[N][Ho][Wo][Co] (+bias), `out_f32` stores float32 whatever `dtype`; stats_partial = pcrl_conv2d_stats_rows(N,Ho,Wo)
 *           rows of [Co][2] (sum, sum^2) for the BatchNorm2d that follows, or NULL.  Hi/Wi = stored input dims (before `up`).
 *   dgrad : dx[N][Hi][Wi][Ci] from dy[N][Ho][Wo][CoP]  (for a fused-upsample forward Hi/Wi are the UPSAMPLED dims; follow with
 *           pcrl_upsample2d_nearest2_bwd)
 *   wgrad : dw float32 [CoP][Ci_out][KH][KW]; ws: pcrl_conv2d_wgrad_ws_bytes */
int64_t pcrl_conv2d_packed_elems(int rows, int taps, int CsP);
int pcrl_conv2d_pack(const float* w_ref, void* out, int Co, int Ci, int KH, int KW, int CsP, int mode, int dtype, pcrl_stream_t stream);
int64_t pcrl_conv2d_stats_rows(int N, int Ho, int Wo);     /* upper bound for any kernel: one row per 128 output pixels */
/* rows of statistics pcrl_conv2d_fwd WRITES for this geometry (depends on the kernel its dispatcher picks): allocate that many, pass the
 * count as `stats_rows` and to pcrl_bn_finalize; more rows may be passed -- the surplus is zero-filled */
int64_t pcrl_conv2d_fwd_stats_rows(int N, int Hi, int Wi, int CiP, int Co, int KH, int KW, int stride, int pad, int up, int out_f32, int dtype);
int pcrl_conv2d_fwd(const void* x, const void* wp, const float* bias, void* y, float* stats_partial, int64_t stats_rows, int N, int Hi, int Wi,
                    int CiP, int Co, int KH, int KW, int stride, int pad, int up, int out_f32, int dtype, pcrl_stream_t stream);
/* y may be NULL where pcrl_conv2d_fwd_stats_only_ok(...) == 1: the statistics rows only -- the 3x3 convolution of a deep-supervision head whose map
 * nothing reads (14 of the 15 heads of a step, pcrlv2_model.py:103-106 / train_2d.py:143-168) runs for its BatchNorm's running statistics alone; its
 * output (537 MB at 512 x 512 x 16 channels, b = 64) is not written.  The statistics are taken from the float32 accumulators either way. */
int64_t pcrl_conv2d_fwd_stats_only_ok(int N, int Hi, int Wi, int CiP, int Co, int KH, int KW, int stride, int pad, int up, int out_f32, int dtype);
/* Inference forward of Conv2d -> BatchNorm2d (-> + identity) -> ReLU in .eval() (torchvision BasicBlock / smp Conv2dReLU as the reference's
 * models/pcrlv2_model.py:68-128,197-209 runs them: aten::convolution -> aten::native_batch_norm on the running statistics -> aten::add -> aten::relu)
 * as ONE pass:  a[m][co] = max(scale[co] * (acc + bias[co]) + shift[co] + (residual ? residual[m][co] : 0), act_lo)  from the float32 accumulators,
 * stored once in `dtype`.  No pre-normalisation tensor, no statistics rows.  x, wp, bias and the geometry: as pcrl_conv2d_fwd (every geometry it
 * computes: `up`, stride 2, 1x1, 7x7, float32); scale, shift: Co floats (gamma / sqrt(running_var + eps), beta - running_mean * scale); residual:
 * NULL or [M][Co] in the layout and dtype of the output; act: PCRL_ACT_RELU or PCRL_ACT_NONE (other codes are an error).
 * Kernels: the one pcrl_conv2d_fwd's route names, with the epilogue (gather, narrow, 4x8x8 brick; wide brick without a residual); a wide-brick
 * call WITH a residual -- that epilogue has no residual operand -- is computed by the gather kernel in one pass.
 * `pcrl_conv2d_fwd_affine_fused` (host only, the same route function) -> 1 where this one pass replaces pcrl_conv2d_fwd + pcrl_bn_act_apply
 * (+ pcrl_add_relu_fwd) on the same kernel family, 0 where the caller should keep separate passes (a wide-brick layer with a residual: the call
 * without the residual is fused, pcrl_add_relu_fwd stays). */
int64_t pcrl_conv2d_fwd_affine_fused(int N, int Hi, int Wi, int CiP, int Co, int KH, int KW, int stride, int pad, int up, int has_residual, int dtype);
int pcrl_conv2d_fwd_affine(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, const void* residual, void* a,
                           int N, int Hi, int Wi, int CiP, int Co, int KH, int KW, int stride, int pad, int up, int act, int dtype, pcrl_stream_t stream);
/* data gradient of a 3x3 / stride 1 / pad 1 convolution that read its input through the nearest x2 upsample (decoder conv1,
 * models/pcrlv2_model.py:114) INCLUDING the upsample's backward (aten::convolution_backward's input gradient + aten::upsample_nearest2d_backward):
 * dx[N][Hc][Wc][Ci] = 2 x 2 block sums of the fine-resolution gradient, which is never stored.  dy: [N][2Hc][2Wc][CoP]; wp_dgrad as for
 * pcrl_conv2d_dgrad.  Only where pcrl_conv2d_dgrad_up_ok() != 0 (both channel counts <= 32, bf16, fine extents multiples of 8 x 32). */
/* which kernel the dispatcher runs for a geometry (no launch): 0 gather implicit GEMM, 1 LDS-halo brick kernel, 2 right-sized narrow kernel,
 * 3 wide-brick kernel */
int64_t pcrl_conv2d_fwd_kind(int N, int Hi, int Wi, int CiP, int Co, int KH, int KW, int stride, int pad, int up, int out_f32, int dtype);
int64_t pcrl_conv2d_dgrad_kind(int N, int Hi, int Wi, int Ci, int Ho, int Wo, int CoP, int KH, int KW, int stride, int pad, int dtype);
int64_t pcrl_conv2d_dgrad_up_ok(int N, int Hc, int Wc, int Ci, int CoP, int dtype);
int pcrl_conv2d_dgrad_up(const void* dy, const void* wp_dgrad, void* dx, int N, int Hc, int Wc, int Ci, int CoP, int dtype, pcrl_stream_t stream);
int pcrl_conv2d_dgrad(const void* dy, const void* wp_dgrad, void* dx, int N, int Hi, int Wi, int Ci, int Ho, int Wo, int CoP, int KH,
                      int KW, int stride, int pad, int dtype, pcrl_stream_t stream);
/* 3x3 / stride 1 / pad 1 data gradient WITH the first pass of the BatchNorm backward of the layer below (the 2D counterpart of
 * pcrl_conv3d_k3_dgrad_bnred): conv2 of a torchvision BasicBlock under relu(bn1(conv1(x))), conv2 of a DecoderBlock under conv1's
 * BatchNorm + ReLU (models/pcrlv2_model.py:113-128) -- activations with one consumer.  dy: [N][H][W][CoP]; dx, bn_y: [N][H][W][Ci];
 * partial: [rows][Ci][2] for pcrl_bn_bwd_finalize(partial, rows, Ci, count = N H W, ...).  _rows == 0: no fused kernel for the shape (two passes). */
int64_t pcrl_conv2d_dgrad_bnred_rows(int N, int H, int W, int Ci, int CoP, int act, int dtype);
int pcrl_conv2d_dgrad_bnred(const void* dy, const void* wp_dgrad, void* dx, const void* bn_y, const float* scale, const float* shift,
                            const float* mean, const float* rstd, float* partial, int N, int H, int W, int Ci, int CoP, int act, int dtype,
                            pcrl_stream_t stream);
/* Stride-2 data gradient without idle taps: the parity classes (a, b) = (ih & 1, iw & 1) of dx are four stride-1 gathers over dy
 * (3x3/pad 1: 1, 2, 2, 4 taps; 1x1/pad 0: class (0,0) only, the caller zero-fills dx).  Hi, Wi even.  pack_s2: rows round32(Ci),
 * K = taps(a) * taps(b) * CoP -> pcrl_conv2d_packed_elems(Ci, taps(a) * taps(b), CoP) elements, taps(0) = 1, taps(1) = 2 (3x3). */
int pcrl_conv2d_pack_s2(const float* w_ref, void* out, int Co, int Ci, int KH, int KW, int CoP, int a, int b, int dtype, pcrl_stream_t stream);
int pcrl_conv2d_dgrad_s2(const void* dy, const void* wp_class, void* dx, int N, int Hi, int Wi, int Ci, int Ho, int Wo, int CoP, int KH, int KW,
                         int a, int b, int dtype, pcrl_stream_t stream);
size_t pcrl_conv2d_wgrad_ws_bytes(int N, int Ho, int Wo, int CiP, int CoP, int KH, int KW);
/* which kernel pcrl_conv2d_wgrad runs for a geometry (no launch; follows the wgrad test hooks): 0 gather, 1 right-sized narrow kernel (16/32-channel
 * layers), 2 LDS-halo brick kernel, 3 one kernel row per block */
int64_t pcrl_conv2d_wgrad_kind(int N, int Hi, int Wi, int CiP, int Ho, int Wo, int CoP, int KH, int KW, int stride, int pad, int up, int dtype);
int pcrl_conv2d_wgrad(const void* x, const void* dy, float* dw_ref, void* ws, size_t ws_bytes, int N, int Hi, int Wi, int CiP, int Ci_out,
                      int Ho, int Wo, int CoP, int KH, int KW, int stride, int pad, int up, int dtype, pcrl_stream_t stream);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of the ResNet stem; idx: uint8 [N][Ho][Wo][C] window position of the maximum. */
int pcrl_maxpool2d_3s2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, int dtype, pcrl_stream_t stream);
int pcrl_maxpool2d_3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C, int dtype, pcrl_stream_t stream);
/* backward of the nearest x2 upsample: dx[N][H][W][C] = sum of the 2x2 block of dy[N][2H][2W][C] */
int pcrl_upsample2d_nearest2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pcrl_stream_t stream);
/* F.interpolate(scale_factor=s, mode="bilinear", align_corners=False) on float32 NHWC maps (pcrlv2_model.py:190); N,H,W: INPUT dims */
int pcrl_upsample2d_bilinear_fwd(const float* x, float* y, int N, int H, int W, int C, int scale, pcrl_stream_t stream);
int pcrl_upsample2d_bilinear_bwd(const float* dy, float* dx, int N, int H, int W, int C, int scale, pcrl_stream_t stream);
/* BasicBlock tail: a = relu(t + r);  backward mask: g = da where a > 0 */
int pcrl_add_relu_fwd(const void* t, const void* r, void* a, int64_t n, int dtype, pcrl_stream_t stream);
int pcrl_relu_mask_bwd(const void* da, const void* a, void* g, int64_t n, int dtype, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * UpTransition's first two linear layers as ONE operator: ConvTranspose3d(Ci -> Cm, k=2, s=2) followed directly by
 * Conv3d(Cm -> Co, 3x3x3, pad 1) -- `self.ops(self.up_conv(x))`, pcrlv2_model_3d.py:64 (layers :52 and :9/33), nothing in between.
 * Same function, same parameters (w_up [Ci][Cm][2][2][2], b_up [Cm], w0 [Co][Cm][3][3][3], b0 [Co], reference layouts, float32) and the
 * same four parameter gradients as the two aten calls, computed on the COARSE grid: a fine voxel 2v+p sees only 2x2x2 coarse voxels
 * through its 3x3x3 window, so the composed operator has 8 taps per output phase (0.30 of the multiply-adds) and the Cm-channel
 * 2x-upsampled tensor (and its gradient) never exists.  See csrc/upconv_fused.hip for the algebra.
 *   compose : wf (dtype [8][Co][8][Ci]), wd (dtype [Ci][64][Co]), optionally w3f (dtype [8*Co][27][Ci]: the same composed weights zero-embedded
 *             in 3x3x3 form, read by the wide-brick kernel on the shapes it tiles: coarse D % 4 == H % 8 == W % 16 == 0, bf16, Co % 64 == 0;
 *             NULL: not produced), optionally wd3 (dtype [Ci][27][8*Co]: the data-gradient weights zero-embedded in 3x3x3 form over the
 *             space-to-depth view of dy0 -- channel = parity * Co + co -- read by the wide-brick kernel where pcrl_upconv_dgrad_uses_brick();
 *             NULL: not produced), bias_tab (float32 [27][Co]: border classes of the fine voxel) from the four parameters; once per
 *             optimizer step.  ws: pcrl_upconv_compose_ws_bytes().
 *   fwd     : x dtype [N][D][H][W][Ci] -> y0 dtype [N][2D][2H][2W][Co];  stats_partial: [pcrl_upconv_stats_rows()][Co][2] (sum, sum^2)
 *             for the BatchNorm that follows (or NULL).
 *   dgrad   : dy0 -> dx (dtype [N][D][H][W][Ci]); wd3 may be NULL unless pcrl_upconv_dgrad_uses_brick() (bf16, coarse D % 4 == H % 8 ==
 *             W % 16 == 0, Ci % 64 == 0, Co = 32 * 2^k).
 *   wgrad   : x, dy0 -> dw_up, db_up, dw0 (float32, reference layouts; db0 is the column sum of dy0 -- identically cancelled by the
 *             BatchNorm that follows in the reference model and not produced here).  ws: pcrl_upconv_wgrad_ws_bytes().
 * Channels are multiples of 32.
 *   wgrad_accum / wgrad_finish: the same in two stages, both linear in their intermediates -- `accum` (once per backward pass) adds the pass's
 *             gradient of the composed weights and border-class sums of dy0 (box_acc, float32 [27][Co]) to caller-owned buffers; `finish` runs the
 *             chain rule to dw_up / db_up / dw0 once after the last pass.  dweff_acc: float32 [Co][Ci][64] (the gradient of the composed weights,
 *             index p*8+q; from the brick weight-gradient kernel where it tiles the coarse grid, else from the gather kernel); flags bit 0: store
 *             instead of add (first pass); bit 1: the caller states that dy0 sums to ZERO over all voxels per channel -- true when it is the output of
 *             the training-mode BatchNorm backward that follows conv1 in the reference -- so the border-class sums read only the border voxels and the
 *             interior class is minus the rest (exact arithmetic's value, free of the rounding of dy0). */
size_t pcrl_upconv_compose_ws_bytes(int Ci, int Cm, int Co, int dtype);
int pcrl_upconv_compose(const float* w_up, const float* b_up, const float* w0, const float* b0, void* wf, void* wd, void* w3f, void* wd3,
                        float* bias_tab, void* ws, size_t ws_bytes, int Ci, int Cm, int Co, int dtype, pcrl_stream_t stream);
int64_t pcrl_upconv_fwd_uses_brick(int N, int D, int H, int W, int Ci, int Co, int dtype);   /* informational: which kernel a shape gets */
int64_t pcrl_upconv_stats_rows(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_upconv_fwd(const void* x, const void* wf, const void* w3f, const float* bias_tab, void* y0, float* stats_partial, int N, int D, int H, int W,
                    int Ci, int Co, int dtype, pcrl_stream_t stream);
int64_t pcrl_upconv_dgrad_uses_brick(int N, int D, int H, int W, int Ci, int Co, int dtype);   /* informational: which kernel a shape gets */
int pcrl_upconv_dgrad(const void* dy0, const void* wd, const void* wd3, void* dx, int N, int D, int H, int W, int Ci, int Co, int dtype,
                      pcrl_stream_t stream);
/* The same with a caller-owned workspace (convolution_backward(input) of :9,33 through :52,64 on SMALL coarse grids -- up_tr256's 8x8x4 and
 * the local views' 2^3 / 4^3): the 64-tap reduction of the gather form is split over the grid's third dimension into float partial sums and
 * summed by a fixed-order finish pass (deterministic), like pcrl_conv3d_k3_fwd_ws.  ws_bytes() == 0: no workspace needed, ws may be NULL. */
int64_t pcrl_upconv_dgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_upconv_dgrad_ws(const void* dy0, const void* wd, const void* wd3, void* dx, void* ws, int64_t ws_bytes, int N, int D, int H, int W,
                         int Ci, int Co, int dtype, pcrl_stream_t stream);
int64_t pcrl_upconv_wgrad_uses_brick(int N, int D, int H, int W, int Ci, int Co, int dtype);   /* informational: which kernel a shape gets */
size_t pcrl_upconv_wgrad_accum_ws_bytes(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_upconv_wgrad_accum(const void* x, const void* dy0, float* dweff_acc, float* box_acc, int flags, void* ws, size_t ws_bytes, int N, int D,
                            int H, int W, int Ci, int Co, int dtype, pcrl_stream_t stream);
size_t pcrl_upconv_wgrad_finish_ws_bytes(int Ci, int Cm, int Co, int dtype);
int pcrl_upconv_wgrad_finish(const float* dweff_acc, const float* box_acc, const float* w_up, const float* b_up, const float* w0, float* dw_up,
                             float* db_up, float* dw0, void* ws, size_t ws_bytes, int Ci, int Cm, int Co, int dtype, pcrl_stream_t stream);
size_t pcrl_upconv_wgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Cm, int Co, int dtype);
int pcrl_upconv_wgrad(const void* x, const void* dy0, const float* w_up, const float* b_up, const float* w0, float* dw_up, float* db_up,
                      float* dw0, void* ws, size_t ws_bytes, int N, int D, int H, int W, int Ci, int Cm, int Co, int dtype,
                      pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * All cosine terms of one step in one call -- train_3d.py:119-134 (13 cos_loss calls = 26 cosine means, :86-92).
 *   out[g] = sum_{t : group[t] == g} w[t] * mean_r cos(x[t][r], y[t][r]),  x[t], y[t]: float32 [rows][C[t]] on the device
 * `x`, `y`, `dx`, `w`, `C`, `group`, `first` are HOST arrays of `nterms` <= 32 entries (device pointers / scalars); they are copied into
 * the kernel arguments.  bwd: dx[t] (device float32 [rows][C[t]]; several terms may name the same buffer) receives
 * the sum, in term order (deterministic), of dout[group[t]] * w[t] * d(mean cos)/dx[t] over the terms that name it; first[t] != 0
 * must mark exactly the first term of every buffer (checked), and terms that share a buffer share C.
 * y is the reference's detached operand: no gradient.  fwd: `ws` = pcrl_cosine_terms_ws_bytes(nterms) bytes of device scratch. */
size_t pcrl_cosine_terms_ws_bytes(int nterms);
int pcrl_cosine_terms_fwd(const void* const* x, const void* const* y, const float* w, const int* C, const int* group, int nterms, int rows,
                          int ngroups, float eps, float* out, void* ws, size_t ws_bytes, pcrl_stream_t stream);
int pcrl_cosine_terms_bwd(const void* const* x, const void* const* y, void* const* dx, const float* w, const int* C, const int* group,
                          const int* first, int nterms, int rows, int ngroups, float eps, const float* dout, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * torch.optim.SGD (momentum, weight decay, dampening 0, no nesterov) over a flat parameter arena --
 * train_3d.py:48-51,151.  `offsets`: int64[ntensors+1] element offsets of each tensor in the arena;
 * `flags`: int32[ntensors], bit0 = tensor has a gradient this step (others are skipped, like
 * params whose .grad is None), bit1 = momentum buffer already initialised (else buf = g).
 * g is multiplied by grad_scale first (1/world_size after an all-reduce sum). */
int pcrl_sgd_step(float* p, const float* g, float* buf, const int64_t* offsets, const int32_t* flags, int ntensors,
                  int64_t total, float lr, float momentum, float weight_decay, float grad_scale, pcrl_stream_t stream);
/* The sum of the gradients several forward passes produced for each parameter, written into the flat gradient arena -- autograd's
 * AccumulateGrad behind `loss.backward()` (train_3d.py:149) for the tensors t0 .. t0 + cnt - 1 of the arena in one launch (per 480 / nsrc
 * tensors): dst[offsets[t] + e] = ((src[t][0][e] + src[t][1][e]) + ...), e < numels[t].  offsets / numels: device arrays (int64[ntensors + 1]
 * / int64[ntensors], slots padded to 4 floats); offsets_host: the same offsets on the host; srcs: HOST array [cnt][nsrc] of device pointers
 * (contiguous float32; 16-byte aligned ones are read with 16-byte loads; NULL = no term; a tensor with no term is left untouched), read
 * before the call returns. */
int pcrl_grad_sum(float* dst, const int64_t* offsets, const int64_t* numels, const int64_t* offsets_host, const void* const* srcs, int t0, int cnt, int nsrc,
                  pcrl_stream_t stream);
/* torch.cat(local_views, dim=0) (train_3d.py:121) as one launch: dst = the n <= 8 contiguous pieces src[k] (nbytes[k] bytes each, multiples
 * of 16, 16-byte aligned) one after the other.  src / nbytes are HOST arrays, read before the call returns. */
int pcrl_concat(const void* const* src, const int64_t* nbytes, int n, void* dst, pcrl_stream_t stream);
/* loss = loss1 + loss2 + loss4 + local_loss with loss4 = beta * l4 (train_3d.py:136-138) from four device scalars in one launch:
 * out[0] = total (the reference's order of additions), out[1] = beta * l4. */
int pcrl_loss_total(const float* l1, const float* l2, const float* l4, const float* l5, float beta, float* out, pcrl_stream_t stream);
/* Its backward (autograd's mul / select_backward / add_ on four scalars, train_3d.py:138,144): out[0..3] = g, beta * g, g, g -- the gradients
 * of loss1, l4 and of the (global, local) pair of cosine groups, which pcrl_cosine_terms_bwd takes as out + 2. */
int pcrl_loss_total_bwd(const float* g, float beta, float* out, pcrl_stream_t stream);
/* The divergence guard of train_3d.py:140-142 (`if loss > 1000 and epoch > 10: continue`) decided ON THE DEVICE, so that epochs 11..240 run
 * without a forward -> backward host synchronisation: pcrl_guard_flag writes out[0] = (loss[0] > threshold) ? 1 : 0 (under data parallelism
 * the caller MAX-all-reduces it: one process, one decision in the reference), pcrl_sgd_step_guarded is pcrl_sgd_step that does NOTHING when
 * skip[0] != 0 -- parameters and momentum buffers stay bit-unchanged, which is what the reference's `continue` leaves behind. */
int pcrl_guard_flag(const float* loss, float threshold, float* out, pcrl_stream_t stream);
int pcrl_sgd_step_guarded(float* p, const float* g, float* buf, const int64_t* offsets, const int32_t* flags, int ntensors,
                          int64_t total, float lr, float momentum, float weight_decay, float grad_scale, const float* skip,
                          pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fine-tuning optimisers over the same arenas (csrc/optim.hip; offsets / flags as for pcrl_sgd_step, bit 0 alone is read): torch.optim.Adam /
 * AdamW's single-tensor arithmetic in float32 with one rounding per operation, the global gradient norm with
 * torch.nn.utils.clip_grad_norm_'s coefficient, and the SGD step with that coefficient.  pcrl_optim_grid_cap: the most blocks any of
 * these streaming passes launches (256 threads x 4 elements each; the rest by grid stride).
 *
 * pcrl_adam_prepare (one thread per tensor, in front of the step): for every tensor with flag bit 0, steps[t] += 1,
 * prods[2t] *= beta1, prods[2t + 1] *= beta2 (float64 running products beta^t, 1.0 before the first step),
 * coefs[2t] = (float)(lr / (1 - beta1^t)), coefs[2t + 1] = (float)sqrt(1 - beta2^t); a tensor without a gradient keeps all of it.
 * pcrl_adam_step, per element of a tensor with flag bit 0 (others keep p, m, v):
 *   g' = (g * grad_scale) * clip_coef[0]            (clip_coef may be NULL: no second product)
 *   decoupled: p = p * decay  [decay = (float)(1 - lr * wd)]      else: g' = g' + decay * p  [decay = wd]
 *   m = m + (g' - m) * one_minus_beta1;   v = v * beta2 + (g' * g') * one_minus_beta2
 *   p = p - coefs[2t] * (m / (sqrtf(v) / coefs[2t + 1] + eps))
 * 16-byte accesses where a group of four lies inside one tensor and p, g, m, v are 16-byte aligned, scalar ones elsewhere.
 * pcrl_grad_norm: norm[0] = sqrt(sum over the tensors with flag bit 0 of ((double)(g * grad_scale))^2), float64 in an order that depends on
 * `total` alone (no atomics); numels (int64[ntensors], may be NULL) keeps a slot's padding out of the sum;
 * coef[0] = (float)min(1, max_norm / (norm + 1e-6)); partials: float64[pcrl_optim_grid_cap()] of scratch.
 * pcrl_sgd_step_clipped: pcrl_sgd_step on (g * grad_scale) * clip_coef[0]; with clip_coef[0] == 1 its result has pcrl_sgd_step's bits. */
int pcrl_optim_grid_cap(void);
int pcrl_adam_prepare(const int32_t* flags, int32_t* steps, double* prods, float* coefs, int ntensors, double lr, double beta1,
                      double beta2, pcrl_stream_t stream);
int pcrl_adam_step(float* p, const float* g, float* m, float* v, const int64_t* offsets, const int32_t* flags, const float* coefs,
                   int ntensors, int64_t total, float decay, int decoupled, float one_minus_beta1, float beta2, float one_minus_beta2,
                   float eps, float grad_scale, const float* clip_coef, pcrl_stream_t stream);
int pcrl_grad_norm(const float* g, const int64_t* offsets, const int64_t* numels, const int32_t* flags, int ntensors, int64_t total,
                   float grad_scale, double max_norm, double* partials, double* norm, float* coef, pcrl_stream_t stream);
int pcrl_sgd_step_clipped(float* p, const float* g, float* buf, const int64_t* offsets, const int32_t* flags, int ntensors,
                          int64_t total, float lr, float momentum, float weight_decay, float grad_scale, const float* clip_coef,
                          pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Input pipeline: the torchio transforms of data.py:73-89 / datasets/lunaDataset.py:28-81 on float32 volumes
 * [B][D][H][W] resident on the device, one random parameter set per volume (drawn by the caller).  Each entry point states the definition
 * it implements and is pinned to it alone, bit for bit or to a derived bound (tests/test_augment_exact_gpu.py); the blur's definition is held
 * to scipy.ndimage.gaussian_filter within the tail mass of its fixed radius.  NOT PINNED: torchio itself (absent from the image; the
 * reference holds no vectors) -- its affine conventions and random streams.  Every entry point refuses null pointers, B <= 0, empty
 * extents (and B > 65535 where B is the grid's y: affine, blur_axis, noise_gamma, znorm); affine and blur_axis refuse x == y.
 *   volume_min : vmin[b] = min over the volume (RandomAffine's default_pad_value='minimum')
 *   affine     : RandomFlip(axes=0) then RandomAffine: y(o) = trilinear sample of flip_d^{flip[b]}(x) at centre + inv[b] (o - centre),
 *                inv[b] row-major 3x3 in (d,h,w) order and isotropic voxel units, samples outside the volume = fill[b]
 *   blur_axis  : one axis (0=d,1=h,2=w) of RandomBlur: Gaussian of std sigma[b] voxels, taps -radius..radius, symmetric borders
 *   noise_gamma: RandomNoise then RandomGamma: v = x + noise_std[b] * n(0,1) (counter-based generator: index, volume and all 64 seed bits
 *                key both Box-Muller draws through two per-volume keys, so no two volumes of a call share a field), y = sign(v) |v|^gamma[b]
 *   meanstd / znorm : ZNormalization: (x - mean[b]) * rstd[b], rstd = 1 / unbiased standard deviation
 *   swap       : RandomSwap, in place: for it < iters, exchange patch origins[it][b][0] with patch origins[it][b][1] ([d,h,w] corners,
 *                patch pd x ph x pw); the caller makes the two corners of a skipped (overlapping) draw equal */
int pcrl_aug_volume_min(const float* x, float* vmin, int B, int64_t S, pcrl_stream_t stream);
int pcrl_aug_affine(const float* x, float* y, const float* inv, const int* flip, const float* fill, int B, int D, int H, int W, pcrl_stream_t stream);
int pcrl_aug_blur_axis(const float* x, float* y, const float* sigma, int B, int D, int H, int W, int axis, int radius, pcrl_stream_t stream);
int pcrl_aug_noise_gamma(const float* x, float* y, const float* noise_std, const float* gamma, int B, int64_t S, int64_t seed, pcrl_stream_t stream);
int pcrl_aug_meanstd(const float* x, float* mean, float* rstd, int B, int64_t S, pcrl_stream_t stream);
int pcrl_aug_znorm(const float* x, float* y, const float* mean, const float* rstd, int B, int64_t S, pcrl_stream_t stream);
int pcrl_aug_swap(float* x, const int* origins, int B, int D, int H, int W, int pd, int ph, int pw, int iters, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 2D (chest X-ray) input pipeline: the torchvision chain of data.py:14-61 / datasets/chestDataset.py:31-48 on uint8 images, restating
 * the Pillow arithmetic every one of its transforms hands over to (csrc/augment2d.hip).  V views of side S (224 global, 96 local), one
 * record of PCRL_AUG2D_NPARAM int32 per view (drawn and packed by pcrlv2_amd/data_chest.py):
 *   [0] byte offset of the view's source in `src` (H x W x C interleaved uint8, C = 1 for a mode-L image, 3 otherwise), [1..3] H, W, C,
 *   [4..7] crop box j, i, w, h (RandomResizedCrop), [8..13] NEAREST rotation as Pillow's 16.16 fixed-point affine a0..a5 (RandomRotation),
 *   [14] flip (RandomHorizontalFlip), [15] grayscale (RandomGrayscale), [16] blur, [17] integer box radius, [18] ww, [19] fw (Pillow's
 *   BoxBlur weights of GaussianBlur(sigma)), [20] number of ColorJitter ops, [21] their order (4 bits each: 0 brightness, 1 contrast,
 *   2 saturation, 3 hue), [22..24] brightness / contrast / saturation factors as float32 bits, [25] hue shift (0..255 added to PIL's H),
 *   [26] Cutout holes, [27..38] up to three clipped holes (y0, y1, x0, x1), [39] byte offset of the view's intermediate in `inter`.
 *   hresample   : horizontal BILINEAR pass of the crop box: inter = [h][S][C] uint8 (max_rows = the largest h)  -- transforms.RandomResizedCrop
 *   spatial     : vertical pass at the pixel the rotation and the flip pick: view = [V][3][S][S] uint8 (C planes used), target = NULL or
 *                 [V][3][S][S] float32 Normalize(ToTensor(view))  -- RandomResizedCrop + RandomRotation + RandomHorizontalFlip,
 *                 chestDataset.py:36-41 (x, x2)
 *   photometric : grayscale, blur, jitter, ToTensor, Normalize, Cutout of the views: out = [V][3][S][S] float32, u8_out = NULL or the
 *                 uint8 planes before ToTensor (tests)  -- data.py:31-44 (train_transform, local_transform), utils.py:60-98 (Cutout) */
#define PCRL_AUG2D_NPARAM 40
int pcrl_aug2d_hresample(const uint8_t* src, const int* params, uint8_t* inter, int V, int S, int max_rows, pcrl_stream_t stream);
int pcrl_aug2d_spatial(const uint8_t* inter, const int* params, uint8_t* view, float* target, int V, int S, pcrl_stream_t stream);
int pcrl_aug2d_photometric(const uint8_t* view, const int* params, float* out, uint8_t* u8_out, int V, int S, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LUNA16 pre-processing (luna_preprocess.py:134-348, csrc/luna_prep.hip, host side pcrlv2_amd/luna_prep.py).  Volumes are int16 in
 * (z, y, x) memory order (GetArrayFromImage); the logical array is its transpose (x, y, z).  float64 arithmetic throughout.
 *   resample : ITK ResampleImageFilter with an identity transform and output spacing 1: output index o has the continuous index
 *              (o * 1.0) / spacing per axis, 0 unless it is < size - 0.5 on every axis; linear interpolation along x, then y, then z
 *              (a + (b - a) * t, the upper neighbour clamped to size - 1); cast by clamping to the int16 range, truncating toward zero.
 *              in = [Z][Y][X], out = [OZ][OY][OX].
 *   windows  : W crop windows of `vol` ([Z][Y][X] int16, reads at z >= Z give the pad value -1000), each normalised
 *              (clip to [-1000, 1000], (v + 1000) / 2000) and resized as skimage.transform.resize(order=1, mode='reflect',
 *              preserve_range=True) does: separable Gaussian (mode mirror on the crop, scipy's symmetric correlate1d order) over the
 *              axes with radius > 0, zoom with grid_mode coordinates (o + 0.5) * ratio - 0.5 and order-1 mirror weights, clip to the
 *              crop's min / max.  One int64 record of PCRL_PREP_NREC per window:
 *                [0..2] start x, y, z in the logical volume, [3..5] source sizes, [6..8] output sizes (z <= 64), [9..11] Gaussian radius
 *                per axis (0: no filter, <= PCRL_PREP_RMAX), [12] offset of the window in `out` (doubles; stored [ox][oy][sd]), [13] sd:
 *                output depths stored, [14] offset of its two workspace buffers in `ws` (doubles; 2 * sx*sy*sz), [15] depth-score
 *                depth D (0: none; D + 2 <= oz).
 *              One double record of PCRL_PREP_NPRM per window: [a * (RMAX + 1) + j] Gaussian weight of taps +-j on axis a,
 *              [3 * (RMAX + 1) + a] zoom ratio in / out of axis a (host-computed).
 *              stats = [W][3] int: the exact depth score 2 * n0 + n1 over d < D (k = the first of 0..2 with w[i,j,d+k] >= 0.425,
 *              2 if none; n0 / n1 count k = 0 / 1), then the crop's raw min and max.  max_src / max_cols bound sx*sy*sz / ox*oy. */
#define PCRL_PREP_NREC 16
#define PCRL_PREP_NPRM 32
#define PCRL_PREP_RMAX 8
int pcrl_prep_resample(const int16_t* in, int16_t* out, int X, int Y, int Z, int OX, int OY, int OZ, double spacing_x, double spacing_y, double spacing_z, pcrl_stream_t stream);
int pcrl_prep_windows(const int16_t* vol, int X, int Y, int Z, const int64_t* rec, const double* prm, int W, int64_t max_src, int max_cols, double* out, int64_t out_len, int* stats, double* ws, int64_t ws_len, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LUNA16 nodule candidates (csrc/luna_cubes.hip, host side pcrlv2_amd/luna_nodules.py): cubes around the points of candidates_V2.csv out of the
 * 1 mm volume that pcrl_prep_resample leaves ([Z][Y][X] int16).
 *   cubes      : out[m][i][j][k] = clip(vol[z0 + k][y0 + j][x0 + i], -1000, 1000) with (x0, y0, z0) = start[m][0..2] (int32 [M][3]; may be negative
 *                or past the edge: a coordinate outside the volume gives -1000).  out_kind 0: int16 [M][CX][CY][CZ]; 1: float32 of the same shape
 *                holding float32((double(v) + 1000.0) / 2000.0), the pre-task's normalisation.  CX, CY, CZ: positive multiples of 8, <= 64; anything
 *                else is PCRL_EINVAL before any launch.  M = 0: nothing happens.  vol 2-byte, start 4-byte, out 16-byte aligned.  One launch, LDS
 *                transpose, no atomics, no workspace: deterministic.
 *   hu_to_unit : out[i] = float32((double(in[i]) + 1000.0) / 2000.0), no clip (for int16 cubes that come from disk); in and out 16-byte aligned. */
int pcrl_prep_cubes(const int16_t* vol, int X, int Y, int Z, const int32_t* start, int M, void* out, int out_kind, int CX, int CY, int CZ, pcrl_stream_t stream);
int pcrl_prep_hu_to_unit(const int16_t* in, float* out, int64_t n, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Test hooks (NOT part of the drop-in surface; process-wide atomics, default 0 / tr 1 = the product path).  They select which
 * of the kernels behind one entry point runs, so that tests can check every kernel against the same reference and probes can
 * time them against each other inside one process (tools/conv_probe.py).  The state they set and the code tables live in csrc/core.hip.
 *   conv  impl: 0 auto (wide-brick kernel, else 4x8x8-brick kernel, where eligible; co-located launch), 1 gather kernel, 2 gather kernel
 *               without split-K, 3 4x8x8-brick kernel on its plain 2-D grid, 4 the 4x8x8-brick kernel also where the 4x8x16-brick one is
 *               eligible, 5 / 6 auto with the wide-brick kernel on 4 x 8 x 16 bricks only / on 8 x 8 x 16 bricks wherever they tile
 *   wgrad impl: 0 auto (brick kernel where eligible, XCD co-located launch), 1 gather kernel, 2 brick kernel on its plain 2-D grid with the
 *               old walk order, 4 / 5 co-located launch with the old walk order / plain grid with the new walk order (experiments),
 *               6 co-located launch with 64 x 64 tiles only (0 also uses 128 x 64, 64 x 128 and 64 x 32 tiles)
 *   wgrad tr  : bf16 fragment fetch of the gather weight-gradient kernel: 1 ds_read_b64_tr_b16, 0 scalar LDS reads
 *   conv2d impl: 0 auto (wide-brick / brick / narrow kernels where eligible), 1 gather kernel, 2 auto without the wide-brick kernel */
void pcrl_debug_set_conv_impl(int impl);
void pcrl_debug_set_wgrad_impl(int impl);
void pcrl_debug_set_wgrad_tr(int on);
void pcrl_debug_set_conv2d_impl(int impl);
/* Timing ablation (tools/double_ablation.py): the non-accumulating fixed-order second passes of the weight gradients are launched n times (idempotent);
 * the step-time difference between n = 2 and n = 1 is what those launches cost inside the multi-stream step.  Default 1. */
void pcrl_debug_set_reduce_repeat(int n);

/* ---------------------------------------------------------------------------------------
 * Backward of one half of the projection / predictor heads (csrc/heads_fused.hip; models/pcrlv2_model_3d.py:55-59,67-70 and
 * models/pcrlv2_model.py:108-111,124-127) in ONE launch: the data gradient of a Linear, the BatchNorm1d (+ReLU) backward of the tensor that
 * gradient belongs to, and the Linear's weight / bias gradients -- aten::mm x 2 + sum (addmm backward), native_batch_norm_backward,
 * threshold_backward.  All float32, row-major:
 *   t[n][c] = add[n][c] + sum_k dy[n][k] * W[k][c]      dy [N][K] (NULL: t = add), W [K][C] (the Linear's weight [out][in]), add [N][C] or NULL
 *   dx, dgamma, dbeta = BatchNorm1d backward of t through xbn [N][C] (the normalisation's input), gamma, mean, rstd [C];
 *                       relu != 0: t is masked where ybn [N][C] (the normalisation's ReLU'd output) is <= 0 first
 *   dW[k][c] = sum_n dy[n][k] * xin[n][c], db[k] = sum_n dy[n][k]      xin [N][C]: the Linear's input in forward
 * N <= 512 rows, C % 4 == 0, K % 4 == 0. */
int pcrl_head_bwd_stage(const float* dy, const float* W, const float* add, const float* xin, const float* xbn, const float* ybn,
                        const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta, float* dW,
                        float* db, int N, int K, int C, int relu, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 2D path, the ResNet stem (csrc/stem2d.hip): conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False) of the ResNet-18 encoder
 * smp.Unet('resnet18', in_channels=3) builds (models/pcrlv2_model.py:200) -- aten::convolution / convolution_backward (weight branch; the
 * image needs no gradient) reading the float32 NCHW image as the loader delivers it (train_2d.py:139-141).  bf16 MFMA, float32 accumulation.
 * Available where pcrl_stem7_ok() != 0: bf16, even H, W with H/2 a multiple of 8 and W/2 a multiple of 32 (else pcrl_conv2d_* on the image
 * padded to 8 channels).
 *   pack  : float32 [64][3][7][7] -> bf16 [64][7][32] (k = kw * 4 + c; zeros at c = 3 and kw = 7): pcrl_stem7_packed_elems() elements
 *   fwd   : y bf16 NHWC [N][H/2][W/2][64]; stats: pcrl_stem7_stats_rows(N, H, W) rows of [64][2] (sum, sum^2) for bn1, or NULL
 *   wgrad : dw_ref float32 [64][3][7][7] from dy bf16 [N][H/2][W/2][64]; ws: pcrl_stem7_wgrad_ws_bytes */
int64_t pcrl_stem7_ok(int N, int H, int W, int dtype);
int64_t pcrl_stem7_packed_elems(void);
int64_t pcrl_stem7_stats_rows(int N, int H, int W);
size_t pcrl_stem7_wgrad_ws_bytes(int N, int H, int W);
int pcrl_stem7_pack(const float* w_ref, void* out, pcrl_stream_t stream);
int pcrl_stem7_fwd(const float* x, const void* wp, void* y, float* stats, int N, int H, int W, int dtype, pcrl_stream_t stream);
int pcrl_stem7_wgrad(const float* x, const void* dy, float* dw_ref, void* ws, size_t ws_bytes, int N, int H, int W, int dtype,
                     pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 2D path, fused passes of the ResNet-18 encoder (csrc/encoder2d.hip): each replaces a chain of separate passes over one tensor and
 * reproduces the chain's values bit for bit (intermediates the chain stored are rounded to `dtype` here too).
 *   bn_add_relu_fwd      : out = relu(T(scale*y + shift) + i), i = r (identity) or T(rscale*r + rshift) (the downsample branch's
 *                          BatchNorm2d; rscale / rshift both NULL or both given) -- torchvision BasicBlock.forward's
 *                          `out = self.bn2(out); out += identity; out = self.relu(out)` (aten::native_batch_norm's apply half, add_, relu_)
 *   relu_mask_sum_bwd    : g = T(da + db) where a > 0, else 0 -- the two gradients that reach a BasicBlock's output (next block's conv1
 *                          branch and identity branch) summed and masked (aten::add + aten::threshold_backward)
 *   bn_relu_maxpool2d_3s2_fwd : p, idx = MaxPool2d(3, 2, 1)(T(relu(scale*y + shift))) from one pass over the stem convolution's output
 *                          (the full-resolution activation has no other consumer on the training path); idx as pcrl_maxpool2d_3s2_fwd
 *   maxpool2d_3s2_bwd_sum: pcrl_maxpool2d_3s2_bwd of T(dy + dy2) (the pooled tensor feeds layer1.0's conv1 and its identity branch) */
int pcrl_bn_add_relu_fwd(const void* y, const float* scale, const float* shift, const void* r, const float* rscale, const float* rshift,
                         void* out, int64_t M, int C, int dtype, pcrl_stream_t stream);
int pcrl_relu_mask_sum_bwd(const void* da, const void* db, const void* a, void* g, int64_t n, int dtype, pcrl_stream_t stream);
int pcrl_bn_relu_maxpool2d_3s2_fwd(const void* y, const float* scale, const float* shift, void* p, uint8_t* idx, int N, int H, int W, int C,
                                   int dtype, pcrl_stream_t stream);
int pcrl_maxpool2d_3s2_bwd_sum(const void* dy, const void* dy2, const uint8_t* idx, void* dx, int N, int H, int W, int C, int dtype,
                               pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 2D path, the 3-channel ends of the step (csrc/heads2d.hip).
 * pcrl_mse2d_fwd / _bwd_pad -- nn.MSELoss()(masks, gt) at train_2d.py:165,167 with the prediction in NHWC memory (float32 [N][HW][C], what
 *   the segmentation / deep-supervision heads write) and the target as the loader delivers it (float32 NCHW [N][C][HW]): no layout copy of
 *   the image.  The backward writes d loss / d masks as `dtype` [N*HW][CP] with zeros in channels C..CP-1 -- the form the convolution
 *   backward kernels take (CP = 8), or unpadded float32 (CP = C) for the bilinear backward -- and leaves colpart[pcrl_rows1024(N*HW)][CP],
 *   per-block column sums whose total (pcrl_colsum) is the bias gradient of the convolution that produced the masks
 *   (aten::mse_loss_backward + the zero-pad copy + the sum over pixels of aten::convolution_backward's bias branch).
 * pcrl_conv2d_1x1_small_bwd -- backward of deep_supervision_head[3] = nn.Conv2d(C, 3, kernel_size=1) (models/pcrlv2_model.py:106;
 *   aten::convolution_backward): x `dtype` [M][Ci], dy float32 [M][3], w float32 [3][Ci] -> dx `dtype` [M][Ci] and
 *   part[pcrl_rows1024(M)][PW] (per block: 3*Ci dw entries, 3 db entries, zeros up to the row pitch PW >= 3*Ci + 3; pcrl_colsum
 *   finishes) in one pass over x and dy. */
int64_t pcrl_rows1024(int64_t M);
size_t pcrl_mse2d_ws_bytes(int64_t M);
int pcrl_mse2d_fwd(const float* p, const float* gt, float* loss, void* ws, size_t ws_bytes, int N, int64_t HW, int C, pcrl_stream_t stream);
int pcrl_mse2d_bwd_pad(const float* p, const float* gt, const float* dloss, void* dy, float* colpart, int N, int64_t HW, int C, int CP,
                       int dtype, pcrl_stream_t stream);
int pcrl_conv2d_1x1_small_bwd(const void* x, const float* dy, const float* w, void* dx, float* part, int64_t M, int Ci, int Co, int PW,
                              int dtype, pcrl_stream_t stream);
/* the network input (train_2d.py:139-141: `.float().cuda()` images, NCHW float32 [N][C][HW], C <= 8) as the `dtype` NHWC tensor [N*HW][CP]
 * with zero padding channels the ResNet stem's convolution reads (aten::zeros + aten::copy_ of a permuted view) */
int pcrl_nchw_to_nhwc_pad(const float* x, void* out, int N, int C, int64_t HW, int CP, int dtype, pcrl_stream_t stream);
/* out = a + b on float32 vectors: the sum of the two gradients that reach x_pro = bn(avgpool(x)) -- directly (the projection is a cosine
 * operand) and through the predictor head (pcrlv2_model.py:125-127, pcrlv2_model_3d.py:69-70) -- autograd's aten::add on a [N, C] matrix */
int pcrl_add_f32(const float* a, const float* b, float* out, int64_t n, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 2D path, supervised fine-tuning (csrc/cls_head.hip, csrc/auroc.hip).
 * pcrl_cls_head_fwd / _bwd -- smp's ClassificationHead(pooling='avg', dropout=p, activation='sigmoid') on the encoder's last feature map and
 *   nn.BCELoss on its output, as one operator (aten::mean + aten::native_dropout + aten::addmm + aten::sigmoid + aten::binary_cross_entropy and
 *   their backwards).  a: `dtype` NHWC [N][H][W][C] (C a power of two, 32..512); keep: uint8 [N][C] dropout keep mask, NULL = no dropout (eval);
 *   keep_scale = 1 / (1 - p); w float32 [K][C], b float32 [K] (K <= 64); labels uint8 [N][K] (non-zero = positive) or NULL.
 *   forward : probs float32 [N][K]; pooled float32 [N][C] (the mean over H*W, BEFORE the mask -- saved for the backward); with labels,
 *             loss[0] = mean over N*K of max(z,0) - y z + log1p(exp(-|z|)) on the logit z (= BCELoss(sigmoid(z), y) wherever that does not clamp
 *             its logarithm), float64 partial per sample + a fixed-order second launch: deterministic.  labels and loss are both NULL or both
 *             given.  ws: pcrl_cls_head_ws_bytes(N), only with labels.  The activation is read once.
 *   backward: from dloss[0] -- da `dtype` [N][H][W][C] (written once; NULL: not wanted), dw float32 [K][C], db float32 [K].  The activation is
 *             not read.  Two launches, no atomics.
 * pcrl_auroc_counts -- per class k of probs float32 [M][K] / labels uint8 [M][K]: counts[k] = {2 #(pos > neg) + #(pos == neg), #pos, #neg} (int64
 *   [K][3]) over all (positive, negative) pairs; exact integer counting, float comparison.  AUROC_k = counts[k][0] / (2 P Q) (host). */
size_t pcrl_cls_head_ws_bytes(int N);
int pcrl_cls_head_fwd(const void* a, const uint8_t* keep, float keep_scale, const float* w, const float* b, const uint8_t* labels, float* probs,
                      float* pooled, float* loss, void* ws, size_t ws_bytes, int N, int H, int W, int C, int K, int dtype, pcrl_stream_t stream);
int pcrl_cls_head_bwd(const float* probs, const uint8_t* labels, const float* dloss, const float* pooled, const uint8_t* keep, float keep_scale,
                      const float* w, void* da, float* dw, float* db, int N, int H, int W, int C, int K, int dtype, pcrl_stream_t stream);
int pcrl_auroc_counts(const float* probs, const uint8_t* labels, int64_t* counts, int64_t M, int K, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, segmentation fine-tuning (csrc/seg_head.hip).
 * pcrl_seg_head_fwd / _bwd / _eval -- out_tr.final_conv (1x1x1, 64 -> K) -> sigmoid -> wb * BCE + wd * (1 - mean_k Dice_k) as one operator.  Replaces,
 *   per class, pcrl_conv3d_to1_fwd + pcrl_sigmoid_fwd (forward) and pcrl_sigmoid_bwd + pcrl_conv3d_to1_wgrad + pcrl_conv3d_to1_dgrad (backward) of the
 *   n_class != 1 constructor variant, and the aten loss passes over [N, K, D, H, W] that a segmentation loss on top of them would add.
 *   a: `dtype` NDHWC rows [N * S][64] (S = D * H * W voxels per sample); w float32 [K][64], b float32 [K], 1 <= K <= 7; labels uint8 [N * S]: bit k = the
 *   voxel belongs to class k (classes may overlap), bit 7 = the voxel is NOT counted (no sum, zero gradient).
 *   BCE = mean over the Mc counted voxels x K of max(z,0) - y z + log1p(exp(-|z|)) (0 when Mc = 0); Dice_k = (2 I_k + 1) / (P_k + G_k + 1) with
 *   I = sum p g, P = sum p, G = sum g over the counted voxels of the whole call.
 *   forward : sums float64 [4 K + 1] = {I_k, P_k, G_k, BCE_k} per class, then Mc; loss float32 [1].  One read of a; per-block float64 partials and a
 *             fixed-order second launch (deterministic; no floating-point atomics); no [M][K] tensor is written.
 *   backward: from dloss[0] and the forward's sums (both on the device) -- recomputes z and p with the forward's arithmetic; dx `dtype` [N * S][64] written
 *             once (NULL: not wanted; rows of uncounted voxels are exactly zero, and their activations enter neither dw nor any sum, finite or not), dw float32 [K][64], db float32 [K] from per-block partials added in
 *             block order.
 *   eval    : the forward (labels may be NULL: nothing labelled, everything counted) plus counts[case_index[n]][k] += {TP, |pred|, |gt|} (int64
 *             [n_cases][K][3], NOT cleared here; 64-bit integer atomics, order-independent) with pred = (z >= 0); case_index int32 [N] or NULL (= n),
 *             an index outside [0, n_cases) is skipped; mask uint8 [N * S] or NULL: the predicted bitmask, 0 where bit 7 of the label is set.
 *   ws: pcrl_seg_head_ws_bytes(N, S, K) bytes for any of the three. */
size_t pcrl_seg_head_ws_bytes(int N, int64_t S, int K);
int pcrl_seg_head_fwd(const void* a, const float* w, const float* b, const uint8_t* labels, double* sums, float* loss, float wb, float wd, void* ws,
                      size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream);
int pcrl_seg_head_bwd(const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums, const float* dloss, float wb, float wd,
                      void* dx, float* dw, float* db, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream);
int pcrl_seg_head_eval(const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts, int n_cases,
                       uint8_t* mask, double* sums, float* loss, float wb, float wd, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                       pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, overlap-blended sliding-window inference of the segmenter (csrc/seg_head.hip, csrc/seg_blend.hip).
 * pcrl_seg_head_logits -- the head's logits and nothing else: z float32 [N * S][K] from a / w / b as above, with the arithmetic of the three kernels
 *   above (a logit is bit-identical to the one pcrl_seg_head_eval thresholds).  One read of a; no workspace.
 * pcrl_seg_cut_patches -- the patches of one case, cut on the device: img [C][X][Y][Z] float32 (src_half = 0) or float16 (src_half = 1); starts int32
 *   [n][3] on the device; out float32 [n][C][cx][cy][cz] (cz a multiple of 4, out 16-byte aligned), 0 outside the volume.  A pure copy, float16 widened exactly.
 * pcrl_seg_blend -- the per-patch logits of ONE case z float32 [P][cx][cy][cz][K], P = nx * ny * nz patches in x-major order (p = (ix * ny + iy) * nz
 *   + iz) at the ascending, distinct starts sx [nx], sy [ny], sz [nz] (int32, device) that cover the volume X x Y x Z, blended with the separable
 *   window wx [cx], wy [cy], wz [cz] (float32, positive).  Per voxel and class, over the covering patches (s <= v < s + crop) in ascending ix, iy, iz:
 *       w = (wx[i] * wy[j]) * wz[k];  num_k = num_k + w * z_k;  den = den + w        plain float32 in this order, no fused multiply-add
 *   labels uint8 [X][Y][Z] or NULL (nothing labelled, everything counted): bits as above.  Outputs, each may be NULL:
 *     mask   uint8 [X][Y][Z]: bit k = (num_k >= 0) -- no division decides a prediction; 0 where bit 7 of the label is set
 *     probs  float32 [K][X][Y][Z]: 1 / (1 + exp(-num_k / den))
 *     numden float32 [2 K + 1][X][Y][Z]: num_k per class, then den, then zbar_k = num_k / den per class (tests)
 *     sums   float64 [4 K + 1] and loss float32 [1] (both or neither): the head's {I, P, G, BCE} per class and Mc from zbar = num / den over the counted
 *            voxels, the loss of the head's formula; per-block float64 partials and the head's fixed-order second launch.  ws: pcrl_seg_blend_ws_bytes.
 *     counts int64 [K][3] (with sums only): {TP, |pred|, |gt|} ADDED to this one row of a counts table with 64-bit integer atomics.
 *   No floating-point atomics: two runs give identical bytes.
 *   PCRL_EINVAL for K outside 1..7, an empty volume or crop, and P != nx * ny * nz.
 * Mirror test-time augmentation and checkpoint ensembles: every further set of per-patch logits is ADDED into z, un-mirrored, so the buffer keeps its
 *   size.  A mirror code `flip` in 0..7 has bit 0 = x, bit 1 = y, bit 2 = z: the patch's first, second and third spatial axis (z is the fastest).
 * pcrl_seg_cut_patches_mirror -- pcrl_seg_cut_patches' output with the patch BOX mirrored along the axes of flip, the zeros it has outside the
 *   volume included: out[p][c][i][j][k] = patch[p][c][fx ? cx-1-i : i][fy ? cy-1-j : j][fz ? cz-1-k : k].  flip = 0 gives pcrl_seg_cut_patches' bytes.
 *   PCRL_EINVAL for flip outside 0..7 and for whatever pcrl_seg_cut_patches refuses.
 * pcrl_seg_head_logits_acc -- pcrl_seg_head_logits of a sample grid cx x cy x cz (S = cx * cy * cz) whose input was mirrored by flip: the logit zk of
 *   voxel s = (i * cy + j) * cz + k of sample n (bit-identical to pcrl_seg_head_logits') goes to the un-mirrored voxel
 *   s' = ((fx ? cx-1-i : i) * cy + (fy ? cy-1-j : j)) * cz + (fz ? cz-1-k : k):
 *       v = first ? zk : z[n][s'][sub] + zk;   z[n][s'][sub] = v * scale;        plain float32: one add, one multiply, in this order
 *   Every element of z is read and written by exactly one thread: no atomics, two runs give identical bytes.  No workspace.
 *   PCRL_EINVAL for flip outside 0..7, S != cx * cy * cz, and whatever pcrl_seg_head_logits refuses. */
int pcrl_seg_head_logits(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, pcrl_stream_t stream);
int pcrl_seg_cut_patches(const void* img, int src_half, const int* starts, float* out, int n, int C, int X, int Y, int Z, int cx, int cy, int cz,
                         pcrl_stream_t stream);
int pcrl_seg_cut_patches_mirror(const void* img, int src_half, const int* starts, float* out, int n, int C, int X, int Y, int Z, int cx, int cy, int cz,
                                int flip, pcrl_stream_t stream);
int pcrl_seg_head_logits_acc(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, int cx, int cy, int cz, int flip,
                             int first, float scale, pcrl_stream_t stream);
size_t pcrl_seg_blend_ws_bytes(int X, int Y, int Z);
int pcrl_seg_blend(const float* z, int64_t P, const int* sx, const int* sy, const int* sz, int nx, int ny, int nz, const float* wx, const float* wy,
                   const float* wz, int cx, int cy, int cz, int X, int Y, int Z, int K, const uint8_t* labels, uint8_t* mask, float* probs, float* numden,
                   int64_t* counts, double* sums, float* loss, float wb, float wd, void* ws, size_t ws_bytes, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, segmentation fine-tuning with a SOFTMAX head over mutually exclusive classes (csrc/seg_head_mc.hip): the sibling of pcrl_seg_head_*.
 *   a, w, b, dtype, N, S as there; 2 <= K <= 16 classes, the background (class 0) included.  labels uint8 [N * S] is a LABEL MAP: y = byte & 0x7F is the
 *   voxel's class index, bit 7 = the voxel is NOT counted (no sum, zero gradient).  The range of y is not checked on the device (the host checks a case when
 *   it opens it): a voxel with y >= K is treated as not counted by every entry point.
 *   Per voxel, in one fixed order shared by all four kernels (the file header states the tree of every sum):
 *       z_k = b_k + sum_c W[k][c] a[c];  m = max_k z_k;  e_k = exp(z_k - m);  s = sum_k e_k;  p_k = e_k / s;  ce = (m - z_y) + log s
 *   forward : sums float64 [4 K + 1] = {I_k = sum_{y=k} p_k, P_k = sum p_k, G_k = #{y = k}, CE_k = sum_{y=k} ce} per class over the counted voxels, then Mc;
 *             loss float32 [1] = wc (sum_k CE_k) / Mc + wd (1 - (1 / (K-1)) sum_{k=1}^{K-1} (2 I_k + 1) / (P_k + G_k + 1)): the background is not in the Dice
 *             mean; Mc = 0: the CE term is 0 and so is the loss.  One read of a, per-block float64 partials, a fixed-order second launch; no
 *             floating-point atomics and no [M][K] tensor.
 *   backward: from dloss[0] = c and the forward's sums (both on the device).  q_0 = 0, q_k = -(c wd / (K-1)) (2 [y=k] / U_k - (2 I_k + 1) / U_k^2),
 *             U_k = P_k + G_k + 1:   dz_j = (c wc / Mc) (p_j - [y=j]) + p_j (q_j - sum_k p_k q_k).
 *             dx `dtype` [N * S][64] written once (NULL: not wanted; rows of uncounted voxels are exactly zero, and their activations, finite or not, enter
 *             nothing); dw float32 [K][64], db float32 [K] from per-block partials added in block order.
 *   eval    : the forward (labels may be NULL: every voxel counted as background) plus counts[case_index[n]][k] += {TP, |pred|, |gt|} (int64
 *             [n_cases][K][3], ALL K rows, NOT cleared here; 64-bit integer atomics) with pred = the LOWEST k with z_k == m; case_index int32 [N] or NULL
 *             (= n), an index outside [0, n_cases) is skipped; labelmap uint8 [N * S] or NULL: the predicted class index, 0 where the voxel is not counted.
 *   logits  : z float32 [N * S][K], each bit-identical to the logit eval takes its maximum over, stored as pcrl_seg_head_logits_acc stores: at the
 *             un-mirrored voxel s' of the sample grid cx x cy x cz (S = cx * cy * cz), v = first ? z_k : z[s'][k] + z_k; z[s'][k] = v * scale (plain float32,
 *             one add, one multiply).  flip = 0, first = 1, scale = 1 is the plain case.  One thread reads and writes each element; no workspace.
 *   ws: pcrl_seg_mc_head_ws_bytes(N, S, K) bytes for fwd / bwd / eval (0 for sizes the entry points refuse).
 *   PCRL_EINVAL for K outside 2..16 and whatever the pcrl_seg_head_* siblings refuse.
 * pcrl_seg_labelmap_to_bits / _keep -- label maps through the bitmask tools (surface distances, connected components), a group of n <= 7 classes
 *   first .. first + n - 1 at a time, `count` bytes:  to_bits: out bit j = ((lab & 0x7F) == first + j), bit 7 carried over;
 *   keep: out = lab, except that a voxel whose class is in the group and whose bit in `bits` is clear becomes background (bit 7 carried over).  out may be lab. */
size_t pcrl_seg_mc_head_ws_bytes(int N, int64_t S, int K);
int pcrl_seg_mc_head_fwd(const void* a, const float* w, const float* b, const uint8_t* labels, double* sums, float* loss, float wc, float wd, void* ws,
                         size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream);
int pcrl_seg_mc_head_bwd(const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums, const float* dloss, float wc, float wd,
                         void* dx, float* dw, float* db, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream);
int pcrl_seg_mc_head_eval(const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts, int n_cases,
                          uint8_t* labelmap, double* sums, float* loss, float wc, float wd, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                          pcrl_stream_t stream);
int pcrl_seg_mc_head_logits(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, int cx, int cy, int cz, int flip,
                            int first, float scale, pcrl_stream_t stream);
/* pcrl_seg_mc_blend -- pcrl_seg_blend's label-map sibling (csrc/seg_blend.hip): the same inputs and the same per-voxel accumulation (w = (wx wy) wz;
 *   num_k += w z_k; den += w; plain float32, covering patches in ascending ix, iy, iz), 2 <= K <= 16.  Outputs, each may be NULL:
 *     labelmap uint8 [X][Y][Z]: the LOWEST k with maximal num_k (no division decides a prediction); 0 where the voxel is not counted
 *     probs  float32 [K][X][Y][Z]: softmax of zbar_k = num_k / den (m = max, e_k = exp(zbar_k - m), s summed in ascending k, e_k / s)
 *     numden float32 [2 K + 1][X][Y][Z]: num_k per class, then den, then zbar_k per class (tests)
 *     sums float64 [4 K + 1] and loss float32 [1] (both or neither): the softmax head's formula on zbar; ws: pcrl_seg_mc_blend_ws_bytes
 *     counts int64 [K][3] (with sums only): {TP, |pred|, |gt|} of all K classes ADDED to this one row (integer atomics)
 *   No floating-point atomics: two runs give identical bytes.  PCRL_EINVAL for K outside 2..16 and whatever pcrl_seg_blend refuses. */
size_t pcrl_seg_mc_blend_ws_bytes(int X, int Y, int Z);
int pcrl_seg_mc_blend(const float* z, int64_t P, const int* sx, const int* sy, const int* sz, int nx, int ny, int nz, const float* wx, const float* wy,
                      const float* wz, int cx, int cy, int cz, int X, int Y, int Z, int K, const uint8_t* labels, uint8_t* labelmap, float* probs,
                      float* numden, int64_t* counts, double* sums, float* loss, float wc, float wd, void* ws, size_t ws_bytes, pcrl_stream_t stream);
int pcrl_seg_labelmap_to_bits(const uint8_t* lab, int first, int n, uint8_t* out, int64_t count, pcrl_stream_t stream);
int pcrl_seg_labelmap_keep(const uint8_t* lab, const uint8_t* bits, int first, int n, uint8_t* out, int64_t count, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, surface-distance metrics of stored segmentation masks: HD95, HD, ASSD (csrc/surface_dist.hip, compiled with -ffp-contract=off).
 *   Masks are the uint8 bitmasks of the segmenter, [X][Y][Z]: bit k = class k, bit 7 of the GROUND TRUTH = the voxel is not counted and belongs to
 *   neither mask.  The definitions are MedPy's hd95 / hd / assd; the host finishes them in float64 (train_seg.surface_metrics).
 * pcrl_surf_extract -- surf_pred, surf_gt uint8 [X][Y][Z]: bit k = the voxel is in class k's mask and at least one of its 6 face neighbours is not
 *   (a neighbour outside the volume is not): m & ~binary_erosion(m, 6-connected cross), all K classes of both masks in one pass; bits >= K are 0.
 *   counts int64 [K][3]: {TP, |pred|, |gt|} of the effective masks ADDED to this row (pcrl_seg_head_eval's convention; 64-bit integer atomics).
 * pcrl_edt_sq -- d2 float64 [X][Y][Z]: the squared distance of every voxel to the nearest voxel whose byte in `surf` has bit `bit` set,
 *       d2 = min over surface voxels of fl(fl(fl(sx dx))^2 + fl(fl(fl(sy dy))^2 + fl(fl(sz dz))^2))     float64, no fused multiply-add, this order
 *   by three in-place line passes Z, Y, X (each min_j fl(fl(s (i - j))^2) + f[j], with an early exit that leaves every bit as it is); +inf
 *   everywhere for an empty surface.  steps int64 [1] or NULL: the scan steps executed (two multiplications, up to two additions and three
 *   comparisons each) are ADDED to it.  An axis may have at most pcrl_edt_max_axis() = 1024 voxels (a line is staged in LDS): PCRL_EINVAL beyond.
 *   ws: pcrl_edt_sq_ws_bytes (0 today: ws may be NULL).
 * pcrl_surf_dist_stats -- one class: A = d2_to_gt at the voxels of surf_pred with bit `bit`, B = d2_to_pred at those of surf_gt, U = A u B as a
 *   multiset of n = n_a + n_b values.  record: 8 slots of 8 bytes
 *       [0] n_a  [1] n_b  [2] lo = floor(q (double)(n - 1))                        int64
 *       [3] [4] [5] the order statistics of d2 over U at ranks lo, min(lo + 1, n - 1), n - 1   float64, EXACT (a radix select on the bit patterns)
 *       [6] sum of sqrt(d2) over A  [7] over B                                      float64, per-block partials added in block order
 *   Slots 2..7 are written only when both surfaces are non-empty.  Integer atomics only: two runs give identical bytes.  0 <= q <= 1.
 *   ws: pcrl_surf_dist_stats_ws_bytes(V), 8-byte aligned; V = X * Y * Z. */
int pcrl_surf_extract(const uint8_t* pred, const uint8_t* gt, uint8_t* surf_pred, uint8_t* surf_gt, int64_t* counts, int X, int Y, int Z, int K,
                      pcrl_stream_t stream);
int64_t pcrl_edt_max_axis(void);
size_t pcrl_edt_sq_ws_bytes(int X, int Y, int Z);
int pcrl_edt_sq(const uint8_t* surf, int bit, double* d2, double sx, double sy, double sz, int64_t* steps, void* ws, size_t ws_bytes, int X, int Y,
                int Z, pcrl_stream_t stream);
size_t pcrl_surf_dist_stats_ws_bytes(int64_t V);
int pcrl_surf_dist_stats(const double* d2_to_gt, const uint8_t* surf_pred, const double* d2_to_pred, const uint8_t* surf_gt, int bit, double q,
                         int64_t* record, void* ws, size_t ws_bytes, int64_t V, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, connected components of a segmentation mask and the clean-up rules on them (csrc/components.hip; integer only).
 *   Masks are the uint8 bitmasks of the segmenter, [X][Y][Z], Z contiguous: bit k = class k.  A class-k voxel is one whose byte has bit k set; every
 *   other bit is ignored by the labelling and copied by the filter.  Limits: 1 <= X * Y * Z < 2^31 (voxel indices are 32-bit), any other shape,
 *   axes of length 1 and shapes that are no multiple of the tile included; bit in 0..6; PCRL_EINVAL otherwise, before any launch.
 * pcrl_ccl_label -- the components of class `bit` under connectivity 6, 18 or 26 (faces; faces and edges; faces, edges and corners:
 *   scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)).
 *       labels int32 [X][Y][Z]   0 for background, otherwise the component's number 1..n
 *       sizes  int32 [>= (X * Y * Z + 1) / 2]   sizes[c - 1] = the voxels of component c; only [0, n) is written (no connectivity has more
 *              than ceil(V / 2) components)
 *       n      int32 [1]   the number of components, on the device
 *   Numbering: components are numbered by the ascending linear index ((x * Y + y) * Z + z) of their first voxel -- scipy.ndimage.label's numbering,
 *   so labels equals its result without any canonicalisation.  Integer atomics only, and every output is independent of their order: two runs give
 *   identical bytes.  ws: pcrl_ccl_ws_bytes(X, Y, Z) bytes, 4-byte aligned (0 for a shape that is refused).
 *   pcrl_ccl_tile: the tile (voxels along X, Y, Z) one block resolves in LDS before tiles are merged.  Both queries are host functions.
 * pcrl_ccl_filter -- out = mask with bit `bit` cleared at every voxel whose component (labels, sizes, n of that bit, as pcrl_ccl_label wrote them)
 *   fails the rule; all other bits, and every voxel with label 0, are copied.
 *       keep_largest != 0   only the component with the most voxels survives; among equals the lowest label (selected on the device by one
 *                           block over sizes[0, n), keys (size << 32) | ~label)
 *       min_voxels > 0      only components of at least min_voxels voxels survive
 *   Both: a component must pass both.  Neither: a copy.  n == 0 (an empty class): a copy.  out must not be mask; min_voxels >= 0.
 *   ws: pcrl_ccl_filter_ws_bytes() bytes, 4-byte aligned. */
int pcrl_ccl_tile(int* tx, int* ty, int* tz);
size_t pcrl_ccl_ws_bytes(int X, int Y, int Z);
int pcrl_ccl_label(const uint8_t* mask, int bit, int connectivity, int* labels, int* sizes, int* n, void* ws, size_t ws_bytes, int X, int Y, int Z,
                   pcrl_stream_t stream);
size_t pcrl_ccl_filter_ws_bytes(void);
int pcrl_ccl_filter(const uint8_t* mask, const int* labels, const int* sizes, const int* n, uint8_t* out, int bit, int keep_largest,
                    int64_t min_voxels, void* ws, size_t ws_bytes, int X, int Y, int Z, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, joint image / label augmentation of segmentation training crops (csrc/seg_augment.hip).
 * pcrl_seg_aug_resample -- ONE launch resamples a batch of source boxes into training crops, image channels and label bitmask through the same
 *   geometry:  src [B][C][Sx][Sy][Sz] float32 (src_half = 0) or float16 (src_half = 1), src_lab uint8 [B][Sx][Sy][Sz]  ->
 *   y float32 [B][C][X][Y][Z], lab uint8 [B][X][Y][Z];  inv float32 [B][12]: the rows (m0 m1 m2 t) of x, y and z;  gain, bias float32 [B][C].
 *   For output voxel i = (ix, iy, iz), in float32:
 *       c = i + 0.5 - (X, Y, Z) / 2          s = M c + t + (Sx, Sy, Sz) / 2 - 0.5      (flips are sign changes of M, folded in by the host)
 *       y[b][ch][i] = gain[b][ch] * T + bias[b][ch],  T = the trilinear sample of channel ch at s, a corner outside the source box contributing 0
 *                     (scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=0)); float16 sources are widened exactly
 *       lab[b][i]   = src_lab[b][n], n = floor(s + 0.5) per axis (a tie goes up: s = -0.5 is voxel 0), 0x80 where n is outside the box
 *                     (order=0, mode='grid-constant', cval=0x80): nearest neighbour, no byte that the source does not hold except 0x80
 *   The coordinate, the corner offsets and the weights are formed once per voxel and shared by all channels and the label.  Every read is
 *   bounds-checked in the kernel: no matrix, NaN included, reaches memory outside the box.  No atomics: two runs give identical bytes.
 *   PCRL_EINVAL, before any launch: a null pointer; B outside 1..65535; C outside 1..16; an extent < 1; a source box or a crop of 2^31 voxels or
 *   more; y or lab overlapping src, src_lab or each other. */
int pcrl_seg_aug_resample(const void* src, int src_half, const uint8_t* src_lab, float* y, uint8_t* lab, const float* inv, const float* gain,
                          const float* bias, int B, int C, int Sx, int Sy, int Sz, int X, int Y, int Z, pcrl_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * 3D path, preparation of raw volumes into the segmenter's cases and the way back (csrc/seg_prep.hip, -ffp-contract=off).
 *   Sources stay in DISK order: src [C][Z][Y][X], x fastest, int16 (src_kind = 0) or float32 (src_kind = 1); src_lab uint8 [Z][Y][X].  Outputs are in
 *   project order, z fastest.  The mask M of a voxel is (any channel != 0).  Common refusals, PCRL_EINVAL before any launch: a null or overlapping
 *   buffer, C outside 1..16, K outside 1..7, an extent < 1, a grid of 2^31 voxels or more.  Integer atomics only; every output element is written
 *   once: two runs give identical bytes.
 * pcrl_segprep_scan -- rec int64 [8] = {x0, x1, y0, y1, z0, z1, |M|, non-finite values}: the half-open bounding box of M (empty: every lower
 *   bound 0x7fffffff, every upper bound 0), the voxels of M and the count of NaN / +-inf over all channels.
 * pcrl_segprep_stats -- stats float64 [C][2] = {mean, population standard deviation} of min(max(x, lo), hi) over M (use_mask != 0; n = rec[6], rec as
 *   pcrl_segprep_scan wrote it) or over every voxel (use_mask = 0; rec may be NULL).  clip float64 [C][2] = {lo, hi} or NULL (no clip).  Two passes,
 *   sum(x) / n then sqrt(sum((x - mean)^2) / n), per-block partials added in block order by a one-block launch: a function of the sizes and the data.
 *   ws: pcrl_segprep_stats_ws_bytes(C, X * Y * Z), 8-byte aligned.
 * pcrl_segprep_select -- out float32 [4]: the EXACT order statistics at ranks r0..r3 (0-based, ascending order) of channel ch over M (use_mask != 0)
 *   or over every voxel; -0.0 counts as +0.0 and is returned as +0.0.  A radix select on order-preserving 32-bit keys, four byte passes.
 *   ws: pcrl_segprep_select_ws_bytes(), 8-byte aligned.
 * pcrl_segprep_resample -- ONE launch: the box [bx, bx + NX) x [by, by + NY) x [bz, bz + NZ) of the source -> img [C][OX][OY][OZ] float32
 *   (out_half = 0) or float16 (out_half = 1) and lab uint8 [OX][OY][OZ].  Tables, built by the host in float64, indices relative to the box:
 *       tab_i int32   i0, i1, nn of x [3][OX], then of y [3][OY], then of z [3][OZ]          tab_w float64   w0, w1 of x [2][OX], y [2][OY], z [2][OZ]
 *   Per output voxel and channel, float64, one operation at a time (v: a corner's value, widened exactly):
 *       u   = (min(max(v, lo), hi) - mean) / max(std, 1e-8)     0.0 where use_mask != 0 and the corner is outside M
 *       acc = 0.0;  for x in (i0, i1): for y in (i0, i1): for z in (i0, i1):  acc = acc + ((u * wx) * wy) * wz
 *   and ONE rounding of acc to the output type (float16 as well: csrc/seg_prep.hip).  stats float64 [C][2] {mean, std} or NULL (0, 1); clip float64
 *   [C][2] {lo, hi} or NULL (-inf, +inf).  lab = region[src_lab[nn_z][nn_y][nn_x]], region uint8 [256]; src_lab NULL (an unlabelled case): lab = 0
 *   and region may be NULL.  K = the number of regions (bits 0..K-1 of region's entries).  Every table entry is clamped to the box inside the kernel.
 *   pcrl_segprep_resample_tile: the output tile (along x and z; one y) and the LDS bytes a launch with these box and output extents uses (host function).
 * pcrl_segprep_restore -- pred uint8 [PX][PY][PZ] (the prepared grid) -> out uint8 [X][Y][Z]: inside the box out = pred[nn_x][nn_y][nn_z] with
 *   tab int32 = nn of x [NX], y [NY], z [NZ] (prepared indices of the box's voxels, clamped in the kernel), 0 outside.  painted uint8 [X][Y][Z] or
 *   NULL: paint[out], paint uint8 [256]. */
int pcrl_segprep_scan(const void* src, int src_kind, int C, int X, int Y, int Z, int64_t* rec, pcrl_stream_t stream);
size_t pcrl_segprep_stats_ws_bytes(int C, int64_t V);
int pcrl_segprep_stats(const void* src, int src_kind, int C, int X, int Y, int Z, int use_mask, const int64_t* rec, const double* clip, double* stats,
                       void* ws, size_t ws_bytes, pcrl_stream_t stream);
size_t pcrl_segprep_select_ws_bytes(void);
int pcrl_segprep_select(const void* src, int src_kind, int C, int ch, int X, int Y, int Z, int use_mask, int64_t r0, int64_t r1, int64_t r2, int64_t r3,
                        float* out, void* ws, size_t ws_bytes, pcrl_stream_t stream);
int pcrl_segprep_resample_tile(int NX, int NZ, int OX, int OZ, int use_mask, int* tx, int* tz, int64_t* lds_bytes);
int pcrl_segprep_resample(const void* src, int src_kind, const uint8_t* src_lab, int C, int X, int Y, int Z, int bx, int by, int bz, int NX, int NY,
                          int NZ, const int32_t* tab_i, const double* tab_w, const double* stats, const double* clip, const uint8_t* region, int K,
                          int use_mask, void* img, int out_half, uint8_t* lab, int OX, int OY, int OZ, pcrl_stream_t stream);
int pcrl_segprep_restore(const uint8_t* pred, int PX, int PY, int PZ, const int32_t* tab, int bx, int by, int bz, int NX, int NY, int NZ,
                         const uint8_t* paint, uint8_t* out, uint8_t* painted, int X, int Y, int Z, pcrl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCRL_HIP_H */
