// Internal interface of the library: the ONE declaration of every function that crosses a translation unit without being part of the
// C ABI (include/pcrl_hip.h), grouped by the file that defines it, and the process-wide test-hook state.  Every .hip that defines or
// calls one of these includes this header; the build compiles with -Werror=missing-prototypes, so a non-static function without a
// declaration here (or in the ABI header) does not compile.  C++ linkage throughout: none of these is exported for callers.
#pragma once
#include "common.h"
#include <atomic>

// ---- core.hip: test-hook state and environment switches --------------------------------------------------------------------------
// What the pcrl_debug_set_* entry points (decoded in core.hip, code table in pcrl_hip.h) leave behind; dispatchers and launchers read it.
struct PcrlHooks {
  std::atomic<int> conv_impl{0};        // 3D forward / dgrad: 0 auto (brick kernels where eligible), 1 always the gather kernel, 2 gather kernel without split-K
  std::atomic<int> brick_ymap{1};       // conv_brick.hip: channel tiles of a brick co-located (0: its plain 2-D grid)
  std::atomic<int> brick16_on{1};       // conv_brick16.hip: the wide-brick kernel is eligible at all
  std::atomic<int> brick16_planes{-1};  // -1: the default rule (4-plane bricks); 0: 4-plane bricks only; 2: 8-plane bricks wherever they tile
  std::atomic<int> wgrad_impl{0};       // 0 auto (brick kernels where eligible), 1 always the gather kernel
  std::atomic<int> wgrad_tr{1};         // bf16 fragment fetch: 1 = ds_read_b64_tr_b16, 0 = scalar LDS reads
  std::atomic<int> wb_xcd{1};           // wgrad_brick.hip: 0: the 2-D grid (a (tile, kd) block range per blockIdx.y)
  std::atomic<int> wb_order{1};         // wgrad_brick.hip: 1 the new walk order, 0 the old one
  std::atomic<int> wb_tiles{1};         // wgrad_brick.hip: 0: 64 x 64 tiles only
  std::atomic<int> conv2d_impl{0};      // 0 auto (wide brick / brick / narrow kernels where eligible), 1 always the gather kernel, 2 auto without the wide brick
  std::atomic<int> reduce_repeat{1};    // launches of the non-accumulating second passes of the weight gradients (timing ablation)
};
extern PcrlHooks g_hooks;

// Environment switches of launch code, read once per process (names, defaults and meaning: README).
struct PcrlEnv {
  bool dgrad_bnred_off;   // PCRL_DGRAD_BNRED=0: no fused data gradient + BatchNorm-backward reduction (3D and 2D)
  int igemm_vmajor_max;   // PCRL_IGEMM_VMAJOR: largest volume (voxels) that takes voxel-major rows; default (and =1) 8, =0 off
  bool upc_pack_tiled;    // PCRL_UPC_PACK_TILED=0: the untiled pack kernel of the composed weights (bit-identical outputs)
};
const PcrlEnv& pcrl_env();

// ---- conv_brick.hip: LDS-halo brick kernel (4 x 8 x 8 voxels; 2D: KD = 1 with the image index as depth) ---------------------------
bool pcrl_brick_conv_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_brick_conv_rows(int N, int D, int H, int W);
int pcrl_brick_conv_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_brick_conv2d_eligible(int N, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_brick_conv2d_rows(int N, int H, int W);
int pcrl_brick_conv2d_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int H, int W, int Ci, int Co, int up, hipStream_t stream);
int pcrl_brick_conv2d_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, const void* res, float act_lo,
                                    void* a, int N, int H, int W, int Ci, int Co, int up, hipStream_t stream);
bool pcrl_brick8_upc_fwd_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_brick8_upc_fwd_launch(const void* x, const void* w3, const float* bias_tab, void* y0, float* stats, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_brick8_upc_dgrad_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_brick8_upc_dgrad_launch(const void* dy0, const void* wd3, void* dx, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_brick16.hip: wide-brick LDS-DMA kernel (4 x 8 x 16 voxels, W % 16 == 0; 2D: MODE 3, 4 images x 8 x 16 pixels, no upsampled source)
bool pcrl_brick16_conv_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_brick16_conv_rows(int N, int D, int H, int W);
int pcrl_brick16_conv_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_brick16_conv2d_eligible(int N, int H, int W, int Ci, int Co, int dtype);
int64_t pcrl_brick16_conv2d_rows(int N, int H, int W);
int pcrl_brick16_conv2d_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_brick16_upc.hip: composed up-conv modes of the wide-brick kernel -------------------------------------------------------
bool pcrl_brick16_upc_fwd_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_brick16_upc_fwd_launch(const void* x, const void* w3, const float* bias_tab, void* y0, float* stats, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_brick16_upc_dgrad_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_brick16_upc_dgrad_launch(const void* dy0, const void* wd3, void* dx, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_brick16_inf.hip: convolution + eval-mode BatchNorm + activation ------------------------------------------------------------
int pcrl_brick16_conv_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, float act_lo, void* a,
                                    int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
int pcrl_brick16_conv2d_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, float act_lo, void* a,
                                      int N, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_brick16_bnr.hip: data gradient + first pass of the BatchNorm backward of the layer below ----------------------------------
int pcrl_brick16_dgrad_bnred_launch(const void* dy, const void* wp, void* dx, const void* bn_y, const float* scale, const float* shift, const float* mean,
                                    const float* rstd, float* partial, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
int pcrl_brick16_dgrad2d_bnred_launch(const void* dy, const void* wp, void* dx, const void* bn_y, const float* scale, const float* shift, const float* mean,
                                      const float* rstd, float* partial, int N, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_up2.hip: ConvTranspose3d(k2, s2) forward ---------------------------------------------------------------------------------
bool pcrl_convt_up2_eligible(int Ci, int Co, int dtype);
int pcrl_convt_up2_launch(const void* x, const void* wp, const float* bias, void* y, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);

// ---- conv_igemm.hip: gather implicit-GEMM forms of the composed up-conv, and plain GEMMs with float32 plane-major results ------------
int pcrl_upc_fwd_launch(const void* x, const void* wf, const float* bias_tab, void* y0, float* stats, int N, int D, int H, int W, int Ci, int Co, int dtype, hipStream_t stream);
int64_t pcrl_upc_dgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Co);   // split-K workspace of the gather form (0: none)
int pcrl_upc_dgrad_launch(const void* dy0, const void* wd, void* dx, void* ws, int64_t ws_bytes, int N, int D, int H, int W, int Ci, int Co, int dtype, hipStream_t stream);
int pcrl_gemm_planes_launch(const void* a, const void* b, float* z, int64_t M, int K, int Nc, int dtype, hipStream_t stream);
int pcrl_pointwise_planes_launch(const void* x, const void* wt, float* z, int64_t M, int C, int dtype, hipStream_t stream);

// ---- conv_to1_brick.hip: LDS-halo brick kernel of the C -> 1 convolution ---------------------------------------------------------------
bool pcrl_to1_brick_eligible(int N, int D, int H, int W, int C, int taps, int dtype);
int64_t pcrl_to1_brick_rows(int N, int D, int H, int W);
int pcrl_to1_brick_launch(const void* x, const float* w_ref, const float* bias, float* y, float* stats, void* ws, size_t ws_bytes, int N, int D, int H, int W, int C, hipStream_t stream);

// ---- conv2d_narrow.hip: right-sized kernel for layers with <= 32 channels on both sides ----------------------------------------------
bool pcrl_conv2d_narrow_eligible(int N, int H, int W, int Cs, int Nc, int ks, int dtype);
int64_t pcrl_conv2d_narrow_rows(int N, int H, int W);
int pcrl_conv2d_narrow_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int H, int W, int Cs, int Nc, int ks, int up, int out_f32, int red2, hipStream_t stream);
int pcrl_conv2d_narrow_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, const void* res, float act_lo,
                                     void* a, int N, int H, int W, int Cs, int Nc, int ks, int up, hipStream_t stream);

// ---- wgrad_brick.hip: LDS-halo brick weight-gradient kernel (3D; composed up-conv mode; 2D with the image index as depth, nkd = 1) ----
bool pcrl_wgrad_brick_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_wgrad_brick_splits(int N, int D, int H, int W, int Ci, int Co);
int pcrl_wgrad_brick_slabs(int N, int D, int H, int W, int Ci, int Co);   // partial slabs the launch writes (<= pcrl_wgrad_brick_splits)
int pcrl_wgrad_brick_launch(const void* x, const void* dy, float* ws, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_wgrad_brick_upc_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype);
int pcrl_wgrad_brick_upc_slabs(int N, int D, int H, int W, int Ci, int Co);
int pcrl_wgrad_brick_upc_launch(const void* x, const void* dy0, float* ws, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream);
bool pcrl_wgrad_brick2d_eligible(int N, int H, int W, int Ci, int Co, int dtype);
int pcrl_wgrad_brick2d_splits(int N, int H, int W, int Ci, int Co);
int pcrl_wgrad_brick2d_launch(const void* x, const void* dy, float* ws, int N, int H, int W, int Ci, int Co, int up, hipStream_t stream);

// ---- wgrad2d_narrow.hip: right-sized weight-gradient kernel for the 16/32-channel 2D layers -------------------------------------------
bool pcrl_wgrad2d_narrow_eligible(int N, int H, int W, int CiP, int CoP, int dtype);
int pcrl_wgrad2d_narrow_slabs(int N, int H, int W);
int pcrl_wgrad2d_narrow_launch(const void* x, const void* dy, float* ws, int N, int H, int W, int CiP, int CoP, int up, hipStream_t stream);

// ---- conv_wgrad.hip: gradient of the COMPOSED up-conv weights, dweff[co][ci][p * 8 + q] (gather form; brick form with its own second pass)
size_t pcrl_upc_wgrad_ws_bytes(int N, int D, int H, int W, int Ci, int Co);
int pcrl_upc_wgrad_launch(const void* dy0, const void* x, float* dweff, void* ws, size_t ws_bytes, int N, int D, int H, int W, int Ci, int Co, int dtype, hipStream_t stream, bool accumulate);
size_t pcrl_upc_wgrad3_ws_bytes(int N, int D, int H, int W, int Ci, int Co);
int pcrl_upc_wgrad3_launch(const void* dy0, const void* x, float* dweff, void* ws, size_t ws_bytes, int N, int D, int H, int W, int Ci, int Co, hipStream_t stream, bool accumulate);

// ---- norm_pool.hip: weighted column sum, the whole weight gradient of a 1x1x1 convolution to one channel -----------------------------
size_t pcrl_weighted_colsum_ws_bytes(int64_t M, int C);
int pcrl_weighted_colsum(const void* v, const float* rowscale, float* out, void* ws, size_t ws_bytes, int64_t M, int C, int dtype, hipStream_t stream);

// ---- seg_head.hip: the fixed-order second launch of the segmentation sums, shared with seg_blend.hip ------------------------------------
// partial [nb][32] float64 per-block sums (slot k * 4 + {I, P, G, BCE}, slot 28: counted voxels) -> sums [4 K + 1] and loss [1], added in block order
constexpr int PCRL_SEG_SLOTS = 32, PCRL_SEG_CNT_SLOT = 28;
void pcrl_seg_sums_launch(const double* partial, int nb, int K, float wb, float wd, double* sums, float* loss, hipStream_t stream);
// ---- seg_head.hip / seg_head_mc.hip: what the sigmoid head and the softmax head (label maps) share ----------------------------------------
// The launch geometry, the prefetching row fetch, the per-`sub` wave sum, the un-mirroring index of the accumulating logits kernels and the
// second launch of the weight gradient.  partial [nb][K * 65] float32 per-block dW [K][64] + db [K] -> dw, db, added in block order.
constexpr int PCRL_SEG_C = 64, PCRL_SEG_MAX_BLOCKS = 1024;
__host__ __device__ inline int pcrl_seg_wstride(int K) { return K * (PCRL_SEG_C + 1); }   // floats of one block's dW [K][64] + db [K] partial
void pcrl_seg_wsum_launch(const float* partial, int nb, int K, float* dw, float* db, hipStream_t stream);

// blocks per sample: enough to fill the device, few enough that the second launches stay short; a function of the sizes only (determinism)
inline int sh_gx(int N, int64_t S) {
  const int64_t want = (S + 31) / 32, cap = PCRL_SEG_MAX_BLOCKS / N > 0 ? PCRL_SEG_MAX_BLOCKS / N : 1;
  return (int)(want < cap ? want : cap);
}

template <typename T>
__device__ __forceinline__ void sh_fetch(const T* __restrict__ a, const uint8_t* __restrict__ labels, int64_t base, int s, int S, int sub, Vec16<T>& x,
                                         unsigned& lab) {
  constexpr int V = Vec16<T>::N;
  if (s < S) {
    x = ld16(a + (base + s) * PCRL_SEG_C + sub * V);
    lab = labels ? labels[base + s] : 0u;
  } else {      // past the sample's end: a zero row that is not counted
#pragma unroll
    for (int j = 0; j < V; ++j) x.v[j] = from_f<T>(0.0f);
    lab = 0x80u;
  }
}

// sum over the lanes of a wave that own the same `sub` (one per voxel group)
template <int LPV, typename A> __device__ __forceinline__ A sh_group_sum(A v) {
#pragma unroll
  for (int o = 32; o >= LPV; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct ShMirror {
  int cx, cy, cz, flip;      // the sample's grid (S = cx * cy * cz, z fastest) and the mirror code: bit 0 = x, bit 1 = y, bit 2 = z
};

// float index in z of class `sub` at the un-mirrored voxel of (i, j, k) of the sample that starts at voxel `base`
__device__ __forceinline__ int64_t sh_unmirrored(const ShMirror& m, int64_t base, int i, int j, int k, int K, int sub) {
  const int ii = (m.flip & 1) ? m.cx - 1 - i : i, jj = (m.flip & 2) ? m.cy - 1 - j : j, kk = (m.flip & 4) ? m.cz - 1 - k : k;
  return (base + ((int64_t)ii * m.cy + jj) * m.cz + kk) * K + sub;
}

// The probability of a logit: the blend's loss equals the head's only because both use this one expression.
__device__ __forceinline__ float seg_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
// CALL(KK) with the compile-time class count KK = K; the entry points have checked 1 <= K <= 7.
#define PCRL_SEG_DISPATCH_K(CALL)            \
  switch (K) {                               \
    case 1: CALL(1); break;                  \
    case 2: CALL(2); break;                  \
    case 3: CALL(3); break;                  \
    case 4: CALL(4); break;                  \
    case 5: CALL(5); break;                  \
    case 6: CALL(6); break;                  \
    default: CALL(7); break;                 \
  }

// ---- seg_head_mc.hip: the softmax head's fixed-order second launch, shared with seg_blend.hip's label-map blend ------------------------------
// partial [nb][72] float64 per-block sums (slot k * 4 + {I, P, G, CE}, slot 4 K: counted voxels) -> sums [4 K + 1] and loss [1], added in block order
constexpr int PCRL_SEG_MC_SLOTS = 72;
void pcrl_seg_mc_sums_launch(const double* partial, int nb, int K, float wc, float wd, double* sums, float* loss, hipStream_t stream);
// CALL(KK) with the compile-time class count KK = K; the entry points have checked 2 <= K <= 16.
#define PCRL_SEG_MC_DISPATCH_K(CALL) \
  switch (K) {                       \
    case 2: CALL(2); break;          \
    case 3: CALL(3); break;          \
    case 4: CALL(4); break;          \
    case 5: CALL(5); break;          \
    case 6: CALL(6); break;          \
    case 7: CALL(7); break;          \
    case 8: CALL(8); break;          \
    case 9: CALL(9); break;          \
    case 10: CALL(10); break;        \
    case 11: CALL(11); break;        \
    case 12: CALL(12); break;        \
    case 13: CALL(13); break;        \
    case 14: CALL(14); break;        \
    case 15: CALL(15); break;        \
    default: CALL(16); break;        \
  }

