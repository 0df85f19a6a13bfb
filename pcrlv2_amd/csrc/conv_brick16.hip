// Plain 3x3x3 instantiations of the wide-brick convolution kernel (conv_brick16.h) and the dispatcher's interface to them.
#include "conv_brick16.h"

// ---- internal interface used by conv_igemm.hip's dispatcher -------------------------------------------------------
bool pcrl_brick16_conv_eligible(int N, int D, int H, int W, int Ci, int Co, int dtype) {
  // the halo plan addresses a brick's source rows by 32-bit offsets from its first halo voxel (up to ten planes of 2 Ci H W bytes), a weight row by a 32-bit offset
  return g_hooks.brick16_on && dtype == PCRL_BF16 && brick16_perm(D, H, W) != 0 && Ci % 32 == 0 && Co % 32 == 0 && (int64_t)N * D * H * W < ((int64_t)1 << 29) &&
         (int64_t)20 * Ci * H * W < ((int64_t)1 << 31) && (int64_t)54 * Ci * Co < ((int64_t)1 << 32);
}
int64_t pcrl_brick16_conv_rows(int N, int D, int H, int W) { return (int64_t)N * D * H * W / (TD * TH * TW); }

int pcrl_brick16_conv_launch(const void* x, const void* wp, const float* bias, void* y, float* stats,
                             int N, int D, int H, int W, int Ci, int Co, hipStream_t stream) {
  Brick16Params p{(const bf16*)x, (const bf16*)wp, bias, (bf16*)y, stats, N, D, H, W, Ci, Co, 0, 0, nullptr, 0};
  const int BN = Co % 64 == 0 ? 64 : 32, ny = Co / BN;
  // 8 x 8 x 16 bricks (one eight-wave block per CU) where there are two or more 64-channel tiles per brick, D % 8 == 0 and the grid still gives
  // every CU a block.  Measured per layer (tools/conv_probe.py, same box): 512->256 at 16x16x8 1445 -> 1544 TFLOP/s, 256->256 1433 -> 1495,
  // 256->128 at 32x32x16 1320 -> 1383, 128->128 1365 -> 1403; the 64-output-channel layers (one tile per brick) do not gain (128->64 at
  // 64x64x32: 1330 -> 1300) and small grids lose (128->128 at 16x16x8, 64 blocks: 1105 -> 805).
  // Round 5: with the halo plan (conv_brick16.h) the 4-plane form is as fast or faster on EVERY layer (same box, tools/conv_probe.py: 64->128 at 32x32x16
  // 1 363 vs 1 225 TFLOP/s, 256->128 1 537 vs 1 480, 128->128 1 492 vs 1 435, the 16x16x8 decoder layers within 1 %; one pass over the model's layers 4.28 vs
  // 4.35 ms) -- what the 8-plane brick saved was halo REQUEST ISSUE, which the plan made cheap.  Off; the instantiation stays behind the test hook
  // (pcrl_debug_set_conv_impl 5: the round-4 rule, 6: every eligible shape), bit-identical to the 4-plane form.
  const int planes = g_hooks.brick16_planes, nw8_mode = planes >= 0 ? planes : 0;
  int64_t bricks = pcrl_brick16_conv_rows(N, D, H, W);
  const bool nw8 = nw8_mode > 0 && BN == 64 && D % 8 == 0 && (nw8_mode == 2 || (ny >= 2 && (bricks / 2) * ny >= 256));
  if (nw8) bricks /= 2;
  if (bricks * ny >= ((int64_t)1 << 31)) return pcrl_fail(PCRL_EINVAL, "brick16_conv: grid too large");
  dim3 grid((unsigned)bricks, ny);
  if (ny > 1) {
    p.ny = ny;
    grid = dim3((unsigned)(bricks * ny));
  }
  if (nw8) return launch16<64, 0, 8>(p, grid, stream, "brick16_conv (8 planes)");
  return BN == 64 ? launch16<64, 0>(p, grid, stream, "brick16_conv") : launch16<32, 0>(p, grid, stream, "brick16_conv");
}


// ---- 2D path (MODE 3): 3x3 / stride 1 / pad 1 convolution of [N][H][W][Ci] images, forward or data gradient (conv2d.hip's dispatcher) ----
// The image index is the brick's d axis (4 images per brick); wp: packed [Co][9][Ci] (pcrl_conv2d_pack); stats [bricks][Co][2] or null.
bool pcrl_brick16_conv2d_eligible(int N, int H, int W, int Ci, int Co, int dtype) {
  return g_hooks.brick16_on && dtype == PCRL_BF16 && N % TD == 0 && brick16_perm(N, H, W) != 0 && Ci % 32 == 0 && Co % 32 == 0 &&
         (int64_t)N * H * W < ((int64_t)1 << 29) && (int64_t)20 * Ci * H * W < ((int64_t)1 << 31) && (int64_t)18 * Ci * Co < ((int64_t)1 << 32);
}
int64_t pcrl_brick16_conv2d_rows(int N, int H, int W) { return (int64_t)N * H * W / (TD * TH * TW); }
int pcrl_brick16_conv2d_launch(const void* x, const void* wp, const float* bias, void* y, float* stats, int N, int H, int W, int Ci, int Co, hipStream_t stream) {
  Brick16Params p{(const bf16*)x, (const bf16*)wp, bias, (bf16*)y, stats, 1, N, H, W, Ci, Co, 0, 0, nullptr, 0};
  const int BN = Co % 64 == 0 ? 64 : 32, ny = Co / BN;
  const int64_t bricks = pcrl_brick16_conv2d_rows(N, H, W);
  if (bricks * ny >= ((int64_t)1 << 31)) return pcrl_fail(PCRL_EINVAL, "brick16_conv2d: grid too large");
  dim3 grid((unsigned)bricks, ny);
  if (ny > 1) {
    p.ny = ny;
    grid = dim3((unsigned)(bricks * ny));
  }
  return BN == 64 ? launch16<64, 3>(p, grid, stream, "brick16_conv2d") : launch16<32, 3>(p, grid, stream, "brick16_conv2d");
}
