// Inference instantiations of the wide-brick convolution kernel (conv_brick16.h, INF): the forward 3x3x3 convolution of an eval-mode LUConv
// (models/pcrlv2_model_3d.py:9,33 in .eval(): aten::convolution -> native_batch_norm on the running statistics -> relu) with the normalisation
// and the activation applied to the float32 accumulators in the epilogue.  A translation unit of its own: the training instantiations
// (conv_brick16.hip, conv_brick16_bnr.hip) sit at the 256-register budget and must not move.
#include "conv_brick16.h"

int pcrl_brick16_conv_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, float act_lo, void* a,
                                    int N, int D, int H, int W, int Ci, int Co, hipStream_t stream) {
  Brick16Params p{(const bf16*)x, (const bf16*)wp, bias, (bf16*)a, nullptr, N, D, H, W, Ci, Co, 0, 0, nullptr, 0, nullptr, scale, shift, nullptr, nullptr, act_lo};
  const int BN = Co % 64 == 0 ? 64 : 32, ny = Co / BN;
  const int64_t bricks = pcrl_brick16_conv_rows(N, D, H, W);
  if (bricks * ny >= ((int64_t)1 << 31)) return pcrl_fail(PCRL_EINVAL, "brick16_conv_affine: grid too large");
  dim3 grid((unsigned)bricks, ny);
  if (ny > 1) {   // the channel tiles of a brick adjacent on one XCD, as in pcrl_brick16_conv_launch
    p.ny = ny;
    grid = dim3((unsigned)(bricks * ny));
  }
  return BN == 64 ? launch16<64, 0, 4, false, true>(p, grid, stream, "brick16_conv_affine") : launch16<32, 0, 4, false, true>(p, grid, stream, "brick16_conv_affine");
}

// 2D path (MODE 3: 4 images x 8 x 16 pixels per brick): the 3x3 convolution of an eval-mode Conv2d -> BatchNorm2d -> ReLU
// (smp Conv2dReLU / torchvision BasicBlock.conv1 in .eval()) in one pass
int pcrl_brick16_conv2d_affine_launch(const void* x, const void* wp, const float* bias, const float* scale, const float* shift, float act_lo, void* a,
                                      int N, int H, int W, int Ci, int Co, hipStream_t stream) {
  Brick16Params p{(const bf16*)x, (const bf16*)wp, bias, (bf16*)a, nullptr, 1, N, H, W, Ci, Co, 0, 0, nullptr, 0, nullptr, scale, shift, nullptr, nullptr, act_lo};
  const int BN = Co % 64 == 0 ? 64 : 32, ny = Co / BN;
  const int64_t bricks = pcrl_brick16_conv2d_rows(N, H, W);
  if (bricks * ny >= ((int64_t)1 << 31)) return pcrl_fail(PCRL_EINVAL, "brick16_conv2d_affine: grid too large");
  dim3 grid((unsigned)bricks, ny);
  if (ny > 1) {
    p.ny = ny;
    grid = dim3((unsigned)(bricks * ny));
  }
  return BN == 64 ? launch16<64, 3, 4, false, true>(p, grid, stream, "brick16_conv2d_affine") : launch16<32, 3, 4, false, true>(p, grid, stream, "brick16_conv2d_affine");
}
