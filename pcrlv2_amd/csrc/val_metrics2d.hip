// Held-out validation metrics of the 2D pre-task: the terms of the training loss (train_2d.py:139-168) evaluated at EVERY one of the five scale
// indices instead of a drawn one, for one batch of eval-mode outputs, added to a device accumulator as batch-size-weighted sums (a validation
// pass reads back once, at its end).  Replaces, per batch, 6 x aten::mse_loss (train_2d.py:165,167), 5 x aten::upsample_bilinear2d
// (pcrlv2_model.py:190) and 5 x (2 + 4 * nlocal) x aten::cosine_similarity(dim=1, eps=1e-8).mean() (train_2d.py:111-117,148-163).
//
// acc[0]      += B * MSE(out1, gt)
// acc[1 + k]  += B * MSE(bilinear_up(mask_k, 2^(4 - k)), gt)      -- the upsampling happens INSIDE the reduction: the full-resolution map is never stored
// acc[6 + k]  += B * -(mean_r cos(pre1_k, pro2_k) + mean_r cos(pre2_k, pro1_k)) / 2
// acc[11 + k] += B * mean over the nlocal local views i and both global views v of -(cos(pre_v, proL_i) + cos(preL_i, pro_v)) / 2
// acc[16]     += B
// out1 and the maps: float32 NHWC, 3 channels (what the heads' convolutions write); gt: float32 NCHW as the loader delivers it (as pcrl_mse2d_fwd
// reads it).  Two stages, fixed order, no atomics, float64 throughout: the inputs are float32 and the interpolation weights of a power-of-two scale
// are dyadic ((2 j + 1) / 2 s), so every product is exact in float64 -- the fused form agrees with float64 torch to rounding of the few additions.
// Index rule of the interpolation: pcrl_upsample2d_bilinear_fwd's (ops2d.hip: align_corners=False, source clamped at 0, last index clamped).
#include "common.h"

namespace {

constexpr int V2_SCALES = 5, V2_PX = 1024;   // output pixels per block of the first stage

struct Val2dMaps {
  const float* out1;
  const float* mask[V2_SCALES];   // [B][H >> (4 - k)][W >> (4 - k)][3]
  const float* gt;                // [B][3][H][W]
  int B, H, W;
};

struct Val2dFeats {
  const float* f[V2_SCALES][6];   // per scale: pro1, pre1, pro2, pre2, proL, preL   (proL / preL: [nlocal * B][C], local view i in rows i * B ..)
  int C[V2_SCALES];
};

__device__ __forceinline__ void bilinear_src_f64(int dst, int s, int in_size, int& i0, int& i1, double& l1) {
  double src = ((double)dst + 0.5) / (double)s - 0.5;   // exact: s is a power of two
  if (src < 0.0) src = 0.0;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (double)i0;
}

__global__ void __launch_bounds__(256) val2d_mse_partial_kernel(const Val2dMaps t, double* __restrict__ ws) {
  __shared__ double red[4];
  const int64_t HW = (int64_t)t.H * t.W, npx = (int64_t)t.B * HW;
  const int64_t beg = (int64_t)blockIdx.x * V2_PX;
  const int64_t end = (beg + V2_PX < npx) ? beg + V2_PX : npx;
  double s[1 + V2_SCALES];
#pragma unroll
  for (int q = 0; q <= V2_SCALES; ++q) s[q] = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
    const int x = (int)(i % t.W);
    const int64_t r = i / t.W;
    const int y = (int)(r % t.H);
    const int64_t b = r / t.H;
    double g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (double)t.gt[(b * 3 + c) * HW + (int64_t)y * t.W + x];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = (double)t.out1[i * 3 + c] - g[c];
      s[0] += d * d;
    }
#pragma unroll
    for (int k = 0; k < V2_SCALES; ++k) {
      const int sh = V2_SCALES - 1 - k, sc = 1 << sh, Hk = t.H >> sh, Wk = t.W >> sh;
      int h0, h1, w0, w1;
      double lh, lw;
      bilinear_src_f64(y, sc, Hk, h0, h1, lh);
      bilinear_src_f64(x, sc, Wk, w0, w1, lw);
      const float* m = t.mask[k] + b * Hk * Wk * 3;
      const float* p00 = m + ((int64_t)h0 * Wk + w0) * 3;
      const float* p01 = m + ((int64_t)h0 * Wk + w1) * 3;
      const float* p10 = m + ((int64_t)h1 * Wk + w0) * 3;
      const float* p11 = m + ((int64_t)h1 * Wk + w1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = (1.0 - lh) * ((1.0 - lw) * (double)p00[c] + lw * (double)p01[c]) + lh * ((1.0 - lw) * (double)p10[c] + lw * (double)p11[c]);
        const double d = v - g[c];
        s[1 + k] += d * d;
      }
    }
  }
#pragma unroll
  for (int q = 0; q <= V2_SCALES; ++q) {
    const double v = block_sum_256(s[q], red);
    if (threadIdx.x == 0) ws[(int64_t)blockIdx.x * (1 + V2_SCALES) + q] = v;
  }
}

// one wave per (scale k = blockIdx.y, term row j): the row order of val_metrics.hip -- j < B: cos(pre1[j], pro2[j]); j < 2B: cos(pre2[r], pro1[r]); then, for
// local view i, row r and q = 0..3: cos(pre1[r], proL[iB + r]), cos(preL[iB + r], pro1[r]), cos(pre2[r], proL[iB + r]), cos(preL[iB + r], pro2[r])
__global__ void __launch_bounds__(256) val2d_cos_rows_kernel(const Val2dFeats t, double* __restrict__ vals, int B, int R, float eps) {
  const int lane = threadIdx.x & 63, k = blockIdx.y;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= R) return;
  const int C = t.C[k];
  int a, ra, b, rb;   // cos(f[a][ra], f[b][rb])
  if (j < B) { a = 1; ra = j; b = 2; rb = j; }
  else if (j < 2 * B) { a = 3; ra = j - B; b = 0; rb = j - B; }
  else {
    const int jj = j - 2 * B, tt = jj / B, r = jj - tt * B, i = tt >> 2, q = tt & 3;
    const int gv = (q >> 1) * 2;   // 0: view 1 (pro1 = 0, pre1 = 1), 2: view 2
    if (q & 1) { a = 5; ra = i * B + r; b = gv; rb = r; }
    else { a = gv + 1; ra = r; b = 4; rb = i * B + r; }
  }
  const float* __restrict__ x = t.f[k][a] + (int64_t)ra * C;
  const float* __restrict__ y = t.f[k][b] + (int64_t)rb * C;
  double dot = 0.0, xx = 0.0, yy = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double u = (double)x[c], v = (double)y[c];
    dot += u * v;
    xx += u * u;
    yy += v * v;
  }
  dot = wave_sum(dot);
  xx = wave_sum(xx);
  yy = wave_sum(yy);
  if (lane == 0) vals[(int64_t)k * R + j] = dot / (fmax(sqrt(xx), (double)eps) * fmax(sqrt(yy), (double)eps));
}

__global__ void __launch_bounds__(256) val2d_finish_kernel(const double* __restrict__ mse_ws, int blocks, const double* __restrict__ vals, int B, int R,
                                                           double inv_S, double w_local, double* __restrict__ acc) {
  __shared__ double red[4];
  double out[1 + 3 * V2_SCALES];
#pragma unroll
  for (int q = 0; q <= V2_SCALES; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) s += mse_ws[(int64_t)i * (1 + V2_SCALES) + q];
    out[q] = block_sum_256(s, red) * inv_S;
  }
#pragma unroll
  for (int k = 0; k < V2_SCALES; ++k) {
    double g = 0.0, l = 0.0;
    for (int j = threadIdx.x; j < R; j += 256) {
      const double v = vals[(int64_t)k * R + j];
      if (j < 2 * B) g += v;
      else l += v;
    }
    out[1 + V2_SCALES + k] = -0.5 * block_sum_256(g, red);
    out[1 + 2 * V2_SCALES + k] = -w_local * block_sum_256(l, red);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 1 + 3 * V2_SCALES; ++q) acc[q] += out[q];
    acc[1 + 3 * V2_SCALES] += (double)B;
  }
}

}  // namespace

extern "C" size_t pcrl_val2d_metrics_ws_bytes(int B, int H, int W, int nlocal) {
  if (B <= 0 || H <= 0 || W <= 0 || nlocal <= 0) return 0;
  const int64_t blocks = ((int64_t)B * H * W + V2_PX - 1) / V2_PX, R = (int64_t)B * (2 + 4 * nlocal);
  return (size_t)(blocks * (1 + V2_SCALES) + V2_SCALES * R) * sizeof(double);
}

extern "C" int pcrl_val2d_metrics(const float* out1, const float* const* masks, const float* gt, const float* const* feats, const int* C, double* acc,
                                  void* ws, size_t ws_bytes, int B, int H, int W, int nlocal, float eps, pcrl_stream_t stream) {
  PCRL_REQUIRE(B > 0 && H > 0 && W > 0 && nlocal > 0, "val2d_metrics: bad sizes B=%d H=%d W=%d nlocal=%d", B, H, W, nlocal);
  PCRL_REQUIRE(H % 16 == 0 && W % 16 == 0, "val2d_metrics: H and W must be multiples of 16 (the coarsest deep-supervision map is H/16 x W/16), got %d x %d", H, W);
  PCRL_REQUIRE(out1 && masks && gt && feats && C && acc, "val2d_metrics: null pointer");
  Val2dMaps m{out1, {}, gt, B, H, W};
  Val2dFeats t;
  for (int k = 0; k < V2_SCALES; ++k) {
    PCRL_REQUIRE(masks[k] && C[k] > 0, "val2d_metrics: null map or bad channel count at scale %d", k);
    m.mask[k] = masks[k];
    t.C[k] = C[k];
    for (int q = 0; q < 6; ++q) {
      PCRL_REQUIRE(feats[k * 6 + q], "val2d_metrics: null feature pointer (scale %d, tensor %d)", k, q);
      t.f[k][q] = feats[k * 6 + q];
    }
  }
  if (!ws || ws_bytes < pcrl_val2d_metrics_ws_bytes(B, H, W, nlocal)) return pcrl_fail(PCRL_EWORKSPACE, "val2d_metrics: workspace too small");
  const int64_t npx = (int64_t)B * H * W, blocks = (npx + V2_PX - 1) / V2_PX;
  PCRL_REQUIRE(blocks < ((int64_t)1 << 31), "val2d_metrics: too many pixels");
  const int R = B * (2 + 4 * nlocal);
  double* mse_ws = static_cast<double*>(ws);
  double* vals = mse_ws + blocks * (1 + V2_SCALES);
  hipLaunchKernelGGL(val2d_mse_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), m, mse_ws);
  hipLaunchKernelGGL(val2d_cos_rows_kernel, dim3((unsigned)((R + 3) / 4), V2_SCALES), dim3(256), 0, as_stream(stream), t, vals, B, R, eps);
  hipLaunchKernelGGL(val2d_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), mse_ws, (int)blocks, vals, B, R, 1.0 / (3.0 * (double)H * (double)W),
                     1.0 / (4.0 * nlocal), acc);
  return pcrl_check_launch("val2d_metrics");
}
