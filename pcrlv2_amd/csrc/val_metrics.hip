// Held-out validation metrics of the 3D pre-task: the terms of the training loss (train_3d.py:113-138) evaluated at EVERY scale index instead of a
// drawn one, for one batch of eval-mode outputs, added to a device accumulator as batch-size-weighted sums -- so that a validation pass reads back
// once, at its end.  Replaces, per batch, 4 x aten::mse_loss (train_3d.py:56,135,137) and 3 x (2 + 4 * nlocal) x aten::cosine_similarity(dim=1,
// eps=1e-8).mean() (train_3d.py:57,86-92,127-134).
//
// acc[0]      += B * MSE(out1, gt)                                          = sum (out1 - gt)^2 / S          (S = voxels per sample)
// acc[1 + k]  += B * MSE(mask_k, gt)
// acc[4 + k]  += B * -(mean_r cos(pre1_k, pro2_k) + mean_r cos(pre2_k, pro1_k)) / 2                          = -1/2 sum over rows
// acc[7 + k]  += B * mean over the nlocal local views i and both global views v of -(cos(pre_v, proL_i) + cos(preL_i, pro_v)) / 2
// acc[10]     += B
// Two stages, fixed order, no atomics, float64 throughout: the inputs are float32, their differences and products are exact in float64, so a metric
// that is nearly zero (a cosine term of 2e-3) keeps its relative accuracy -- validation numbers are compared across epochs and runs.  (The kernels
// are bound by reading the five maps once; the float64 arithmetic rides along.)
#include "common.h"

namespace {

constexpr int VM_CHUNK = 4096;

struct ValFeats {
  const float* f[3][6];   // per scale: pro1, pre1, pro2, pre2, proL, preL   (proL / preL: [nlocal * B][C], local view i in rows i * B ..)
  int C[3];
};

__global__ void __launch_bounds__(256) val_mse_partial_kernel(const float* __restrict__ out1, const float* __restrict__ m0, const float* __restrict__ m1,
                                                              const float* __restrict__ m2, const float* __restrict__ gt, double* __restrict__ ws, int64_t n) {
  __shared__ double red[4];
  const int64_t beg = (int64_t)blockIdx.x * VM_CHUNK;
  const int64_t end = (beg + VM_CHUNK < n) ? beg + VM_CHUNK : n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
    const double g = (double)gt[i];
    const double d0 = (double)out1[i] - g, d1 = (double)m0[i] - g, d2 = (double)m1[i] - g, d3 = (double)m2[i] - g;
    s0 += d0 * d0;
    s1 += d1 * d1;
    s2 += d2 * d2;
    s3 += d3 * d3;
  }
  s0 = block_sum_256(s0, red);
  s1 = block_sum_256(s1, red);
  s2 = block_sum_256(s2, red);
  s3 = block_sum_256(s3, red);
  if (threadIdx.x == 0) {
    double* o = ws + (int64_t)blockIdx.x * 4;
    o[0] = s0;
    o[1] = s1;
    o[2] = s2;
    o[3] = s3;
  }
}

// one wave per (scale k = blockIdx.y, term row j): j < B: cos(pre1[j], pro2[j]); j < 2B: cos(pre2[r], pro1[r]); then, for local view i, row r and
// q = 0..3: cos(pre1[r], proL[iB + r]), cos(preL[iB + r], pro1[r]), cos(pre2[r], proL[iB + r]), cos(preL[iB + r], pro2[r])
__global__ void __launch_bounds__(256) val_cos_rows_kernel(const ValFeats t, double* __restrict__ vals, int B, int R, float eps) {
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

__global__ void __launch_bounds__(256) val_finish_kernel(const double* __restrict__ mse_ws, int blocks, const double* __restrict__ vals, int B, int R,
                                                         double inv_S, double w_local, double* __restrict__ acc) {
  __shared__ double red[4];
  double out[10];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) s += mse_ws[(int64_t)i * 4 + q];
    out[q] = block_sum_256(s, red) * inv_S;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double g = 0.0, l = 0.0;
    for (int j = threadIdx.x; j < R; j += 256) {
      const double v = vals[(int64_t)k * R + j];
      if (j < 2 * B) g += v;
      else l += v;
    }
    out[4 + k] = -0.5 * block_sum_256(g, red);
    out[7 + k] = -w_local * block_sum_256(l, red);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 10; ++q) acc[q] += out[q];
    acc[10] += (double)B;
  }
}

}  // namespace

extern "C" size_t pcrl_val_metrics_ws_bytes(int64_t n, int B, int nlocal) {
  if (n <= 0 || B <= 0 || nlocal <= 0) return 0;
  const int64_t blocks = (n + VM_CHUNK - 1) / VM_CHUNK, R = (int64_t)B * (2 + 4 * nlocal);
  return (size_t)(blocks * 4 + 3 * R) * sizeof(double);
}

extern "C" int pcrl_val_metrics(const float* out1, const float* mask0, const float* mask1, const float* mask2, const float* gt,
                                const float* pro1_0, const float* pre1_0, const float* pro2_0, const float* pre2_0, const float* proL_0, const float* preL_0,
                                const float* pro1_1, const float* pre1_1, const float* pro2_1, const float* pre2_1, const float* proL_1, const float* preL_1,
                                const float* pro1_2, const float* pre1_2, const float* pro2_2, const float* pre2_2, const float* proL_2, const float* preL_2,
                                double* acc, void* ws, size_t ws_bytes, int B, int64_t S, int nlocal, int C0, int C1, int C2, float eps,
                                pcrl_stream_t stream) {
  PCRL_REQUIRE(B > 0 && S > 0 && nlocal > 0 && C0 > 0 && C1 > 0 && C2 > 0, "val_metrics: bad sizes B=%d S=%lld nlocal=%d C=%d,%d,%d", B, (long long)S, nlocal, C0, C1, C2);
  const ValFeats t{{{pro1_0, pre1_0, pro2_0, pre2_0, proL_0, preL_0}, {pro1_1, pre1_1, pro2_1, pre2_1, proL_1, preL_1}, {pro1_2, pre1_2, pro2_2, pre2_2, proL_2, preL_2}},
                   {C0, C1, C2}};
  for (int k = 0; k < 3; ++k)
    for (int q = 0; q < 6; ++q) PCRL_REQUIRE(t.f[k][q], "val_metrics: null feature pointer (scale %d, tensor %d)", k, q);
  PCRL_REQUIRE(out1 && mask0 && mask1 && mask2 && gt && acc, "val_metrics: null pointer");
  const int64_t n = (int64_t)B * S;
  if (!ws || ws_bytes < pcrl_val_metrics_ws_bytes(n, B, nlocal)) return pcrl_fail(PCRL_EWORKSPACE, "val_metrics: workspace too small");
  const int64_t blocks = (n + VM_CHUNK - 1) / VM_CHUNK;
  PCRL_REQUIRE(blocks < ((int64_t)1 << 31), "val_metrics: too many elements");
  const int R = B * (2 + 4 * nlocal);
  double* mse_ws = static_cast<double*>(ws);
  double* vals = mse_ws + blocks * 4;
  hipLaunchKernelGGL(val_mse_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), out1, mask0, mask1, mask2, gt, mse_ws, n);
  hipLaunchKernelGGL(val_cos_rows_kernel, dim3((unsigned)((R + 3) / 4), 3), dim3(256), 0, as_stream(stream), t, vals, B, R, eps);
  hipLaunchKernelGGL(val_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), mse_ws, (int)blocks, vals, B, R, 1.0 / (double)S, 1.0 / (4.0 * nlocal), acc);
  return pcrl_check_launch("val_metrics");
}
