// The classification head of supervised 2D fine-tuning and its loss as ONE operator: smp's ClassificationHead(pooling='avg', dropout=p,
// activation='sigmoid') -- AdaptiveAvgPool2d(1) -> Flatten -> Dropout(p) -> Linear(C, K) -> Sigmoid -- followed by nn.BCELoss (mean over N * K).
//
// forward   one block per sample reads the sample's [H*W][C] slab of layer4's activation ONCE with 16-byte loads along C, pools it in float32,
//           applies the keep mask and 1 / (1 - p), takes the K dot products against the float32 weight (one wave per class, a wave reduction
//           each), writes probabilities, the pooled vector and -- with labels -- its K loss terms as one float64 partial; a one-block second
//           launch sums the N partials in a fixed order.  The loss term comes from the LOGIT, max(z, 0) - y z + log1p(exp(-|z|)): no logarithm
//           of a rounded probability, no clamp.
// backward  the activation is NOT read: d_a[n][s][c] = keep[n][c] / (1 - p) / (H W) * sum_k W[k][c] (p[n][k] - y[n][k]) dloss / (N K) is the same
//           row for every pixel of a sample -- one block per sample computes it once and stores it H*W times with 16-byte stores.  dW and db
//           sum over the samples in a fixed order in a second launch.  No atomics, no full-size intermediate.
// The [K][C] weight is read from global memory: a block uses every element exactly once (forward: coalesced float4 per lane; backward: lane = channel,
// a coalesced row per class), so a copy in LDS would be written and read once -- there is no weight tile in LDS and hence no bank conflict on one.
// LDS holds the pooled partials (written j-major: thread t at [j][t], conflict-free) and the pooled vector (read as contiguous float4 per lane).
#include "common.h"

namespace {

constexpr int CH_THREADS = 256, CH_MAX_C = 512, CH_MAX_K = 64;

__device__ __forceinline__ float ch_keep(const uint8_t* keep, int64_t n, int C, int c, float scale) {
  return keep ? (keep[n * C + c] ? scale : 0.0f) : 1.0f;
}

// grid = N; block = 256.  NV = C / Vec16<T>::N vectors per pixel row, 256 % NV == 0: a thread owns vector (t % NV) of the rows t / NV, t / NV + 256 / NV, ...
template <typename T>
__global__ void __launch_bounds__(CH_THREADS) cls_head_fwd_kernel(const T* __restrict__ a, const uint8_t* __restrict__ keep, float scale,
                                                                 const float* __restrict__ W, const float* __restrict__ bias,
                                                                 const uint8_t* __restrict__ labels, float* __restrict__ probs,
                                                                 float* __restrict__ pooled, double* __restrict__ partial, int HW, int C, int K) {
  constexpr int V = Vec16<T>::N;
  __shared__ float part[V * CH_THREADS];                  // [j][thread]
  __shared__ __attribute__((aligned(16))) float g[CH_MAX_C];
  __shared__ double red[CH_THREADS / 64];
  const int t = threadIdx.x, NV = C / V, G = CH_THREADS / NV;
  const int64_t n = blockIdx.x;
  const int v = t % NV, r0 = t / NV;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.0f;
  const T* __restrict__ src = a + n * (int64_t)HW * C + (int64_t)v * V;
  for (int s = r0; s < HW; s += G) {
    const Vec16<T> x = ld16(src + (int64_t)s * C);
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] += to_f(x.v[j]);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) part[j * CH_THREADS + t] = acc[j];
  __syncthreads();
  // channel c = vv * V + j: consecutive threads take consecutive vectors vv (consecutive LDS words); the G row groups are added in a fixed order
  for (int idx = t; idx < C; idx += CH_THREADS) {
    const int vv = idx % NV, j = idx / NV, c = vv * V + j;
    float s = 0.0f;
    for (int r = 0; r < G; ++r) s += part[j * CH_THREADS + r * NV + vv];
    const float m = s / (float)HW;
    pooled[n * C + c] = m;
    g[c] = m * ch_keep(keep, n, C, c, scale);
  }
  __syncthreads();
  const int lane = t & 63, wid = t >> 6;
  double lsum = 0.0;
  for (int k = wid; k < K; k += CH_THREADS / 64) {
    float dot = 0.0f;
    for (int c4 = lane; c4 < C / 4; c4 += 64) {
      const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)k * C + 4 * c4);
      const float4 x = *reinterpret_cast<const float4*>(g + 4 * c4);
      dot += w.x * x.x + w.y * x.y + w.z * x.z + w.w * x.w;
    }
    dot = wave_sum(dot);
    if (lane == 0) {
      const float z = dot + bias[k];
      probs[n * K + k] = 1.0f / (1.0f + expf(-z));
      if (labels) {
        const float y = labels[n * K + k] ? 1.0f : 0.0f;
        lsum += (double)(fmaxf(z, 0.0f) - y * z + log1pf(expf(-fabsf(z))));
      }
    }
  }
  if (partial) {
    if (lane == 0) red[wid] = lsum;
    __syncthreads();
    if (t == 0) partial[n] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

__global__ void __launch_bounds__(CH_THREADS) cls_head_loss_kernel(const double* __restrict__ partial, int N, double inv_count, float* __restrict__ loss) {
  __shared__ double red[CH_THREADS / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += CH_THREADS) s += partial[i];
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) loss[0] = (float)(s * inv_count);
}

// grid = N; block = 256.  The row of d_a of sample n, once, then H*W stores of it.
template <typename T>
__global__ void __launch_bounds__(CH_THREADS) cls_head_bwd_act_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ labels,
                                                                     const float* __restrict__ dloss, const uint8_t* __restrict__ keep, float scale,
                                                                     const float* __restrict__ W, T* __restrict__ da, int HW, int C, int K, float inv_count) {
  constexpr int V = Vec16<T>::N;
  __shared__ float dz[CH_MAX_K];
  __shared__ __attribute__((aligned(16))) T row[CH_MAX_C];
  const int t = threadIdx.x, NV = C / V, G = CH_THREADS / NV;
  const int64_t n = blockIdx.x;
  if (t < K) dz[t] = (probs[n * K + t] - (labels[n * K + t] ? 1.0f : 0.0f)) * (dloss[0] * inv_count);
  __syncthreads();
  const float inv_hw = 1.0f / (float)HW;
  for (int c = t; c < C; c += CH_THREADS) {
    float s = 0.0f;
    for (int k = 0; k < K; ++k) s += W[(int64_t)k * C + c] * dz[k];      // dz[k]: one LDS word for the whole wave (broadcast)
    row[c] = from_f<T>(s * (ch_keep(keep, n, C, c, scale) * inv_hw));
  }
  __syncthreads();
  const int v = t % NV;
  const Vec16<T> x = ld16(row + v * V);
  T* __restrict__ dst = da + n * (int64_t)HW * C + (int64_t)v * V;
  for (int s = t / NV; s < HW; s += G) st16(dst + (int64_t)s * C, x);
}

// grid = (C / 256 rounded up, K); dW[k][c] = sum_n dz[n][k] * pooled[n][c] * keep[n][c] * scale, n ascending; block x = 0 also leaves db[k]
__global__ void __launch_bounds__(CH_THREADS) cls_head_bwd_param_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ labels,
                                                                       const float* __restrict__ dloss, const float* __restrict__ pooled,
                                                                       const uint8_t* __restrict__ keep, float scale, float* __restrict__ dW,
                                                                       float* __restrict__ db, int N, int C, int K, float inv_count) {
  const int k = blockIdx.y, c = blockIdx.x * CH_THREADS + threadIdx.x;
  const float coef = dloss[0] * inv_count;
  if (c < C) {
    float s = 0.0f;
    for (int64_t n = 0; n < N; ++n) {
      const float d = (probs[n * K + k] - (labels[n * K + k] ? 1.0f : 0.0f)) * coef;
      s += d * (pooled[n * C + c] * ch_keep(keep, n, C, c, scale));
    }
    dW[(int64_t)k * C + c] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    float s = 0.0f;
    for (int64_t n = threadIdx.x; n < N; n += 64) s += (probs[n * K + k] - (labels[n * K + k] ? 1.0f : 0.0f)) * coef;
    s = wave_sum(s);
    if (threadIdx.x == 0) db[k] = s;
  }
}

int cls_head_check(const char* what, int N, int H, int W, int C, int K, int dtype) {
  PCRL_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "%s: bad sizes N=%d H=%d W=%d", what, N, H, W);
  PCRL_REQUIRE(dtype == PCRL_F32 || dtype == PCRL_BF16, "%s: dtype must be float32 or bfloat16", what);
  PCRL_REQUIRE(C >= 32 && C <= CH_MAX_C && (C & (C - 1)) == 0, "%s: C must be a power of two in 32..%d (the encoder's last width is 512), got %d", what, CH_MAX_C, C);
  PCRL_REQUIRE(K > 0 && K <= CH_MAX_K, "%s: 1 <= K <= %d classes, got %d", what, CH_MAX_K, K);
  return PCRL_OK;
}

}  // namespace

extern "C" size_t pcrl_cls_head_ws_bytes(int N) { return N > 0 ? (size_t)N * sizeof(double) : 0; }

extern "C" int pcrl_cls_head_fwd(const void* a, const uint8_t* keep, float keep_scale, const float* w, const float* b, const uint8_t* labels, float* probs,
                                 float* pooled, float* loss, void* ws, size_t ws_bytes, int N, int H, int W, int C, int K, int dtype, pcrl_stream_t stream) {
  if (int rc = cls_head_check("cls_head_fwd", N, H, W, C, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && probs && pooled, "cls_head_fwd: null pointer");
  PCRL_REQUIRE((labels == nullptr) == (loss == nullptr), "cls_head_fwd: labels and loss come together");
  double* partial = nullptr;
  if (labels) {
    if (!ws || ws_bytes < pcrl_cls_head_ws_bytes(N)) return pcrl_fail(PCRL_EWORKSPACE, "cls_head_fwd: workspace too small");
    partial = static_cast<double*>(ws);
  }
  if (dtype == PCRL_BF16)
    hipLaunchKernelGGL(cls_head_fwd_kernel<bf16>, dim3(N), dim3(CH_THREADS), 0, as_stream(stream), static_cast<const bf16*>(a), keep, keep_scale, w, b, labels,
                       probs, pooled, partial, H * W, C, K);
  else
    hipLaunchKernelGGL(cls_head_fwd_kernel<float>, dim3(N), dim3(CH_THREADS), 0, as_stream(stream), static_cast<const float*>(a), keep, keep_scale, w, b, labels,
                       probs, pooled, partial, H * W, C, K);
  if (labels)
    hipLaunchKernelGGL(cls_head_loss_kernel, dim3(1), dim3(CH_THREADS), 0, as_stream(stream), partial, N, 1.0 / ((double)N * (double)K), loss);
  return pcrl_check_launch("cls_head_fwd");
}

extern "C" int pcrl_cls_head_bwd(const float* probs, const uint8_t* labels, const float* dloss, const float* pooled, const uint8_t* keep, float keep_scale,
                                 const float* w, void* da, float* dw, float* db, int N, int H, int W, int C, int K, int dtype, pcrl_stream_t stream) {
  if (int rc = cls_head_check("cls_head_bwd", N, H, W, C, K, dtype)) return rc;
  PCRL_REQUIRE(probs && labels && dloss && pooled && w && dw && db, "cls_head_bwd: null pointer");
  const float inv_count = (float)(1.0 / ((double)N * (double)K));
  if (da) {
    if (dtype == PCRL_BF16)
      hipLaunchKernelGGL(cls_head_bwd_act_kernel<bf16>, dim3(N), dim3(CH_THREADS), 0, as_stream(stream), probs, labels, dloss, keep, keep_scale, w,
                         static_cast<bf16*>(da), H * W, C, K, inv_count);
    else
      hipLaunchKernelGGL(cls_head_bwd_act_kernel<float>, dim3(N), dim3(CH_THREADS), 0, as_stream(stream), probs, labels, dloss, keep, keep_scale, w,
                         static_cast<float*>(da), H * W, C, K, inv_count);
  }
  hipLaunchKernelGGL(cls_head_bwd_param_kernel, dim3((C + CH_THREADS - 1) / CH_THREADS, K), dim3(CH_THREADS), 0, as_stream(stream), probs, labels, dloss, pooled,
                     keep, keep_scale, dw, db, N, C, K, inv_count);
  return pcrl_check_launch("cls_head_bwd");
}
