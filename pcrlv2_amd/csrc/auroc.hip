// Per-class AUROC of a multi-label classifier by EXACT pair counting (what sklearn.metrics.roc_auc_score computes per column: the
// Mann-Whitney statistic with ties counted one half), for the chest X-ray validation / test pass of fine-tuning.
//
// counts[k][0] = 2 * #{(i, j): y_i = 1, y_j = 0, s_i > s_j} + #{(i, j): y_i = 1, y_j = 0, s_i == s_j},  counts[k][1] = P,  counts[k][2] = Q;
// AUROC_k = counts[k][0] / (2 P Q), taken on the host in float64.  Float comparisons (-0.0 == +0.0; a NaN score compares false both ways);
// integer counting, so the result does not depend on the order of the additions -- block sums go to the output with 64-bit integer atomics.
// No sort, no cap on M: block (x, k) owns 1024 rows i of class k (four per thread) and walks ALL rows j in tiles of 1024 staged in LDS, where a row
// that is not a negative is stored as NaN (it then counts for nothing).  Every lane reads the same float4 of the tile (a broadcast: no bank conflict)
// and compares it with its four scores: 16 comparisons per LDS read.
#include "common.h"

namespace {

constexpr int AU_THREADS = 256, AU_IPT = 4, AU_TILE = 1024;

__device__ __forceinline__ unsigned au_cmp(float si, float sj) { return (si > sj ? 2u : 0u) + (si == sj ? 1u : 0u); }

__global__ void __launch_bounds__(AU_THREADS) auroc_counts_kernel(const float* __restrict__ probs, const uint8_t* __restrict__ labels, int64_t M, int K,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) float tile[AU_TILE];
  __shared__ unsigned long long red[3][AU_THREADS / 64];
  const int k = blockIdx.y, t = threadIdx.x;
  const float nan = __builtin_nanf("");
  float si[AU_IPT];
  unsigned long long pos = 0, neg = 0, cnt = 0;
#pragma unroll
  for (int q = 0; q < AU_IPT; ++q) {
    const int64_t i = (int64_t)blockIdx.x * (AU_THREADS * AU_IPT) + q * AU_THREADS + t;
    si[q] = nan;
    if (i < M) {
      const bool y = labels[i * K + k] != 0;
      if (y) si[q] = probs[i * K + k];
      pos += y ? 1 : 0;
      neg += y ? 0 : 1;
    }
  }
  for (int64_t j0 = 0; j0 < M; j0 += AU_TILE) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AU_TILE / AU_THREADS; ++q) {
      const int64_t j = j0 + q * AU_THREADS + t;
      tile[q * AU_THREADS + t] = (j < M && labels[j * K + k] == 0) ? probs[j * K + k] : nan;
    }
    __syncthreads();
    unsigned c = 0;      // at most 2 * 4 * 1024 per tile
#pragma unroll 4
    for (int jj = 0; jj < AU_TILE; jj += 4) {
      const float4 s = *reinterpret_cast<const float4*>(tile + jj);
#pragma unroll
      for (int q = 0; q < AU_IPT; ++q) c += au_cmp(si[q], s.x) + au_cmp(si[q], s.y) + au_cmp(si[q], s.z) + au_cmp(si[q], s.w);
    }
    cnt += c;
  }
  // integer block sums: wave shuffles, four LDS words per quantity, one atomic per quantity and block
  unsigned long long v[3] = {cnt, pos, neg};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[a] += __shfl_xor(v[a], o, 64);
  }
  __syncthreads();
  if ((t & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) red[a][t >> 6] = v[a];
  }
  __syncthreads();
  if (t < 3) atomicAdd(&counts[(int64_t)k * 3 + t], red[t][0] + red[t][1] + red[t][2] + red[t][3]);
}

}  // namespace

extern "C" int pcrl_auroc_counts(const float* probs, const uint8_t* labels, int64_t* counts, int64_t M, int K, pcrl_stream_t stream) {
  PCRL_REQUIRE(M > 0 && K > 0 && K <= 65535, "auroc_counts: bad sizes M=%lld K=%d", (long long)M, K);
  PCRL_REQUIRE(probs && labels && counts, "auroc_counts: null pointer");
  const int64_t blocks = (M + AU_THREADS * AU_IPT - 1) / (AU_THREADS * AU_IPT);
  PCRL_REQUIRE(blocks < ((int64_t)1 << 31), "auroc_counts: too many rows");
  if (hipMemsetAsync(counts, 0, (size_t)K * 3 * sizeof(int64_t), as_stream(stream)) != hipSuccess) return pcrl_fail(PCRL_EINVAL, "auroc_counts: memset failed");
  hipLaunchKernelGGL(auroc_counts_kernel, dim3((unsigned)blocks, (unsigned)K), dim3(AU_THREADS), 0, as_stream(stream), probs, labels, M, K,
                     reinterpret_cast<unsigned long long*>(counts));
  return pcrl_check_launch("auroc_counts");
}
