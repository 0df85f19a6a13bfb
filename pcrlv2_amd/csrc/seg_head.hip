// The output head of 3D segmentation fine-tuning and its loss as ONE operator: out_tr.final_conv (1x1x1, 64 -> K) -> sigmoid -> wb * BCE + wd * (1 - mean_k Dice_k)
// against a uint8 bitmask (bit k: the voxel belongs to class k, classes may overlap; bit 7: the voxel is NOT counted -- no sum, zero gradient).  The
// voxel-wise sibling of cls_head.hip: no [M][K] tensor of logits or probabilities exists in training.
//
// mapping   LPV = 64 / (16 / sizeof(T)) lanes per voxel (16 for float32, 8 for bf16), each owning ONE 16-byte vector of the voxel's 64 channels, so a
//           wave reads 4 (8) whole 256-byte (128-byte) rows per load: fully coalesced.  A block (256 threads) belongs to one sample (blockIdx.y) and strides
//           over its voxels; the next vector is loaded before the current one is used.  The K dot products of a voxel are V fused multiply-adds per
//           lane followed by log2(LPV) xor-shuffle steps -- the same order for every voxel and in all three kernels (sh_logit), which is what lets the
//           backward RECOMPUTE z and p instead of reading them.  Lane k of a voxel then owns class k (K <= 7 < LPV): logit, sigmoid, loss term, sums.
// forward   one read of a; per-lane float64 sums of I = sum p g, P = sum p, G = sum g, BCE (from the logit, as cls_head.hip) and the counted voxels;
//           per-block float64 partials; a second one-block launch adds them in block order into sums[K][4] (+ count at sums[4 K]) and writes the loss.
// backward  reads a, labels, sums, dloss; the per-class coefficients come from sums on the device (no host read-back); dz_k is broadcast from lane k to
//           the voxel's lanes, dx[v][c] = sum_k W[k][c] dz_k is stored once with 16-byte stores, dW / db accumulate per lane in float32, are combined
//           per block and left as per-block partials that a second launch adds in block order.  No floating-point atomics anywhere.
// eval      the forward plus exact integer counts of TP, |pred|, |gt| per (case, class) with pred = (z >= 0) (= p >= 0.5 without a rounded sigmoid);
//           block sums enter counts[case][k][3] with 64-bit integer atomics (order-independent, as auroc.hip), and optionally the predicted bitmask.
// logits    the same read of a and the same sh_logit, nothing else: lane sub < K of a voxel stores z_k as float32 at z[voxel][sub].  The voxels of a
//           wave are consecutive, so a store instruction writes one contiguous run of (64 / LPV) * K floats.  No LDS, no sums, no workspace.  This is
//           what overlap-blended sliding windows (seg_blend.hip) average; a logit is bit-identical to the one the eval kernel thresholds.
// logits+   the accumulating sibling for mirror test-time augmentation and checkpoint ensembles (seg_head_logits_acc): the network saw the patch mirrored
//           along the axes of `flip`, so the logit of voxel s = (i, j, k) belongs to the un-mirrored voxel s' = (fx ? cx-1-i : i, fy ? cy-1-j : j,
//           fz ? cz-1-k : k).  The read of a, sh_fetch and sh_logit are the plain kernel's; the store is v = first ? z_k : z[s'][sub] + z_k, then
//           z[s'][sub] = v * scale (one add, one multiply, plain float32).  What a wave sees: its 64 / LPV voxels are consecutive along z, so without a
//           z mirror it stores the plain kernel's one contiguous run of (64 / LPV) * K floats, moved as a whole by an x / y mirror (rows of cz voxels
//           keep their inside and change places); with a z mirror the runs of K floats of the wave's consecutive voxels are the SAME addresses in
//           reverse voxel order (a wave whose voxels cross the end of a z row has two such runs, one per row) -- the same cache lines, each
//           written once in full.  The added read of z (not on a first pass) has exactly the store's addresses, one pass earlier:
//           it is issued one iteration ahead next to the prefetch of a, and reads (64 / LPV) * K floats per wave where the row of a is 64 / LPV
//           vectors of 256 (128) bytes, i.e. K / 16 (K / 8) of the bytes the kernel reads anyway.  s -> s' is a bijection of the sample's voxels and
//           lane sub of voxel s alone touches z[s'][sub]: no atomics, no LDS, no workspace, two runs give identical bytes.
// The weight lives in registers: lane `sub` holds W[k][sub * V .. sub * V + V) for every k (K * V floats), read once per block from global memory.
// LDS is used only for the block-level combination at the end of a block: red[wave][slot] (float64), redc[wave][k * 3 + q] (integers) and
// redw[wave][k * 64 + c] (float32).  Writers are the first LPV lanes of each wave: one scalar store per (k, j), lane `sub` at word k * 64 + sub * V + j,
// so the LPV <= 16 lanes of a store are V words apart -- at most 16 distinct banks of the 64, each hit once: conflict-free; readers are consecutive
// threads at consecutive words of one wave's row, four rows in turn (conflict-free).  There is no LDS traffic inside the voxel loop.
#include "internal.h"

namespace {

constexpr int SH_THREADS = 256, SH_C = PCRL_SEG_C, SH_MAX_K = 7, SH_SLOTS = 32, SH_CNT = 28, SH_SLICES = 8;
constexpr float SH_EPS = 1.0f;
static_assert(SH_SLOTS == PCRL_SEG_SLOTS && SH_CNT == PCRL_SEG_CNT_SLOT, "seg_blend.hip writes its partials in this layout");

__host__ __device__ inline int sh_wstride(int K) { return pcrl_seg_wstride(K); }

template <typename T, int K>
__device__ __forceinline__ void sh_load_w(const float* __restrict__ W, int sub, float (&w)[K][Vec16<T>::N]) {
  constexpr int V = Vec16<T>::N;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) w[k][j] = W[k * SH_C + sub * V + j];
}

// The voxel's row `x` (this lane's vector of it) -> the logit of class `sub` (lanes sub >= K: bk alone).  Every lane of the voxel computes every class's
// dot product -- the xor butterfly leaves the same sum in all of them -- and keeps its own.
template <typename T, int K>
__device__ __forceinline__ float sh_logit(const Vec16<T>& x, const float (&w)[K][Vec16<T>::N], float bk, int sub) {
  constexpr int V = Vec16<T>::N, LPV = 64 / V;
  float z = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float d = 0.0f;
#pragma unroll
    for (int j = 0; j < V; ++j) d = fmaf(w[k][j], to_f(x.v[j]), d);
#pragma unroll
    for (int o = LPV / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    if (sub == k) z = d;
  }
  return z + bk;
}

// grid = (gx, N); block = 256.  partial[block][SH_SLOTS] float64: slot k * 4 + {0: I, 1: P, 2: G, 3: BCE}, slot SH_CNT: counted voxels.
template <typename T, int K, bool EVAL>
__global__ void __launch_bounds__(SH_THREADS) seg_head_fwd_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                                 const uint8_t* __restrict__ labels, double* __restrict__ partial,
                                                                 const int* __restrict__ case_index, unsigned long long* __restrict__ counts, int n_cases,
                                                                 uint8_t* __restrict__ mask, int S) {
  constexpr int V = Vec16<T>::N, LPV = 64 / V, GPB = SH_THREADS / LPV;
  __shared__ double red[SH_THREADS / 64][SH_SLOTS];
  __shared__ unsigned redc[SH_THREADS / 64][SH_MAX_K * 3 + 3];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, sub = t % LPV, grp = t / LPV;
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * S;
  float w[K][V];
  sh_load_w<T, K>(W, sub, w);
  const float bk = sub < K ? bias[sub] : 0.0f;
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  double sI = 0.0, sP = 0.0, sG = 0.0, sB = 0.0;
  unsigned cnt = 0, cTP = 0, cPr = 0, cGt = 0;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  sh_fetch(a, labels, base, it < iters ? it * GPB + grp : S, S, sub, x, lab);
  for (; it < iters; it += step) {
    Vec16<T> xn;
    unsigned labn;
    sh_fetch(a, labels, base, it + step < iters ? (it + step) * GPB + grp : S, S, sub, xn, labn);
    const float z = sh_logit<T, K>(x, w, bk, sub);
    const bool counted = sub < K && !(lab & 0x80u);
    const bool g = (lab >> sub) & 1u;
    if (counted) {
      const float p = seg_sigmoid(z), y = g ? 1.0f : 0.0f;
      sI += (double)(g ? p : 0.0f);
      sP += (double)p;
      sG += (double)y;
      sB += (double)(fmaxf(z, 0.0f) - y * z + log1pf(expf(-fabsf(z))));
    }
    cnt += (sub == 0 && !(lab & 0x80u)) ? 1u : 0u;
    if (EVAL) {
      const bool pred = counted && z >= 0.0f;
      cTP += (pred && g) ? 1u : 0u;
      cPr += pred ? 1u : 0u;
      cGt += (counted && g) ? 1u : 0u;
      if (mask) {
        unsigned m = pred ? (1u << sub) : 0u;
#pragma unroll
        for (int o = LPV / 2; o > 0; o >>= 1) m |= (unsigned)__shfl_xor((int)m, o, 64);
        const int s = it * GPB + grp;
        if (sub == 0 && s < S) mask[base + s] = (uint8_t)m;
      }
    }
    x = xn;
    lab = labn;
  }
  sI = sh_group_sum<LPV>(sI);
  sP = sh_group_sum<LPV>(sP);
  sG = sh_group_sum<LPV>(sG);
  sB = sh_group_sum<LPV>(sB);
  cnt = sh_group_sum<LPV>(cnt);
  if (lane < K) {
    red[wid][lane * 4 + 0] = sI;
    red[wid][lane * 4 + 1] = sP;
    red[wid][lane * 4 + 2] = sG;
    red[wid][lane * 4 + 3] = sB;
  }
  if (lane == 0) red[wid][SH_CNT] = (double)cnt;
  if (EVAL) {
    cTP = sh_group_sum<LPV>(cTP);
    cPr = sh_group_sum<LPV>(cPr);
    cGt = sh_group_sum<LPV>(cGt);
    if (lane < K) {
      redc[wid][lane * 3 + 0] = cTP;
      redc[wid][lane * 3 + 1] = cPr;
      redc[wid][lane * 3 + 2] = cGt;
    }
  }
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (t < 4 * K || t == SH_CNT) partial[blk * SH_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (EVAL && t < 3 * K) {
    const int ci = case_index ? case_index[n] : n;
    if (ci >= 0 && ci < n_cases)
      atomicAdd(&counts[(int64_t)ci * K * 3 + t], (unsigned long long)redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t]);
  }
}

// grid = 1; block = 256: the per-block partials in block order (SH_SLICES contiguous ranges, then the ranges in order) -> sums [4 K + 1], loss
__global__ void __launch_bounds__(SH_THREADS) seg_head_sums_kernel(const double* __restrict__ partial, int nb, int K, float wb, float wd,
                                                                  double* __restrict__ sums, float* __restrict__ loss) {
  __shared__ double red[SH_SLICES][SH_SLOTS];
  const int t = threadIdx.x, slot = t % SH_SLOTS, slice = t / SH_SLOTS;
  const bool valid = slot < 4 * K || slot == SH_CNT;
  const int per = (nb + SH_SLICES - 1) / SH_SLICES, b0 = slice * per, b1 = b0 + per < nb ? b0 + per : nb;
  double s = 0.0;
  if (valid)      // eight loads in flight, added in block order (one load per addition left the launch at the latency of nb / 8 dependent loads)
    for (int b = b0; b < b1; b += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? partial[(int64_t)(b + u) * SH_SLOTS + slot] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b + u < b1) s += v[u];
    }
  red[slice][slot] = s;
  __syncthreads();
  if (t < SH_SLOTS && valid) {
    double tot = red[0][t];
#pragma unroll
    for (int i = 1; i < SH_SLICES; ++i) tot += red[i][t];
    sums[t == SH_CNT ? 4 * K : t] = tot;
    red[0][t] = tot;
  }
  __syncthreads();
  if (t == 0) {
    const double Mc = red[0][SH_CNT];
    double bce = 0.0, dice = 0.0;
    for (int k = 0; k < K; ++k) {
      bce += red[0][k * 4 + 3];
      dice += (2.0 * red[0][k * 4] + (double)SH_EPS) / (red[0][k * 4 + 1] + red[0][k * 4 + 2] + (double)SH_EPS);
    }
    bce = Mc > 0.0 ? bce / (Mc * (double)K) : 0.0;
    loss[0] = (float)((double)wb * bce + (double)wd * (1.0 - dice / (double)K));
  }
}

// grid = (gx, N); block = 256.  partial[block][K * 65] float32: dW [K][64] then db [K] of the block's voxels.
template <typename T, int K>
__global__ void __launch_bounds__(SH_THREADS) seg_head_bwd_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                                 const uint8_t* __restrict__ labels, const double* __restrict__ sums,
                                                                 const float* __restrict__ dloss, float wb, float wd, T* __restrict__ dx,
                                                                 float* __restrict__ partial, int S) {
  constexpr int V = Vec16<T>::N, LPV = 64 / V, GPB = SH_THREADS / LPV;
  __shared__ __attribute__((aligned(16))) float redw[SH_THREADS / 64][SH_MAX_K * (SH_C + 1)];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, sub = t % LPV, grp = t / LPV;
  const int64_t base = (int64_t)blockIdx.y * S;
  float w[K][V], aw[K][V];
  sh_load_w<T, K>(W, sub, w);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) aw[k][j] = 0.0f;
  const float bk = sub < K ? bias[sub] : 0.0f;
  // dz = cA (p - g) - p (1 - p) (g e1 - e0) for this lane's class, with c = dloss and every constant factor folded into the three coefficients:
  //   cA = c wb / (Mc K);  e1 = (c wd / K) 2 / U_k;  e0 = (c wd / K) (2 I_k + eps) / U_k^2;  U_k = P_k + G_k + eps
  // i.e. g e1 - e0 = (c wd / K) (2 g U_k - (2 I_k + eps)) / U_k^2, the Dice term of the header's formula
  float cA = 0.0f, e1 = 0.0f, e0 = 0.0f;
  if (sub < K) {
    const double c = (double)dloss[0], Mc = sums[4 * K], cd = c * (double)wd / (double)K;
    const double U = sums[sub * 4 + 1] + sums[sub * 4 + 2] + (double)SH_EPS, num = 2.0 * sums[sub * 4] + (double)SH_EPS;
    cA = Mc > 0.0 ? (float)(c * (double)wb / (Mc * (double)K)) : 0.0f;
    e1 = (float)(cd * 2.0 / U);
    e0 = (float)(cd * num / (U * U));
  }
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  float sdb = 0.0f;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  sh_fetch(a, labels, base, it < iters ? it * GPB + grp : S, S, sub, x, lab);
  for (; it < iters; it += step) {
    Vec16<T> xn;
    unsigned labn;
    sh_fetch(a, labels, base, it + step < iters ? (it + step) * GPB + grp : S, S, sub, xn, labn);
    const float z = sh_logit<T, K>(x, w, bk, sub);
    float dz = 0.0f;
    if (sub < K && !(lab & 0x80u)) {
      const float p = seg_sigmoid(z), y = ((lab >> sub) & 1u) ? 1.0f : 0.0f;
      dz = cA * (p - y) - p * (1.0f - p) * (y * e1 - e0);
    }
    sdb += dz;
    float d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = __shfl(dz, (lane & ~(LPV - 1)) + k, 64);
    const int s = it * GPB + grp;
    if (dx && s < S) {
      Vec16<T> o;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) acc = fmaf(w[k][j], d[k], acc);
        o.v[j] = from_f<T>(acc);
      }
      st16(dx + (base + s) * SH_C + sub * V, o);
    }
    // an uncounted voxel enters no sum: its row is not multiplied by its zero dz (0 * NaN would poison dW)
    if (!(lab & 0x80u)) {
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) aw[k][j] = fmaf(d[k], to_f(x.v[j]), aw[k][j]);
    }
    x = xn;
    lab = labn;
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float v = sh_group_sum<LPV>(aw[k][j]);
      if (lane < LPV) redw[wid][k * SH_C + sub * V + j] = v;
    }
  sdb = sh_group_sum<LPV>(sdb);
  if (lane < K) redw[wid][K * SH_C + lane] = sdb;
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int i = t; i < sh_wstride(K); i += SH_THREADS) partial[blk * sh_wstride(K) + i] = ((redw[0][i] + redw[1][i]) + redw[2][i]) + redw[3][i];
}

// grid = ceil(K * 65 / 64); block = 256 = 64 outputs x 4 contiguous block ranges, the ranges then added in order
__global__ void __launch_bounds__(SH_THREADS) seg_head_wsum_kernel(const float* __restrict__ partial, int nb, int K, float* __restrict__ dW,
                                                                  float* __restrict__ db) {
  __shared__ float red[SH_THREADS / 64][64];
  const int t = threadIdx.x, col = t & 63, slice = t >> 6, o = blockIdx.x * 64 + col, n_out = sh_wstride(K);
  const int per = (nb + 3) / 4, b0 = slice * per, b1 = b0 + per < nb ? b0 + per : nb;
  float s = 0.0f;
  if (o < n_out)      // eight loads in flight, added in block order
    for (int b = b0; b < b1; b += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? partial[(int64_t)(b + u) * n_out + o] : 0.0f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b + u < b1) s += v[u];
    }
  red[slice][col] = s;
  __syncthreads();
  if (slice == 0 && o < n_out) {
    const float tot = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
    if (o < K * SH_C) dW[o] = tot;
    else db[o - K * SH_C] = tot;
  }
}

// grid = (gx, N); block = 256.  z float32 [N * S][K]: the logits, and nothing else.
template <typename T, int K>
__global__ void __launch_bounds__(SH_THREADS) seg_head_logits_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                                    float* __restrict__ z, int S) {
  constexpr int V = Vec16<T>::N, LPV = 64 / V, GPB = SH_THREADS / LPV;
  const int t = threadIdx.x, sub = t % LPV, grp = t / LPV;
  const int64_t base = (int64_t)blockIdx.y * S;
  float w[K][V];
  sh_load_w<T, K>(W, sub, w);
  const float bk = sub < K ? bias[sub] : 0.0f;
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  sh_fetch<T>(a, nullptr, base, it < iters ? it * GPB + grp : S, S, sub, x, lab);
  for (; it < iters; it += step) {
    Vec16<T> xn;
    sh_fetch<T>(a, nullptr, base, it + step < iters ? (it + step) * GPB + grp : S, S, sub, xn, lab);
    const float zk = sh_logit<T, K>(x, w, bk, sub);
    const int s = it * GPB + grp;
    if (sub < K && s < S) z[(base + s) * K + sub] = zk;
    x = xn;
  }
}

// grid = (gx, N); block = 256.  The logits kernel with an un-mirroring, accumulating store: lane sub < K of voxel s = (i, j, k) owns z[n][s'][sub] at the
// un-mirrored voxel s', reads it (unless FIRST), adds its logit and stores the sum times `scale`.  s -> s' is a bijection of the sample's voxels, so
// every element of z is read and written by this one lane of the call.  (i, j, k) is divided out once and then advanced by the block stride with carries.
template <typename T, int K, bool FIRST>
__global__ void __launch_bounds__(SH_THREADS) seg_head_logits_acc_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                                        float* z, int S, ShMirror m, float scale) {
  constexpr int V = Vec16<T>::N, LPV = 64 / V, GPB = SH_THREADS / LPV;
  const int t = threadIdx.x, sub = t % LPV, grp = t / LPV;
  const int64_t base = (int64_t)blockIdx.y * S;
  float w[K][V];
  sh_load_w<T, K>(W, sub, w);
  const float bk = sub < K ? bias[sub] : 0.0f;
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  const int adv = step * GPB, plane = m.cy * m.cz;      // voxels between two iterations of a thread (<= 1024 * 32)
  const int dk = adv % m.cz, dj = (adv / m.cz) % m.cy, di = adv / plane;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  int s = it < iters ? it * GPB + grp : S;
  int k = s % m.cz, j = (s / m.cz) % m.cy, i = s / plane;
  sh_fetch<T>(a, nullptr, base, s, S, sub, x, lab);
  float zo = 0.0f;
  if (!FIRST && sub < K && s < S) zo = z[sh_unmirrored(m, base, i, j, k, K, sub)];
  for (; it < iters; it += step) {
    const int sn = it + step < iters ? s + adv : S;
    int kn = k + dk, jn = j + dj, in = i + di;
    if (kn >= m.cz) {
      kn -= m.cz;
      ++jn;
    }
    if (jn >= m.cy) {
      jn -= m.cy;
      ++in;
    }
    Vec16<T> xn;
    sh_fetch<T>(a, nullptr, base, sn, S, sub, xn, lab);
    float zn = 0.0f;      // the next voxel's element is not the one stored below (the bijection), so it may be read ahead of that store
    if (!FIRST && sub < K && sn < S) zn = z[sh_unmirrored(m, base, in, jn, kn, K, sub)];
    const float zk = sh_logit<T, K>(x, w, bk, sub);
    if (sub < K && s < S) {
      const float v = FIRST ? zk : zo + zk;
      z[sh_unmirrored(m, base, i, j, k, K, sub)] = v * scale;
    }
    x = xn;
    zo = zn;
    s = sn;
    i = in;
    j = jn;
    k = kn;
  }
}

int seg_head_check(const char* what, int N, int64_t S, int K, int dtype) {
  PCRL_REQUIRE(N > 0 && S > 0 && S < ((int64_t)1 << 31) - 4096, "%s: bad sizes N=%d S=%lld", what, N, (long long)S);
  PCRL_REQUIRE(N <= 65535, "%s: at most 65535 samples per call, got %d", what, N);
  PCRL_REQUIRE(dtype == PCRL_F32 || dtype == PCRL_BF16, "%s: dtype must be float32 or bfloat16", what);
  PCRL_REQUIRE(K >= 1 && K <= SH_MAX_K, "%s: 1 <= K <= %d classes (bit 7 of a label byte means 'not counted'), got %d", what, SH_MAX_K, K);
  return PCRL_OK;
}

template <typename T, int K>
void seg_head_launch_fwd(bool eval, dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, const uint8_t* labels, double* partial,
                         const int* case_index, int64_t* counts, int n_cases, uint8_t* mask, int S) {
  if (eval)
    hipLaunchKernelGGL((seg_head_fwd_kernel<T, K, true>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, partial, case_index,
                       reinterpret_cast<unsigned long long*>(counts), n_cases, mask, S);
  else
    hipLaunchKernelGGL((seg_head_fwd_kernel<T, K, false>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, partial, nullptr, nullptr, 0,
                       nullptr, S);
}

template <typename T, int K>
void seg_head_launch_bwd(dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums,
                         const float* dloss, float wb, float wd, void* dx, float* partial, int S) {
  hipLaunchKernelGGL((seg_head_bwd_kernel<T, K>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, sums, dloss, wb, wd,
                     static_cast<T*>(dx), partial, S);
}

int seg_head_forward(const char* what, bool eval, const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts,
                     int n_cases, uint8_t* mask, double* sums, float* loss, float wb, float wd, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                     pcrl_stream_t stream) {
  if (int rc = seg_head_check(what, N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && sums && loss, "%s: null pointer", what);
  if (!ws || ws_bytes < pcrl_seg_head_ws_bytes(N, S, K)) return pcrl_fail(PCRL_EWORKSPACE, "%s: workspace too small", what);
  const int gx = sh_gx(N, S);
  const dim3 grid(gx, N);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
#define SH_FWD(KK)                                                                                                                   \
  if (dtype == PCRL_BF16) seg_head_launch_fwd<bf16, KK>(eval, grid, st, a, w, b, labels, partial, case_index, counts, n_cases, mask, (int)S); \
  else seg_head_launch_fwd<float, KK>(eval, grid, st, a, w, b, labels, partial, case_index, counts, n_cases, mask, (int)S)
  PCRL_SEG_DISPATCH_K(SH_FWD)
#undef SH_FWD
  pcrl_seg_sums_launch(partial, gx * N, K, wb, wd, sums, loss, st);
  return pcrl_check_launch(what);
}

template <typename T, int K>
void seg_head_launch_logits(dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, float* z, int S) {
  hipLaunchKernelGGL((seg_head_logits_kernel<T, K>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, z, S);
}

template <typename T, int K>
void seg_head_launch_logits_acc(bool first, dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, float* z, int S, const ShMirror& m,
                                float scale) {
  if (first)
    hipLaunchKernelGGL((seg_head_logits_acc_kernel<T, K, true>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, z, S, m, scale);
  else
    hipLaunchKernelGGL((seg_head_logits_acc_kernel<T, K, false>), grid, dim3(SH_THREADS), 0, st, static_cast<const T*>(a), w, b, z, S, m, scale);
}

}  // namespace

void pcrl_seg_sums_launch(const double* partial, int nb, int K, float wb, float wd, double* sums, float* loss, hipStream_t stream) {
  hipLaunchKernelGGL(seg_head_sums_kernel, dim3(1), dim3(SH_THREADS), 0, stream, partial, nb, K, wb, wd, sums, loss);
}

void pcrl_seg_wsum_launch(const float* partial, int nb, int K, float* dw, float* db, hipStream_t stream) {
  hipLaunchKernelGGL(seg_head_wsum_kernel, dim3((sh_wstride(K) + 63) / 64), dim3(SH_THREADS), 0, stream, partial, nb, K, dw, db);
}

extern "C" int pcrl_seg_head_logits(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, pcrl_stream_t stream) {
  if (int rc = seg_head_check("seg_head_logits", N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && z, "seg_head_logits: null pointer");
  const dim3 grid(sh_gx(N, S), N);
  hipStream_t st = as_stream(stream);
#define SH_LOGITS(KK)                                                                                  \
  if (dtype == PCRL_BF16) seg_head_launch_logits<bf16, KK>(grid, st, a, w, b, z, (int)S);             \
  else seg_head_launch_logits<float, KK>(grid, st, a, w, b, z, (int)S)
  PCRL_SEG_DISPATCH_K(SH_LOGITS)
#undef SH_LOGITS
  return pcrl_check_launch("seg_head_logits");
}

extern "C" int pcrl_seg_head_logits_acc(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, int cx, int cy, int cz,
                                        int flip, int first, float scale, pcrl_stream_t stream) {
  if (int rc = seg_head_check("seg_head_logits_acc", N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && z, "seg_head_logits_acc: null pointer");
  PCRL_REQUIRE(flip >= 0 && flip <= 7, "seg_head_logits_acc: flip %d is no mirror code (bit 0 = x, bit 1 = y, bit 2 = z: 0..7)", flip);
  PCRL_REQUIRE(cx > 0 && cy > 0 && cz > 0 && (int64_t)cx * cy * cz == S, "seg_head_logits_acc: S = %lld voxels per sample against a grid of %d x %d x %d",
               (long long)S, cx, cy, cz);
  const dim3 grid(sh_gx(N, S), N);
  const ShMirror m{cx, cy, cz, flip};
  hipStream_t st = as_stream(stream);
#define SH_LOGITS_ACC(KK)                                                                                                  \
  if (dtype == PCRL_BF16) seg_head_launch_logits_acc<bf16, KK>(first != 0, grid, st, a, w, b, z, (int)S, m, scale);       \
  else seg_head_launch_logits_acc<float, KK>(first != 0, grid, st, a, w, b, z, (int)S, m, scale)
  PCRL_SEG_DISPATCH_K(SH_LOGITS_ACC)
#undef SH_LOGITS_ACC
  return pcrl_check_launch("seg_head_logits_acc");
}

extern "C" size_t pcrl_seg_head_ws_bytes(int N, int64_t S, int K) {
  if (N <= 0 || S <= 0 || K < 1 || K > SH_MAX_K) return 0;
  const size_t nb = (size_t)sh_gx(N, S) * (size_t)N, f = nb * SH_SLOTS * sizeof(double), r = nb * (size_t)sh_wstride(K) * sizeof(float);
  return f > r ? f : r;
}

extern "C" int pcrl_seg_head_fwd(const void* a, const float* w, const float* b, const uint8_t* labels, double* sums, float* loss, float wb, float wd, void* ws,
                                 size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream) {
  PCRL_REQUIRE(labels, "seg_head_fwd: null pointer");
  return seg_head_forward("seg_head_fwd", false, a, w, b, labels, nullptr, nullptr, 0, nullptr, sums, loss, wb, wd, ws, ws_bytes, N, S, K, dtype, stream);
}

extern "C" int pcrl_seg_head_eval(const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts, int n_cases,
                                  uint8_t* mask, double* sums, float* loss, float wb, float wd, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                                  pcrl_stream_t stream) {
  PCRL_REQUIRE(counts && n_cases > 0, "seg_head_eval: counts [n_cases][K][3] is required");
  return seg_head_forward("seg_head_eval", true, a, w, b, labels, case_index, counts, n_cases, mask, sums, loss, wb, wd, ws, ws_bytes, N, S, K, dtype, stream);
}

extern "C" int pcrl_seg_head_bwd(const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums, const float* dloss, float wb,
                                 float wd, void* dx, float* dw, float* db, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream) {
  if (int rc = seg_head_check("seg_head_bwd", N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && labels && sums && dloss && dw && db, "seg_head_bwd: null pointer");
  if (!ws || ws_bytes < pcrl_seg_head_ws_bytes(N, S, K)) return pcrl_fail(PCRL_EWORKSPACE, "seg_head_bwd: workspace too small");
  const int gx = sh_gx(N, S);
  const dim3 grid(gx, N);
  float* partial = static_cast<float*>(ws);
  hipStream_t st = as_stream(stream);
#define SH_BWD(KK)                                                                                                        \
  if (dtype == PCRL_BF16) seg_head_launch_bwd<bf16, KK>(grid, st, a, w, b, labels, sums, dloss, wb, wd, dx, partial, (int)S); \
  else seg_head_launch_bwd<float, KK>(grid, st, a, w, b, labels, sums, dloss, wb, wd, dx, partial, (int)S)
  PCRL_SEG_DISPATCH_K(SH_BWD)
#undef SH_BWD
  pcrl_seg_wsum_launch(partial, gx * N, K, dw, db, st);
  return pcrl_check_launch("seg_head_bwd");
}
