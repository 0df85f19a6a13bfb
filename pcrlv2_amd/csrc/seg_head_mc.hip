// The SOFTMAX output head of 3D segmentation fine-tuning and its loss as ONE operator: out_tr.final_conv (1x1x1, 64 -> K) -> softmax over the K
// mutually exclusive classes -> wc * CE + wd * (1 - mean_{k >= 1} Dice_k) against a uint8 LABEL MAP (bits 0..6: the class index y, 0 = background;
// bit 7: the voxel is NOT counted -- no sum, zero gradient).  2 <= K <= 16, the background counted in K.  The sibling of seg_head.hip (per-class
// sigmoids against a bitmask, K <= 7); no [M][K] tensor of logits or probabilities exists in training.  A label y >= K is not checked here (the host
// checks a case when it is opened): such a voxel is treated as NOT counted by every kernel below, so it is harmless.
//
// per voxel, in this order in ALL kernels (the backward recomputes, a logit is bit-identical wherever it appears):
//     z_k = tree_k + b_k;   m = max_k z_k;   e_k = exp(z_k - m);   s = sum_k e_k;   p_k = e_k / s;   ce = (m - z_y) + log s
// mapping   seg_head.hip's rows: LPV = 64 / V lanes per voxel (V = 16 / sizeof(T): 16 lanes of 4 floats, 8 lanes of 8 bf16), lane `sub` owning ONE
//           16-byte vector of the voxel's 64 channels, a block (256 threads) striding over one sample's voxels with the next vector loaded before
//           the current one is used (sh_fetch, shared through internal.h).  What differs is what follows the load, because K = 16 does not fit
//           "every lane keeps every class's full dot product and W in registers" (128 VGPRs of W in bf16, K log2(LPV) shuffles):
//   weight  W [K][64] float32 sits in LDS (<= 4 KB, staged once per block).  Lane `sub` reads W[k][sub * V .. + V) as 16-byte ds_read_b128s.
//           Banks: the lanes of one b128 group carry every `sub` (f32: once each, bf16: twice each = the same address, a broadcast), and the
//           distinct addresses are the 16-byte slots sub * V * 4 + {0, 16} bytes of ONE 256-byte row of W: every bank at most once -- conflict-free.
//   dots    lane `sub` forms its PARTIAL dot product of every class: d_k = fma(W[k][sub V + j], x[j], d_k), j ascending from d_k = 0.
//   tree    a reduce-scatter butterfly over the voxel's lanes, offsets o = LPV/2, LPV/4, .., 1.  With KP = K rounded up to a power of two (the padded
//           classes hold 0) and `cnt` values per lane (KP at the start): while cnt > 1 a lane keeps the half of its values named by bit o of `sub`
//           (clear: the lower classes), sends the other half to lane sub ^ o and adds what it receives: d_i = keep_i + recv_i, cnt /= 2; once
//           cnt = 1 the remaining steps are the plain xor butterfly d_0 += shfl_xor(d_0, o).  Both lanes of a pair add the same two numbers, so
//           the tree of a class is fixed: ((lanes differing in bit LPV/2), then bit LPV/4, ...), the same for every voxel and kernel.  It costs
//           KP/2 + KP/4 + ... shuffles (15 at K = 16 in float32, 14 in bf16) instead of K log2(LPV).  Afterwards lane `sub` owns
//           CPL = max(1, KP / LPV) classes, kb + i with kb = (sub / DUP) * CPL, where DUP = max(1, LPV / KP) lanes hold the same class when KP < LPV
//           (the one with sub % DUP == 0 is its `owner` and alone contributes to sums and stores).
//   softmax m by log2(LPV) xor steps of fmaxf (order-free); e_k = expf(z_k - m) on the owned classes only (CPL exps per lane, not K);
//           s = the owner lanes' (e_kb + e_kb+1 ..) summed by log2(LPV) xor steps (offsets LPV/2 .. 1) -- a fixed tree, identical in every lane.
// forward   one read of a; per-lane float64 sums of I_k = sum_{y=k} p_k, P_k = sum p_k, G_k = #{y = k}, CE_k = sum_{y=k} ce for the owned classes
//           and the counted voxels; per-block float64 partials [72]; a second one-block launch adds them in block order (8 contiguous ranges, then
//           the ranges in order -- seg_head.hip's scheme with more slots; shared with seg_blend.hip's label-map blend) into sums [4 K + 1] and the loss
//               wc (sum_k CE_k) / Mc + wd (1 - (1 / (K - 1)) sum_{k=1}^{K-1} (2 I_k + 1) / (P_k + G_k + 1))          (CE term 0 when Mc = 0)
// backward  reads a, labels, sums, dloss; with U_k = P_k + G_k + 1, q_0 = 0 and q_k = -(c wd / (K-1)) (2 [y=k] / U_k - (2 I_k + 1) / U_k^2):
//               dz_j = (c wc / Mc) (p_j - [y=j]) + p_j (q_j - sum_k p_k q_k)
//           sum_k p_k q_k by one more xor butterfly; every lane of the voxel then collects the K values dz_k (K shuffles from the owners),
//           dx[v][c] = sum_k W[k][c] dz_k (k ascending, fused) is stored once with 16-byte stores, dW / db accumulate per lane in float32, are
//           combined per block and left as per-block partials [K * 65] that seg_head.hip's second launch (pcrl_seg_wsum_launch) adds in block
//           order.  An uncounted voxel's row is not multiplied by its zero dz.  No floating-point atomics anywhere.
// eval      the forward plus pred = the LOWEST k with z_k == m (a min butterfly over the owners' candidates) and exact integer counts of TP,
//           |pred|, |gt| for ALL K classes; block sums enter counts[case][k][3] with 64-bit integer atomics; optionally the predicted label map
//           (0 where the voxel is not counted).
// logits    ONE kernel with pcrl_seg_head_logits_acc's un-mirroring, accumulating store (flip = 0, first = 1, scale = 1 is the plain case: v * 1.0f
//           is v): the owner of class k of voxel s alone reads and writes z[s'][k] (v = first ? z_k : z[s'][k] + z_k; z[s'][k] = v * scale), s -> s'
//           a bijection of the sample's voxels: no atomics, no LDS beyond W, no workspace.
// LDS beyond W is used only at the end of a block: red[wave][slot] (float64), redc[wave][k * 3 + q] (integers), redw[wave][k * 64 + c] (float32),
// written by the first LPV lanes of each wave V words apart (<= 16 distinct banks, each once) and read by consecutive threads at consecutive words.
// Also here: two byte-wise kernels that let the bitmask tools (surface distances, connected components) work on label maps seven classes at a time.
#include "internal.h"

namespace {

constexpr int MC_THREADS = 256, MC_C = PCRL_SEG_C, MC_MIN_K = 2, MC_MAX_K = 16, MC_SLOTS = PCRL_SEG_MC_SLOTS, MC_SLICES = 8, MC_SUM_THREADS = 1024;
constexpr float MC_EPS = 1.0f;
static_assert(4 * MC_MAX_K + 1 <= MC_SLOTS && MC_SLICES * 128 == MC_SUM_THREADS && MC_SLOTS <= 128, "the second launch's layout");

constexpr int mc_pow2(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

template <typename T, int K> struct McGeom {
  static constexpr int V = Vec16<T>::N, LPV = 64 / V, KP = mc_pow2(K);
  static constexpr int CPL = KP >= LPV ? KP / LPV : 1;      // classes a lane owns after the tree
  static constexpr int DUP = KP >= LPV ? 1 : LPV / KP;      // lanes of a voxel that hold the same class
};

__device__ __forceinline__ void mc_stage_w(const float* __restrict__ W, int K, float* Wl) {
  for (int i = threadIdx.x; i < K * MC_C; i += MC_THREADS) Wl[i] = W[i];
  __syncthreads();
}

// one step of the reduce-scatter butterfly at offset O with CNT values per lane; then the next offset
template <int CNT, int O> __device__ __forceinline__ void mc_tree(float (&d)[CNT > 1 ? CNT : 1], int sub) {
  if constexpr (O > 0) {
    if constexpr (CNT > 1) {
      constexpr int H = CNT / 2;
      const bool hi = (sub & O) != 0;
      float n[H];
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const float keep = hi ? d[i + H] : d[i], send = hi ? d[i] : d[i + H];
        n[i] = keep + __shfl_xor(send, O, 64);
      }
      mc_tree<H, O / 2>(n, sub);
#pragma unroll
      for (int i = 0; i < H; ++i) d[i] = n[i];      // the first max(1, H >> steps left) entries are the result
    } else {
      d[0] += __shfl_xor(d[0], O, 64);
      mc_tree<1, O / 2>(d, sub);
    }
  }
}

// The voxel's row `x` (this lane's vector of it) -> the logits of the CPL classes this lane owns, z[i] of class kb + i (classes >= K: the bias slot is 0).
template <typename T, int K>
__device__ __forceinline__ void mc_logit(const Vec16<T>& x, const float* Wl, const float (&bk)[McGeom<T, K>::CPL], int sub, float (&z)[McGeom<T, K>::CPL]) {
  using G = McGeom<T, K>;
  constexpr int V = G::V;
  float d[G::KP];
#pragma unroll
  for (int k = 0; k < G::KP; ++k) d[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int h = 0; h < V / 4; ++h) {
      const float4 w4 = *reinterpret_cast<const float4*>(Wl + k * MC_C + sub * V + 4 * h);
      d[k] = fmaf(w4.x, to_f(x.v[4 * h + 0]), d[k]);
      d[k] = fmaf(w4.y, to_f(x.v[4 * h + 1]), d[k]);
      d[k] = fmaf(w4.z, to_f(x.v[4 * h + 2]), d[k]);
      d[k] = fmaf(w4.w, to_f(x.v[4 * h + 3]), d[k]);
    }
  mc_tree<G::KP, G::LPV / 2>(d, sub);
#pragma unroll
  for (int i = 0; i < G::CPL; ++i) z[i] = d[i] + bk[i];
}

template <int LPV> __device__ __forceinline__ float mc_vox_max(float v) {
#pragma unroll
  for (int o = LPV / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int LPV> __device__ __forceinline__ float mc_vox_sum(float v) {
#pragma unroll
  for (int o = LPV / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int LPV> __device__ __forceinline__ int mc_vox_min(int v) {
#pragma unroll
  for (int o = LPV / 2; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

// m, e_i = exp(z_i - m) of the owned classes (0 for a padded class) and s, identical in every lane of the voxel
template <typename T, int K>
__device__ __forceinline__ void mc_softmax(const float (&z)[McGeom<T, K>::CPL], int kb, bool owner, float (&e)[McGeom<T, K>::CPL], float& m, float& s) {
  using G = McGeom<T, K>;
  float mm = -INFINITY;
#pragma unroll
  for (int i = 0; i < G::CPL; ++i)
    if (kb + i < K) mm = fmaxf(mm, z[i]);
  m = mc_vox_max<G::LPV>(mm);
  float ss = 0.0f;
#pragma unroll
  for (int i = 0; i < G::CPL; ++i) {
    e[i] = kb + i < K ? expf(z[i] - m) : 0.0f;
    if (owner) ss += e[i];
  }
  s = mc_vox_sum<G::LPV>(ss);
}

template <typename T, int K> __device__ __forceinline__ void mc_bias(const float* __restrict__ bias, int kb, float (&bk)[McGeom<T, K>::CPL]) {
#pragma unroll
  for (int i = 0; i < McGeom<T, K>::CPL; ++i) bk[i] = kb + i < K ? bias[kb + i] : 0.0f;
}

// counted: bit 7 clear and the class index inside 0..K-1
__device__ __forceinline__ bool mc_counted(unsigned lab, int K) { return !(lab & 0x80u) && (int)(lab & 0x7Fu) < K; }

// grid = (gx, N); block = 256.  partial[block][MC_SLOTS] float64: slot k * 4 + {0: I, 1: P, 2: G, 3: CE}, slot 4 K: counted voxels.
template <typename T, int K, bool EVAL>
__global__ void __launch_bounds__(MC_THREADS) seg_mc_fwd_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                               const uint8_t* __restrict__ labels, double* __restrict__ partial,
                                                               const int* __restrict__ case_index, unsigned long long* __restrict__ counts, int n_cases,
                                                               uint8_t* __restrict__ labelmap, int S) {
  using G = McGeom<T, K>;
  constexpr int LPV = G::LPV, GPB = MC_THREADS / LPV, CPL = G::CPL;
  __shared__ __attribute__((aligned(16))) float Wl[K * MC_C];
  __shared__ double red[MC_THREADS / 64][MC_SLOTS];
  __shared__ unsigned redc[MC_THREADS / 64][MC_MAX_K * 3];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, sub = t % LPV, grp = t / LPV;
  const int kb = (sub / G::DUP) * CPL;
  const bool owner = sub % G::DUP == 0;
  const int n = blockIdx.y;
  const int64_t base = (int64_t)n * S;
  mc_stage_w(W, K, Wl);
  float bk[CPL];
  mc_bias<T, K>(bias, kb, bk);
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  double sI[CPL], sP[CPL], sG[CPL], sC[CPL];
  unsigned cTP[CPL], cPr[CPL], cGt[CPL], cnt = 0;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    sI[i] = sP[i] = sG[i] = sC[i] = 0.0;
    cTP[i] = cPr[i] = cGt[i] = 0;
  }
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  sh_fetch(a, labels, base, it < iters ? it * GPB + grp : S, S, sub, x, lab);
  for (; it < iters; it += step) {
    Vec16<T> xn;
    unsigned labn;
    sh_fetch(a, labels, base, it + step < iters ? (it + step) * GPB + grp : S, S, sub, xn, labn);
    float z[CPL], e[CPL], m, s;
    mc_logit<T, K>(x, Wl, bk, sub, z);
    mc_softmax<T, K>(z, kb, owner, e, m, s);
    const bool counted = mc_counted(lab, K);
    const int y = (int)(lab & 0x7Fu);
    if (counted && owner) {
      const float ls = logf(s);
#pragma unroll
      for (int i = 0; i < CPL; ++i)
        if (kb + i < K) {
          const float p = e[i] / s;
          const bool g = y == kb + i;
          sP[i] += (double)p;
          if (g) {
            sI[i] += (double)p;
            sG[i] += 1.0;
            sC[i] += (double)((m - z[i]) + ls);
          }
        }
    }
    cnt += (sub == 0 && counted) ? 1u : 0u;
    if (EVAL) {
      int cand = MC_MAX_K;
#pragma unroll
      for (int i = CPL - 1; i >= 0; --i)
        if (kb + i < K && z[i] == m) cand = kb + i;
      const int pred = mc_vox_min<LPV>(cand);
      if (counted && owner) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const bool pr = pred == kb + i, g = y == kb + i;      // a padded class is neither
          cTP[i] += (pr && g) ? 1u : 0u;
          cPr[i] += pr ? 1u : 0u;
          cGt[i] += g ? 1u : 0u;
        }
      }
      const int sv = it * GPB + grp;
      if (labelmap && sub == 0 && sv < S) labelmap[base + sv] = (uint8_t)(counted ? pred : 0);
    }
    x = xn;
    lab = labn;
  }
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    sI[i] = sh_group_sum<LPV>(sI[i]);
    sP[i] = sh_group_sum<LPV>(sP[i]);
    sG[i] = sh_group_sum<LPV>(sG[i]);
    sC[i] = sh_group_sum<LPV>(sC[i]);
    if (lane < LPV && owner && kb + i < K) {
      red[wid][(kb + i) * 4 + 0] = sI[i];
      red[wid][(kb + i) * 4 + 1] = sP[i];
      red[wid][(kb + i) * 4 + 2] = sG[i];
      red[wid][(kb + i) * 4 + 3] = sC[i];
    }
  }
  cnt = sh_group_sum<LPV>(cnt);
  if (lane == 0) red[wid][4 * K] = (double)cnt;
  if (EVAL) {
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      cTP[i] = sh_group_sum<LPV>(cTP[i]);
      cPr[i] = sh_group_sum<LPV>(cPr[i]);
      cGt[i] = sh_group_sum<LPV>(cGt[i]);
      if (lane < LPV && owner && kb + i < K) {
        redc[wid][(kb + i) * 3 + 0] = cTP[i];
        redc[wid][(kb + i) * 3 + 1] = cPr[i];
        redc[wid][(kb + i) * 3 + 2] = cGt[i];
      }
    }
  }
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (t <= 4 * K) partial[blk * MC_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (EVAL && t < 3 * K) {
    const int ci = case_index ? case_index[n] : n;
    if (ci >= 0 && ci < n_cases)
      atomicAdd(&counts[(int64_t)ci * K * 3 + t], (unsigned long long)redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t]);
  }
}

// grid = 1; block = 1024 = 128 slots x 8 contiguous block ranges: the per-block partials in block order (the ranges, then the ranges in order) -> sums
// [4 K + 1] and the softmax head's loss.
__global__ void __launch_bounds__(1024) seg_mc_sums_kernel(const double* __restrict__ partial, int nb, int K, float wc, float wd,
                                                            double* __restrict__ sums, float* __restrict__ loss) {
  __shared__ double red[MC_SLICES][MC_SLOTS];
  const int t = threadIdx.x, slot = t & 127, slice = t >> 7;
  const bool valid = slot <= 4 * K;
  const int per = (nb + MC_SLICES - 1) / MC_SLICES, b0 = slice * per, b1 = b0 + per < nb ? b0 + per : nb;
  double s = 0.0;
  if (valid)      // eight loads in flight, added in block order
    for (int b = b0; b < b1; b += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? partial[(int64_t)(b + u) * MC_SLOTS + slot] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (b + u < b1) s += v[u];
    }
  if (valid) red[slice][slot] = s;
  __syncthreads();
  if (t <= 4 * K) {
    double tot = red[0][t];
#pragma unroll
    for (int i = 1; i < MC_SLICES; ++i) tot += red[i][t];
    sums[t] = tot;
    red[0][t] = tot;
  }
  __syncthreads();
  if (t == 0) {
    const double Mc = red[0][4 * K];
    double ce = 0.0, dice = 0.0;
    for (int k = 0; k < K; ++k) ce += red[0][k * 4 + 3];
    for (int k = 1; k < K; ++k) dice += (2.0 * red[0][k * 4] + (double)MC_EPS) / (red[0][k * 4 + 1] + red[0][k * 4 + 2] + (double)MC_EPS);
    ce = Mc > 0.0 ? ce / Mc : 0.0;
    // nothing counted: the Dice ratios are all 1 and the loss is exactly 0
    loss[0] = (float)((double)wc * ce + (double)wd * (1.0 - dice / (double)(K - 1)));
  }
}

// grid = (gx, N); block = 256.  partial[block][K * 65] float32: dW [K][64] then db [K] of the block's voxels.
template <typename T, int K>
__global__ void __launch_bounds__(MC_THREADS) seg_mc_bwd_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                               const uint8_t* __restrict__ labels, const double* __restrict__ sums,
                                                               const float* __restrict__ dloss, float wc, float wd, T* __restrict__ dx,
                                                               float* __restrict__ partial, int S) {
  using G = McGeom<T, K>;
  constexpr int V = G::V, LPV = G::LPV, GPB = MC_THREADS / LPV, CPL = G::CPL, WS = K * (MC_C + 1);
  __shared__ __attribute__((aligned(16))) float Wl[K * MC_C];
  __shared__ __attribute__((aligned(16))) float redw[MC_THREADS / 64][WS];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, sub = t % LPV, grp = t / LPV;
  const int kb = (sub / G::DUP) * CPL;
  const bool owner = sub % G::DUP == 0;
  const int64_t base = (int64_t)blockIdx.y * S;
  mc_stage_w(W, K, Wl);
  float bk[CPL];
  mc_bias<T, K>(bias, kb, bk);
  float aw[K][V];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < V; ++j) aw[k][j] = 0.0f;
  // dz_j = cA (p_j - [y=j]) + p_j (q_j - sum_k p_k q_k) with c = dloss, cA = c wc / Mc and q_k = e0_k - [y=k] e1_k:
  //   e1_k = (c wd / (K-1)) 2 / U_k;  e0_k = (c wd / (K-1)) (2 I_k + eps) / U_k^2;  U_k = P_k + G_k + eps;  e1_0 = e0_0 = 0 (no background Dice)
  float cA, e1[CPL], e0[CPL], sdb[CPL];
  {
    const double c = (double)dloss[0], Mc = sums[4 * K], cd = c * (double)wd / (double)(K - 1);
    cA = Mc > 0.0 ? (float)(c * (double)wc / Mc) : 0.0f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int k = kb + i;
      e1[i] = e0[i] = sdb[i] = 0.0f;
      if (k >= 1 && k < K) {
        const double U = sums[k * 4 + 1] + sums[k * 4 + 2] + (double)MC_EPS, num = 2.0 * sums[k * 4] + (double)MC_EPS;
        e1[i] = (float)(cd * 2.0 / U);
        e0[i] = (float)(cd * num / (U * U));
      }
    }
  }
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  sh_fetch(a, labels, base, it < iters ? it * GPB + grp : S, S, sub, x, lab);
  for (; it < iters; it += step) {
    Vec16<T> xn;
    unsigned labn;
    sh_fetch(a, labels, base, it + step < iters ? (it + step) * GPB + grp : S, S, sub, xn, labn);
    float z[CPL], e[CPL], m, s;
    mc_logit<T, K>(x, Wl, bk, sub, z);
    mc_softmax<T, K>(z, kb, owner, e, m, s);
    const bool counted = mc_counted(lab, K);
    const int y = (int)(lab & 0x7Fu);
    float p[CPL], q[CPL], pq = 0.0f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      p[i] = e[i] / s;
      q[i] = y == kb + i ? e0[i] - e1[i] : e0[i];
      if (owner && kb + i < K) pq += p[i] * q[i];
    }
    pq = mc_vox_sum<LPV>(pq);
    float dz[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      dz[i] = 0.0f;
      if (counted && owner && kb + i < K) dz[i] = cA * (p[i] - (y == kb + i ? 1.0f : 0.0f)) + p[i] * (q[i] - pq);
      sdb[i] += dz[i];
    }
    float d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = __shfl(dz[k % CPL], (lane & ~(LPV - 1)) + (k / CPL) * G::DUP, 64);
    const int sv = it * GPB + grp;
    if (dx && sv < S) {
      Vec16<T> o;
#pragma unroll
      for (int h = 0; h < V / 4; ++h) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float4 w4 = *reinterpret_cast<const float4*>(Wl + k * MC_C + sub * V + 4 * h);
          acc[0] = fmaf(w4.x, d[k], acc[0]);
          acc[1] = fmaf(w4.y, d[k], acc[1]);
          acc[2] = fmaf(w4.z, d[k], acc[2]);
          acc[3] = fmaf(w4.w, d[k], acc[3]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[4 * h + j] = from_f<T>(acc[j]);
      }
      st16(dx + (base + sv) * MC_C + sub * V, o);
    }
    // an uncounted voxel enters no sum: its row is not multiplied by its zero dz (0 * NaN would poison dW)
    if (counted) {
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
      if (lane < LPV) redw[wid][k * MC_C + sub * V + j] = v;
    }
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const float v = sh_group_sum<LPV>(sdb[i]);
    if (lane < LPV && owner && kb + i < K) redw[wid][K * MC_C + kb + i] = v;
  }
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int i = t; i < WS; i += MC_THREADS) partial[blk * WS + i] = ((redw[0][i] + redw[1][i]) + redw[2][i]) + redw[3][i];
}

// grid = (gx, N); block = 256.  z float32 [N * S][K]: the owner of class k of voxel s = (i, j, k3) reads (unless FIRST) and writes z[s'][k] at the
// un-mirrored voxel s'; (i, j, k3) is divided out once and then advanced by the block stride with carries (seg_head.hip's accumulating kernel).
template <typename T, int K, bool FIRST>
__global__ void __launch_bounds__(MC_THREADS) seg_mc_logits_kernel(const T* __restrict__ a, const float* __restrict__ W, const float* __restrict__ bias,
                                                                  float* z, int S, ShMirror mr, float scale) {
  using G = McGeom<T, K>;
  constexpr int LPV = G::LPV, GPB = MC_THREADS / LPV, CPL = G::CPL;
  __shared__ __attribute__((aligned(16))) float Wl[K * MC_C];
  const int t = threadIdx.x, sub = t % LPV, grp = t / LPV;
  const int kb = (sub / G::DUP) * CPL;
  const bool owner = sub % G::DUP == 0;
  const int64_t base = (int64_t)blockIdx.y * S;
  mc_stage_w(W, K, Wl);
  float bk[CPL];
  mc_bias<T, K>(bias, kb, bk);
  const int iters = (S + GPB - 1) / GPB, step = gridDim.x;
  const int adv = step * GPB, plane = mr.cy * mr.cz;      // voxels between two iterations of a thread (<= 1024 * 32)
  const int dk = adv % mr.cz, dj = (adv / mr.cz) % mr.cy, di = adv / plane;
  Vec16<T> x;
  unsigned lab;
  int it = blockIdx.x;
  int s = it < iters ? it * GPB + grp : S;
  int k3 = s % mr.cz, j = (s / mr.cz) % mr.cy, i = s / plane;
  sh_fetch<T>(a, nullptr, base, s, S, sub, x, lab);
  float zo[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) zo[c] = (!FIRST && owner && kb + c < K && s < S) ? z[sh_unmirrored(mr, base, i, j, k3, K, kb + c)] : 0.0f;
  for (; it < iters; it += step) {
    const int sn = it + step < iters ? s + adv : S;
    int kn = k3 + dk, jn = j + dj, in = i + di;
    if (kn >= mr.cz) {
      kn -= mr.cz;
      ++jn;
    }
    if (jn >= mr.cy) {
      jn -= mr.cy;
      ++in;
    }
    Vec16<T> xn;
    sh_fetch<T>(a, nullptr, base, sn, S, sub, xn, lab);
    float zn[CPL];      // the next voxel's elements are not the ones stored below (the bijection), so they may be read ahead of that store
#pragma unroll
    for (int c = 0; c < CPL; ++c) zn[c] = (!FIRST && owner && kb + c < K && sn < S) ? z[sh_unmirrored(mr, base, in, jn, kn, K, kb + c)] : 0.0f;
    float zk[CPL];
    mc_logit<T, K>(x, Wl, bk, sub, zk);
    if (owner && s < S) {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (kb + c < K) {
          const float v = FIRST ? zk[c] : zo[c] + zk[c];
          z[sh_unmirrored(mr, base, i, j, k3, K, kb + c)] = v * scale;
        }
    }
    x = xn;
#pragma unroll
    for (int c = 0; c < CPL; ++c) zo[c] = zn[c];
    s = sn;
    i = in;
    j = jn;
    k3 = kn;
  }
}

// out[v] bit j (j < n) = ((lab[v] & 0x7F) == first + j); bit 7 carried over.  One byte per thread, grid-stride.
__global__ void __launch_bounds__(256) seg_labelmap_to_bits_kernel(const uint8_t* __restrict__ lab, int first, int n, uint8_t* __restrict__ out, int64_t count) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < count; v += (int64_t)gridDim.x * 256) {
    const unsigned b = lab[v];
    const int c = (int)(b & 0x7Fu) - first;
    out[v] = (uint8_t)((b & 0x80u) | ((c >= 0 && c < n) ? (1u << c) : 0u));
  }
}

// out[v] = lab[v], except that a voxel whose class is in first .. first + n - 1 and whose bit in `bits` is clear becomes background (bit 7 carried over)
__global__ void __launch_bounds__(256) seg_labelmap_keep_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ bits, int first, int n,
                                                               uint8_t* __restrict__ out, int64_t count) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < count; v += (int64_t)gridDim.x * 256) {
    const unsigned b = lab[v];
    const int c = (int)(b & 0x7Fu) - first;
    const bool drop = c >= 0 && c < n && !((bits[v] >> c) & 1u);
    out[v] = (uint8_t)(drop ? (b & 0x80u) : b);
  }
}

int seg_mc_check(const char* what, int N, int64_t S, int K, int dtype) {
  PCRL_REQUIRE(N > 0 && S > 0 && S < ((int64_t)1 << 31) - 4096, "%s: bad sizes N=%d S=%lld", what, N, (long long)S);
  PCRL_REQUIRE(N <= 65535, "%s: at most 65535 samples per call, got %d", what, N);
  PCRL_REQUIRE(dtype == PCRL_F32 || dtype == PCRL_BF16, "%s: dtype must be float32 or bfloat16", what);
  PCRL_REQUIRE(K >= MC_MIN_K && K <= MC_MAX_K, "%s: %d <= K <= %d mutually exclusive classes, the background included (a label byte holds the class index in bits 0..6), got %d",
               what, MC_MIN_K, MC_MAX_K, K);
  return PCRL_OK;
}

template <typename T, int K>
void seg_mc_launch_fwd(bool eval, dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, const uint8_t* labels, double* partial,
                       const int* case_index, int64_t* counts, int n_cases, uint8_t* labelmap, int S) {
  if (eval)
    hipLaunchKernelGGL((seg_mc_fwd_kernel<T, K, true>), grid, dim3(MC_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, partial, case_index,
                       reinterpret_cast<unsigned long long*>(counts), n_cases, labelmap, S);
  else
    hipLaunchKernelGGL((seg_mc_fwd_kernel<T, K, false>), grid, dim3(MC_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, partial, nullptr, nullptr, 0,
                       nullptr, S);
}

template <typename T, int K>
void seg_mc_launch_bwd(dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums,
                       const float* dloss, float wc, float wd, void* dx, float* partial, int S) {
  hipLaunchKernelGGL((seg_mc_bwd_kernel<T, K>), grid, dim3(MC_THREADS), 0, st, static_cast<const T*>(a), w, b, labels, sums, dloss, wc, wd,
                     static_cast<T*>(dx), partial, S);
}

template <typename T, int K>
void seg_mc_launch_logits(bool first, dim3 grid, hipStream_t st, const void* a, const float* w, const float* b, float* z, int S, const ShMirror& m,
                          float scale) {
  if (first)
    hipLaunchKernelGGL((seg_mc_logits_kernel<T, K, true>), grid, dim3(MC_THREADS), 0, st, static_cast<const T*>(a), w, b, z, S, m, scale);
  else
    hipLaunchKernelGGL((seg_mc_logits_kernel<T, K, false>), grid, dim3(MC_THREADS), 0, st, static_cast<const T*>(a), w, b, z, S, m, scale);
}

int seg_mc_forward(const char* what, bool eval, const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts,
                   int n_cases, uint8_t* labelmap, double* sums, float* loss, float wc, float wd, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                   pcrl_stream_t stream) {
  if (int rc = seg_mc_check(what, N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && sums && loss, "%s: null pointer", what);
  if (!ws || ws_bytes < pcrl_seg_mc_head_ws_bytes(N, S, K)) return pcrl_fail(PCRL_EWORKSPACE, "%s: workspace too small", what);
  const int gx = sh_gx(N, S);
  const dim3 grid(gx, N);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
#define MC_FWD(KK)                                                                                                                        \
  if (dtype == PCRL_BF16) seg_mc_launch_fwd<bf16, KK>(eval, grid, st, a, w, b, labels, partial, case_index, counts, n_cases, labelmap, (int)S); \
  else seg_mc_launch_fwd<float, KK>(eval, grid, st, a, w, b, labels, partial, case_index, counts, n_cases, labelmap, (int)S)
  PCRL_SEG_MC_DISPATCH_K(MC_FWD)
#undef MC_FWD
  pcrl_seg_mc_sums_launch(partial, gx * N, K, wc, wd, sums, loss, st);
  return pcrl_check_launch(what);
}

int seg_labelmap_check(const char* what, const void* lab, const void* out, int first, int n, int64_t count) {
  PCRL_REQUIRE(lab && out, "%s: null pointer", what);
  PCRL_REQUIRE(count > 0, "%s: %lld voxels", what, (long long)count);
  PCRL_REQUIRE(n >= 1 && n <= 7 && first >= 0 && first + n <= 128, "%s: a group is 1..7 classes inside 0..127, got first=%d n=%d", what, first, n);
  return PCRL_OK;
}

}  // namespace

void pcrl_seg_mc_sums_launch(const double* partial, int nb, int K, float wc, float wd, double* sums, float* loss, hipStream_t stream) {
  hipLaunchKernelGGL(seg_mc_sums_kernel, dim3(1), dim3(MC_SUM_THREADS), 0, stream, partial, nb, K, wc, wd, sums, loss);
}

extern "C" size_t pcrl_seg_mc_head_ws_bytes(int N, int64_t S, int K) {
  if (N <= 0 || S <= 0 || K < MC_MIN_K || K > MC_MAX_K) return 0;
  const size_t nb = (size_t)sh_gx(N, S) * (size_t)N, f = nb * MC_SLOTS * sizeof(double), r = nb * (size_t)pcrl_seg_wstride(K) * sizeof(float);
  return f > r ? f : r;
}

extern "C" int pcrl_seg_mc_head_fwd(const void* a, const float* w, const float* b, const uint8_t* labels, double* sums, float* loss, float wc, float wd,
                                    void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype, pcrl_stream_t stream) {
  PCRL_REQUIRE(labels, "seg_mc_head_fwd: null pointer");
  return seg_mc_forward("seg_mc_head_fwd", false, a, w, b, labels, nullptr, nullptr, 0, nullptr, sums, loss, wc, wd, ws, ws_bytes, N, S, K, dtype, stream);
}

extern "C" int pcrl_seg_mc_head_eval(const void* a, const float* w, const float* b, const uint8_t* labels, const int* case_index, int64_t* counts,
                                     int n_cases, uint8_t* labelmap, double* sums, float* loss, float wc, float wd, void* ws, size_t ws_bytes, int N, int64_t S,
                                     int K, int dtype, pcrl_stream_t stream) {
  PCRL_REQUIRE(counts && n_cases > 0, "seg_mc_head_eval: counts [n_cases][K][3] is required");
  return seg_mc_forward("seg_mc_head_eval", true, a, w, b, labels, case_index, counts, n_cases, labelmap, sums, loss, wc, wd, ws, ws_bytes, N, S, K, dtype,
                        stream);
}

extern "C" int pcrl_seg_mc_head_bwd(const void* a, const float* w, const float* b, const uint8_t* labels, const double* sums, const float* dloss, float wc,
                                    float wd, void* dx, float* dw, float* db, void* ws, size_t ws_bytes, int N, int64_t S, int K, int dtype,
                                    pcrl_stream_t stream) {
  if (int rc = seg_mc_check("seg_mc_head_bwd", N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && labels && sums && dloss && dw && db, "seg_mc_head_bwd: null pointer");
  if (!ws || ws_bytes < pcrl_seg_mc_head_ws_bytes(N, S, K)) return pcrl_fail(PCRL_EWORKSPACE, "seg_mc_head_bwd: workspace too small");
  const int gx = sh_gx(N, S);
  const dim3 grid(gx, N);
  float* partial = static_cast<float*>(ws);
  hipStream_t st = as_stream(stream);
#define MC_BWD(KK)                                                                                                          \
  if (dtype == PCRL_BF16) seg_mc_launch_bwd<bf16, KK>(grid, st, a, w, b, labels, sums, dloss, wc, wd, dx, partial, (int)S); \
  else seg_mc_launch_bwd<float, KK>(grid, st, a, w, b, labels, sums, dloss, wc, wd, dx, partial, (int)S)
  PCRL_SEG_MC_DISPATCH_K(MC_BWD)
#undef MC_BWD
  pcrl_seg_wsum_launch(partial, gx * N, K, dw, db, st);
  return pcrl_check_launch("seg_mc_head_bwd");
}

extern "C" int pcrl_seg_mc_head_logits(const void* a, const float* w, const float* b, float* z, int N, int64_t S, int K, int dtype, int cx, int cy, int cz,
                                       int flip, int first, float scale, pcrl_stream_t stream) {
  if (int rc = seg_mc_check("seg_mc_head_logits", N, S, K, dtype)) return rc;
  PCRL_REQUIRE(a && w && b && z, "seg_mc_head_logits: null pointer");
  PCRL_REQUIRE(flip >= 0 && flip <= 7, "seg_mc_head_logits: flip %d is no mirror code (bit 0 = x, bit 1 = y, bit 2 = z: 0..7)", flip);
  PCRL_REQUIRE(cx > 0 && cy > 0 && cz > 0 && (int64_t)cx * cy * cz == S, "seg_mc_head_logits: S = %lld voxels per sample against a grid of %d x %d x %d",
               (long long)S, cx, cy, cz);
  const dim3 grid(sh_gx(N, S), N);
  const ShMirror m{cx, cy, cz, flip};
  hipStream_t st = as_stream(stream);
#define MC_LOGITS(KK)                                                                                            \
  if (dtype == PCRL_BF16) seg_mc_launch_logits<bf16, KK>(first != 0, grid, st, a, w, b, z, (int)S, m, scale);   \
  else seg_mc_launch_logits<float, KK>(first != 0, grid, st, a, w, b, z, (int)S, m, scale)
  PCRL_SEG_MC_DISPATCH_K(MC_LOGITS)
#undef MC_LOGITS
  return pcrl_check_launch("seg_mc_head_logits");
}

extern "C" int pcrl_seg_labelmap_to_bits(const uint8_t* lab, int first, int n, uint8_t* out, int64_t count, pcrl_stream_t stream) {
  if (int rc = seg_labelmap_check("seg_labelmap_to_bits", lab, out, first, n, count)) return rc;
  hipLaunchKernelGGL(seg_labelmap_to_bits_kernel, dim3(capped_blocks(count, 256, 4096)), dim3(256), 0, as_stream(stream), lab, first, n, out, count);
  return pcrl_check_launch("seg_labelmap_to_bits");
}

extern "C" int pcrl_seg_labelmap_keep(const uint8_t* lab, const uint8_t* bits, int first, int n, uint8_t* out, int64_t count, pcrl_stream_t stream) {
  if (int rc = seg_labelmap_check("seg_labelmap_keep", lab, out, first, n, count)) return rc;
  PCRL_REQUIRE(bits, "seg_labelmap_keep: null pointer");
  hipLaunchKernelGGL(seg_labelmap_keep_kernel, dim3(capped_blocks(count, 256, 4096)), dim3(256), 0, as_stream(stream), lab, bits, first, n, out, count);
  return pcrl_check_launch("seg_labelmap_keep");
}
