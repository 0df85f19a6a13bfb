// Overlap-blended sliding-window inference of the 3D segmenter: the patches of one case are cut on the device (seg_cut_patches), the network turns
// each into logits (seg_head.hip's logits kernel), and seg_blend folds the per-patch logits into the case's prediction.  Compiled with
// -ffp-contract=off: the blend is pinned bit for bit against a float32 restatement that multiplies and adds one operation at a time.
//
// blend     one thread per VOLUME voxel, all K classes; consecutive threads move along Z, so the rows of K floats a wave reads from one patch are
//           consecutive (a contiguous run of 64 K floats where the wave stays inside one patch row), and the mask store is one byte per thread, 64
//           consecutive bytes per wave.  Per axis the covering patches s <= v < s + crop are a contiguous range of the ascending start list, found once
//           per voxel by two binary searches; the voxel then visits ix, iy, iz in ascending order:
//               w = (wx[i] * wy[j]) * wz[k];   num_k = num_k + w * z_k;   den = den + w            plain float32, this order, no fused multiply-add
//           pred_k = (num_k >= 0): den > 0, so no division decides a prediction.  zbar = num / den feeds the probabilities and, with `sums`, the head's
//           per-voxel terms (I, P, G, BCE: seg_head.hip's expressions) in per-thread float64 sums and the integer counts {TP, |pred|, |gt|}.
//           Every read of z is guarded by its own coverage test, so a start list that breaks the contract (not ascending) cannot index outside z.
// label map the softmax head's sibling (seg_mc_blend, 2 <= K <= 16 mutually exclusive classes): the SAME walk (sb_walk) and checks (sb_check), then the
//           lowest k with the largest num_k, softmax(num / den) and the head's {I, P, G, CE}; described at its kernel below.
// sums      wave shuffle sums, then LDS red[wave][slot] (float64) and redc[wave][k * 3 + q] (integers), as seg_head.hip: per-block float64 partials
//           that seg_head.hip's one-block launch adds in block order (pcrl_seg_sums_launch), and ONE 64-bit integer atomic per (block, k, q) into the
//           case's row of counts.  No floating-point atomics: two runs give identical bytes.
// LDS       only this combination at the end of a block.  After the shuffle sums every lane holds the wave's totals; lane 0 of each wave alone writes
//           them, one scalar store per slot -- a store instruction with ONE active lane has no second address to conflict with.  The readers are
//           threads t < 29 (t < 3 K) at consecutive float64 (uint32) words of one wave's row, the four rows in turn: consecutive banks, each hit
//           once per instruction -- conflict-free.  There is no LDS traffic inside the voxel loop.
// cut       a pure copy: thread = 4 consecutive z of one (patch, channel, x, y) row; four scalar loads (the source run starts at any z), one 16-byte
//           store; what lies outside the volume is 0, and float16 sources are widened exactly.
// mirror    the cutter's MIRROR instantiation for mirror test-time augmentation (seg_cut_patches_mirror; flip bit 0 = x, bit 1 = y, bit 2 = z): the same thread ->
//           output mapping and the same 16-byte store; the patch BOX is mirrored, its zeros outside the volume included.  An x / y mirror moves
//           whole source rows; with a z mirror a thread's four scalar loads run backwards, and the 64 threads of a wave still read one contiguous
//           span of source rows (the same cache lines, in reverse).
#include "internal.h"

namespace {

constexpr int SB_THREADS = 256, SB_MAX_K = 7, SB_MC_MAX_K = 16, SB_MAX_BLOCKS = 1024;

struct SbGeom {
  int X, Y, Z, cx, cy, cz, nx, ny, nz;
};

// first index i of the ascending list s[0..n) with s[i] > t (n: none)
__device__ __forceinline__ int sb_first_above(const int* __restrict__ s, int n, int t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The patch walk both blend kernels share: num_k and den of volume voxel (xc, yc, zc) over its covering patches in ascending ix, iy, iz.
template <int K>
__device__ __forceinline__ void sb_walk(const float* __restrict__ z, const int* __restrict__ sx, const int* __restrict__ sy, const int* __restrict__ sz,
                                        const float* __restrict__ wx, const float* __restrict__ wy, const float* __restrict__ wz, const SbGeom& g, int xc,
                                        int yc, int zc, float (&num)[K], float& den) {
  const int x0 = sb_first_above(sx, g.nx, xc - g.cx), x1 = sb_first_above(sx, g.nx, xc);
  const int y0 = sb_first_above(sy, g.ny, yc - g.cy), y1 = sb_first_above(sy, g.ny, yc);
  const int z0 = sb_first_above(sz, g.nz, zc - g.cz), z1 = sb_first_above(sz, g.nz, zc);
  den = 0.0f;
#pragma unroll
  for (int c = 0; c < K; ++c) num[c] = 0.0f;
  for (int ix = x0; ix < x1; ++ix) {
    const int i = xc - sx[ix];
    if ((unsigned)i >= (unsigned)g.cx) continue;
    const float wi = wx[i];
    for (int iy = y0; iy < y1; ++iy) {
      const int j = yc - sy[iy];
      if ((unsigned)j >= (unsigned)g.cy) continue;
      const float wij = wi * wy[j];
      const int64_t prow = ((((int64_t)ix * g.ny + iy) * g.nz) * g.cx + i) * g.cy + j;       // (patch (ix, iy, 0), i, j) in rows of cz voxels
      for (int iz = z0; iz < z1; ++iz) {
        const int k = zc - sz[iz];
        if ((unsigned)k >= (unsigned)g.cz) continue;
        const float w = wij * wz[k];
        const float* __restrict__ row = z + ((prow + (int64_t)iz * g.cx * g.cy) * g.cz + k) * K;
#pragma unroll
        for (int c = 0; c < K; ++c) num[c] = num[c] + w * row[c];
        den = den + w;
      }
    }
  }
}

// grid = capped_blocks(V, 256, SB_MAX_BLOCKS); block = 256.  partial[block][32] float64 (seg_head.hip's slots) with STATS.
template <int K, bool STATS>
__global__ void __launch_bounds__(SB_THREADS) seg_blend_kernel(const float* __restrict__ z, const int* __restrict__ sx, const int* __restrict__ sy,
                                                              const int* __restrict__ sz, const float* __restrict__ wx, const float* __restrict__ wy,
                                                              const float* __restrict__ wz, SbGeom g, const uint8_t* __restrict__ labels,
                                                              uint8_t* __restrict__ mask, float* __restrict__ probs, float* __restrict__ numden,
                                                              unsigned long long* __restrict__ counts, double* __restrict__ partial) {
  __shared__ double red[SB_THREADS / 64][PCRL_SEG_SLOTS];
  __shared__ unsigned redc[SB_THREADS / 64][SB_MAX_K * 3 + 3];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int64_t V = (int64_t)g.X * g.Y * g.Z;
  double sI[K], sP[K], sG[K], sB[K];
  unsigned cTP[K], cPr[K], cGt[K], cnt = 0;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    sI[c] = sP[c] = sG[c] = sB[c] = 0.0;
    cTP[c] = cPr[c] = cGt[c] = 0u;
  }
  for (int64_t v = (int64_t)blockIdx.x * SB_THREADS + t; v < V; v += (int64_t)gridDim.x * SB_THREADS) {
    const int zc = (int)(v % g.Z), yc = (int)((v / g.Z) % g.Y), xc = (int)(v / ((int64_t)g.Z * g.Y));
    float num[K], den;
    sb_walk<K>(z, sx, sy, sz, wx, wy, wz, g, xc, yc, zc, num, den);
    const unsigned lab = labels ? labels[v] : 0u;
    const bool counted = !(lab & 0x80u);
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const bool pred = counted && num[c] >= 0.0f;
      m |= pred ? (1u << c) : 0u;
      if (numden) {
        numden[(int64_t)c * V + v] = num[c];
        numden[(int64_t)(K + 1 + c) * V + v] = num[c] / den;
      }
      if (probs || STATS) {
        const float zb = num[c] / den, p = seg_sigmoid(zb);
        if (probs) probs[(int64_t)c * V + v] = p;
        if (STATS && counted) {
          const bool gt = (lab >> c) & 1u;
          const float y = gt ? 1.0f : 0.0f;
          sI[c] += (double)(gt ? p : 0.0f);
          sP[c] += (double)p;
          sG[c] += (double)y;
          sB[c] += (double)(fmaxf(zb, 0.0f) - y * zb + log1pf(expf(-fabsf(zb))));
          cTP[c] += (pred && gt) ? 1u : 0u;
          cPr[c] += pred ? 1u : 0u;
          cGt[c] += gt ? 1u : 0u;
        }
      }
    }
    if (numden) numden[(int64_t)K * V + v] = den;
    if (mask) mask[v] = (uint8_t)m;
    cnt += counted ? 1u : 0u;
  }
  if (!STATS) return;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const double a = wave_sum(sI[c]), b = wave_sum(sP[c]), d = wave_sum(sG[c]), e = wave_sum(sB[c]);
    const unsigned p = wave_sum(cTP[c]), q = wave_sum(cPr[c]), r = wave_sum(cGt[c]);
    if (lane == 0) {
      red[wid][c * 4 + 0] = a;
      red[wid][c * 4 + 1] = b;
      red[wid][c * 4 + 2] = d;
      red[wid][c * 4 + 3] = e;
      redc[wid][c * 3 + 0] = p;
      redc[wid][c * 3 + 1] = q;
      redc[wid][c * 3 + 2] = r;
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0) red[wid][PCRL_SEG_CNT_SLOT] = (double)cnt;
  __syncthreads();
  if (t < 4 * K || t == PCRL_SEG_CNT_SLOT) partial[(int64_t)blockIdx.x * PCRL_SEG_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (counts && t < 3 * K) atomicAdd(&counts[t], (unsigned long long)redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t]);
}

template <int K>
void seg_blend_launch(bool stats, int nb, hipStream_t st, const float* z, const int* sx, const int* sy, const int* sz, const float* wx, const float* wy,
                      const float* wz, const SbGeom& g, const uint8_t* labels, uint8_t* mask, float* probs, float* numden, int64_t* counts, double* partial) {
  if (stats)
    hipLaunchKernelGGL((seg_blend_kernel<K, true>), dim3(nb), dim3(SB_THREADS), 0, st, z, sx, sy, sz, wx, wy, wz, g, labels, mask, probs, numden,
                       reinterpret_cast<unsigned long long*>(counts), partial);
  else
    hipLaunchKernelGGL((seg_blend_kernel<K, false>), dim3(nb), dim3(SB_THREADS), 0, st, z, sx, sy, sz, wx, wy, wz, g, labels, mask, probs, numden, nullptr,
                       nullptr);
}

// The label-map sibling (softmax head, 2 <= K <= 16 mutually exclusive classes): the same walk, then per voxel
//     pred = the LOWEST k with maximal num_k (den > 0: no division decides a prediction; 0 where the voxel is not counted)
//     zbar_k = num_k / den;  m = max_k zbar_k;  e_k = exp(zbar_k - m);  s = sum_k e_k (ascending k);  p_k = e_k / s;  ce = (m - zbar_y) + log s
// and, with STATS, the softmax head's {I, P, G, CE} per class in per-thread float64 sums (a class other than y adds to P alone), wave shuffle sums, LDS
// red[wave][slot] and per-block partials [PCRL_SEG_MC_SLOTS] that seg_head_mc.hip's one-block launch adds in block order.  The counts {TP, |pred|, |gt|}
// go through 32-bit INTEGER atomics on a block's LDS table (order-independent) and ONE 64-bit integer atomic per (block, k, q).  No floating-point atomics.
template <int K, bool STATS>
__global__ void __launch_bounds__(SB_THREADS) seg_mc_blend_kernel(const float* __restrict__ z, const int* __restrict__ sx, const int* __restrict__ sy,
                                                                 const int* __restrict__ sz, const float* __restrict__ wx, const float* __restrict__ wy,
                                                                 const float* __restrict__ wz, SbGeom g, const uint8_t* __restrict__ labels,
                                                                 uint8_t* __restrict__ labelmap, float* __restrict__ probs, float* __restrict__ numden,
                                                                 unsigned long long* __restrict__ counts, double* __restrict__ partial) {
  __shared__ double red[SB_THREADS / 64][PCRL_SEG_MC_SLOTS];
  __shared__ unsigned cs[SB_MC_MAX_K * 3];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int64_t V = (int64_t)g.X * g.Y * g.Z;
  double sI[K], sP[K], sG[K], sC[K];
  unsigned cnt = 0;
#pragma unroll
  for (int c = 0; c < K; ++c) sI[c] = sP[c] = sG[c] = sC[c] = 0.0;
  if (STATS) {
    if (t < K * 3) cs[t] = 0u;
    __syncthreads();
  }
  for (int64_t v = (int64_t)blockIdx.x * SB_THREADS + t; v < V; v += (int64_t)gridDim.x * SB_THREADS) {
    const int zc = (int)(v % g.Z), yc = (int)((v / g.Z) % g.Y), xc = (int)(v / ((int64_t)g.Z * g.Y));
    float num[K], den;
    sb_walk<K>(z, sx, sy, sz, wx, wy, wz, g, xc, yc, zc, num, den);
    const unsigned lab = labels ? labels[v] : 0u;
    const int y = (int)(lab & 0x7Fu);
    const bool counted = !(lab & 0x80u) && y < K;
    int pred = 0;
#pragma unroll
    for (int c = 1; c < K; ++c)
      if (num[c] > num[pred]) pred = c;
    if (labelmap) labelmap[v] = (uint8_t)(counted ? pred : 0);
    if (numden) {
#pragma unroll
      for (int c = 0; c < K; ++c) {
        numden[(int64_t)c * V + v] = num[c];
        numden[(int64_t)(K + 1 + c) * V + v] = num[c] / den;
      }
      numden[(int64_t)K * V + v] = den;
    }
    if (probs || STATS) {
      float zb[K], m = -INFINITY, s = 0.0f;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        zb[c] = num[c] / den;
        m = fmaxf(m, zb[c]);
      }
#pragma unroll
      for (int c = 0; c < K; ++c) {
        zb[c] = zb[c] - m;            // <= 0; the class's exponent
        s = s + expf(zb[c]);
      }
      const float ls = logf(s);
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const float p = expf(zb[c]) / s;
        if (probs) probs[(int64_t)c * V + v] = p;
        if (STATS && counted) {
          sP[c] += (double)p;
          if (c == y) {
            sI[c] += (double)p;
            sG[c] += 1.0;
            sC[c] += (double)(ls - zb[c]);      // (m - zbar_y) + log s
          }
        }
      }
    }
    if (STATS && counted) {
      atomicAdd(&cs[pred * 3 + 1], 1u);
      atomicAdd(&cs[y * 3 + 2], 1u);
      if (pred == y) atomicAdd(&cs[y * 3 + 0], 1u);
      cnt += 1u;
    }
  }
  if (!STATS) return;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const double a = wave_sum(sI[c]), b = wave_sum(sP[c]), d = wave_sum(sG[c]), e = wave_sum(sC[c]);
    if (lane == 0) {
      red[wid][c * 4 + 0] = a;
      red[wid][c * 4 + 1] = b;
      red[wid][c * 4 + 2] = d;
      red[wid][c * 4 + 3] = e;
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0) red[wid][4 * K] = (double)cnt;
  __syncthreads();
  if (t <= 4 * K) partial[(int64_t)blockIdx.x * PCRL_SEG_MC_SLOTS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (counts && t < 3 * K && cs[t]) atomicAdd(&counts[t], (unsigned long long)cs[t]);
}

template <int K>
void seg_mc_blend_launch(bool stats, int nb, hipStream_t st, const float* z, const int* sx, const int* sy, const int* sz, const float* wx, const float* wy,
                         const float* wz, const SbGeom& g, const uint8_t* labels, uint8_t* labelmap, float* probs, float* numden, int64_t* counts,
                         double* partial) {
  if (stats)
    hipLaunchKernelGGL((seg_mc_blend_kernel<K, true>), dim3(nb), dim3(SB_THREADS), 0, st, z, sx, sy, sz, wx, wy, wz, g, labels, labelmap, probs, numden,
                       reinterpret_cast<unsigned long long*>(counts), partial);
  else
    hipLaunchKernelGGL((seg_mc_blend_kernel<K, false>), dim3(nb), dim3(SB_THREADS), 0, st, z, sx, sy, sz, wx, wy, wz, g, labels, labelmap, probs, numden,
                       nullptr, nullptr);
}

// grid = ceil(total / 256) with total = n * C * cx * cy * (cz / 4); block = 256.  MIRROR: output voxel (i, j, k) of a patch is voxel (fx ? cx-1-i : i,
// fy ? cy-1-j : j, fz ? cz-1-k : k) of the patch BOX, zeros outside the volume included -- the same grid and the same thread -> output mapping; with a
// z-mirror the four scalar loads of a thread run backwards.  Without MIRROR `flip` is not read.
template <typename T, bool MIRROR>
__global__ void __launch_bounds__(SB_THREADS) seg_cut_kernel(const T* __restrict__ img, const int* __restrict__ starts, float* __restrict__ out, int64_t total,
                                                            int C, int X, int Y, int Z, int cx, int cy, int cz, int flip) {
  const int64_t q = (int64_t)blockIdx.x * SB_THREADS + threadIdx.x;
  if (q >= total) return;
  const int cz4 = cz >> 2;
  const int k4 = (int)(q % cz4);
  int64_t r = q / cz4;
  const int j = (int)(r % cy);
  r /= cy;
  const int i = (int)(r % cx);
  r /= cx;
  const int c = (int)(r % C);
  const int64_t p = r / C;
  const int pi = (MIRROR && (flip & 1)) ? cx - 1 - i : i, pj = (MIRROR && (flip & 2)) ? cy - 1 - j : j;
  const int pk0 = (MIRROR && (flip & 4)) ? cz - 1 - 4 * k4 : 4 * k4, dk = (MIRROR && (flip & 4)) ? -1 : 1;
  const int64_t x = (int64_t)starts[p * 3] + pi, y = (int64_t)starts[p * 3 + 1] + pj, z0 = (int64_t)starts[p * 3 + 2] + pk0;
  const bool row_in = x >= 0 && x < X && y >= 0 && y < Y;
  const T* __restrict__ src = img + (((int64_t)c * X + (row_in ? x : 0)) * Y + (row_in ? y : 0)) * Z;
  float4 o;
  float* ov = reinterpret_cast<float*>(&o);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t zz = z0 + dk * u;
    ov[u] = (row_in && zz >= 0 && zz < Z) ? (float)src[zz] : 0.0f;
  }
  *reinterpret_cast<float4*>(out + q * 4) = o;
}

// The checks and the launch both cutters share; `who` is the entry point's name in the messages.
template <bool MIRROR>
int seg_cut_launch(const char* who, const void* img, int src_half, const int* starts, float* out, int n, int C, int X, int Y, int Z, int cx, int cy, int cz,
                   int flip, pcrl_stream_t stream) {
  PCRL_REQUIRE(img && starts && out, "%s: null pointer", who);
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(out) % 16 == 0, "%s: out must be 16-byte aligned (16-byte stores)", who);
  PCRL_REQUIRE(n > 0 && C > 0 && X > 0 && Y > 0 && Z > 0, "%s: bad sizes n=%d C=%d volume %d x %d x %d", who, n, C, X, Y, Z);
  PCRL_REQUIRE(cx > 0 && cy > 0 && cz > 0 && cz % 4 == 0, "%s: bad crop %d x %d x %d (cz is a multiple of 4)", who, cx, cy, cz);
  const int64_t total = (int64_t)n * C * cx * cy * (cz / 4), blocks = (total + SB_THREADS - 1) / SB_THREADS;
  PCRL_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many output voxels in one call", who);
  hipStream_t st = as_stream(stream);
  if (src_half)
    hipLaunchKernelGGL((seg_cut_kernel<_Float16, MIRROR>), dim3((unsigned)blocks), dim3(SB_THREADS), 0, st, static_cast<const _Float16*>(img), starts, out,
                       total, C, X, Y, Z, cx, cy, cz, flip);
  else
    hipLaunchKernelGGL((seg_cut_kernel<float, MIRROR>), dim3((unsigned)blocks), dim3(SB_THREADS), 0, st, static_cast<const float*>(img), starts, out, total, C,
                       X, Y, Z, cx, cy, cz, flip);
  return pcrl_check_launch(who);
}

// what both blends refuse, after their own check of K; `who` is the entry point's name in the messages
int sb_check(const char* who, const float* z, int64_t P, const int* sx, const int* sy, const int* sz, int nx, int ny, int nz, const float* wx, const float* wy,
             const float* wz, int cx, int cy, int cz, int X, int Y, int Z, const int64_t* counts, const double* sums, const float* loss) {
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "%s: empty volume %d x %d x %d", who, X, Y, Z);
  PCRL_REQUIRE(cx > 0 && cy > 0 && cz > 0, "%s: bad crop %d x %d x %d", who, cx, cy, cz);
  PCRL_REQUIRE(nx > 0 && ny > 0 && nz > 0 && (int64_t)nx * ny * nz == P, "%s: %lld patches against start lists of %d x %d x %d", who, (long long)P, nx, ny,
               nz);
  PCRL_REQUIRE(z && sx && sy && sz && wx && wy && wz, "%s: null pointer", who);
  PCRL_REQUIRE((sums != nullptr) == (loss != nullptr), "%s: sums and loss are both given or both NULL", who);
  PCRL_REQUIRE(!counts || sums, "%s: counts are produced with the sums", who);
  return PCRL_OK;
}

}  // namespace

extern "C" size_t pcrl_seg_blend_ws_bytes(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0) return 0;
  return (size_t)capped_blocks((int64_t)X * Y * Z, SB_THREADS, SB_MAX_BLOCKS) * PCRL_SEG_SLOTS * sizeof(double);
}

extern "C" int pcrl_seg_blend(const float* z, int64_t P, const int* sx, const int* sy, const int* sz, int nx, int ny, int nz, const float* wx,
                              const float* wy, const float* wz, int cx, int cy, int cz, int X, int Y, int Z, int K, const uint8_t* labels, uint8_t* mask,
                              float* probs, float* numden, int64_t* counts, double* sums, float* loss, float wb, float wd, void* ws, size_t ws_bytes,
                              pcrl_stream_t stream) {
  PCRL_REQUIRE(K >= 1 && K <= SB_MAX_K, "seg_blend: 1 <= K <= %d classes (bit 7 of a label byte means 'not counted'), got %d", SB_MAX_K, K);
  if (int rc = sb_check("seg_blend", z, P, sx, sy, sz, nx, ny, nz, wx, wy, wz, cx, cy, cz, X, Y, Z, counts, sums, loss)) return rc;
  const bool stats = sums != nullptr;
  if (stats && (!ws || ws_bytes < pcrl_seg_blend_ws_bytes(X, Y, Z))) return pcrl_fail(PCRL_EWORKSPACE, "seg_blend: workspace too small");
  const SbGeom g{X, Y, Z, cx, cy, cz, nx, ny, nz};
  const int nb = capped_blocks((int64_t)X * Y * Z, SB_THREADS, SB_MAX_BLOCKS);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
#define SB_BLEND(KK) seg_blend_launch<KK>(stats, nb, st, z, sx, sy, sz, wx, wy, wz, g, labels, mask, probs, numden, counts, partial)
  PCRL_SEG_DISPATCH_K(SB_BLEND)
#undef SB_BLEND
  if (stats) pcrl_seg_sums_launch(partial, nb, K, wb, wd, sums, loss, st);
  return pcrl_check_launch("seg_blend");
}

extern "C" int pcrl_seg_cut_patches(const void* img, int src_half, const int* starts, float* out, int n, int C, int X, int Y, int Z, int cx, int cy, int cz,
                                    pcrl_stream_t stream) {
  return seg_cut_launch<false>("seg_cut_patches", img, src_half, starts, out, n, C, X, Y, Z, cx, cy, cz, 0, stream);
}

extern "C" int pcrl_seg_cut_patches_mirror(const void* img, int src_half, const int* starts, float* out, int n, int C, int X, int Y, int Z, int cx, int cy,
                                           int cz, int flip, pcrl_stream_t stream) {
  PCRL_REQUIRE(flip >= 0 && flip <= 7, "seg_cut_patches_mirror: flip %d is no mirror code (bit 0 = x, bit 1 = y, bit 2 = z: 0..7)", flip);
  return seg_cut_launch<true>("seg_cut_patches_mirror", img, src_half, starts, out, n, C, X, Y, Z, cx, cy, cz, flip, stream);
}

extern "C" size_t pcrl_seg_mc_blend_ws_bytes(int X, int Y, int Z) {
  if (X <= 0 || Y <= 0 || Z <= 0) return 0;
  return (size_t)capped_blocks((int64_t)X * Y * Z, SB_THREADS, SB_MAX_BLOCKS) * PCRL_SEG_MC_SLOTS * sizeof(double);
}

extern "C" int pcrl_seg_mc_blend(const float* z, int64_t P, const int* sx, const int* sy, const int* sz, int nx, int ny, int nz, const float* wx,
                                 const float* wy, const float* wz, int cx, int cy, int cz, int X, int Y, int Z, int K, const uint8_t* labels,
                                 uint8_t* labelmap, float* probs, float* numden, int64_t* counts, double* sums, float* loss, float wc, float wd, void* ws,
                                 size_t ws_bytes, pcrl_stream_t stream) {
  PCRL_REQUIRE(K >= 2 && K <= SB_MC_MAX_K, "seg_mc_blend: 2 <= K <= %d mutually exclusive classes, the background included, got %d", SB_MC_MAX_K, K);
  if (int rc = sb_check("seg_mc_blend", z, P, sx, sy, sz, nx, ny, nz, wx, wy, wz, cx, cy, cz, X, Y, Z, counts, sums, loss)) return rc;
  const bool stats = sums != nullptr;
  if (stats && (!ws || ws_bytes < pcrl_seg_mc_blend_ws_bytes(X, Y, Z))) return pcrl_fail(PCRL_EWORKSPACE, "seg_mc_blend: workspace too small");
  const SbGeom g{X, Y, Z, cx, cy, cz, nx, ny, nz};
  const int nb = capped_blocks((int64_t)X * Y * Z, SB_THREADS, SB_MAX_BLOCKS);
  double* partial = static_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
#define SB_MC_BLEND(KK) seg_mc_blend_launch<KK>(stats, nb, st, z, sx, sy, sz, wx, wy, wz, g, labels, labelmap, probs, numden, counts, partial)
  PCRL_SEG_MC_DISPATCH_K(SB_MC_BLEND)
#undef SB_MC_BLEND
  if (stats) pcrl_seg_mc_sums_launch(partial, nb, K, wc, wd, sums, loss, st);
  return pcrl_check_launch("seg_mc_blend");
}
