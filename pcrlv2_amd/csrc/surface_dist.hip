// Surface-distance metrics of 3D segmentation masks (HD95, HD, ASSD: MedPy's definitions) on the device: surface extraction, an exact Euclidean
// distance transform with physical voxel spacing, and an order-statistic selection without a sort.  Compiled with -ffp-contract=off: the squared
// distances are pinned bit for bit against a float64 restatement that multiplies and adds one operation at a time.
//
// extract   thread = SE_ZPT (4) consecutive z of one (x, y) row, consecutive threads along Z.  The prediction and ground-truth bytes of a voxel are
//           masked (bit 7 of the ground truth: the voxel is in neither mask; bits >= K dropped) and packed into one 16-bit word, so ONE chain of five
//           ANDs erodes all K classes of both masks:  surf = m & ~(m[x-1] & m[x+1] & m[y-1] & m[y+1] & m[z-1] & m[z+1]),  0 outside the volume.  The
//           four x / y neighbours are only loaded where m != 0.  {TP, |pred|, |gt|} per class: popcounts of the four packed bytes, wave shuffle
//           sums, LDS redc[wave][k * 3 + q], ONE 64-bit integer atomic per (block, k, q).
// edt       three launches of one line-pass kernel, Z then Y then X, each rewriting d2 IN PLACE:  out[i] = min_j (fl(fl(s (i - j))^2) + f[j]).
//           A block owns a tile of whole lines, stages it in LDS, synchronises, and only then writes: no line is shared between blocks, so the pass
//           needs no second buffer.  Z pass (INNER): a tile is R consecutive (x, y) lines = one contiguous run of R * Z voxels, read straight from
//           the bitmask as 0 / +inf (at most 4096 voxels and 512 lines).  Y and X passes: a tile is a run of R neighbouring inner positions (z for Y; (y, z) for X, whose lines are all
//           independent) x the whole line, so a global access of 64 consecutive threads covers runs of R * 8 contiguous bytes.
//           A line of the tile without a finite value (flagged in LDS while the tile is staged) is +inf afterwards as before: it is not scanned.
//           Early exit: a thread scans outwards, d = 1, 2, ...; c(d) = fl(fl(s d)^2) is non-decreasing in d and f >= 0, so fl(c + f) >= c, and the
//           scan stops at the first c(d) >= the running minimum -- every term left out is >= the minimum, the result is bit-identical.
// LDS       the tile is stored in thread order: element e of the tile (INNER: e = line * L + i; otherwise e = i * nr + r with nr the tile's run) lives
//           at tile[e], and thread t handles e = t, t + 512, ...  At scan distance d a wave reads tile[e -+ d * step] with ONE d for the lanes that
//           are still scanning (step = 1 or nr, uniform): 64 consecutive float64, i.e. each 32-lane half of the ds_read_b64 covers 256 consecutive
//           bytes = every one of the 64 banks once -- conflict-free; lanes that have left the scan are masked off and only leave banks idle.  The
//           line flags are read once per element, outside the scan: has[e / L] is one or two words per wave (a broadcast), has[e % nr] consecutive
//           words, wrapping at nr <= 64 -- equal addresses broadcast; where the wrap falls inside a 32-lane half and nr > 32, words w and w + 32 meet
//           on one of ds_read_b32's 32 banks: at worst 2-way, once per element.  The
//           stores that fill the tile are 64 consecutive float64 per wave as well.
// stats     count: one pass over both (mask, d2) pairs -- n_a, n_b (integer atomics) and the two sums of sqrt(d2): per-thread float64, wave shuffle,
//           LDS red[wave][2], per-block partials that the one-thread `start` launch adds in block order.  select: radix select (radix_select.h) on the 64-bit
//           pattern of the non-negative doubles (their order is the integers' order), most significant byte first: eight passes, each a 256-bin
//           histogram PER RANK (lo, hi, n - 1) of the values that share the rank's prefix so far -- LDS integer atomics, then one 64-bit integer
//           atomic per non-empty (block, rank, bin) -- and a tiny `pick` launch that walks the bins, extends the prefixes and clears the
//           histogram.  No host read-back in between, no floating-point atomics: the result does not depend on any order.  The LDS traffic of a
//           histogram is atomics on data-dependent bins; equal values serialise on one bin, which is what counting them takes.
#include "radix_select.h"

namespace {

constexpr int SD_THREADS = 256, SD_MAX_K = 7, SD_MAX_BLOCKS = 1024;
constexpr int SE_ZPT = 4;
constexpr int EDT_THREADS = 512, EDT_LDS = 8128, EDT_INNER_TILE = 4096, EDT_INNER_LINES = 512, EDT_MAX_RUN = 64, EDT_MAX_AXIS = 1024;

// ---- surface extraction -------------------------------------------------------------------------------------------------------------
// prediction in bits 0..6, ground truth in bits 8..14 of one word; a voxel that is not counted belongs to neither mask
__device__ __forceinline__ unsigned se_eff(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int64_t idx, unsigned kmask) {
  const unsigned g = gt[idx], p = pred[idx];
  const unsigned keep = (g & 0x80u) ? 0u : kmask;
  return (p & keep) | ((g & keep) << 8);
}

// grid = capped_blocks(X * Y * ceil(Z / 4), 256, SD_MAX_BLOCKS); block = 256.  VEC: Z % 4 == 0 and both outputs 4-byte aligned -- one 32-bit store per thread and mask.
template <bool VEC>
__global__ void __launch_bounds__(SD_THREADS) surf_extract_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, uint8_t* __restrict__ sp,
                                                                 uint8_t* __restrict__ sg, unsigned long long* __restrict__ counts, int X, int Y, int Z, int K) {
  __shared__ unsigned redc[SD_THREADS / 64][SD_MAX_K * 3];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const unsigned kmask = (1u << K) - 1u;
  const int zq = (Z + SE_ZPT - 1) / SE_ZPT;
  const int64_t items = (int64_t)X * Y * zq, sx = (int64_t)Y * Z;
  unsigned cTP[SD_MAX_K], cPr[SD_MAX_K], cGt[SD_MAX_K];
#pragma unroll
  for (int c = 0; c < SD_MAX_K; ++c) cTP[c] = cPr[c] = cGt[c] = 0u;
  for (int64_t it = (int64_t)blockIdx.x * SD_THREADS + t; it < items; it += (int64_t)gridDim.x * SD_THREADS) {
    const int zb = (int)(it % zq) * SE_ZPT;
    const int64_t r = it / zq;
    const int y = (int)(r % Y), x = (int)(r / Y);
    const int64_t row = ((int64_t)x * Y + y) * Z;
    unsigned c[SE_ZPT + 2];
#pragma unroll
    for (int u = 0; u < SE_ZPT + 2; ++u) {
      const int zz = zb - 1 + u;
      c[u] = (zz >= 0 && zz < Z) ? se_eff(pred, gt, row + zz, kmask) : 0u;
    }
    unsigned wp = 0, wg = 0, wsp = 0, wsg = 0;
#pragma unroll
    for (int u = 0; u < SE_ZPT; ++u) {
      const int zz = zb + u;
      const unsigned m = c[u + 1];
      unsigned s = 0;
      if (m) {      // zz < Z here: c is 0 past the row's end
        unsigned nb = c[u] & c[u + 2];
        nb &= x > 0 ? se_eff(pred, gt, row - sx + zz, kmask) : 0u;
        nb &= x < X - 1 ? se_eff(pred, gt, row + sx + zz, kmask) : 0u;
        nb &= y > 0 ? se_eff(pred, gt, row - Z + zz, kmask) : 0u;
        nb &= y < Y - 1 ? se_eff(pred, gt, row + Z + zz, kmask) : 0u;
        s = m & ~nb;
      }
      wp |= (m & 0x7fu) << (8 * u);
      wg |= ((m >> 8) & 0x7fu) << (8 * u);
      wsp |= (s & 0x7fu) << (8 * u);
      wsg |= ((s >> 8) & 0x7fu) << (8 * u);
    }
    if (VEC) {
      *reinterpret_cast<uint32_t*>(sp + row + zb) = wsp;
      *reinterpret_cast<uint32_t*>(sg + row + zb) = wsg;
    } else {
#pragma unroll
      for (int u = 0; u < SE_ZPT; ++u) {
        if (zb + u < Z) {
          sp[row + zb + u] = (uint8_t)(wsp >> (8 * u));
          sg[row + zb + u] = (uint8_t)(wsg >> (8 * u));
        }
      }
    }
    const unsigned wtp = wp & wg;
#pragma unroll
    for (int k = 0; k < SD_MAX_K; ++k) {
      const unsigned sel = 0x01010101u << k;
      cTP[k] += __popc(wtp & sel);
      cPr[k] += __popc(wp & sel);
      cGt[k] += __popc(wg & sel);
    }
  }
#pragma unroll
  for (int k = 0; k < SD_MAX_K; ++k) {
    const unsigned p = wave_sum(cTP[k]), q = wave_sum(cPr[k]), g = wave_sum(cGt[k]);
    if (lane == 0) {
      redc[wid][k * 3 + 0] = p;
      redc[wid][k * 3 + 1] = q;
      redc[wid][k * 3 + 2] = g;
    }
  }
  __syncthreads();
  if (t < 3 * K) {
    const unsigned long long v = (unsigned long long)redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t];
    if (v) atomicAdd(&counts[t], v);
  }
}

// ---- squared Euclidean distance transform --------------------------------------------------------------------------------------------
// The volume seen from one pass: A outer positions x L positions along the pass's axis x B inner positions; tiles of R (inner, or whole lines: INNER).
struct EdtGeom {
  int64_t A, B;
  int L, R;
  int64_t tiles_per_a;
};

// grid = number of tiles; block = 512; LDS = one tile of at most EDT_LDS float64 (EDT_INNER_TILE: INNER) and one flag per line of the tile, 64 KiB in all.
template <bool INNER>
__global__ void __launch_bounds__(EDT_THREADS) edt_line_kernel(const uint8_t* __restrict__ surf, unsigned bit, double* __restrict__ d2, double s, EdtGeom g,
                                                              unsigned long long* __restrict__ steps) {
  __shared__ double tile[INNER ? EDT_INNER_TILE : EDT_LDS];
  __shared__ int has[INNER ? EDT_INNER_LINES : EDT_MAX_RUN];      // the line holds a finite value
  const int t = threadIdx.x, L = g.L;
  const double inf = __builtin_inf();
  if (t < (INNER ? EDT_INNER_LINES : EDT_MAX_RUN)) has[t] = 0;
  __syncthreads();
  int ne, nr;
  int64_t base;       // INNER: the tile's first voxel; otherwise voxel (a, 0, b0)
  if (INNER) {
    const int64_t a0 = (int64_t)blockIdx.x * g.R;
    const int64_t nl = g.A - a0 < g.R ? g.A - a0 : g.R;
    nr = 1;
    ne = (int)nl * L;
    base = a0 * L;
    for (int e = t; e < ne; e += EDT_THREADS) {
      const bool on = (surf[base + e] & bit) != 0;
      tile[e] = on ? 0.0 : inf;
      if (on) has[e / L] = 1;      // every writer stores the same value
    }
  } else {
    const int64_t a = blockIdx.x / g.tiles_per_a, b0 = (blockIdx.x % g.tiles_per_a) * g.R;
    nr = (int)(g.B - b0 < g.R ? g.B - b0 : g.R);
    ne = L * nr;
    base = a * L * g.B + b0;
    for (int e = t; e < ne; e += EDT_THREADS) {
      const double v = d2[base + (int64_t)(e / nr) * g.B + (e % nr)];
      tile[e] = v;
      if (v < inf) has[e % nr] = 1;
    }
  }
  __syncthreads();
  unsigned long long mine = 0;
  for (int e = t; e < ne; e += EDT_THREADS) {
    const int i = INNER ? e % L : e / nr;
    const int left = i, right = L - 1 - i, far = left > right ? left : right;
    double best = tile[e];
    int d = 1;
    if (!has[INNER ? e / L : e % nr]) d = far + 1;      // nothing finite on this line: every voxel of it stays +inf, no scan
    for (; d <= far; ++d) {
      const double sd = s * (double)d;
      const double c = sd * sd;
      if (c >= best) break;
      if (d <= left) {
        const double v = c + tile[e - d * nr];
        best = v < best ? v : best;
      }
      if (d <= right) {
        const double v = c + tile[e + d * nr];
        best = v < best ? v : best;
      }
    }
    mine += has[INNER ? e / L : e % nr] ? (unsigned)(d - 1) : 0u;
    d2[INNER ? base + e : base + (int64_t)i * g.B + (e % nr)] = best;
  }
  if (steps) {
    mine = wave_sum(mine);
    if ((t & 63) == 0 && mine) atomicAdd(steps, mine);
  }
}

// ---- distance statistics of one class -------------------------------------------------------------------------------------------------
using SdSel = RadixSelect<uint64_t, 3>;      // the ranks lo, hi, n - 1
struct SdState {
  unsigned long long cnt[2];     // n_a, n_b
  unsigned long long active;     // both surfaces non-empty: the selection runs
  SdSel sel;
};
constexpr size_t SD_STATE_BYTES = sizeof(SdState);

// grid = capped_blocks(V, 256, SD_MAX_BLOCKS); block = 256.  partial [nb][2] float64.
__global__ void __launch_bounds__(SD_THREADS) sd_count_kernel(const double* __restrict__ d2a, const uint8_t* __restrict__ ma, const double* __restrict__ d2b,
                                                             const uint8_t* __restrict__ mb, unsigned bit, int64_t V, SdState* __restrict__ st,
                                                             double* __restrict__ partial) {
  __shared__ double red[SD_THREADS / 64][2];
  __shared__ unsigned redc[SD_THREADS / 64][2];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  double sa = 0.0, sb = 0.0;
  unsigned na = 0, nb = 0;
  for (int64_t v = (int64_t)blockIdx.x * SD_THREADS + t; v < V; v += (int64_t)gridDim.x * SD_THREADS) {
    if (ma[v] & bit) {
      sa += sqrt(d2a[v]);
      ++na;
    }
    if (mb[v] & bit) {
      sb += sqrt(d2b[v]);
      ++nb;
    }
  }
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  na = wave_sum(na);
  nb = wave_sum(nb);
  if (lane == 0) {
    red[wid][0] = sa;
    red[wid][1] = sb;
    redc[wid][0] = na;
    redc[wid][1] = nb;
  }
  __syncthreads();
  if (t < 2) {
    partial[(int64_t)blockIdx.x * 2 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    const unsigned long long c = (unsigned long long)redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t];
    if (c) atomicAdd(&st->cnt[t], c);
  }
}

// one thread: the counts into the record; with both surfaces non-empty the three ranks and the two sums, added in block order
__global__ void sd_start_kernel(SdState* __restrict__ st, const double* __restrict__ partial, int nb, double q, long long* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long na = (long long)st->cnt[0], nbv = (long long)st->cnt[1];
  rec[0] = na;
  rec[1] = nbv;
  if (na == 0 || nbv == 0) {
    st->active = 0;
    return;
  }
  const long long n = na + nbv;
  long long lo = (long long)floor(q * (double)(n - 1));
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  const long long hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  st->sel.rank[0] = (unsigned long long)lo;
  st->sel.rank[1] = (unsigned long long)hi;
  st->sel.rank[2] = (unsigned long long)(n - 1);
  st->sel.prefix[0] = st->sel.prefix[1] = st->sel.prefix[2] = 0;
  st->active = 1;
  rec[2] = lo;
  double sa = 0.0, sb = 0.0;
  for (int b = 0; b < nb; ++b) {
    sa += partial[b * 2];
    sb += partial[b * 2 + 1];
  }
  double* recd = reinterpret_cast<double*>(rec);
  recd[6] = sa;
  recd[7] = sb;
}

// grid = capped_blocks(V, 256, SD_MAX_BLOCKS); block = 256.  A voxel yields a key for each surface it lies on: the bit pattern of its distance.
__global__ void __launch_bounds__(SD_THREADS) sd_hist_kernel(const double* __restrict__ d2a, const uint8_t* __restrict__ ma, const double* __restrict__ d2b,
                                                            const uint8_t* __restrict__ mb, unsigned bit, int64_t V, int pass, SdState* __restrict__ st) {
  __shared__ unsigned h[3 * 256];
  if (!st->active) return;      // uniform over the grid
  RadixPass<uint64_t, 3, SD_THREADS> rp;
  rp.begin(&st->sel, pass, h);
  for (int64_t v = (int64_t)blockIdx.x * SD_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * SD_THREADS) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (!((side ? mb[v] : ma[v]) & bit)) continue;
      rp.add((uint64_t)__double_as_longlong(side ? d2b[v] : d2a[v]));
    }
  }
  rp.flush(&st->sel);
}

// one block of 64 threads; thread r < 3 picks rank r, and after the last pass leaves its key in the record
__global__ void sd_sel_pick_kernel(SdState* __restrict__ st, int pass, long long* __restrict__ rec) {
  if (!st->active) return;
  const int r = threadIdx.x;
  if (r >= 3) return;
  const uint64_t pre = radix_pick(&st->sel, r);
  if (pass == SdSel::PASSES - 1) rec[3 + r] = (long long)pre;
}

}  // namespace

extern "C" int pcrl_surf_extract(const uint8_t* pred, const uint8_t* gt, uint8_t* surf_pred, uint8_t* surf_gt, int64_t* counts, int X, int Y, int Z, int K,
                                 pcrl_stream_t stream) {
  PCRL_REQUIRE(K >= 1 && K <= SD_MAX_K, "surf_extract: 1 <= K <= %d classes (bit 7 of a label byte means 'not counted'), got %d", SD_MAX_K, K);
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "surf_extract: empty volume %d x %d x %d", X, Y, Z);
  PCRL_REQUIRE(pred && gt && surf_pred && surf_gt && counts, "surf_extract: null pointer");
  const int nb = capped_blocks((int64_t)X * Y * ((Z + SE_ZPT - 1) / SE_ZPT), SD_THREADS, SD_MAX_BLOCKS);
  const bool vec = Z % SE_ZPT == 0 && reinterpret_cast<uintptr_t>(surf_pred) % 4 == 0 && reinterpret_cast<uintptr_t>(surf_gt) % 4 == 0;
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  if (vec)
    hipLaunchKernelGGL(surf_extract_kernel<true>, dim3(nb), dim3(SD_THREADS), 0, as_stream(stream), pred, gt, surf_pred, surf_gt, c, X, Y, Z, K);
  else
    hipLaunchKernelGGL(surf_extract_kernel<false>, dim3(nb), dim3(SD_THREADS), 0, as_stream(stream), pred, gt, surf_pred, surf_gt, c, X, Y, Z, K);
  return pcrl_check_launch("surf_extract");
}

extern "C" int64_t pcrl_edt_max_axis(void) { return EDT_MAX_AXIS; }

extern "C" size_t pcrl_edt_sq_ws_bytes(int X, int Y, int Z) {
  (void)X, (void)Y, (void)Z;
  return 0;      // every pass rewrites its lines in place from LDS
}

extern "C" int pcrl_edt_sq(const uint8_t* surf, int bit, double* d2, double sx, double sy, double sz, int64_t* steps, void* ws, size_t ws_bytes, int X, int Y,
                           int Z, pcrl_stream_t stream) {
  (void)ws;
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "edt_sq: empty volume %d x %d x %d", X, Y, Z);
  PCRL_REQUIRE(X <= EDT_MAX_AXIS && Y <= EDT_MAX_AXIS && Z <= EDT_MAX_AXIS,
               "edt_sq: volume %d x %d x %d: an axis may have at most %d voxels (a whole line is staged in LDS)", X, Y, Z, EDT_MAX_AXIS);
  PCRL_REQUIRE(bit >= 0 && bit < SD_MAX_K, "edt_sq: bit %d outside 0..%d", bit, SD_MAX_K - 1);
  PCRL_REQUIRE(surf && d2, "edt_sq: null pointer");
  PCRL_REQUIRE(sx > 0 && sy > 0 && sz > 0 && __builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_isfinite(sz),
               "edt_sq: the spacing must be three positive finite numbers, got %g, %g, %g", sx, sy, sz);
  if (ws_bytes < pcrl_edt_sq_ws_bytes(X, Y, Z)) return pcrl_fail(PCRL_EWORKSPACE, "edt_sq: workspace too small");
  hipStream_t st = as_stream(stream);
  unsigned long long* sp = reinterpret_cast<unsigned long long*>(steps);
  const unsigned b = 1u << bit;
  {      // Z: whole lines, R consecutive ones per tile
    EdtGeom g{(int64_t)X * Y, 1, Z, 0, 1};
    g.R = EDT_INNER_TILE / Z < EDT_INNER_LINES ? EDT_INNER_TILE / Z : EDT_INNER_LINES;      // Z <= 1024: at least 4
    const int64_t tiles = (g.A + g.R - 1) / g.R;
    hipLaunchKernelGGL(edt_line_kernel<true>, dim3((unsigned)tiles), dim3(EDT_THREADS), 0, st, surf, b, d2, sz, g, sp);
  }
  const int axis_len[2] = {Y, X};
  const int64_t outer[2] = {X, 1}, inner[2] = {Z, (int64_t)Y * Z};
  const double spacing[2] = {sy, sx};
  for (int p = 0; p < 2; ++p) {      // Y, then X: a run of R neighbouring inner positions x the whole line
    EdtGeom g{outer[p], inner[p], axis_len[p], 0, 0};
    int64_t R = EDT_LDS / g.L;
    R = R > EDT_MAX_RUN ? EDT_MAX_RUN : R;
    g.R = (int)(R > g.B ? g.B : R);
    g.tiles_per_a = (g.B + g.R - 1) / g.R;
    const int64_t tiles = g.A * g.tiles_per_a;      // <= 1024 * 1024 * 1024 / 7
    hipLaunchKernelGGL(edt_line_kernel<false>, dim3((unsigned)tiles), dim3(EDT_THREADS), 0, st, surf, b, d2, spacing[p], g, sp);
  }
  return pcrl_check_launch("edt_sq");
}

extern "C" size_t pcrl_surf_dist_stats_ws_bytes(int64_t V) {
  if (V <= 0) return 0;
  return SD_STATE_BYTES + (size_t)capped_blocks(V, SD_THREADS, SD_MAX_BLOCKS) * 2 * sizeof(double);
}

extern "C" int pcrl_surf_dist_stats(const double* d2_to_gt, const uint8_t* surf_pred, const double* d2_to_pred, const uint8_t* surf_gt, int bit, double q,
                                    int64_t* record, void* ws, size_t ws_bytes, int64_t V, pcrl_stream_t stream) {
  PCRL_REQUIRE(V > 0, "surf_dist_stats: empty volume (%lld voxels)", (long long)V);
  PCRL_REQUIRE(bit >= 0 && bit < SD_MAX_K, "surf_dist_stats: bit %d outside 0..%d", bit, SD_MAX_K - 1);
  PCRL_REQUIRE(q >= 0.0 && q <= 1.0, "surf_dist_stats: the quantile %g is outside [0, 1]", q);
  PCRL_REQUIRE(d2_to_gt && surf_pred && d2_to_pred && surf_gt && record, "surf_dist_stats: null pointer");
  if (!ws || ws_bytes < pcrl_surf_dist_stats_ws_bytes(V)) return pcrl_fail(PCRL_EWORKSPACE, "surf_dist_stats: workspace too small");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "surf_dist_stats: the workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  SdState* state = static_cast<SdState*>(ws);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(ws) + SD_STATE_BYTES);
  long long* rec = reinterpret_cast<long long*>(record);
  const int nb = capped_blocks(V, SD_THREADS, SD_MAX_BLOCKS);
  const unsigned b = 1u << bit;
  if (hipMemsetAsync(state, 0, SD_STATE_BYTES, st) != hipSuccess) return pcrl_fail(PCRL_EINVAL, "surf_dist_stats: memset failed");
  hipLaunchKernelGGL(sd_count_kernel, dim3(nb), dim3(SD_THREADS), 0, st, d2_to_gt, surf_pred, d2_to_pred, surf_gt, b, V, state, partial);
  hipLaunchKernelGGL(sd_start_kernel, dim3(1), dim3(64), 0, st, state, partial, nb, q, rec);
  for (int pass = 0; pass < SdSel::PASSES; ++pass) {
    hipLaunchKernelGGL(sd_hist_kernel, dim3(nb), dim3(SD_THREADS), 0, st, d2_to_gt, surf_pred, d2_to_pred, surf_gt, b, V, pass, state);
    hipLaunchKernelGGL(sd_sel_pick_kernel, dim3(1), dim3(64), 0, st, state, pass, rec);
  }
  return pcrl_check_launch("surf_dist_stats");
}
