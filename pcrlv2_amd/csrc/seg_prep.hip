// 3D segmentation, data side (host: pcrlv2_amd/seg_prep.py): raw volumes -> prepared cases, and predictions back to the scanner's grid.
// Compiled with -ffp-contract=off (pcrlv2_amd/build.py): every float64 expression below is pinned against a numpy restatement
// (tests/seg_prep_reference.py) that multiplies, adds and divides one operation at a time.
//
// The source volumes stay in DISK order -- src [C][Z][Y][X], x fastest, int16 or float32; src_lab uint8 [Z][Y][X] -- and the outputs are in
// PROJECT order, z fastest.  int16 and float32 values are widened to float64 exactly.
//
//   pcrl_segprep_scan      one pass over the C channels: the bounding box of (any channel != 0) by 64-bit integer atomicMin / atomicMax, the
//                          voxels inside that mask and the non-finite values (integer atomicAdd).  One atomic per (block, slot).
//   pcrl_segprep_stats     per channel over the mask M, mean and population standard deviation in float64, two passes: sum(x) / n, then
//                          sum((x - mean)^2) / n.  Per thread a grid-stride sum, a 64-lane shuffle tree, four wave partials added in wave order,
//                          one partial per (block, channel); a one-block second launch adds them in block order (seg_head.hip's scheme).  The grid
//                          is a function of the voxel count alone, so the result is a function of the sizes and the data, never of timing.
//   pcrl_segprep_select    exact order statistics of one channel's masked values for four ranks at once: radix_select.h's selection on the
//                          32-bit order-preserving key of the float32 value (all bits of a negative flipped, the sign bit of the rest; -0.0 takes
//                          +0.0's key and comes back as +0.0): four byte passes, most significant first, each a 256-bin LDS histogram per rank
//                          (LDS integer atomics, then one 64-bit integer atomic per non-empty (block, rank, bin)) and a four-thread `pick` launch.
//   pcrl_segprep_resample  ONE launch per case: img [C][OX][OY][OZ] (float32 or float16) and lab uint8 [OX][OY][OZ] from the box
//                          [bx, bx + NX) x [by, by + NY) x [bz, bz + NZ) of the source, through per-axis tables that the host builds in float64.
//   pcrl_segprep_restore   the label half in the other direction: prepared uint8 [PX][PY][PZ] -> the original grid [X][Y][Z], nearest neighbour
//                          through the inverse tables inside the box, 0 outside, optionally a second output painted through a 256-entry table.
//                          Both sides have z innermost: no transpose, one thread per output voxel, consecutive lanes on consecutive bytes.
//
// Resample arithmetic, per output voxel and channel, float64 (v: a corner's source value, widened):
//     u = (min(max(v, lo), hi) - mean) / max(std, 1e-8)          0.0 instead where use_mask and the corner is outside M (every channel 0 there)
//     acc = 0.0;  for bx in 0, 1: for by in 0, 1: for bz in 0, 1:  acc = acc + ((u * wx[bx]) * wy[by]) * wz[bz]           z fastest
// and ONE rounding of acc to the output type.  float16: that is one rounding too -- acc is first rounded to ODD into float32 (truncate towards
// zero, set the last bit when inexact), which keeps everything a later round-to-nearest-even into the 11-bit significand needs (24 >= 2 * 11 + 2
// bits), so the hardware's float32 -> float16 conversion gives the float16 nearest to acc, ties to even: numpy's float64.astype(float16).
//
// Resample tiling.  The innermost axis changes from x (source) to z (output): a transpose of 2- or 4-byte elements through LDS.  One
// 256-thread block = one output y and a TX x TZ tile of output (x, z) (32 x 32, halved on the axis with the longer source span until the tile
// fits 40 KB: a strong down-sampling only shrinks the tile).  The tile needs source rows y in {j0, j1} of the span [xlo, xhi] x [zlo, zhi]: at
// most ceil((T - 1) n_in / n_out) + 3 per axis, which the entry point derives from the sizes alone -- the kernel clamps every table entry to
// the box and every tile-local index to the staged span, so tables that break the host's promise give wrong values, never a wild address.
//   stage   consecutive lanes take consecutive x of one source row (yy, zz): 64 lanes = 256 contiguous bytes (128 for int16) of global memory
//           whatever X is -- the loads are one element per lane, so no row needs an alignment shift (luna_cubes.hip shifts because it loads four
//           elements per lane).  Values are widened to float32 (exact) and written to tile[(yy * SZ + zz) * pitch + xx]: consecutive dwords,
//           conflict-free for `ds_write_b32` (32-lane groups on bank = dword mod 32).  With use_mask a first pass ORs (value != 0) over all C
//           channels into a byte tile of the same layout, and the label row y = nn_y is staged as bytes; the channels are then staged one after
//           the other into the same float tile (the second read of a span comes from L2: a block's spans are a few KB).
//   drain   consecutive lanes take consecutive output z of one output x: a 32-lane group stores 128 contiguous bytes (float16: 64).  Lane
//           (ox, oz) reads tile[(yy * SZ + zz(oz)) * pitch + xx(ox)] with xx, yy the same for the whole group: bank = (zz * pitch + const) mod 32.
//           pitch = SX | 1 is ODD, so zz -> zz * pitch mod 32 is a bijection of Z/32: lanes with different zz mod 32 hit different banks, lanes
//           with the same zz (up-sampling) read the same dword (a broadcast).  Two lanes of a group conflict only where their zz differ by a
//           multiple of 32, i.e. n_in / n_out > 1 along z: 2-way up to a ratio of 2, which is one extra LDS cycle on a read that feeds eight
//           float64 divisions.  (An even pitch would put every second row on the same bank; a power of two all of them.)  The byte tiles are
//           read as `ds_read_u8`, four rows' bytes per dword: lanes with equal dword broadcast, the others are at most 2-way by the same argument.
// Every output element is written once, by one thread; no floating-point atomics anywhere in this file: two runs give identical bytes.
#include "radix_select.h"

namespace {

constexpr int SP_THREADS = 256, SP_MAX_BLOCKS = 1024, SP_MAX_C = 16, SP_MAX_K = 7;
constexpr int SP_TILE = 32, SP_LDS_BUDGET = 40 * 1024;
constexpr unsigned long long SP_BOX_EMPTY = 0x7fffffffull;

__device__ __forceinline__ int sp_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ bool sp_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool sp_finite(int16_t) { return true; }

// ---- scan ---------------------------------------------------------------------------------------------------------------------------
// rec: [x0, x1, y0, y1, z0, z1, count, non-finite], the box half-open; empty: x0 = y0 = z0 = 0x7fffffff, x1 = y1 = z1 = 0
__global__ void sp_scan_init_kernel(unsigned long long* __restrict__ rec) {
  const int t = threadIdx.x;
  if (t < 8) rec[t] = (t < 6 && !(t & 1)) ? SP_BOX_EMPTY : 0ull;
}

template <typename T>
__global__ void __launch_bounds__(SP_THREADS) sp_scan_kernel(const T* __restrict__ src, int C, int X, int Y, int64_t V, unsigned long long* __restrict__ rec) {
  __shared__ int red[SP_THREADS / 64][8];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {0, 0, 0};
  unsigned cnt = 0, bad = 0;      // per thread at most V * C / 256 < 2^27
  for (int64_t v = (int64_t)blockIdx.x * SP_THREADS + t; v < V; v += (int64_t)gridDim.x * SP_THREADS) {
    bool nz = false;
    for (int c = 0; c < C; ++c) {
      const T s = src[(int64_t)c * V + v];
      nz = nz || ((float)s != 0.0f);
      bad += sp_finite(s) ? 0u : 1u;
    }
    if (nz) {
      const int x = (int)(v % X);
      const int64_t r = v / X;
      const int p[3] = {x, (int)(r % Y), (int)(r / Y)};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = p[a] < lo[a] ? p[a] : lo[a];
        hi[a] = p[a] + 1 > hi[a] ? p[a] + 1 : hi[a];
      }
      ++cnt;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int l = wave_min(lo[a]), h = wave_max(hi[a]);
    if (lane == 0) {
      red[wid][2 * a] = l;
      red[wid][2 * a + 1] = h;
    }
  }
  cnt = wave_sum(cnt);
  bad = wave_sum(bad);
  if (lane == 0) {
    red[wid][6] = (int)cnt;
    red[wid][7] = (int)bad;
  }
  __syncthreads();
  if (t < 6) {
    int v = red[0][t];
    for (int w = 1; w < SP_THREADS / 64; ++w) v = (t & 1) ? (red[w][t] > v ? red[w][t] : v) : (red[w][t] < v ? red[w][t] : v);
    if (t & 1) {
      if (v > 0) atomicMax(&rec[t], (unsigned long long)v);
    } else if (v != 0x7fffffff) {
      atomicMin(&rec[t], (unsigned long long)v);
    }
  } else if (t < 8) {
    unsigned long long v = 0;
    for (int w = 0; w < SP_THREADS / 64; ++w) v += (unsigned)red[w][t];
    if (v) atomicAdd(&rec[t], v);
  }
}

// ---- stats --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sp_clip(double v, double lo, double hi) {
  v = v < lo ? lo : v;      // numpy's clip: minimum(maximum(v, lo), hi)
  return v > hi ? hi : v;
}

// PASS 0: sum(x); PASS 1: sum((x - mean)^2) with mean = stats[c][0].  partial [gridDim.x][C].
template <typename T, int PASS>
__global__ void __launch_bounds__(SP_THREADS) sp_sum_kernel(const T* __restrict__ src, int C, int64_t V, int use_mask, const double* __restrict__ clip,
                                                           const double* __restrict__ stats, double* __restrict__ partial) {
  __shared__ double red[SP_THREADS / 64];
  double acc[SP_MAX_C], mean[SP_MAX_C], lo[SP_MAX_C], hi[SP_MAX_C];
#pragma unroll
  for (int c = 0; c < SP_MAX_C; ++c) {
    acc[c] = 0.0;
    mean[c] = (PASS == 1 && c < C) ? stats[2 * c] : 0.0;
    lo[c] = (clip && c < C) ? clip[2 * c] : -__builtin_inf();
    hi[c] = (clip && c < C) ? clip[2 * c + 1] : __builtin_inf();
  }
  for (int64_t v = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * SP_THREADS) {
    float f[SP_MAX_C];
    bool nz = false;
#pragma unroll
    for (int c = 0; c < SP_MAX_C; ++c) {
      f[c] = c < C ? (float)src[(int64_t)c * V + v] : 0.0f;
      nz = nz || (f[c] != 0.0f);
    }
    if (use_mask && !nz) continue;
#pragma unroll
    for (int c = 0; c < SP_MAX_C; ++c) {
      const double x = sp_clip((double)f[c], lo[c], hi[c]);
      if (PASS == 0) {
        acc[c] = acc[c] + x;
      } else {
        const double d = x - mean[c];
        acc[c] = acc[c] + d * d;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < SP_MAX_C; ++c) {
    if (c < C) {      // uniform
      const double s = block_sum_256(acc[c], red);
      if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * C + c] = s;
    }
  }
}

// one block; thread c adds channel c's partials in block order.  n = rec[6] (use_mask) or V.
template <int PASS>
__global__ void sp_sum_final_kernel(const double* __restrict__ partial, int nb, int C, int64_t V, int use_mask, const unsigned long long* __restrict__ rec,
                                    double* __restrict__ stats) {
  const int c = threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s = s + partial[(int64_t)b * C + c];
  const double n = use_mask ? (double)rec[6] : (double)V;
  if (PASS == 0) stats[2 * c] = n > 0.0 ? s / n : 0.0;
  else stats[2 * c + 1] = n > 0.0 ? sqrt(s / n) : 0.0;
}

// ---- select -------------------------------------------------------------------------------------------------------------------------
using SpSel = RadixSelect<uint32_t, 4>;

__device__ __forceinline__ unsigned sp_key(float v) {
  unsigned b = __float_as_uint(v);
  if (v == 0.0f) b = 0u;      // -0.0 and +0.0 are one value
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ void sp_sel_init_kernel(SpSel* __restrict__ st, long long r0, long long r1, long long r2, long long r3) {
  const int t = threadIdx.x;
  for (int i = t; i < 4 * 256; i += blockDim.x) (&st->hist[0][0])[i] = 0ull;
  if (t < 4) {
    st->rank[t] = (unsigned long long)(t == 0 ? r0 : t == 1 ? r1 : t == 2 ? r2 : r3);
    st->prefix[t] = 0u;
  }
}

template <typename T>
__global__ void __launch_bounds__(SP_THREADS) sp_hist_kernel(const T* __restrict__ src, int C, int ch, int64_t V, int use_mask, int pass, SpSel* __restrict__ st) {
  __shared__ unsigned h[4 * 256];
  RadixPass<uint32_t, 4, SP_THREADS> rp;
  rp.begin(st, pass, h);
  for (int64_t v = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * SP_THREADS) {
    if (use_mask) {
      bool nz = false;
      for (int c = 0; c < C; ++c) nz = nz || ((float)src[(int64_t)c * V + v] != 0.0f);
      if (!nz) continue;
    }
    rp.add(sp_key((float)src[(int64_t)ch * V + v]));
  }
  rp.flush(st);
}

// one block of 64 threads; thread r < 4 picks rank r, and after the last pass turns its key back into the value
__global__ void sp_sel_pick_kernel(SpSel* __restrict__ st, int pass, float* __restrict__ out) {
  const int r = threadIdx.x;
  if (r >= 4) return;
  const uint32_t pre = radix_pick(st, r);
  if (pass == SpSel::PASSES - 1) out[r] = sp_unkey(pre);
}

// ---- resample -----------------------------------------------------------------------------------------------------------------------
struct SpGeom {
  int X, Y, Z;          // the source volume
  int bx, by, bz;       // the box's first voxel
  int NX, NY, NZ;       // the box's extents: the tables index [0, N)
  int OX, OY, OZ;       // the output
  int TX, TZ;           // output tile
  int SXcap, SZcap, pitch;
  int C, use_mask, has_lab;
};

// float64 -> float16 with ONE rounding (see the file header)
__device__ __forceinline__ _Float16 sp_to_half(double d) {
  float f = (float)d;
  if ((double)f != d) {      // inexact (a NaN also comes here and stays a NaN: both comparisons are false, the last bit is set)
    unsigned b = __float_as_uint(f);
    if (__builtin_fabs((double)f) > __builtin_fabs(d)) b -= 1u;      // towards zero (also from +-inf to the largest finite)
    f = __uint_as_float(b | 1u);
  }
  return (_Float16)f;
}
__device__ __forceinline__ void sp_store(float* p, double v) { *p = (float)v; }
__device__ __forceinline__ void sp_store(_Float16* p, double v) { *p = sp_to_half(v); }

// grid = OY * ceil(OX / TX) * ceil(OZ / TZ) blocks (y fastest: neighbouring blocks share a source row); dynamic LDS: see sp_lds_bytes.
// tab_i int32: i0, i1, nn of x [3 OX], of y [3 OY], of z [3 OZ]; tab_w float64: w0, w1 of x [2 OX], of y [2 OY], of z [2 OZ].
template <typename T, typename O>
__global__ void __launch_bounds__(SP_THREADS) sp_resample_kernel(const T* __restrict__ src, const uint8_t* __restrict__ src_lab, const int32_t* __restrict__ tab_i,
                                                                const double* __restrict__ tab_w, const double* __restrict__ stats,
                                                                const double* __restrict__ clip, const uint8_t* __restrict__ region, O* __restrict__ img,
                                                                uint8_t* __restrict__ lab, SpGeom g) {
  extern __shared__ __align__(16) float sp_smem[];
  const int t = threadIdx.x;
  const int plane = g.SZcap * g.pitch;
  float* tile = sp_smem;
  uint8_t* mtile = reinterpret_cast<uint8_t*>(sp_smem + 2 * plane);
  uint8_t* ltile = mtile + (g.use_mask ? 2 * plane : 0);

  const int oy = blockIdx.x % g.OY;
  const int rest = blockIdx.x / g.OY;
  const int ntz = (g.OZ + g.TZ - 1) / g.TZ;
  const int ox0 = (rest / ntz) * g.TX, oz0 = (rest % ntz) * g.TZ;
  const int nox = g.OX - ox0 < g.TX ? g.OX - ox0 : g.TX, noz = g.OZ - oz0 < g.TZ ? g.OZ - oz0 : g.TZ;
  if (ox0 >= g.OX || nox < 1 || noz < 1) return;      // uniform; a grid larger than the tiling

  const int32_t *tix = tab_i, *tiy = tab_i + 3 * (int64_t)g.OX, *tiz = tiy + 3 * (int64_t)g.OY;
  const double *twx = tab_w, *twy = tab_w + 2 * (int64_t)g.OX, *twz = twy + 2 * (int64_t)g.OY;
  // the staged span: from the first i0 to the last i1 of the tile, clamped to the box and to the LDS that was sized for it
  const int xlo = sp_clampi(tix[ox0], 0, g.NX - 1), zlo = sp_clampi(tiz[oz0], 0, g.NZ - 1);
  int SX = sp_clampi(tix[g.OX + ox0 + nox - 1], 0, g.NX - 1) - xlo + 1, SZ = sp_clampi(tiz[g.OZ + oz0 + noz - 1], 0, g.NZ - 1) - zlo + 1;
  SX = sp_clampi(SX, 1, g.SXcap < g.NX - xlo ? g.SXcap : g.NX - xlo);
  SZ = sp_clampi(SZ, 1, g.SZcap < g.NZ - zlo ? g.SZcap : g.NZ - zlo);
  const int jy[2] = {sp_clampi(tiy[oy], 0, g.NY - 1), sp_clampi(tiy[g.OY + oy], 0, g.NY - 1)};
  const int jn = sp_clampi(tiy[2 * g.OY + oy], 0, g.NY - 1);
  const int64_t V = (int64_t)g.X * g.Y * g.Z;
  const int64_t OV = (int64_t)g.OX * g.OY * g.OZ;
  const int items = 2 * SZ * SX;

  // ---- mask and label tiles
  if (g.use_mask) {
    for (int it = t; it < items; it += SP_THREADS) {
      const int xx = it % SX, r = it / SX, zz = r % SZ, yy = r / SZ;
      const int64_t a = ((int64_t)(g.bz + zlo + zz) * g.Y + (g.by + jy[yy])) * g.X + (g.bx + xlo + xx);
      bool nz = false;
      for (int c = 0; c < g.C; ++c) nz = nz || ((float)src[(int64_t)c * V + a] != 0.0f);
      mtile[(yy * g.SZcap + zz) * g.pitch + xx] = nz ? 1 : 0;
    }
  }
  if (g.has_lab) {
    for (int it = t; it < SZ * SX; it += SP_THREADS) {
      const int xx = it % SX, zz = it / SX;
      ltile[zz * g.pitch + xx] = src_lab[((int64_t)(g.bz + zlo + zz) * g.Y + (g.by + jn)) * g.X + (g.bx + xlo + xx)];
    }
  }
  __syncthreads();
  for (int it = t; it < nox * g.TZ; it += SP_THREADS) {
    const int oz_l = it % g.TZ, ox_l = it / g.TZ;
    if (oz_l >= noz) continue;
    const int ox = ox0 + ox_l, oz = oz0 + oz_l;
    uint8_t out = 0;
    if (g.has_lab) {
      const int xx = sp_clampi(sp_clampi(tix[2 * g.OX + ox], 0, g.NX - 1) - xlo, 0, SX - 1);
      const int zz = sp_clampi(sp_clampi(tiz[2 * g.OZ + oz], 0, g.NZ - 1) - zlo, 0, SZ - 1);
      out = region[ltile[zz * g.pitch + xx]];
    }
    lab[((int64_t)ox * g.OY + oy) * g.OZ + oz] = out;
  }

  // ---- the channels, one after the other through the float tile
  for (int c = 0; c < g.C; ++c) {
    __syncthreads();      // the previous channel's drain is done with the tile
    const T* s = src + (int64_t)c * V;
    for (int it = t; it < items; it += SP_THREADS) {
      const int xx = it % SX, r = it / SX, zz = r % SZ, yy = r / SZ;
      tile[(yy * g.SZcap + zz) * g.pitch + xx] = (float)s[((int64_t)(g.bz + zlo + zz) * g.Y + (g.by + jy[yy])) * g.X + (g.bx + xlo + xx)];
    }
    __syncthreads();
    const double mean = stats ? stats[2 * c] : 0.0;
    const double sd0 = stats ? stats[2 * c + 1] : 1.0;
    const double sd = sd0 > 1e-8 ? sd0 : 1e-8;
    const double lo = clip ? clip[2 * c] : -__builtin_inf(), hi = clip ? clip[2 * c + 1] : __builtin_inf();
    const double wy[2] = {twy[oy], twy[g.OY + oy]};
    for (int it = t; it < nox * g.TZ; it += SP_THREADS) {
      const int oz_l = it % g.TZ, ox_l = it / g.TZ;
      if (oz_l >= noz) continue;
      const int ox = ox0 + ox_l, oz = oz0 + oz_l;
      const int xx[2] = {sp_clampi(sp_clampi(tix[ox], 0, g.NX - 1) - xlo, 0, SX - 1), sp_clampi(sp_clampi(tix[g.OX + ox], 0, g.NX - 1) - xlo, 0, SX - 1)};
      const int zz[2] = {sp_clampi(sp_clampi(tiz[oz], 0, g.NZ - 1) - zlo, 0, SZ - 1), sp_clampi(sp_clampi(tiz[g.OZ + oz], 0, g.NZ - 1) - zlo, 0, SZ - 1)};
      const double wx[2] = {twx[ox], twx[g.OX + ox]}, wz[2] = {twz[oz], twz[g.OZ + oz]};
      double acc = 0.0;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const int idx = (b * g.SZcap + zz[d]) * g.pitch + xx[a];
            double u = (sp_clip((double)tile[idx], lo, hi) - mean) / sd;
            if (g.use_mask && !mtile[idx]) u = 0.0;
            acc = acc + ((u * wx[a]) * wy[b]) * wz[d];
          }
      sp_store(img + (int64_t)c * OV + ((int64_t)ox * g.OY + oy) * g.OZ + oz, acc);
    }
  }
}

// the tile and its LDS for given sizes: a function of the sizes alone
inline void sp_plan(SpGeom& g) {
  g.TX = g.TZ = SP_TILE;
  for (;;) {
    const int64_t sx = ((int64_t)(g.TX - 1) * g.NX + g.OX - 1) / g.OX + 3, sz = ((int64_t)(g.TZ - 1) * g.NZ + g.OZ - 1) / g.OZ + 3;
    g.SXcap = (int)(sx < g.NX ? sx : g.NX);
    g.SZcap = (int)(sz < g.NZ ? sz : g.NZ);
    g.pitch = g.SXcap | 1;
    const int64_t bytes = (int64_t)g.SZcap * g.pitch * (8 + (g.use_mask ? 2 : 0) + 1);
    if (bytes <= SP_LDS_BUDGET || (g.TX == 1 && g.TZ == 1)) return;
    if ((g.SXcap >= g.SZcap && g.TX > 1) || g.TZ == 1) g.TX >>= 1;
    else g.TZ >>= 1;
  }
}
inline size_t sp_lds_bytes(const SpGeom& g) {
  const size_t plane = (size_t)g.SZcap * g.pitch;
  return ((plane * (8 + (g.use_mask ? 2 : 0) + 1)) + 15) & ~(size_t)15;
}

// ---- restore ------------------------------------------------------------------------------------------------------------------------
// tab int32: nn of x [NX], of y [NY], of z [NZ] -- prepared indices for the box's voxels
__global__ void __launch_bounds__(SP_THREADS) sp_restore_kernel(const uint8_t* __restrict__ pred, int PX, int PY, int PZ, const int32_t* __restrict__ tab, int bx, int by,
                                                               int bz, int NX, int NY, int NZ, const uint8_t* __restrict__ paint, uint8_t* __restrict__ out,
                                                               uint8_t* __restrict__ painted, int X, int Y, int Z) {
  const int64_t V = (int64_t)X * Y * Z;
  for (int64_t v = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; v < V; v += (int64_t)gridDim.x * SP_THREADS) {
    const int z = (int)(v % Z);
    const int64_t r = v / Z;
    const int y = (int)(r % Y), x = (int)(r / Y);
    const int lx = x - bx, ly = y - by, lz = z - bz;
    uint8_t m = 0;
    if (lx >= 0 && lx < NX && ly >= 0 && ly < NY && lz >= 0 && lz < NZ) {
      const int px = sp_clampi(tab[lx], 0, PX - 1), py = sp_clampi(tab[NX + ly], 0, PY - 1), pz = sp_clampi(tab[NX + NY + lz], 0, PZ - 1);
      m = pred[((int64_t)px * PY + py) * PZ + pz];
    }
    out[v] = m;
    if (painted) painted[v] = paint[m];
  }
}

inline bool sp_grid_ok(int X, int Y, int Z) { return X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y * Z < ((int64_t)1 << 31); }

}  // namespace

extern "C" int pcrl_segprep_scan(const void* src, int src_kind, int C, int X, int Y, int Z, int64_t* rec, pcrl_stream_t stream) {
  PCRL_REQUIRE(src_kind == 0 || src_kind == 1, "segprep_scan: src_kind %d (0: int16, 1: float32)", src_kind);
  PCRL_REQUIRE(C >= 1 && C <= SP_MAX_C, "segprep_scan: C = %d channels (1..%d)", C, SP_MAX_C);
  PCRL_REQUIRE(sp_grid_ok(X, Y, Z), "segprep_scan: volume %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", X, Y, Z);
  PCRL_REQUIRE(src && rec, "segprep_scan: null pointer");
  const int64_t V = (int64_t)X * Y * Z;
  PCRL_REQUIRE(!ranges_overlap(src, (size_t)V * C * (src_kind ? 4 : 2), rec, 64), "segprep_scan: rec overlaps src");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(rec) % 8 == 0, "segprep_scan: rec must be 8-byte aligned");
  hipStream_t s = as_stream(stream);
  unsigned long long* r = reinterpret_cast<unsigned long long*>(rec);
  hipLaunchKernelGGL(sp_scan_init_kernel, dim3(1), dim3(64), 0, s, r);
  if (src_kind) hipLaunchKernelGGL(sp_scan_kernel<float>, dim3(capped_blocks(V, SP_THREADS, SP_MAX_BLOCKS)), dim3(SP_THREADS), 0, s, static_cast<const float*>(src), C, X, Y, V, r);
  else hipLaunchKernelGGL(sp_scan_kernel<int16_t>, dim3(capped_blocks(V, SP_THREADS, SP_MAX_BLOCKS)), dim3(SP_THREADS), 0, s, static_cast<const int16_t*>(src), C, X, Y, V, r);
  return pcrl_check_launch("segprep_scan");
}

extern "C" size_t pcrl_segprep_stats_ws_bytes(int C, int64_t V) {
  if (C < 1 || C > SP_MAX_C || V < 1) return 0;
  return (size_t)capped_blocks(V, SP_THREADS, SP_MAX_BLOCKS) * C * sizeof(double);
}

extern "C" int pcrl_segprep_stats(const void* src, int src_kind, int C, int X, int Y, int Z, int use_mask, const int64_t* rec, const double* clip,
                                  double* stats, void* ws, size_t ws_bytes, pcrl_stream_t stream) {
  PCRL_REQUIRE(src_kind == 0 || src_kind == 1, "segprep_stats: src_kind %d (0: int16, 1: float32)", src_kind);
  PCRL_REQUIRE(C >= 1 && C <= SP_MAX_C, "segprep_stats: C = %d channels (1..%d)", C, SP_MAX_C);
  PCRL_REQUIRE(sp_grid_ok(X, Y, Z), "segprep_stats: volume %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", X, Y, Z);
  PCRL_REQUIRE(src && stats && (rec || !use_mask), "segprep_stats: null pointer");
  const int64_t V = (int64_t)X * Y * Z;
  const size_t nsrc = (size_t)V * C * (src_kind ? 4 : 2);
  PCRL_REQUIRE(!ranges_overlap(src, nsrc, stats, (size_t)C * 16) && !ranges_overlap(src, nsrc, ws, ws_bytes) && !ranges_overlap(stats, (size_t)C * 16, ws, ws_bytes),
               "segprep_stats: overlapping buffers");
  if (!ws || ws_bytes < pcrl_segprep_stats_ws_bytes(C, V)) return pcrl_fail(PCRL_EWORKSPACE, "segprep_stats: workspace too small");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0 && reinterpret_cast<uintptr_t>(stats) % 8 == 0, "segprep_stats: stats and ws must be 8-byte aligned");
  hipStream_t s = as_stream(stream);
  const int nb = capped_blocks(V, SP_THREADS, SP_MAX_BLOCKS);
  double* partial = static_cast<double*>(ws);
  const unsigned long long* r = reinterpret_cast<const unsigned long long*>(rec);
  if (src_kind) {
    const float* p = static_cast<const float*>(src);
    hipLaunchKernelGGL((sp_sum_kernel<float, 0>), dim3(nb), dim3(SP_THREADS), 0, s, p, C, V, use_mask, clip, stats, partial);
    hipLaunchKernelGGL(sp_sum_final_kernel<0>, dim3(1), dim3(64), 0, s, partial, nb, C, V, use_mask, r, stats);
    hipLaunchKernelGGL((sp_sum_kernel<float, 1>), dim3(nb), dim3(SP_THREADS), 0, s, p, C, V, use_mask, clip, stats, partial);
  } else {
    const int16_t* p = static_cast<const int16_t*>(src);
    hipLaunchKernelGGL((sp_sum_kernel<int16_t, 0>), dim3(nb), dim3(SP_THREADS), 0, s, p, C, V, use_mask, clip, stats, partial);
    hipLaunchKernelGGL(sp_sum_final_kernel<0>, dim3(1), dim3(64), 0, s, partial, nb, C, V, use_mask, r, stats);
    hipLaunchKernelGGL((sp_sum_kernel<int16_t, 1>), dim3(nb), dim3(SP_THREADS), 0, s, p, C, V, use_mask, clip, stats, partial);
  }
  hipLaunchKernelGGL(sp_sum_final_kernel<1>, dim3(1), dim3(64), 0, s, partial, nb, C, V, use_mask, r, stats);
  return pcrl_check_launch("segprep_stats");
}

extern "C" size_t pcrl_segprep_select_ws_bytes(void) { return sizeof(SpSel); }

extern "C" int pcrl_segprep_select(const void* src, int src_kind, int C, int ch, int X, int Y, int Z, int use_mask, int64_t r0, int64_t r1, int64_t r2,
                                   int64_t r3, float* out, void* ws, size_t ws_bytes, pcrl_stream_t stream) {
  PCRL_REQUIRE(src_kind == 0 || src_kind == 1, "segprep_select: src_kind %d (0: int16, 1: float32)", src_kind);
  PCRL_REQUIRE(C >= 1 && C <= SP_MAX_C, "segprep_select: C = %d channels (1..%d)", C, SP_MAX_C);
  PCRL_REQUIRE(ch >= 0 && ch < C, "segprep_select: channel %d of %d", ch, C);
  PCRL_REQUIRE(sp_grid_ok(X, Y, Z), "segprep_select: volume %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", X, Y, Z);
  const int64_t V = (int64_t)X * Y * Z;
  PCRL_REQUIRE(r0 >= 0 && r1 >= 0 && r2 >= 0 && r3 >= 0 && r0 < V && r1 < V && r2 < V && r3 < V, "segprep_select: a rank outside [0, %lld)", (long long)V);
  PCRL_REQUIRE(src && out, "segprep_select: null pointer");
  if (!ws || ws_bytes < sizeof(SpSel)) return pcrl_fail(PCRL_EWORKSPACE, "segprep_select: workspace too small");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0, "segprep_select: ws must be 8-byte, out 4-byte aligned");
  const size_t nsrc = (size_t)V * C * (src_kind ? 4 : 2);
  PCRL_REQUIRE(!ranges_overlap(src, nsrc, out, 16) && !ranges_overlap(src, nsrc, ws, ws_bytes) && !ranges_overlap(out, 16, ws, ws_bytes), "segprep_select: overlapping buffers");
  hipStream_t s = as_stream(stream);
  SpSel* st = static_cast<SpSel*>(ws);
  const int nb = capped_blocks(V, SP_THREADS, SP_MAX_BLOCKS);
  hipLaunchKernelGGL(sp_sel_init_kernel, dim3(1), dim3(256), 0, s, st, (long long)r0, (long long)r1, (long long)r2, (long long)r3);
  for (int pass = 0; pass < SpSel::PASSES; ++pass) {
    if (src_kind) hipLaunchKernelGGL(sp_hist_kernel<float>, dim3(nb), dim3(SP_THREADS), 0, s, static_cast<const float*>(src), C, ch, V, use_mask, pass, st);
    else hipLaunchKernelGGL(sp_hist_kernel<int16_t>, dim3(nb), dim3(SP_THREADS), 0, s, static_cast<const int16_t*>(src), C, ch, V, use_mask, pass, st);
    hipLaunchKernelGGL(sp_sel_pick_kernel, dim3(1), dim3(64), 0, s, st, pass, out);
  }
  return pcrl_check_launch("segprep_select");
}

static int sp_resample_geom(const char* who, int C, int X, int Y, int Z, int bx, int by, int bz, int NX, int NY, int NZ, int OX, int OY, int OZ, int use_mask,
                            int has_lab, SpGeom* g) {
  PCRL_REQUIRE(C >= 1 && C <= SP_MAX_C, "%s: C = %d channels (1..%d)", who, C, SP_MAX_C);
  PCRL_REQUIRE(sp_grid_ok(X, Y, Z), "%s: source %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", who, X, Y, Z);
  PCRL_REQUIRE(sp_grid_ok(OX, OY, OZ), "%s: output %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", who, OX, OY, OZ);
  PCRL_REQUIRE(NX >= 1 && NY >= 1 && NZ >= 1 && bx >= 0 && by >= 0 && bz >= 0 && (int64_t)bx + NX <= X && (int64_t)by + NY <= Y && (int64_t)bz + NZ <= Z,
               "%s: box [%d, +%d) x [%d, +%d) x [%d, +%d) is empty or outside the volume %d x %d x %d", who, bx, NX, by, NY, bz, NZ, X, Y, Z);
  *g = SpGeom{X, Y, Z, bx, by, bz, NX, NY, NZ, OX, OY, OZ, 0, 0, 0, 0, 0, C, use_mask ? 1 : 0, has_lab ? 1 : 0};
  sp_plan(*g);
  return 0;
}

extern "C" int pcrl_segprep_resample_tile(int NX, int NZ, int OX, int OZ, int use_mask, int* tx, int* tz, int64_t* lds_bytes) {
  SpGeom g;
  const int rc = sp_resample_geom("segprep_resample_tile", 1, NX, 1, NZ, 0, 0, 0, NX, 1, NZ, OX, 1, OZ, use_mask, 1, &g);
  if (rc) return rc;
  if (tx) *tx = g.TX;
  if (tz) *tz = g.TZ;
  if (lds_bytes) *lds_bytes = (int64_t)sp_lds_bytes(g);
  return 0;
}

extern "C" int pcrl_segprep_resample(const void* src, int src_kind, const uint8_t* src_lab, int C, int X, int Y, int Z, int bx, int by, int bz, int NX, int NY,
                                     int NZ, const int32_t* tab_i, const double* tab_w, const double* stats, const double* clip, const uint8_t* region,
                                     int K, int use_mask, void* img, int out_half, uint8_t* lab, int OX, int OY, int OZ, pcrl_stream_t stream) {
  PCRL_REQUIRE(src_kind == 0 || src_kind == 1, "segprep_resample: src_kind %d (0: int16, 1: float32)", src_kind);
  PCRL_REQUIRE(out_half == 0 || out_half == 1, "segprep_resample: out_half %d (0: float32, 1: float16)", out_half);
  PCRL_REQUIRE(K >= 1 && K <= SP_MAX_K, "segprep_resample: K = %d regions (1..%d: bit k of a label byte, bit 7 means 'not counted')", K, SP_MAX_K);
  SpGeom g;
  const int rc = sp_resample_geom("segprep_resample", C, X, Y, Z, bx, by, bz, NX, NY, NZ, OX, OY, OZ, use_mask, src_lab != nullptr, &g);
  if (rc) return rc;
  PCRL_REQUIRE(src && tab_i && tab_w && img && lab && (region || !src_lab), "segprep_resample: null pointer");
  const int64_t V = (int64_t)X * Y * Z, OV = (int64_t)OX * OY * OZ;
  const size_t nsrc = (size_t)V * C * (src_kind ? 4 : 2), nimg = (size_t)OV * C * (out_half ? 2 : 4);
  PCRL_REQUIRE(!ranges_overlap(img, nimg, src, nsrc) && !ranges_overlap(img, nimg, src_lab, (size_t)V) && !ranges_overlap(lab, (size_t)OV, src, nsrc) &&
                   !ranges_overlap(lab, (size_t)OV, src_lab, (size_t)V) && !ranges_overlap(img, nimg, lab, (size_t)OV),
               "segprep_resample: img or lab overlaps a source or the other output");
  const size_t nti = (size_t)3 * ((size_t)OX + OY + OZ) * 4, ntw = (size_t)2 * ((size_t)OX + OY + OZ) * 8;
  PCRL_REQUIRE(!ranges_overlap(img, nimg, tab_i, nti) && !ranges_overlap(img, nimg, tab_w, ntw) && !ranges_overlap(lab, (size_t)OV, tab_i, nti) &&
                   !ranges_overlap(lab, (size_t)OV, tab_w, ntw) && !ranges_overlap(img, nimg, stats, (size_t)C * 16) && !ranges_overlap(img, nimg, clip, (size_t)C * 16) &&
                   !ranges_overlap(lab, (size_t)OV, stats, (size_t)C * 16) && !ranges_overlap(lab, (size_t)OV, clip, (size_t)C * 16) &&
                   !ranges_overlap(img, nimg, region, 256) && !ranges_overlap(lab, (size_t)OV, region, 256),
               "segprep_resample: img or lab overlaps a table");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(src) % (src_kind ? 4 : 2) == 0 && reinterpret_cast<uintptr_t>(img) % (out_half ? 2 : 4) == 0 &&
                   reinterpret_cast<uintptr_t>(tab_i) % 4 == 0 && reinterpret_cast<uintptr_t>(tab_w) % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(stats) % 8 == 0 && reinterpret_cast<uintptr_t>(clip) % 8 == 0,
               "segprep_resample: a buffer is not aligned to its element");
  const int64_t blocks = (int64_t)OY * ((OX + g.TX - 1) / g.TX) * ((OZ + g.TZ - 1) / g.TZ);
  PCRL_REQUIRE(blocks <= 0x7fffffff, "segprep_resample: %lld tiles are too many for one launch", (long long)blocks);
  const size_t lds = sp_lds_bytes(g);
  PCRL_REQUIRE(lds <= 64 * 1024, "segprep_resample: a tile of %zu bytes does not fit the LDS", lds);
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)blocks), block(SP_THREADS);
#define SP_LAUNCH(T, O)                                                                                                                              \
  hipLaunchKernelGGL((sp_resample_kernel<T, O>), grid, block, lds, s, static_cast<const T*>(src), src_lab, tab_i, tab_w, stats, clip, region, \
                     static_cast<O*>(img), lab, g)
  if (src_kind && out_half) SP_LAUNCH(float, _Float16);
  else if (src_kind) SP_LAUNCH(float, float);
  else if (out_half) SP_LAUNCH(int16_t, _Float16);
  else SP_LAUNCH(int16_t, float);
#undef SP_LAUNCH
  return pcrl_check_launch("segprep_resample");
}

extern "C" int pcrl_segprep_restore(const uint8_t* pred, int PX, int PY, int PZ, const int32_t* tab, int bx, int by, int bz, int NX, int NY, int NZ,
                                    const uint8_t* paint, uint8_t* out, uint8_t* painted, int X, int Y, int Z, pcrl_stream_t stream) {
  PCRL_REQUIRE(sp_grid_ok(PX, PY, PZ), "segprep_restore: prepared grid %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", PX, PY, PZ);
  PCRL_REQUIRE(sp_grid_ok(X, Y, Z), "segprep_restore: original grid %d x %d x %d (every extent >= 1, fewer than 2^31 voxels)", X, Y, Z);
  PCRL_REQUIRE(NX >= 1 && NY >= 1 && NZ >= 1 && bx >= 0 && by >= 0 && bz >= 0 && (int64_t)bx + NX <= X && (int64_t)by + NY <= Y && (int64_t)bz + NZ <= Z,
               "segprep_restore: box [%d, +%d) x [%d, +%d) x [%d, +%d) is empty or outside the volume %d x %d x %d", bx, NX, by, NY, bz, NZ, X, Y, Z);
  PCRL_REQUIRE(pred && tab && out && (paint || !painted), "segprep_restore: null pointer");
  const size_t V = (size_t)X * Y * Z, PV = (size_t)PX * PY * PZ, nt = ((size_t)NX + NY + NZ) * 4;
  PCRL_REQUIRE(!ranges_overlap(out, V, pred, PV) && !ranges_overlap(out, V, tab, nt) && !ranges_overlap(out, V, paint, 256) && !ranges_overlap(painted, V, pred, PV) &&
                   !ranges_overlap(painted, V, tab, nt) && !ranges_overlap(painted, V, paint, 256) && !ranges_overlap(out, V, painted, V),
               "segprep_restore: overlapping buffers");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(tab) % 4 == 0, "segprep_restore: tab must be 4-byte aligned");
  hipLaunchKernelGGL(sp_restore_kernel, dim3(capped_blocks((int64_t)V, SP_THREADS, SP_MAX_BLOCKS)), dim3(SP_THREADS), 0, as_stream(stream), pred, PX, PY, PZ, tab, bx, by, bz, NX, NY, NZ, paint,
                     out, painted, X, Y, Z);
  return pcrl_check_launch("segprep_restore");
}
