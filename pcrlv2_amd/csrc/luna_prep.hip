// LUNA16 pre-processing of the reference's luna_preprocess.py as gfx950 kernels (host side: pcrlv2_amd/luna_prep.py):
//
//   load_sitk_with_resample (SimpleITK ResampleImageFilter, identity transform, linear, output spacing 1 mm)
//       -> pcrl_prep_resample (one thread per output voxel, int16 in, int16 out)
//   HU window + crop + skimage.transform.resize(order=1, mode='reflect', preserve_range=True) + the depth-map score
//       -> pcrl_prep_windows: per batch of W window records,
//          norm    : normalised crop into workspace buffer A ([sz][sy][sx], x fastest like the volume) + the crop's raw min / max
//          filter  : the anti-aliasing Gaussian along x, y, z (ping-pong A <-> B; an axis with radius 0 is skipped)
//          zoom    : one thread per (i, j) output column: order-1 zoom, clip, store, and the exact integer depth score
//
// Built with -ffp-contract=off (pcrlv2_amd/build.py): every double expression rounds in the order scipy's / ITK's C code does, so the
// outputs are bit-identical to the float64 restatement (tests/luna_prep_reference.py).  Every weight or coordinate that needs exp() or a
// division of sizes comes in from the host; the only device divisions are ITK's (o * 1.0) / spacing and the HU scaling.  Reductions are
// integer (min, max, sum): deterministic.
#include "common.h"

#include <climits>

namespace {

enum { R_X0 = 0, R_Y0, R_Z0, R_SX, R_SY, R_SZ, R_OX, R_OY, R_OZ, R_RX, R_RY, R_RZ, R_OUT, R_SD, R_WS, R_SCORED, R_COUNT };
static_assert(R_COUNT == PCRL_PREP_NREC, "pcrl_hip.h and luna_prep.hip disagree on the window record");
constexpr int RMAX = PCRL_PREP_RMAX;
constexpr int P_RATIO = 3 * (RMAX + 1);
static_assert(P_RATIO + 3 <= PCRL_PREP_NPRM, "window parameter record too small");

constexpr double HU_MIN = -1000.0, HU_MAX = 1000.0;
constexpr double HU_THRED = (-150.0 - HU_MIN) / (HU_MAX - HU_MIN);   // luna_preprocess.py:66

__device__ __forceinline__ double normalise(int v) {
  double x = (double)v;
  x = x < HU_MIN ? HU_MIN : x > HU_MAX ? HU_MAX : x;
  return 1.0 * (x - HU_MIN) / (HU_MAX - HU_MIN);
}

__device__ __forceinline__ int mirror(int i, int n) {     // scipy.ndimage mode 'mirror'
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i = (i < 0 ? -i : i) % p;
  return i >= n ? p - i : i;
}

// ---- ITK linear resample to 1 mm ----
__device__ __forceinline__ void lerp_axis(int o, int n, double spacing, bool& inside, int& f0, int& f1, double& t) {
  const double ci = ((double)o * 1.0) / spacing;
  inside = ci < (double)n - 0.5;
  f0 = (int)floor(ci);
  if (f0 > n - 1) f0 = n - 1;
  f1 = f0 + 1 < n ? f0 + 1 : n - 1;
  t = ci - (double)f0;
}

__global__ void __launch_bounds__(256) resample_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out, int X, int Y, int Z,
                                                       int OX, int OY, int OZ, double spx, double spy, double spz) {
  const int64_t total = (int64_t)OX * OY * OZ;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int ox = (int)(idx % OX);
    const int64_t r = idx / OX;
    const int oy = (int)(r % OY), oz = (int)(r / OY);
    bool ix, iy, iz;
    int x0, x1, y0, y1, z0, z1;
    double tx, ty, tz;
    lerp_axis(ox, X, spx, ix, x0, x1, tx);
    lerp_axis(oy, Y, spy, iy, y0, y1, ty);
    lerp_axis(oz, Z, spz, iz, z0, z1, tz);
    int16_t res = 0;
    if (ix && iy && iz) {
      auto g = [&](int z, int y, int x) { return (double)in[((int64_t)z * Y + y) * X + x]; };
      const double v000 = g(z0, y0, x0), v100 = g(z0, y0, x1), v010 = g(z0, y1, x0), v110 = g(z0, y1, x1);
      const double v001 = g(z1, y0, x0), v101 = g(z1, y0, x1), v011 = g(z1, y1, x0), v111 = g(z1, y1, x1);
      const double x00 = v000 + (v100 - v000) * tx;
      const double x10 = v010 + (v110 - v010) * tx;
      const double xy0 = x00 + (x10 - x00) * ty;
      const double x01 = v001 + (v101 - v001) * tx;
      const double x11 = v011 + (v111 - v011) * tx;
      const double xy1 = x01 + (x11 - x01) * ty;
      double v = xy0 + (xy1 - xy0) * tz;
      v = v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v;
      res = (int16_t)(int)v;
    }
    out[idx] = res;
  }
}

// ---- windows ----
__global__ void init_stats_kernel(int* __restrict__ stats, int W) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) {
    stats[3 * w] = 0;
    stats[3 * w + 1] = INT_MAX;
    stats[3 * w + 2] = INT_MIN;
  }
}

__global__ void __launch_bounds__(256) norm_kernel(const int16_t* __restrict__ vol, int X, int Y, int Z, const int64_t* __restrict__ rec,
                                                   int* __restrict__ stats, double* __restrict__ ws, int64_t ws_len) {
  const int w = blockIdx.y;
  const int64_t* r = rec + (int64_t)w * PCRL_PREP_NREC;
  const int x0 = (int)r[R_X0], y0 = (int)r[R_Y0], z0 = (int)r[R_Z0];
  const int sx = (int)r[R_SX], sy = (int)r[R_SY], sz = (int)r[R_SZ];
  const int64_t n = (int64_t)sx * sy * sz, base = r[R_WS];
  int lo = INT_MAX, hi = INT_MIN;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % sx);
    const int64_t t = idx / sx;
    const int y = (int)(t % sy), z = (int)(t / sy);
    const int gx = x0 + x, gy = y0 + y, gz = z0 + z;
    const bool in = gx >= 0 && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z;
    const int v = in ? (int)vol[((int64_t)gz * Y + gy) * X + gx] : (int)HU_MIN;   // z beyond the volume: the reference's end pad
    lo = min(lo, v);
    hi = max(hi, v);
    if (base + idx < ws_len) ws[base + idx] = normalise(v);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&stats[3 * w + 1], lo);
    atomicMax(&stats[3 * w + 2], hi);
  }
}

template <int AXIS>
__global__ void __launch_bounds__(256) filter_kernel(const int64_t* __restrict__ rec, const double* __restrict__ prm, double* __restrict__ ws,
                                                     int64_t ws_len) {
  const int w = blockIdx.y;
  const int64_t* r = rec + (int64_t)w * PCRL_PREP_NREC;
  const int rad = (int)r[R_RX + AXIS];
  if (rad <= 0) return;
  const int sx = (int)r[R_SX], sy = (int)r[R_SY], sz = (int)r[R_SZ];
  const int64_t n = (int64_t)sx * sy * sz, base = r[R_WS];
  if (base + 2 * n > ws_len) return;
  const int parity = (AXIS >= 1 && r[R_RX] > 0) + (AXIS >= 2 && r[R_RY] > 0);
  const double* src = ws + base + (parity & 1 ? n : 0);
  double* dst = ws + base + (parity & 1 ? 0 : n);
  const double* c = prm + (int64_t)w * PCRL_PREP_NPRM + AXIS * (RMAX + 1);
  const int L = AXIS == 0 ? sx : AXIS == 1 ? sy : sz;
  const int64_t st = AXIS == 0 ? 1 : AXIS == 1 ? (int64_t)sx : (int64_t)sx * sy;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(idx % sx);
    const int64_t t = idx / sx;
    const int y = (int)(t % sy), z = (int)(t / sy);
    const int p = AXIS == 0 ? x : AXIS == 1 ? y : z;
    const int64_t line = idx - (int64_t)p * st;
    double acc = src[idx] * c[0];
    for (int j = rad; j >= 1; --j)       // scipy's symmetric correlate1d: the farthest pair first
      acc += (src[line + (int64_t)mirror(p - j, L) * st] + src[line + (int64_t)mirror(p + j, L) * st]) * c[j];
    dst[idx] = acc;
  }
}

struct ZoomAxis {
  int i0, i1;
  double w0, w1;
  __device__ ZoomAxis(int o, int n, double ratio) {
    if (n == 1) {
      i0 = i1 = 0;
      w0 = 1.0;
      w1 = 0.0;
      return;
    }
    double cc = ((double)o + 0.5) * ratio - 0.5;
    if (cc < 0.0) cc = -cc;
    const double f = floor(cc);
    const double t = cc - f;
    i0 = (int)f;
    i1 = i0 + 1;
    if (i1 >= n) i1 = 2 * n - 2 - i1;
    w0 = 1.0 - t;
    w1 = 1.0 - w0;
  }
};

__global__ void __launch_bounds__(256) zoom_kernel(const int64_t* __restrict__ rec, const double* __restrict__ prm, const double* __restrict__ ws,
                                                   int64_t ws_len, double* __restrict__ out, int64_t out_len, int* __restrict__ stats) {
  const int w = blockIdx.y;
  const int64_t* r = rec + (int64_t)w * PCRL_PREP_NREC;
  const int sx = (int)r[R_SX], sy = (int)r[R_SY], sz = (int)r[R_SZ];
  const int ox = (int)r[R_OX], oy = (int)r[R_OY], oz = (int)r[R_OZ], sd = (int)r[R_SD], D = (int)r[R_SCORED];
  const int64_t n = (int64_t)sx * sy * sz, obase = r[R_OUT];
  if (r[R_WS] + 2 * n > ws_len) return;
  const int parity = (r[R_RX] > 0) + (r[R_RY] > 0) + (r[R_RZ] > 0);
  const double* F = ws + r[R_WS] + (parity & 1 ? n : 0);
  const double* ratio = prm + (int64_t)w * PCRL_PREP_NPRM + P_RATIO;
  const double lo = normalise(stats[3 * w + 1]), hi = normalise(stats[3 * w + 2]);
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  int score = 0;
  if (col < ox * oy) {
    const int i = col / oy, j = col - (col / oy) * oy;
    const ZoomAxis ax(i, sx, ratio[0]), ay(j, sy, ratio[1]);
    const int xs[2] = {ax.i0, ax.i1}, ys[2] = {ay.i0, ay.i1};
    const double wx[2] = {ax.w0, ax.w1}, wy[2] = {ay.w0, ay.w1};
    double* o = out + obase + (int64_t)col * sd;
    uint64_t ge = 0;
    for (int d = 0; d < oz; ++d) {
      const ZoomAxis az(d, sz, ratio[2]);
      const int zs[2] = {az.i0, az.i1};
      const double wz[2] = {az.w0, az.w1};
      double acc = 0.0;                  // scipy's zoom: corners with the last axis fastest, ((v * wx) * wy) * wz each
#pragma unroll
      for (int b0 = 0; b0 < 2; ++b0)
#pragma unroll
        for (int b1 = 0; b1 < 2; ++b1)
#pragma unroll
          for (int b2 = 0; b2 < 2; ++b2)
            acc += ((F[((int64_t)zs[b2] * sy + ys[b1]) * sx + xs[b0]] * wx[b0]) * wy[b1]) * wz[b2];
      const double v = acc > hi ? hi : acc < lo ? lo : acc;     // np.clip(out, min, max)
      if (d < sd && obase + (int64_t)col * sd + d < out_len) o[d] = v;
      if (v >= HU_THRED) ge |= 1ull << d;
    }
    for (int d = 0; d < D; ++d) {
      if ((ge >> d) & 1ull) score += 2;
      else if ((ge >> (d + 1)) & 1ull) score += 1;
    }
  }
  if (D > 0) {
    score = wave_sum(score);
    if ((threadIdx.x & 63) == 0 && score != 0) atomicAdd(&stats[3 * w], score);
  }
}

}  // namespace

extern "C" int pcrl_prep_resample(const int16_t* in, int16_t* out, int X, int Y, int Z, int OX, int OY, int OZ, double spacing_x,
                                  double spacing_y, double spacing_z, pcrl_stream_t stream) {
  PCRL_REQUIRE(in && out, "prep_resample: null pointer");
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0 && OX > 0 && OY > 0 && OZ > 0, "prep_resample: bad shape");
  PCRL_REQUIRE(spacing_x > 0.0 && spacing_y > 0.0 && spacing_z > 0.0, "prep_resample: spacing must be positive");
  const int64_t total = (int64_t)OX * OY * OZ;
  hipLaunchKernelGGL(resample_kernel, dim3(capped_blocks(total, 256, 8192)), dim3(256), 0, as_stream(stream), in, out, X, Y, Z, OX, OY, OZ, spacing_x,
                     spacing_y, spacing_z);
  return pcrl_check_launch("prep_resample");
}

extern "C" int pcrl_prep_windows(const int16_t* vol, int X, int Y, int Z, const int64_t* rec, const double* prm, int W, int64_t max_src,
                                 int max_cols, double* out, int64_t out_len, int* stats, double* ws, int64_t ws_len, pcrl_stream_t stream) {
  PCRL_REQUIRE(vol && rec && prm && out && stats && ws, "prep_windows: null pointer");
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0 && W > 0 && W <= 65535, "prep_windows: bad shape");
  PCRL_REQUIRE(max_src > 0 && max_cols > 0 && out_len > 0 && ws_len > 0, "prep_windows: bad sizes");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(init_stats_kernel, dim3((W + 255) / 256), dim3(256), 0, s, stats, W);
  const unsigned gs = capped_blocks(max_src, 256, 1024);
  hipLaunchKernelGGL(norm_kernel, dim3(gs, W), dim3(256), 0, s, vol, X, Y, Z, rec, stats, ws, ws_len);
  hipLaunchKernelGGL(filter_kernel<0>, dim3(gs, W), dim3(256), 0, s, rec, prm, ws, ws_len);
  hipLaunchKernelGGL(filter_kernel<1>, dim3(gs, W), dim3(256), 0, s, rec, prm, ws, ws_len);
  hipLaunchKernelGGL(filter_kernel<2>, dim3(gs, W), dim3(256), 0, s, rec, prm, ws, ws_len);
  hipLaunchKernelGGL(zoom_kernel, dim3(capped_blocks(max_cols, 256, 65535), W), dim3(256), 0, s, rec, prm, ws, ws_len, out, out_len, stats);
  return pcrl_check_launch("prep_windows");
}
