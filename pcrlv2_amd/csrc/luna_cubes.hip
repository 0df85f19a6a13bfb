// LUNA16 nodule classification, data side (host: pcrlv2_amd/luna_nodules.py): candidate cubes out of a 1 mm volume.
//
//   pcrl_prep_cubes      vol int16 [Z][Y][X]  ->  out [M][CX][CY][CZ] (z innermost: the pre-task crops' axis order), clipped to the HU window,
//                        int16 or normalised float32; coordinates outside the volume read -1000 (air, the pad value of luna_prep.py)
//   pcrl_prep_hu_to_unit the same normalisation elementwise, for int16 cubes that come from disk
//
// The output's innermost axis is the volume's outermost: the kernel is a transpose of 2-byte elements and goes through LDS.
//
// Tiling.  One 256-thread block = one cube m and JB consecutive y (JB = the largest of 8, 4, 2, 1 with JB * CZ <= 128: 4 at the flagship
// 64 x 64 x 32).  Stage: the JB * CZ rows (y, z) of CX elements are read along x -- the volume's contiguous axis, consecutive lanes on
// consecutive vectors of one row -- with 8-byte loads (four elements) whatever X is: every ROW has its own shift s = (address of
// vol[z][y][x0] in elements) mod 4, which makes its vectors aligned in memory AND in LDS (element t of the row lies at LDS index t + s).
// The shift is the same for every row when X % 4 == 0, alternates between two values when X % 4 == 2 and takes all four when X is odd (a
// resampled series has any X); the drain recomputes it per row, a few integer operations.  Vectors that straddle the cube's or the volume's
// edge are taken element by element.  Drain: a thread gathers 8 consecutive z of one (x, y) column, clips (and normalises) and
// writes ONE 16-byte store (float32: two); consecutive lanes hold consecutive chunks of out[m][i][j0 .. j0 + JB)[0 .. CZ), a contiguous
// run of JB * CZ elements (256 B int16 / 512 B float32 at the flagship shape), then the next i.
//
// LDS pitch.  L = JB * CZ / 8 chunks per x column (16 wherever CZ is a power of two >= 16).  Row (jj, k) of the stage is stored at LDS row
// (k % 8) * L + n, n = jj * CZ / 8 + k / 8: the L rows that the lanes of one column read in the same instruction are ADJACENT.  Pitch
// P = 34 dwords (68 int16: CX + 3 <= 67 fit).  Think in dwords (two int16 share a bank word; 64 banks of 4 bytes, `ds_read_u16` is
// served in two groups of 32 lanes on bank = dword mod 32):
//   drain  a 32-lane group is 2 columns x 16 rows: lane (i, n) reads dword (e * L + n) * 34 + (i + s) / 2.  n * 34 mod 32 = 2 n is even and
//          distinct for n < 16; the two columns share a dword (broadcast) or take d and d + 1: 32 lanes, 32 different banks or the same
//          word.  (With the power-of-two pitch 32 all sixteen rows would sit on ONE bank.)  CZ = 8 has L = 8, four columns per group over up
//          to three dwords: pitch 36 (n * 4 apart).  The depths that are no power of two (24, 40, 48, 56: L = 12, 10, 12, 14) keep pitch 34;
//          a group then straddles up to four columns and can be 2-way.  The above is X % 4 == 0, where every row has the same s.  Otherwise
//          s differs between the rows of one instruction and (i + s) / 2 spans d .. d + 2: bank 2 n + {0, 1, 2}, which two rows can share --
//          at most 2-way.
//   stage  16 lanes of a `ds_write_b64` group (32 of b32 / b16) write consecutive words of one row: conflict-free; a group that straddles
//          the seam of two rows is at most 2-way, which a store does not pay for (its cycles are set by the register transfer).
// The tile is 128 rows x 36 dwords = 18 KB: eight blocks per CU.
//
// No atomics, no workspace; every output element is written once by one thread: deterministic.  Built with -ffp-contract=off
// (pcrlv2_amd/build.py) like luna_prep.hip: float32((double(v) + 1000) / 2000) rounds as numpy's float64 expression does.
#include "common.h"

namespace {

constexpr int HU_LO = -1000, HU_HI = 1000;
constexpr int TILE_ROWS = 128, TILE_PITCH_MAX = 36;   // dwords

__device__ __forceinline__ int clip_hu(int v) { return v < HU_LO ? HU_LO : v > HU_HI ? HU_HI : v; }
__device__ __forceinline__ float unit_of(int v) { return (float)(((double)v + 1000.0) / 2000.0); }

// Shift of the row (y, z): its first element's address, in elements, modulo 4.  Only the residue matters, so unsigned arithmetic that wraps
// is exact, also for rows outside the volume (any value serves there, as long as the stage and the drain agree).
__device__ __forceinline__ int row_shift(uint32_t base, uint32_t x0, int64_t y, int64_t z, int X, int Y) {
  return (int)((base + x0 + ((uint32_t)z * (uint32_t)Y + (uint32_t)y) * (uint32_t)X) & 3u);
}

template <bool F32>
__global__ void __launch_bounds__(256) cubes_kernel(const int16_t* __restrict__ vol, int X, int Y, int Z, const int32_t* __restrict__ start,
                                                    void* __restrict__ out_, int CX, int CY, int CZ, int JB, int P) {
  __shared__ __align__(16) int16_t tile[TILE_ROWS * TILE_PITCH_MAX * 2];
  const int nyb = CY / JB;
  const int m = blockIdx.x / nyb, j0 = (blockIdx.x - m * nyb) * JB;
  // Starts are the caller's: anything an int32 holds.  Coordinates are int64, so a start near INT_MAX or INT_MIN reads air, not overflow.
  const int64_t x0 = start[3 * m], y0 = (int64_t)start[3 * m + 1] + j0, z0 = start[3 * m + 2];
  const uint32_t base = (uint32_t)(reinterpret_cast<uintptr_t>(vol) >> 1);
  const int G = CX / 4 + 1;                   // vectors that cover LDS indices [0, CX + 4) of a row
  const int rows = JB * CZ, kz8 = CZ >> 3, L = JB * kz8, pitch = 2 * P;

  for (int item = threadIdx.x; item < rows * G; item += 256) {
    const int rr = item / G, g = item - rr * G;
    const int jj = rr / CZ, k = rr - jj * CZ;
    const int64_t y = y0 + jj, z = z0 + k;
    const bool row_in = y >= 0 && y < Y && z >= 0 && z < Z;
    const int64_t row = row_in ? (z * Y + y) * X : 0;
    const int s = row_shift(base, (uint32_t)x0, y, z, X, Y);
    int16_t* dst = tile + ((k & 7) * L + jj * kz8 + (k >> 3)) * pitch + g * 4;
    const int t0 = g * 4 - s;
    const int64_t x = x0 + t0;
    if (row_in && t0 >= 0 && t0 + 4 <= CX && x >= 0 && x + 4 <= X) {
      *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(vol + row + x);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = t0 + q;
        const int64_t xx = x + q;
        if (t >= 0 && t < CX) dst[q] = (row_in && xx >= 0 && xx < X) ? vol[row + xx] : (int16_t)HU_LO;
      }
    }
  }
  __syncthreads();

  const int64_t cube = (int64_t)CY * CZ;
  for (int c = threadIdx.x; c < CX * L; c += 256) {
    const int i = c / L, n = c - i * L;
    const int jj = n / kz8, kb = (n - jj * kz8) * 8;
    const int16_t* src = tile + n * pitch + i;
    int v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = clip_hu((int)src[e * L * pitch + row_shift(base, (uint32_t)x0, y0 + jj, z0 + kb + e, X, Y)]);
    const int64_t o = ((int64_t)m * CX + i) * cube + (int64_t)j0 * CZ + n * 8;
    if (F32) {
      float* out = static_cast<float*>(out_) + o;
      Vec16<float> a, b;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a.v[e] = unit_of(v[e]);
        b.v[e] = unit_of(v[4 + e]);
      }
      st16(out, a);
      st16(out + 4, b);
    } else {
      Vec16<int16_t> a;
#pragma unroll
      for (int e = 0; e < 8; ++e) a.v[e] = (int16_t)v[e];
      st16(static_cast<int16_t*>(out_) + o, a);
    }
  }
}

__global__ void __launch_bounds__(256) hu_to_unit_kernel(const int16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
  const int64_t n8 = n >> 3, stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t c = tid; c < n8; c += stride) {
    const Vec16<int16_t> v = ld16(in + 8 * c);
    Vec16<float> a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a.v[e] = unit_of((int)v.v[e]);
      b.v[e] = unit_of((int)v.v[4 + e]);
    }
    st16(out + 8 * c, a);
    st16(out + 8 * c + 4, b);
  }
  for (int64_t idx = 8 * n8 + tid; idx < n; idx += stride) out[idx] = unit_of((int)in[idx]);
}

inline bool cube_side(int c) { return c > 0 && c <= 64 && c % 8 == 0; }

}  // namespace

extern "C" int pcrl_prep_cubes(const int16_t* vol, int X, int Y, int Z, const int32_t* start, int M, void* out, int out_kind, int CX, int CY,
                               int CZ, pcrl_stream_t stream) {
  PCRL_REQUIRE(cube_side(CX) && cube_side(CY) && cube_side(CZ), "prep_cubes: cube %d x %d x %d (each side a positive multiple of 8, <= 64)", CX, CY, CZ);
  PCRL_REQUIRE(M >= 0, "prep_cubes: M = %d", M);
  PCRL_REQUIRE(out_kind == 0 || out_kind == 1, "prep_cubes: out_kind %d (0: int16, 1: float32)", out_kind);
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "prep_cubes: bad volume shape %d x %d x %d", X, Y, Z);
  if (M == 0) return 0;
  PCRL_REQUIRE(vol && start && out, "prep_cubes: null pointer");
  PCRL_REQUIRE((reinterpret_cast<uintptr_t>(vol) & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(start) & 3) == 0,
               "prep_cubes: vol must be 2-byte, start 4-byte and out 16-byte aligned");
  int JB = 8;
  while (JB * CZ > TILE_ROWS) JB >>= 1;
  const int L = JB * CZ / 8;
  const int P = L == 8 ? 36 : 34;
  const int64_t blocks = (int64_t)M * (CY / JB);
  PCRL_REQUIRE(blocks <= 0x7fffffff, "prep_cubes: M = %d is too many cubes for one launch", M);
  hipStream_t s = as_stream(stream);
  if (out_kind == 1) hipLaunchKernelGGL((cubes_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, s, vol, X, Y, Z, start, out, CX, CY, CZ, JB, P);
  else hipLaunchKernelGGL((cubes_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, s, vol, X, Y, Z, start, out, CX, CY, CZ, JB, P);
  return pcrl_check_launch("prep_cubes");
}

extern "C" int pcrl_prep_hu_to_unit(const int16_t* in, float* out, int64_t n, pcrl_stream_t stream) {
  PCRL_REQUIRE(n >= 0, "prep_hu_to_unit: n = %lld", (long long)n);
  if (n == 0) return 0;
  PCRL_REQUIRE(in && out, "prep_hu_to_unit: null pointer");
  PCRL_REQUIRE((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "prep_hu_to_unit: in and out must be 16-byte aligned");
  const int64_t g = (n / 8 + 255) / 256;
  hipLaunchKernelGGL(hu_to_unit_kernel, dim3((unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g)), dim3(256), 0, as_stream(stream), in, out, n);
  return pcrl_check_launch("prep_hu_to_unit");
}
