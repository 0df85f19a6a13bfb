// Training-time augmentation of 3D segmentation crops: ONE launch resamples a batch of source boxes -- C image channels
// and the label bitmask of every sample through the same affine geometry -- into training crops.  The host (pcrlv2_amd/data_seg.py) draws the
// parameters, cuts a source box around every crop and folds rotation, scale and the per-axis flips into one inverse matrix per sample.
//
//   output voxel i = (ix, iy, iz):   c = i + 0.5 - (X, Y, Z) / 2        s = M c + t + (Sx, Sy, Sz) / 2 - 0.5       (affine_kernel's shape of
//                                                                                                                  augment.hip plus a translation)
//   image   y[b][ch][i] = gain[b][ch] * T + bias[b][ch],  T = the trilinear sample of channel ch at s; a corner outside the source box adds 0
//           (scipy.ndimage.affine_transform(order=1, mode='grid-constant', cval=0))
//   label   lab[b][i] = src_lab[b][n],  n = floor(s + 0.5) per axis, 0x80 ('not counted') where n is outside the box
//           (order=0, mode='grid-constant', cval=0x80); a bit pattern is never interpolated
//
// thread = one output voxel, threads along z (the fastest axis of both layouts: the stores coalesce, and so do the loads of an unrotated sample);
// the coordinate, the eight corner offsets and the eight weights are formed once and shared by all C channels and the label.  An HBM/latency-bound
// gather over a few tens of MB: 256-thread blocks, registers only, no LDS staging.  Every read is bounds-checked here -- a coordinate is clamped
// to [-2, S + 1] before it becomes an integer (beyond that every corner is outside anyway; NaN goes to -2), so NO matrix reaches memory outside the
// box, whatever the host's source-extent bound says.  Noise and gamma are pcrl_aug_noise_gamma's (augment.hip), run afterwards over [B * C] volumes.
//
// PINNED (tests/test_seg_aug_gpu.py, case table and derivations in tests/seg_aug_cases.py, restatement tests/seg_aug_reference.py): image bits and
// label bytes on the dyadic lattice (signed permutations, scales, shears, zoom-out, translations; ties at .5; float32 and float16 sources; C = 1,
// 3, 4; a z row longer than a wave); generic rotations to a derived float32 bound; every refusal.  NOT PINNED: torchio, MONAI or nnU-Net (none
// installed) -- their conventions and random streams.
#include "common.h"

namespace {

constexpr int SA_THREADS = 256, SA_MAX_C = 16;

struct SaGeom {
  int C, Sx, Sy, Sz, X, Y, Z;
};

// s clamped to [-2, S + 1]: inside that range nothing changes; outside it every corner and the nearest voxel are outside the box on this axis
// before and after, and the conversion to int is defined.  fmaxf(NaN, -2) = -2.
__device__ __forceinline__ float sa_clamp(float s, int S) { return fminf(fmaxf(s, -2.0f), (float)S + 1.0f); }

// grid = (ceil(X * Y * Z / 256), B); block = 256
template <typename T>
__global__ void __launch_bounds__(SA_THREADS) seg_aug_kernel(const T* __restrict__ src, const uint8_t* __restrict__ src_lab, float* __restrict__ y,
                                                             uint8_t* __restrict__ lab, const float* __restrict__ inv, const float* __restrict__ gain,
                                                             const float* __restrict__ bias, SaGeom g) {
  const int b = blockIdx.y;
  const int V = g.X * g.Y * g.Z, SV = g.Sx * g.Sy * g.Sz;
  const int i = blockIdx.x * SA_THREADS + threadIdx.x;
  if (i >= V) return;
  const int iz = i % g.Z, iy = (i / g.Z) % g.Y, ix = i / (g.Z * g.Y);
  const float* m = inv + b * 12;
  const float cx = ix + 0.5f - 0.5f * g.X, cy = iy + 0.5f - 0.5f * g.Y, cz = iz + 0.5f - 0.5f * g.Z;
  const float sx = sa_clamp(m[0] * cx + m[1] * cy + m[2] * cz + m[3] + (0.5f * g.Sx - 0.5f), g.Sx);
  const float sy = sa_clamp(m[4] * cx + m[5] * cy + m[6] * cz + m[7] + (0.5f * g.Sy - 0.5f), g.Sy);
  const float sz = sa_clamp(m[8] * cx + m[9] * cy + m[10] * cz + m[11] + (0.5f * g.Sz - 0.5f), g.Sz);
  const float fx = floorf(sx), fy = floorf(sy), fz = floorf(sz);
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  const float tx = sx - fx, ty = sy - fy, tz = sz - fz;
  int off[8];            // corner offset inside one channel of the source box, -1: outside
  float w[8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int xx = x0 + a, yy = y0 + bb, zz = z0 + c, k = a * 4 + bb * 2 + c;
        const bool in = (unsigned)xx < (unsigned)g.Sx && (unsigned)yy < (unsigned)g.Sy && (unsigned)zz < (unsigned)g.Sz;
        off[k] = in ? (xx * g.Sy + yy) * g.Sz + zz : -1;
        w[k] = ((a ? tx : 1.0f - tx) * (bb ? ty : 1.0f - ty)) * (c ? tz : 1.0f - tz);
      }
  const T* v = src + (int64_t)b * g.C * SV;
  float* out = y + (int64_t)b * g.C * V + i;
  for (int ch = 0; ch < g.C; ++ch, v += SV, out += V) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += (off[k] >= 0 ? (float)v[off[k]] : 0.0f) * w[k];
    *out = gain[b * g.C + ch] * acc + bias[b * g.C + ch];
  }
  const int nx = (int)floorf(sx + 0.5f), ny = (int)floorf(sy + 0.5f), nz = (int)floorf(sz + 0.5f);
  const bool in = (unsigned)nx < (unsigned)g.Sx && (unsigned)ny < (unsigned)g.Sy && (unsigned)nz < (unsigned)g.Sz;
  lab[(int64_t)b * V + i] = in ? src_lab[(int64_t)b * SV + (nx * g.Sy + ny) * g.Sz + nz] : (uint8_t)0x80;
}

}  // namespace

extern "C" int pcrl_seg_aug_resample(const void* src, int src_half, const uint8_t* src_lab, float* y, uint8_t* lab, const float* inv, const float* gain,
                                     const float* bias, int B, int C, int Sx, int Sy, int Sz, int X, int Y, int Z, pcrl_stream_t stream) {
  PCRL_REQUIRE(src && src_lab && y && lab && inv && gain && bias, "seg_aug_resample: null pointer");
  PCRL_REQUIRE(B >= 1 && B <= 65535, "seg_aug_resample: 1 <= B <= 65535 samples, got %d", B);
  PCRL_REQUIRE(C >= 1 && C <= SA_MAX_C, "seg_aug_resample: 1 <= C <= %d channels, got %d", SA_MAX_C, C);
  PCRL_REQUIRE(Sx >= 1 && Sy >= 1 && Sz >= 1 && X >= 1 && Y >= 1 && Z >= 1, "seg_aug_resample: empty extent, source %d x %d x %d -> crop %d x %d x %d", Sx,
               Sy, Sz, X, Y, Z);
  const int64_t SV = (int64_t)Sx * Sy * Sz, V = (int64_t)X * Y * Z, lim = (int64_t)1 << 31;
  PCRL_REQUIRE(SV < lim && V < lim, "seg_aug_resample: a source box or a crop of 2^31 voxels or more (voxel indices are 32-bit)");
  const int64_t src_bytes = (int64_t)B * C * SV * (src_half ? 2 : 4), y_bytes = (int64_t)B * C * V * 4;
  PCRL_REQUIRE(!ranges_overlap(y, y_bytes, src, src_bytes) && !ranges_overlap(y, y_bytes, src_lab, B * SV) && !ranges_overlap(lab, B * V, src, src_bytes) &&
                   !ranges_overlap(lab, B * V, src_lab, B * SV) && !ranges_overlap(y, y_bytes, lab, B * V),
               "seg_aug_resample: the outputs overlap the sources or each other (a gather cannot run in place)");
  const SaGeom g{C, Sx, Sy, Sz, X, Y, Z};
  const dim3 grid((unsigned)((V + SA_THREADS - 1) / SA_THREADS), (unsigned)B);
  if (src_half)
    hipLaunchKernelGGL(seg_aug_kernel<_Float16>, grid, dim3(SA_THREADS), 0, as_stream(stream), static_cast<const _Float16*>(src), src_lab, y, lab, inv,
                       gain, bias, g);
  else
    hipLaunchKernelGGL(seg_aug_kernel<float>, grid, dim3(SA_THREADS), 0, as_stream(stream), static_cast<const float*>(src), src_lab, y, lab, inv, gain,
                       bias, g);
  return pcrl_check_launch("seg_aug_resample");
}
