// Fine-tuning optimiser kernels over FusedSGD's flat arenas: Adam / AdamW (torch.optim's single-tensor arithmetic, one float32 rounding per
// operation), the global gradient norm with torch.nn.utils.clip_grad_norm_'s coefficient, and the SGD step with that coefficient folded in.
// Compiled with -ffp-contract=off (build.FILE_FLAGS): tests/optim_reference.py restates every kernel here one operation at a time, and the
// only fused multiply-adds are the ones written out below.  The pre-training SGD kernels stay in heads_loss.hip.
#include "common.h"

namespace {

// Streaming passes of 16-28 bytes per element: 256 threads x 4 elements per group, at most 2048 blocks (8 per CU), the rest by grid stride.
constexpr int kGridCap = 2048;
inline unsigned optim_grid(int64_t groups) { return (unsigned)capped_blocks(groups, 256, kGridCap); }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// t with offsets[t] <= i < offsets[t + 1]
__device__ __forceinline__ int find_tensor(const int64_t* __restrict__ offsets, int ntensors, int64_t i) {
  int lo = 0, hi = ntensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------
// Adam: per-tensor step counts, running products and coefficients, advanced on the device (one thread per tensor)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) adam_prepare_kernel(const int32_t* __restrict__ flags, int32_t* __restrict__ steps, double* __restrict__ prods,
                                                           float* __restrict__ coefs, int ntensors, double lr, double beta1, double beta2) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntensors || !(flags[t] & 1)) return;
  steps[t] += 1;
  const double b1 = prods[2 * t] * beta1, b2 = prods[2 * t + 1] * beta2;     // beta^t by one multiply per step: no pow, numpy reproduces it
  prods[2 * t] = b1;
  prods[2 * t + 1] = b2;
  coefs[2 * t] = (float)(lr / (1.0 - b1));
  coefs[2 * t + 1] = (float)sqrt(1.0 - b2);
}

struct AdamArgs {
  float gscale, decay, one_minus_b1, beta2, one_minus_b2, eps;      // decay: 1 - lr * wd (decoupled) or wd (L2)
  int decoupled;
};

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a, float clip, bool clipped, float step_size,
                                      float rsqrt_bc2) {
  float gg = g * a.gscale;
  if (clipped) gg = gg * clip;
  if (a.decoupled) p = p * a.decay;
  else gg = gg + a.decay * p;
  m = m + (gg - m) * a.one_minus_b1;
  v = v * a.beta2 + (gg * gg) * a.one_minus_b2;
  p = p - step_size * (m / (sqrtf(v) / rsqrt_bc2 + a.eps));
}

// sgd4_kernel's structure: four elements per thread, 16-byte accesses where the group lies inside one tensor and the pointers are aligned,
// the scalar update where a group straddles tensors.  Reads p, g, m, v and writes p, m, v: 28 bytes per parameter.
__global__ void __launch_bounds__(256) adam4_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    const int64_t* __restrict__ offsets, const int32_t* __restrict__ flags,
                                                    const float* __restrict__ coefs, int ntensors, int64_t total, AdamArgs a,
                                                    const float* __restrict__ clip_coef, int aligned) {
  const bool clipped = clip_coef != nullptr;
  const float clip = clipped ? *clip_coef : 1.f;
  const int64_t ngroups = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int lo = find_tensor(offsets, ntensors, i);
    if (aligned && i + 4 <= total && offsets[lo + 1] >= i + 4) {
      if (!(flags[lo] & 1)) continue;
      const float step_size = coefs[2 * lo], rsqrt_bc2 = coefs[2 * lo + 1];
      float4 pv = *reinterpret_cast<const float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<const float4*>(m + i);
      float4 vv = *reinterpret_cast<const float4*>(v + i);
      adam1(pv.x, gv.x, mv.x, vv.x, a, clip, clipped, step_size, rsqrt_bc2);
      adam1(pv.y, gv.y, mv.y, vv.y, a, clip, clipped, step_size, rsqrt_bc2);
      adam1(pv.z, gv.z, mv.z, vv.z, a, clip, clipped, step_size, rsqrt_bc2);
      adam1(pv.w, gv.w, mv.w, vv.w, a, clip, clipped, step_size, rsqrt_bc2);
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      *reinterpret_cast<float4*>(p + i) = pv;
    } else {
      for (int64_t e = i; e < i + 4 && e < total; ++e) {
        int t = lo;
        while (t + 1 < ntensors && offsets[t + 1] <= e) ++t;
        if (!(flags[t] & 1)) continue;
        float pv = p[e], mv = m[e], vv = v[e];
        adam1(pv, g[e], mv, vv, a, clip, clipped, coefs[2 * t], coefs[2 * t + 1]);
        m[e] = mv;
        v[e] = vv;
        p[e] = pv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Global L2 norm of grad_scale * g over the tensors that have a gradient: float64, two stages, no atomics.  Which block and thread adds which
// element, and in which order, depends on `total` alone.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq(float g, float gscale) {
  const double d = (double)(g * gscale);
  return d * d;
}

__global__ void __launch_bounds__(256) grad_norm_partial_kernel(const float* __restrict__ g, const int64_t* __restrict__ offsets,
                                                                const int64_t* __restrict__ numels, const int32_t* __restrict__ flags, int ntensors,
                                                                int64_t total, float gscale, double* __restrict__ partials, int aligned) {
  __shared__ double red[4];
  double acc = 0.0;
  const int64_t ngroups = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int lo = find_tensor(offsets, ntensors, i);
    const int64_t end = numels ? offsets[lo] + numels[lo] : offsets[lo + 1];      // the slot's padding does not count
    if (aligned && i + 4 <= total && end >= i + 4) {
      if (!(flags[lo] & 1)) continue;
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      acc += sq(gv.x, gscale);
      acc += sq(gv.y, gscale);
      acc += sq(gv.z, gscale);
      acc += sq(gv.w, gscale);
    } else {
      for (int64_t e = i; e < i + 4 && e < total; ++e) {
        int t = lo;
        while (t + 1 < ntensors && offsets[t + 1] <= e) ++t;
        if (!(flags[t] & 1) || (numels && e - offsets[t] >= numels[t])) continue;
        acc += sq(g[e], gscale);
      }
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// norm[0] = sqrt(sum of the partials); coef[0] = (float)min(1, max_norm / (norm + 1e-6)): clip_grad_norm_'s arithmetic and clamp (a NaN norm
// gives a NaN coefficient, an infinite one 0, as torch's error_if_nonfinite=False does)
__global__ void __launch_bounds__(256) grad_norm_final_kernel(const double* __restrict__ partials, int nparts, double max_norm,
                                                              double* __restrict__ norm, float* __restrict__ coef) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) acc += partials[k];
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) {
    const double n = sqrt(acc);
    double c = max_norm / (n + 1e-6);
    if (c > 1.0) c = 1.0;
    norm[0] = n;
    coef[0] = (float)c;
  }
}

// ---------------------------------------------------------------------------------------------
// pcrl_sgd_step with the clip coefficient: (g * grad_scale) * coef.  heads_loss.hip is compiled with contraction on, and its two SGD kernels
// came out with these fused multiply-adds (read from their gfx950 code): weight decay as fma(wd, p, g') in the 16-byte path and as two
// products and an add in the scalar paths, momentum and the parameter update as one fma each.  They are written out here, so that
// coef == 1 gives pcrl_sgd_step's bits.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void sgd1(float& p, float g, float& buf, int f, float lr, float momentum, float wd, float gscale, float coef, bool vec) {
  const float gs = (g * gscale) * coef;
  const float gg = vec ? __builtin_fmaf(wd, p, gs) : gs + wd * p;
  const float b = (f & 2) ? __builtin_fmaf(momentum, buf, gg) : gg;
  buf = b;
  p = __builtin_fmaf(-lr, b, p);
}

__global__ void __launch_bounds__(256) sgd4_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                           const int64_t* __restrict__ offsets, const int32_t* __restrict__ flags, int ntensors,
                                                           int64_t total, float lr, float momentum, float wd, float gscale,
                                                           const float* __restrict__ clip_coef, int aligned) {
  const float coef = *clip_coef;
  const int64_t ngroups = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int lo = find_tensor(offsets, ntensors, i);
    if (aligned && i + 4 <= total && offsets[lo + 1] >= i + 4) {
      const int f = flags[lo];
      if (!(f & 1)) continue;
      float4 pv = *reinterpret_cast<const float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 bv = (f & 2) ? *reinterpret_cast<const float4*>(buf + i) : float4{0.f, 0.f, 0.f, 0.f};
      sgd1(pv.x, gv.x, bv.x, f, lr, momentum, wd, gscale, coef, true);
      sgd1(pv.y, gv.y, bv.y, f, lr, momentum, wd, gscale, coef, true);
      sgd1(pv.z, gv.z, bv.z, f, lr, momentum, wd, gscale, coef, true);
      sgd1(pv.w, gv.w, bv.w, f, lr, momentum, wd, gscale, coef, true);
      *reinterpret_cast<float4*>(buf + i) = bv;
      *reinterpret_cast<float4*>(p + i) = pv;
    } else {
      for (int64_t e = i; e < i + 4 && e < total; ++e) {
        int t = lo;
        while (t + 1 < ntensors && offsets[t + 1] <= e) ++t;
        const int f = flags[t];
        if (!(f & 1)) continue;
        float pv = p[e], bv = (f & 2) ? buf[e] : 0.f;
        sgd1(pv, g[e], bv, f, lr, momentum, wd, gscale, coef, false);
        buf[e] = bv;
        p[e] = pv;
      }
    }
  }
}

}  // namespace

extern "C" int pcrl_optim_grid_cap(void) { return kGridCap; }

extern "C" int pcrl_adam_prepare(const int32_t* flags, int32_t* steps, double* prods, float* coefs, int ntensors, double lr, double beta1,
                                 double beta2, pcrl_stream_t stream) {
  PCRL_REQUIRE(flags && steps && prods && coefs && ntensors > 0, "adam_prepare: bad arguments");
  hipLaunchKernelGGL(adam_prepare_kernel, dim3((ntensors + 255) / 256), dim3(256), 0, as_stream(stream), flags, steps, prods, coefs, ntensors, lr,
                     beta1, beta2);
  return pcrl_check_launch("adam_prepare");
}

extern "C" int pcrl_adam_step(float* p, const float* g, float* m, float* v, const int64_t* offsets, const int32_t* flags, const float* coefs,
                              int ntensors, int64_t total, float decay, int decoupled, float one_minus_beta1, float beta2, float one_minus_beta2,
                              float eps, float grad_scale, const float* clip_coef, pcrl_stream_t stream) {
  PCRL_REQUIRE(p && g && m && v && offsets && flags && coefs && ntensors > 0 && total > 0, "adam_step: bad arguments");
  const AdamArgs a{grad_scale, decay, one_minus_beta1, beta2, one_minus_beta2, eps, decoupled ? 1 : 0};
  const int aligned = al16(p) && al16(g) && al16(m) && al16(v);
  hipLaunchKernelGGL(adam4_kernel, dim3(optim_grid((total + 3) / 4)), dim3(256), 0, as_stream(stream), p, g, m, v, offsets, flags, coefs, ntensors,
                     total, a, clip_coef, aligned);
  return pcrl_check_launch("adam_step");
}

extern "C" int pcrl_grad_norm(const float* g, const int64_t* offsets, const int64_t* numels, const int32_t* flags, int ntensors, int64_t total,
                              float grad_scale, double max_norm, double* partials, double* norm, float* coef, pcrl_stream_t stream) {
  PCRL_REQUIRE(g && offsets && flags && partials && norm && coef && ntensors > 0 && total > 0, "grad_norm: bad arguments");
  const unsigned grid = optim_grid((total + 3) / 4);
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(grid), dim3(256), 0, as_stream(stream), g, offsets, numels, flags, ntensors, total, grad_scale,
                     partials, (int)al16(g));
  const int rc = pcrl_check_launch("grad_norm");
  if (rc) return rc;
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, (int)grid, max_norm, norm, coef);
  return pcrl_check_launch("grad_norm_final");
}

extern "C" int pcrl_sgd_step_clipped(float* p, const float* g, float* buf, const int64_t* offsets, const int32_t* flags, int ntensors,
                                     int64_t total, float lr, float momentum, float weight_decay, float grad_scale, const float* clip_coef,
                                     pcrl_stream_t stream) {
  PCRL_REQUIRE(p && g && buf && offsets && flags && clip_coef && ntensors > 0 && total > 0, "sgd_step_clipped: bad arguments");
  const int aligned = al16(p) && al16(g) && al16(buf);
  hipLaunchKernelGGL(sgd4_clipped_kernel, dim3(optim_grid((total + 3) / 4)), dim3(256), 0, as_stream(stream), p, g, buf, offsets, flags, ntensors,
                     total, lr, momentum, weight_decay, grad_scale, clip_coef, aligned);
  return pcrl_check_launch("sgd_step_clipped");
}
