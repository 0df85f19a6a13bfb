// Device-side augmentation of the 2D (chest X-ray) pre-task images: the torchvision chain of the reference's chest loader
// (data.py:14-61 -> datasets/chestDataset.py:31-48) as hand-written gfx950 kernels on uint8 sources.  On PIL images every torchvision
// transform of that chain hands its arithmetic to Pillow, so each kernel restates Pillow's integer / float arithmetic exactly:
//
//   RandomResizedCrop (crop + BILINEAR resize: Pillow's two-pass fixed-point resampler, horizontal pass first)
//       -> pcrl_aug2d_hresample (horizontal pass of the crop box into a uint8 intermediate).  Pillow itself runs the vertical pass first on a
//          crop more than 100 times as tall as wide: exact for crops up to 100 : 1 (the drawn ones are 3/4 .. 4/3)
//   RandomRotation (NEAREST, 16.16 fixed-point affine, fill 0) + RandomHorizontalFlip
//       -> pcrl_aug2d_spatial (the vertical pass evaluated only at the resized pixel the rotation and the flip pick; writes the uint8 view
//          and, for the global views, the float32 target Normalize(ToTensor(view)))
//   RandomGrayscale + RandomApply(GaussianBlur = Pillow's 3-pass extended box blur) + ColorJitter (brightness, contrast, saturation,
//   hue in the drawn order) + ToTensor + Normalize + Cutout
//       -> pcrl_aug2d_photometric (one workgroup per view, the view held in LDS)
//
// A 1-plane (mode L) source stays one plane through the whole chain: on a gray image grayscale, saturation and hue are identities
// and contrast's mean is the pixel mean, so the result equals the 3-plane result of the same image replicated to RGB.  Built with
// -ffp-contract=off (pcrlv2_amd/build.py): the float and double expressions below round as the C code of Pillow and torch's CPU
// kernels do.  The parameters are drawn on the host (pcrlv2_amd/data_chest.py) and packed per view (layout in pcrl_hip.h).
#include "common.h"

namespace {

enum {
  P_SRC = 0, P_H, P_W, P_C, P_J, P_I, P_CW, P_CH, P_A0, P_A1, P_A2, P_A3, P_A4, P_A5, P_FLIP, P_GRAY, P_BLUR, P_BR, P_WW, P_FW,
  P_NOPS, P_ORDER, P_BRI, P_CON, P_SAT, P_HUE, P_NHOLES, P_HOLES, P_INTER = P_HOLES + 12, P_COUNT
};
static_assert(P_COUNT == PCRL_AUG2D_NPARAM, "pcrl_hip.h and augment2d.hip disagree on the parameter record");

constexpr int PRECISION_BITS = 22;     // Pillow Resample.c: 32 - 8 - 2
constexpr int BLUR_RMAX = 4;           // integer box radius bound (sigma <= 2 gives 1)

__device__ __forceinline__ uint8_t clip8(int ss) {
  const int v = ss >> PRECISION_BITS;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ double bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for ONE output index: the box [0, in_size) resized to out_size.  -> xmin, n taps;
// kk(t) recomputes the double weight of tap t (twice: the sum first, then the normalised value) instead of keeping an array.
struct Coeffs {
  double scale, support, ss, center, ww;
  int xmin, n;
  __device__ Coeffs(int in_size, int out_size, int xx) {
    scale = (double)(float)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    support = 1.0 * filterscale;
    center = 0.0 + (xx + 0.5) * scale;
    ss = 1.0 / filterscale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    n = xmax - xmin;
    ww = 0.0;
    for (int t = 0; t < n; ++t) ww += w(t);
  }
  __device__ double w(int t) const { return bilinear(((double)(t + xmin) - center + 0.5) * ss); }
  __device__ int kk(int t) const {
    double k = w(t);
    if (ww != 0.0) k /= ww;
    return k < 0 ? (int)(-0.5 + k * (1 << PRECISION_BITS)) : (int)(0.5 + k * (1 << PRECISION_BITS));
  }
};

// ---- horizontal pass of the crop box: inter[v] = [CH][S][C] uint8 ----
__global__ void __launch_bounds__(256) hresample_kernel(const uint8_t* __restrict__ src, const int* __restrict__ params,
                                                        uint8_t* __restrict__ inter, int S) {
  const int* p = params + blockIdx.y * PCRL_AUG2D_NPARAM;
  const int W = p[P_W], C = p[P_C], j = p[P_J], i = p[P_I], cw = p[P_CW], ch = p[P_CH];
  const uint8_t* s = src + p[P_SRC];
  uint8_t* o = inter + p[P_INTER];
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < ch * S; idx += gridDim.x * blockDim.x) {
    const int row = idx / S, xx = idx - row * S;
    const Coeffs k(cw, S, xx);
    const uint8_t* line = s + ((int64_t)(i + row) * W + j + k.xmin) * C;
    int ss0 = 1 << (PRECISION_BITS - 1), ss1 = ss0, ss2 = ss0;
    for (int t = 0; t < k.n; ++t) {
      const int kt = k.kk(t);
      ss0 += line[t * C] * kt;
      if (C == 3) {
        ss1 += line[t * C + 1] * kt;
        ss2 += line[t * C + 2] * kt;
      }
    }
    uint8_t* q = o + ((int64_t)row * S + xx) * C;
    q[0] = clip8(ss0);
    if (C == 3) {
      q[1] = clip8(ss1);
      q[2] = clip8(ss2);
    }
  }
}

__device__ __forceinline__ float normalize(int u, int c) {
  // ToTensor + Normalize in torch's float32 order: (u / 255 - mean) / std, the constants rounded from double as torch.as_tensor does
  const float mean = c == 0 ? (float)0.485 : c == 1 ? (float)0.456 : (float)0.406;
  const float stdv = c == 0 ? (float)0.229 : c == 1 ? (float)0.224 : (float)0.225;
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), mean), stdv);
}

// ---- vertical pass at the resized pixel picked by the nearest rotation and the flip: view[v] = [C][S][S] uint8, target[v] = [3][S][S] ----
__global__ void __launch_bounds__(256) spatial_kernel(const uint8_t* __restrict__ inter, const int* __restrict__ params,
                                                      uint8_t* __restrict__ view, float* __restrict__ target, int S) {
  const int v = blockIdx.y;
  const int* p = params + v * PCRL_AUG2D_NPARAM;
  const int C = p[P_C], ch = p[P_CH];
  const int a0 = p[P_A0], a1 = p[P_A1], a2 = p[P_A2], a3 = p[P_A3], a4 = p[P_A4], a5 = p[P_A5];
  const int SS = S * S;
  const uint8_t* in = inter + p[P_INTER];
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < SS; idx += gridDim.x * blockDim.x) {
    const int y = idx / S, x = idx - y * S;
    const int xf = p[P_FLIP] ? S - 1 - x : x;
    const int xin = (a2 + y * a1 + xf * a0) >> 16;     // Geometry.c affine_fixed: xx = a2 + y a1 + x a0 in 16.16
    const int yin = (a5 + y * a4 + xf * a3) >> 16;
    int r[3] = {0, 0, 0};
    if (xin >= 0 && xin < S && yin >= 0 && yin < S) {
      const Coeffs k(ch, S, yin);
      int ss0 = 1 << (PRECISION_BITS - 1), ss1 = ss0, ss2 = ss0;
      for (int t = 0; t < k.n; ++t) {
        const int kt = k.kk(t);
        const uint8_t* q = in + ((int64_t)(k.xmin + t) * S + xin) * C;
        ss0 += q[0] * kt;
        if (C == 3) {
          ss1 += q[1] * kt;
          ss2 += q[2] * kt;
        }
      }
      r[0] = clip8(ss0);
      r[1] = clip8(ss1);
      r[2] = clip8(ss2);
    }
    uint8_t* vo = view + (int64_t)v * 3 * SS;
    for (int c = 0; c < C; ++c) vo[c * SS + idx] = (uint8_t)r[c];
    if (target != nullptr) {
      float* to = target + (int64_t)v * 3 * SS;
      for (int c = 0; c < 3; ++c) to[c * SS + idx] = normalize(r[C == 3 ? c : 0], c);
    }
  }
}

// ---- photometric chain: one workgroup per view ----
__device__ __forceinline__ int luma(int r, int g, int b) {     // Convert.c rgb2l: ITU-R 601-2 in 16.16
  return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}

__device__ __forceinline__ int blend(int a, int b, float alpha) {   // Blend.c ImagingBlend: float arithmetic, truncation, clip when extrapolating
  if (alpha == 0.0f) return a;
  if (alpha == 1.0f) return b;
  const float t = __fadd_rn((float)a, __fmul_rn(alpha, (float)(b - a)));
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (int)t;
}

// Convert.c rgb2hsv / hsv2rgb with their float and double intermediates, and the hue shift of torchvision's adjust_hue in between
__device__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  if (minc == maxc) return;      // h = s = 0: hsv2rgb gives (v, v, v) back
  const float cr = (float)(maxc - minc);
  const float s = __fdiv_rn(cr, (float)maxc);
  const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
  float h;
  if (r == maxc) h = __fsub_rn(bc, gc);
  else if (g == maxc) h = (float)__dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
  else h = (float)__dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
  double hd = __dadd_rn(__ddiv_rn((double)h, 6.0), 1.0);
  hd = hd >= 1.0 ? hd - 1.0 : hd;                          // fmod(hd, 1.0) on (0, 2): exact
  h = (float)hd;
  int uh = (int)__dmul_rn((double)h, 255.0), us = (int)__dmul_rn((double)s, 255.0);
  uh = min(max(uh, 0), 255);
  us = min(max(us, 0), 255);
  const int v = maxc;
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = v;
    return;
  }
  const double h6 = __ddiv_rn(__dmul_rn((double)(float)uh, 6.0), 255.0);
  const int i = (int)floor(h6);
  const float f = (float)__dsub_rn(h6, (double)(float)i);
  const float fs = (float)__ddiv_rn((double)(float)us, 255.0);
  const int pp = (int)round(__dmul_rn((double)(float)v, __dsub_rn(1.0, (double)fs)));
  const int qq = (int)round(__dmul_rn((double)(float)v, __dsub_rn(1.0, (double)__fmul_rn(fs, f))));
  const int tt = (int)round(__dmul_rn((double)(float)v, __dsub_rn(1.0, __dmul_rn((double)fs, __dsub_rn(1.0, (double)f)))));
  const int up = min(max(pp, 0), 255), uq = min(max(qq, 0), 255), ut = min(max(tt, 0), 255);
  switch (i % 6) {
    case 0: r = v; g = ut; b = up; break;
    case 1: r = uq; g = v; b = up; break;
    case 2: r = up; g = v; b = ut; break;
    case 3: r = up; g = uq; b = v; break;
    case 4: r = ut; g = up; b = v; break;
    default: r = v; g = up; b = uq; break;
  }
}

// One pass of BoxBlur.c ImagingLineBoxBlur8 over a line of n pixels at stride `step`, in place: out[x] = (ww * sum in[x-r..x+r] +
// fw * (in[x-r-1] + in[x+r+1]) + 2^23) >> 24 with edge-replicated indices.  hist keeps the ORIGINAL in[x-RMAX-1 .. x-1] (already overwritten).
__device__ void box_line(uint8_t* line, int n, int step, int r, unsigned ww, unsigned fw) {
  unsigned hist[BLUR_RMAX + 1];
#pragma unroll
  for (int k = 0; k <= BLUR_RMAX; ++k) hist[k] = line[0];
  for (int x = 0; x < n; ++x) {
    unsigned acc = 0, far = 0;
#pragma unroll
    for (int k = 0; k <= BLUR_RMAX; ++k) {       // hist[k] = in[x - RMAX - 1 + k]
      if (k == BLUR_RMAX - r) far = hist[k];
      if (k > BLUR_RMAX - r) acc += hist[k];
    }
    for (int d = 0; d <= r; ++d) acc += line[min(x + d, n - 1) * step];
    far += line[min(x + r + 1, n - 1) * step];
    const unsigned cur = line[x * step];
    line[x * step] = (uint8_t)((acc * ww + far * fw + (1u << 23)) >> 24);
#pragma unroll
    for (int k = 0; k < BLUR_RMAX; ++k) hist[k] = hist[k + 1];
    hist[BLUR_RMAX] = cur;
  }
}

template <int S>
__global__ void __launch_bounds__(1024) photometric_kernel(const uint8_t* __restrict__ view, const int* __restrict__ params,
                                                           float* __restrict__ out, uint8_t* __restrict__ u8_out) {
  constexpr int SS = S * S;
  __shared__ uint8_t px[3 * SS];
  __shared__ int red[16];
  const int v = blockIdx.x;
  const int* p = params + v * PCRL_AUG2D_NPARAM;
  const int C = p[P_C];
  const int tid = threadIdx.x, nt = blockDim.x;
  const uint8_t* vi = view + (int64_t)v * 3 * SS;
  for (int k = tid; k < C * SS; k += nt) px[k] = vi[k];
  __syncthreads();
  if (p[P_GRAY] && C == 3) {            // RandomGrayscale: convert('L') replicated to three channels
    for (int k = tid; k < SS; k += nt) {
      const uint8_t l = (uint8_t)luma(px[k], px[SS + k], px[2 * SS + k]);
      px[k] = px[SS + k] = px[2 * SS + k] = l;
    }
    __syncthreads();
  }
  if (p[P_BLUR]) {                      // ImageFilter.GaussianBlur: 3 horizontal box passes, then 3 vertical ones
    const int r = p[P_BR];
    const unsigned ww = (unsigned)p[P_WW], fw = (unsigned)p[P_FW];
    for (int axis = 0; axis < 2; ++axis)
      for (int pass = 0; pass < 3; ++pass) {
        for (int t = tid; t < C * S; t += nt) {
          const int c = t / S, l = t - c * S;
          uint8_t* base = px + c * SS + (axis == 0 ? l * S : l);
          box_line(base, S, axis == 0 ? 1 : S, r, ww, fw);
        }
        __syncthreads();
      }
  }
  const int nops = p[P_NOPS], order = p[P_ORDER];
  for (int o = 0; o < nops; ++o) {
    const int op = (order >> (4 * o)) & 15;
    if (op == 0) {                      // Brightness: blend with black
      const float a = __int_as_float(p[P_BRI]);
      for (int k = tid; k < C * SS; k += nt) px[k] = (uint8_t)blend(0, px[k], a);
    } else if (op == 1) {               // Contrast: blend with the grey int(mean(L) + 0.5), an exact integer reduction
      int sum = 0;
      for (int k = tid; k < SS; k += nt) sum += C == 3 ? luma(px[k], px[SS + k], px[2 * SS + k]) : px[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
      if ((tid & 63) == 0) red[tid >> 6] = sum;
      __syncthreads();
      int64_t tot = 0;
      for (int w = 0; w < (nt >> 6); ++w) tot += red[w];
      const int mean = (int)((2 * tot + SS) / (2 * (int64_t)SS));
      const float a = __int_as_float(p[P_CON]);
      for (int k = tid; k < C * SS; k += nt) px[k] = (uint8_t)blend(mean, px[k], a);
    } else if (op == 2) {               // Color (saturation): blend with convert('L'); an identity on one plane
      if (C == 3) {
        const float a = __int_as_float(p[P_SAT]);
        for (int k = tid; k < SS; k += nt) {
          const int r = px[k], g = px[SS + k], b = px[2 * SS + k];
          const int l = luma(r, g, b);
          px[k] = (uint8_t)blend(l, r, a);
          px[SS + k] = (uint8_t)blend(l, g, a);
          px[2 * SS + k] = (uint8_t)blend(l, b, a);
        }
      }
    } else if (op == 3) {               // hue: through PIL's HSV; an identity on one plane
      if (C == 3) {
        const int shift = p[P_HUE];
        for (int k = tid; k < SS; k += nt) {
          int r = px[k], g = px[SS + k], b = px[2 * SS + k];
          hue_shift(r, g, b, shift);
          px[k] = (uint8_t)r;
          px[SS + k] = (uint8_t)g;
          px[2 * SS + k] = (uint8_t)b;
        }
      }
    }
    __syncthreads();
  }
  if (u8_out != nullptr)
    for (int k = tid; k < C * SS; k += nt) u8_out[(int64_t)v * 3 * SS + k] = px[k];
  const int nholes = p[P_NHOLES];
  float* o = out + (int64_t)v * 3 * SS;
  for (int k = tid; k < 3 * SS; k += nt) {
    const int c = k / SS, e = k - c * SS, y = e / S, x = e - y * S;
    float m = 1.0f;                     // Cutout: img * mask (a masked negative value becomes -0.0, as on the CPU)
    for (int h = 0; h < nholes; ++h) {
      const int* hb = p + P_HOLES + 4 * h;
      if (y >= hb[0] && y < hb[1] && x >= hb[2] && x < hb[3]) m = 0.0f;
    }
    o[k] = __fmul_rn(normalize(px[(C == 3 ? c : 0) * SS + e], c), m);
  }
}

}  // namespace

extern "C" int pcrl_aug2d_hresample(const uint8_t* src, const int* params, uint8_t* inter, int V, int S, int max_rows, pcrl_stream_t stream) {
  PCRL_REQUIRE(src && params && inter, "aug2d_hresample: null pointer");
  PCRL_REQUIRE(V > 0 && V <= 65535 && S > 0 && max_rows > 0, "aug2d_hresample: bad shape");
  const int64_t work = (int64_t)max_rows * S;
  const unsigned gx = (unsigned)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
  hipLaunchKernelGGL(hresample_kernel, dim3(gx, V), dim3(256), 0, as_stream(stream), src, params, inter, S);
  return pcrl_check_launch("aug2d_hresample");
}

extern "C" int pcrl_aug2d_spatial(const uint8_t* inter, const int* params, uint8_t* view, float* target, int V, int S, pcrl_stream_t stream) {
  PCRL_REQUIRE(inter && params && view, "aug2d_spatial: null pointer");
  PCRL_REQUIRE(V > 0 && V <= 65535 && S > 0 && S <= 4096, "aug2d_spatial: bad shape");
  const unsigned gx = (unsigned)((S * S + 255) / 256);
  hipLaunchKernelGGL(spatial_kernel, dim3(gx, V), dim3(256), 0, as_stream(stream), inter, params, view, target, S);
  return pcrl_check_launch("aug2d_spatial");
}

extern "C" int pcrl_aug2d_photometric(const uint8_t* view, const int* params, float* out, uint8_t* u8_out, int V, int S, pcrl_stream_t stream) {
  PCRL_REQUIRE(view && params && out, "aug2d_photometric: null pointer");
  PCRL_REQUIRE(V > 0, "aug2d_photometric: bad shape");
  if (S == 224)
    hipLaunchKernelGGL(photometric_kernel<224>, dim3(V), dim3(1024), 0, as_stream(stream), view, params, out, u8_out);
  else if (S == 96)
    hipLaunchKernelGGL(photometric_kernel<96>, dim3(V), dim3(1024), 0, as_stream(stream), view, params, out, u8_out);
  else
    return pcrl_fail(PCRL_EINVAL, "aug2d_photometric: view side %d (224 and 96 are built)", S);
  return pcrl_check_launch("aug2d_photometric");
}
