// rt_denoise.h -- the arithmetic of rt_denoise (include/rt_hip.h, "denoising"), the one copy the kernels
// (rt_denoise.hip) and the host loop (denoise_host, rt_dev_denoise_host) run: the per-pixel step of the prepare pass
// and of an a-trous pass, templated on the working type T (float for RT_PREC_F32, double for RT_PREC_F64), and the
// parameter rules. No HIP: a plain C++ compiler takes this header (tests/native/denoise_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "../../include/rt_hip.h"

// a plain C++ compiler knows no function qualifiers
#if !defined(__HIP__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace rtd {

// The working records, 16 bytes (fp32) or 32 bytes (fp64) each:
//   colour  {c.r, c.g, c.b, v}   the demodulated colour and the variance of its channel mean (two buffers, ping-pong)
//   guide   {n.x, n.y, n.z, z}   the mean normal and depth over the hits; a miss pixel: n = 0, z = -1
//   grad    {gx, gy}             the depth gradient, depth per pixel
template <class T>
struct alignas(4 * sizeof(T)) DnV4 {
  T x, y, z, w;
};
template <class T>
struct alignas(2 * sizeof(T)) DnV2 {
  T x, y;
};
constexpr int kDnScratchT = 14;  // T values of scratch a pixel: two colour records, a guide record, a gradient

template <class T>
struct DnParams {
  int32_t W, H;
  int32_t demod;
  T albedo_eps, color_eps, depth_eps;
  T sc2;          // sigma_color^2
  T inv_sn2;      // 1 / sigma_normal^2
  T sigma_depth;
};

template <class T>
inline DnParams<T> dn_params(const rt_denoise_params& p) {
  DnParams<T> d;
  d.W = p.width;
  d.H = p.height;
  d.demod = (p.flags & RT_DENOISE_DEMODULATE) != 0;
  d.albedo_eps = (T)p.albedo_eps;
  d.color_eps = (T)p.color_eps;
  d.depth_eps = (T)p.depth_eps;
  d.sc2 = (T)p.sigma_color * (T)p.sigma_color;
  d.inv_sn2 = (T)1 / ((T)p.sigma_normal * (T)p.sigma_normal);
  d.sigma_depth = (T)p.sigma_depth;
  return d;
}

// The parameter rules of rt_denoise_params (rt_denoise_check): nullptr, or what is wrong with them.
inline const char* denoise_params_error(const rt_denoise_params& p) {
  auto finite = [](double x) { return x - x == 0.0; };
  if (p.width < 1 || p.height < 1) return "empty image";
  if (p.width > 65535 || p.height > 65535) return "image wider or taller than 65535 pixels";
  if ((int64_t)p.width * p.height >= (1ll << 31)) return "width * height outside [1, 2^31)";
  if (p.iterations < 1 || p.iterations > 8) return "iterations outside [1, 8]";
  if (p.precision != RT_PREC_F32 && p.precision != RT_PREC_F64) return "unknown precision";
  if (p.flags & ~RT_DENOISE_DEMODULATE) return "unknown flag";
  if (!finite(p.sigma_color) || !(p.sigma_color > 0.0)) return "sigma_color must be positive and finite";
  if (!finite(p.sigma_normal) || !(p.sigma_normal > 0.0)) return "sigma_normal must be positive and finite";
  if (!finite(p.sigma_depth) || !(p.sigma_depth > 0.0)) return "sigma_depth must be positive and finite";
  if (!finite(p.albedo_eps) || !(p.albedo_eps >= 0.0)) return "albedo_eps must be >= 0 and finite";
  if (!finite(p.color_eps) || !(p.color_eps >= 0.0)) return "color_eps must be >= 0 and finite";
  if (!finite(p.depth_eps) || !(p.depth_eps >= 0.0)) return "depth_eps must be >= 0 and finite";
  if ((p.flags & RT_DENOISE_DEMODULATE) && !(p.albedo_eps > 0.0)) return "albedo_eps must be positive when demodulating";
  return nullptr;
}

template <class T>
__host__ __device__ inline bool dn_finite(T x) {
  return x - x == (T)0;
}
template <class T>
__host__ __device__ inline bool dn_finite4(const DnV4<T>& a) {
  return dn_finite(a.x) && dn_finite(a.y) && dn_finite(a.z) && dn_finite(a.w);
}
__host__ __device__ inline float dn_exp(float x) { return expf(x); }
__host__ __device__ inline double dn_exp(double x) { return exp(x); }
__host__ __device__ inline float dn_abs(float x) { return fabsf(x); }
__host__ __device__ inline double dn_abs(double x) { return fabs(x); }
// the a-trous filter's taps: [1 4 6 4 1] / 16 at k = -2 .. 2
template <class T>
__host__ __device__ inline T dn_h(int k) {
  return (T)(k == 0 ? 6 : (k == 1 || k == -1) ? 4 : 1) / (T)16;
}

// a pixel's feature row f = albedo[3], normal[3], depth, hit (rt_render_aov's)
// a: the factor the colour is divided by before the filter and multiplied with after it
template <class T>
__host__ __device__ inline void dn_albedo(const DnParams<T>& P, const double* f, T a[3]) {
  for (int k = 0; k < 3; k++) a[k] = P.demod ? (T)f[k] + P.albedo_eps : (T)1;
}
// z: the mean depth over the hits, -1 for a miss pixel (hit > 0 fails; depths are distances, never negative)
template <class T>
__host__ __device__ inline T dn_depth(const double* f) {
  const T hit = (T)f[7];
  return hit > (T)0 ? (T)f[6] / hit : (T)-1;
}
// v0: the variance of a demodulated channel mean, from the summed variance of the three channel means
template <class T>
__host__ __device__ inline T dn_v0(const DnParams<T>& P, const double* f, double var) {
  T a[3];
  dn_albedo(P, f, a);
  const T m = (a[0] + a[1] + a[2]) / (T)3;
  return (T)var / (T)3 / (m * m);
}
// one axis of the depth gradient at a pixel with depth z: zm, zp the depths one pixel before and after it, hm, hp
// whether those pixels are inside the image. A difference exists when both its pixels are inside and neither is a miss.
template <class T>
__host__ __device__ inline T dn_grad(T zm, bool hm, T z, T zp, bool hp) {
  const bool b = hm && zm >= (T)0 && z >= (T)0, f = hp && zp >= (T)0 && z >= (T)0;
  const T db = z - zm, df = zp - z;
  return b && f ? (df + db) * (T)0.5 : f ? df : b ? db : (T)0;
}

// The prepare pass at pixel (x, y): rgb npix x 3 T, feat npix x 8 doubles, var npix doubles or null.
template <class T>
__host__ __device__ inline void dn_prepare_pixel(const DnParams<T>& P, const T* rgb, const double* feat,
                                                 const double* var, int x, int y, DnV4<T>& c, DnV4<T>& n, DnV2<T>& g) {
  const int W = P.W, H = P.H;
  const size_t p = (size_t)y * W + x;
  const double* f = feat + 8 * p;
  T a[3];
  dn_albedo(P, f, a);
  c.x = rgb[3 * p] / a[0];
  c.y = rgb[3 * p + 1] / a[1];
  c.z = rgb[3 * p + 2] / a[2];
  if (var) {  // the 3 x 3 binomial mean of v0 over the taps inside the image
    T sv = 0, sw = 0;
    for (int j = -1; j <= 1; j++) {
      const int yy = y + j;
      if (yy < 0 || yy >= H) continue;
      for (int i = -1; i <= 1; i++) {
        const int xx = x + i;
        if (xx < 0 || xx >= W) continue;
        const size_t q = (size_t)yy * W + xx;
        const T w = (T)((i == 0 ? 2 : 1) * (j == 0 ? 2 : 1));
        sv += w * dn_v0(P, feat + 8 * q, var[q]);
        sw += w;
      }
    }
    c.w = sv / sw;
  } else {
    c.w = (T)1;
  }
  const T hit = (T)f[7];
  const T z = dn_depth<T>(f);
  if (hit > (T)0) {
    n.x = (T)f[3] / hit;
    n.y = (T)f[4] / hit;
    n.z = (T)f[5] / hit;
  } else {
    n.x = n.y = n.z = (T)0;
  }
  n.w = z;
  const bool xm = x > 0, xp = x + 1 < W, ym = y > 0, yp = y + 1 < H;
  g.x = dn_grad(xm ? dn_depth<T>(f - 8) : (T)-1, xm, z, xp ? dn_depth<T>(f + 8) : (T)-1, xp);
  g.y = dn_grad(ym ? dn_depth<T>(f - 8 * (size_t)W) : (T)-1, ym, z, yp ? dn_depth<T>(f + 8 * (size_t)W) : (T)-1, yp);
}

// One a-trous pass with step s at pixel (x, y): the 25 taps p + s (i, j), j outer, i inner, those outside the image
// skipped. C, N, G: the colour, guide and gradient records of the whole image. Returns {c', v'}.
template <class T>
__host__ __device__ inline DnV4<T> dn_atrous_pixel(const DnParams<T>& P, const DnV4<T>* C, const DnV4<T>* N,
                                                   const DnV2<T>* G, int x, int y, int s) {
  const int W = P.W, H = P.H;
  const size_t p = (size_t)y * W + x;
  const DnV4<T> cp = C[p], np = N[p];
  const DnV2<T> g = G[p];
  const bool pfin = dn_finite4(cp);  // a broken pixel takes no colour distance: it is rebuilt from its neighbours
  const T kc = pfin ? (T)1 / ((T)3 * (P.sc2 * cp.w + P.color_eps)) : (T)0;
  const bool pmiss = np.w < (T)0;
  const T ez = P.depth_eps * dn_abs(np.w);
  T sw = 0, sr = 0, sg = 0, sb = 0, sv = 0;
  for (int j = -2; j <= 2; j++) {
    const int yy = y + s * j;
    if (yy < 0 || yy >= H) continue;
    for (int i = -2; i <= 2; i++) {
      const int xx = x + s * i;
      if (xx < 0 || xx >= W) continue;
      const size_t q = (size_t)yy * W + xx;
      const DnV4<T> cq = C[q], nq = N[q];
      if (!dn_finite4(cq)) continue;
      if ((nq.w < (T)0) != pmiss) continue;  // exactly one of the two is a miss pixel
      T d = 0;
      if (pfin) {
        const T dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
        d = (dr * dr + dg * dg + db * db) * kc;
      }
      const T nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
      d += (nx * nx + ny * ny + nz * nz) * P.inv_sn2;
      if (!pmiss && np.w != nq.w)
        d += dn_abs(np.w - nq.w) / (P.sigma_depth * dn_abs(g.x * (T)(s * i) + g.y * (T)(s * j)) + ez);
      const T w = dn_h<T>(i) * dn_h<T>(j) * dn_exp(-d);
      sw += w;
      sr += w * cq.x;
      sg += w * cq.y;
      sb += w * cq.z;
      sv += w * w * cq.w;
    }
  }
  DnV4<T> o;
  if (sw > (T)0) {
    o.x = sr / sw;
    o.y = sg / sw;
    o.z = sb / sw;
    o.w = sv / (sw * sw);
  } else {  // no tap left
    o.x = o.y = o.z = o.w = (T)0;
  }
  return o;
}

// The end of the last pass: the filtered colour times the pixel's albedo factor, 3 T into out.
template <class T>
__host__ __device__ inline void dn_remodulate(const DnParams<T>& P, const double* f, const DnV4<T>& c, T* out) {
  T a[3];
  dn_albedo(P, f, a);
  out[0] = c.x * a[0];
  out[1] = c.y * a[1];
  out[2] = c.z * a[2];
}

// rt_denoise's passes as a host loop over the functions above (checked parameters; rgb_out may be rgb_in).
template <class T>
inline void denoise_host(const rt_denoise_params& prm, const T* rgb_in, const double* feat, const double* var,
                         T* rgb_out) {
  const DnParams<T> P = dn_params<T>(prm);
  const size_t npix = (size_t)P.W * P.H;
  std::vector<DnV4<T>> c0(npix), c1(npix), n(npix);
  std::vector<DnV2<T>> g(npix);
  for (int y = 0; y < P.H; y++)
    for (int x = 0; x < P.W; x++) {
      const size_t p = (size_t)y * P.W + x;
      dn_prepare_pixel(P, rgb_in, feat, var, x, y, c0[p], n[p], g[p]);
    }
  DnV4<T>*src = c0.data(), *dst = c1.data();
  for (int k = 0; k < prm.iterations; k++) {
    for (int y = 0; y < P.H; y++)
      for (int x = 0; x < P.W; x++) dst[(size_t)y * P.W + x] = dn_atrous_pixel(P, src, n.data(), g.data(), x, y, 1 << k);
    DnV4<T>* t = src;
    src = dst;
    dst = t;
  }
  for (size_t p = 0; p < npix; p++) dn_remodulate(P, feat + 8 * p, src[p], rgb_out + 3 * p);
}

}  // namespace rtd
