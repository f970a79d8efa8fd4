// rt_temporal.h -- the arithmetic of rt_temporal (include/rt_hip.h, "temporal accumulation"), the one copy the kernel
// (rt_temporal.hip) and the host loop (temporal_host, rt_dev_temporal_host) run: the whole per-pixel step -- current
// sample, reprojection, the four history taps, blend -- templated on the working type T (float for RT_PREC_F32,
// double for RT_PREC_F64), the history's layout, and the parameter and camera rules. No HIP: a plain C++ compiler
// takes this header (tests/native/temporal_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/rt_hip.h"

// a plain C++ compiler knows no function qualifiers
#if !defined(__HIP__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace rtd {

// A record of the two record planes, {c.r, c.g, c.b, v} or {n.x, n.y, n.z, z}: 16 bytes (fp32) or 32 bytes (fp64),
// read and written whole. Aligned to 16 bytes only, which is what the call asks of the history's address.
template <class T>
struct alignas(16) TpRec {
  T x, y, z, w;
};

constexpr int32_t kTpUnknownId = -2;  // the id plane's value when the frame came without ids

// The four planes of a history of npix pixels at `base` (include/rt_hip.h)
template <class T>
struct TpHist {
  TpRec<T>* C;   // {c, v}
  TpRec<T>* G;   // {n, z}
  T* N;          // the count
  int32_t* id;   // the object id
};
template <class T>
__host__ __device__ inline TpHist<T> tp_planes(void* base, size_t npix) {
  TpHist<T> h{};
  if (!base) return h;  // a first frame: no history to read
  h.C = (TpRec<T>*)base;
  h.G = h.C + npix;
  h.N = (T*)(h.G + npix);
  h.id = (int32_t*)(h.N + npix);
  return h;
}
inline size_t tp_history_bytes(size_t npix, bool f64) { return npix * (9 * (f64 ? 8 : 4) + 4); }

// What the per-pixel step needs of the parameters and the two cameras
template <class T>
struct TpParams {
  int32_t W, H;
  int32_t demod;
  int32_t have_hist;  // hist_in given
  int32_t same_cam;   // *cam and *prev_cam byte-equal: (fx, fy) = (x, y), z' = z
  T albedo_eps, alpha_min, min_weight, max_history;
  double depth_tol, normal_cos;
  // this frame's camera: d_c = fd + u rw + v uh with u = (x + 0.5) / W - 0.5, v = 0.5 - (y + 0.5) / H
  double pos[3], fd[3], rw[3], uh[3];
  // the camera before: A = r . pa, B f' / vw' = r . pb, C f' / vh' = r . pc
  double ppos[3], pa[3], pb[3], pc[3];
};

template <class T>
inline TpParams<T> tp_params(const rt_temporal_params& p, const rt_camera_desc* cam, const rt_camera_desc* prev,
                             bool have_hist) {
  TpParams<T> d{};
  d.W = p.width;
  d.H = p.height;
  d.demod = (p.flags & RT_TEMPORAL_DEMODULATE) != 0;
  d.have_hist = have_hist && prev;
  d.same_cam = d.have_hist && memcmp(cam, prev, sizeof(rt_camera_desc)) == 0;
  d.albedo_eps = (T)p.albedo_eps;
  d.alpha_min = (T)p.alpha_min;
  d.min_weight = (T)p.min_weight;
  d.max_history = (T)p.max_history;
  d.depth_tol = p.depth_tol;
  d.normal_cos = p.normal_cos;
  if (d.have_hist && !d.same_cam) {
    auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    const double dd = dot(prev->dir, prev->dir), rr = dot(prev->right, prev->right), uu = dot(prev->up, prev->up);
    for (int k = 0; k < 3; k++) {
      d.pos[k] = cam->pos[k];
      d.fd[k] = cam->focal_length * cam->dir[k];
      d.rw[k] = cam->viewport_width * cam->right[k];
      d.uh[k] = cam->viewport_height * cam->up[k];
      d.ppos[k] = prev->pos[k];
      d.pa[k] = prev->dir[k] / dd;
      d.pb[k] = prev->right[k] / rr * (prev->focal_length / prev->viewport_width);
      d.pc[k] = prev->up[k] / uu * (prev->focal_length / prev->viewport_height);
    }
  }
  return d;
}

// The parameter rules of rt_temporal_params (rt_temporal_check): nullptr, or what is wrong with them.
inline const char* temporal_params_error(const rt_temporal_params& p) {
  auto finite = [](double x) { return x - x == 0.0; };
  if (p.width < 1 || p.height < 1) return "empty image";
  if (p.width > 65535 || p.height > 65535) return "image wider or taller than 65535 pixels";
  if ((int64_t)p.width * p.height >= (1ll << 31)) return "width * height outside [1, 2^31)";
  if (p.precision != RT_PREC_F32 && p.precision != RT_PREC_F64) return "unknown precision";
  if (p.flags & ~RT_TEMPORAL_DEMODULATE) return "unknown flag";
  if (p.max_history < 1) return "max_history must be at least 1";
  if (!(p.alpha_min >= 0.0 && p.alpha_min <= 1.0)) return "alpha_min outside [0, 1]";
  if (!finite(p.depth_tol) || !(p.depth_tol > 0.0)) return "depth_tol must be positive and finite";
  if (!(p.normal_cos >= -1.0 && p.normal_cos <= 1.0)) return "normal_cos outside [-1, 1]";
  if (!(p.min_weight >= 0.0 && p.min_weight < 1.0)) return "min_weight outside [0, 1)";
  if (!finite(p.albedo_eps) || !(p.albedo_eps >= 0.0)) return "albedo_eps must be >= 0 and finite";
  if ((p.flags & RT_TEMPORAL_DEMODULATE) && !(p.albedo_eps > 0.0)) return "albedo_eps must be positive when demodulating";
  return nullptr;
}
// The camera rule (step 2), for checked parameters and a prev that is not null: nullptr, or what is unsupported.
inline const char* temporal_camera_error(const rt_temporal_params& p, const rt_camera_desc& cam,
                                         const rt_camera_desc& prev) {
  if (memcmp(&cam, &prev, sizeof(rt_camera_desc)) == 0) return nullptr;
  if (cam.mode != RT_CAM_PERSPECTIVE || prev.mode != RT_CAM_PERSPECTIVE)
    return "cameras that differ must both be perspective cameras";
  if (cam.image_width != p.width || cam.image_height != p.height || prev.image_width != p.width ||
      prev.image_height != p.height)
    return "cameras that differ must both have the image size of the parameters";
  return nullptr;
}

// What rt_temporal_check says of the parameters and the cameras (prev may be null: a first frame): RT_OK, or the
// status with the reason in *why.
inline rt_status temporal_check(const rt_temporal_params* prm, const rt_camera_desc* cam, const rt_camera_desc* prev,
                                const char** why) {
  *why = !prm || !cam ? "null argument" : temporal_params_error(*prm);
  if (*why) return RT_ERR_INVALID_ARGUMENT;
  *why = prev ? temporal_camera_error(*prm, *cam, *prev) : nullptr;
  return *why ? RT_ERR_UNSUPPORTED : RT_OK;
}

// [a, a + n) and [b, b + n) share a byte
inline bool tp_overlap(const void* a, const void* b, size_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < n : x - y < n;
}

template <class T>
__host__ __device__ inline bool tp_finite(T x) {
  return x - x == (T)0;
}

// What the step leaves of pixel p: its history record, rgb_out and var_out
template <class T>
struct TpOut {
  TpRec<T> c, g;
  T N;
  int32_t id;
  T rgb[3];
  double var;
};

// The whole step at pixel (x, y). rgb npix x 3 T, feat npix x 8 doubles (rows aligned to 16 bytes), ids npix x 4
// int32 or null, var npix doubles or null, Hin the history of the frame before (read only with P.have_hist).
template <class T>
__host__ __device__ inline TpOut<T> tp_pixel(const TpParams<T>& P, const T* rgb, const double* feat,
                                             const int32_t* ids, const double* var, const TpHist<T>& Hin, int x,
                                             int y) {
  const int W = P.W, H = P.H;
  const size_t p = (size_t)y * W + x;
  // ---- 1. the current sample (the row as whole 16-byte loads)
  const double* fr = (const double*)__builtin_assume_aligned(feat + 8 * p, 16);
  double f[8];
  for (int k = 0; k < 8; k++) f[k] = fr[k];
  T a[3], cc[3];
  for (int k = 0; k < 3; k++) {
    a[k] = P.demod ? (T)f[k] + P.albedo_eps : (T)1;
    cc[k] = rgb[3 * p + k] / a[k];
  }
  const T m = (a[0] + a[1] + a[2]) / (T)3;
  const T vc = var ? (T)var[p] / (T)3 / (m * m) : (T)1;
  const T hit = (T)f[7];
  const bool miss = !(hit > (T)0);
  TpOut<T> o;
  o.g.x = miss ? (T)0 : (T)f[3] / hit;
  o.g.y = miss ? (T)0 : (T)f[4] / hit;
  o.g.z = miss ? (T)0 : (T)f[5] / hit;
  o.g.w = miss ? (T)-1 : (T)f[6] / hit;
  o.id = ids ? ids[4 * p] : kTpUnknownId;
  const bool cur_ok = tp_finite(cc[0]) && tp_finite(cc[1]) && tp_finite(cc[2]) && tp_finite(vc);

  // ---- 2. where p was, in double
  bool look = P.have_hist != 0;
  double fx = (double)x, fy = (double)y, zp = (double)o.g.w;
  if (look && !P.same_cam) {
    const double u = ((double)x + 0.5) / (double)W - 0.5, v = 0.5 - ((double)y + 0.5) / (double)H;
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = P.fd[k] + u * P.rw[k] + v * P.uh[k];
    if (!miss) {
      const double s = (double)o.g.w / sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      for (int k = 0; k < 3; k++) r[k] = P.pos[k] + r[k] * s - P.ppos[k];
      zp = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    const double A = r[0] * P.pa[0] + r[1] * P.pa[1] + r[2] * P.pa[2];
    const double B = r[0] * P.pb[0] + r[1] * P.pb[1] + r[2] * P.pb[2];
    const double C = r[0] * P.pc[0] + r[1] * P.pc[1] + r[2] * P.pc[2];
    fx = (B / A + 0.5) * (double)W - 0.5;
    fy = (0.5 - C / A) * (double)H - 0.5;
    look = A > 0.0;
  }
  // (every tap of a position outside (-1, W) x (-1, H) is outside the image; a NaN position fails the comparisons)
  look = look && fx > -1.0 && fx < (double)W && fy > -1.0 && fy < (double)H;

  // ---- 3. the taps
  T Wv = 0, sr = 0, sg = 0, sb = 0, sv = 0, sn = 0;
  if (look) {
    const double x0f = floor(fx), y0f = floor(fy);
    const int x0 = (int)x0f, y0 = (int)y0f;  // in [-1, W - 1] x [-1, H - 1]
    const double tx = fx - x0f, ty = fy - y0f;
    for (int j = 0; j < 2; j++) {
      const int qy = y0 + j;
      if (qy < 0 || qy >= H) continue;
      for (int i = 0; i < 2; i++) {
        const int qx = x0 + i;
        if (qx < 0 || qx >= W) continue;
        const double wd = (i ? tx : 1.0 - tx) * (j ? ty : 1.0 - ty);
        if (wd == 0.0) continue;
        const size_t q = (size_t)qy * W + qx;
        const TpRec<T> cq = Hin.C[q], gq = Hin.G[q];
        const T nq = Hin.N[q];
        const int32_t idq = Hin.id[q];
        if (!(tp_finite(cq.x) && tp_finite(cq.y) && tp_finite(cq.z) && tp_finite(cq.w)) || !(nq > (T)0)) continue;
        if (miss) {
          if (!(gq.w < (T)0)) continue;
        } else {
          const double zq = (double)gq.w;
          if (!(zq >= 0.0) || !(fabs(zq - zp) <= P.depth_tol * zp)) continue;
          const double nd = (double)o.g.x * (double)gq.x + (double)o.g.y * (double)gq.y + (double)o.g.z * (double)gq.z;
          if (!(nd >= P.normal_cos)) continue;
          if (o.id != idq && o.id != kTpUnknownId && idq != kTpUnknownId) continue;
        }
        const T w = (T)wd;
        Wv += w;
        sr += w * cq.x;
        sg += w * cq.y;
        sb += w * cq.z;
        sv += w * w * cq.w;
        sn += w * nq;
      }
    }
  }

  // ---- 4. the blend
  if (Wv >= P.min_weight && Wv > (T)0) {
    const T ch[3] = {sr / Wv, sg / Wv, sb / Wv};
    const T vh = sv / (Wv * Wv), nh = sn / Wv;
    if (cur_ok) {
      const T one = (T)1, inv = one / (nh + one);
      const T alpha = P.alpha_min > inv ? P.alpha_min : inv;
      const T keep = one - alpha;
      o.c.x = keep * ch[0] + alpha * cc[0];
      o.c.y = keep * ch[1] + alpha * cc[1];
      o.c.z = keep * ch[2] + alpha * cc[2];
      o.c.w = keep * keep * vh + alpha * alpha * vc;
      o.N = nh + one < P.max_history ? nh + one : P.max_history;
    } else {  // the frame contributes nothing
      o.c.x = ch[0];
      o.c.y = ch[1];
      o.c.z = ch[2];
      o.c.w = vh;
      o.N = nh;
    }
  } else {
    o.c.x = cc[0];
    o.c.y = cc[1];
    o.c.z = cc[2];
    o.c.w = vc;
    o.N = cur_ok ? (T)1 : (T)0;
  }

  // ---- 5. the outputs
  o.rgb[0] = o.c.x * a[0];
  o.rgb[1] = o.c.y * a[1];
  o.rgb[2] = o.c.z * a[2];
  o.var = (double)((T)3 * (m * m) * o.c.w);
  return o;
}

// One pixel's results into the caller's arrays (rgb_out may be the rgb the step read, var_out its var: a pixel reads
// only its own entry of either, before this).
template <class T>
__host__ __device__ inline void tp_store(const TpOut<T>& o, size_t p, const TpHist<T>& Hout, T* rgb_out,
                                         double* var_out) {
  Hout.C[p] = o.c;
  Hout.G[p] = o.g;
  Hout.N[p] = o.N;
  Hout.id[p] = o.id;
  rgb_out[3 * p] = o.rgb[0];
  rgb_out[3 * p + 1] = o.rgb[1];
  rgb_out[3 * p + 2] = o.rgb[2];
  if (var_out) var_out[p] = o.var;
}

// rt_temporal as a host loop over the functions above (checked parameters and cameras; hist_in null or not
// overlapping hist_out).
template <class T>
inline void temporal_host(const rt_temporal_params& prm, const rt_camera_desc* cam, const rt_camera_desc* prev,
                          const T* rgb_in, const double* feat, const int32_t* ids, const double* var,
                          const void* hist_in, void* hist_out, T* rgb_out, double* var_out) {
  const TpParams<T> P = tp_params<T>(prm, cam, prev, hist_in != nullptr);
  const size_t npix = (size_t)P.W * P.H;
  const TpHist<T> Hin = tp_planes<T>((void*)hist_in, npix), Hout = tp_planes<T>(hist_out, npix);
  for (int y = 0; y < P.H; y++)
    for (int x = 0; x < P.W; x++)
      tp_store(tp_pixel(P, rgb_in, feat, ids, var, Hin, x, y), (size_t)y * P.W + x, Hout, rgb_out, var_out);
}

}  // namespace rtd
