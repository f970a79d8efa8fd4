// rt_denoise.hip -- the kernels of rt_denoise (include/rt_hip.h, "denoising"): the prepare pass and the a-trous
// passes over rt_denoise.h's per-pixel functions, their launch function, and the two host-only entry points
// (rt_denoise_check, rt_dev_denoise_host). rt_denoise itself, which owns the context's scratch, is in rt_render.hip,
// which includes this file at its end: the two are one translation unit (Makefile).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/rt_hip.h"
#include "rt_denoise.h"
#include "rt_launch.h"

namespace rtd {

namespace {

// A wave is 64 consecutive x of one row, a block a 64 x 4 tile: a wave's row of taps is one contiguous run of
// records at every step s (s only shifts it), so the 25 gathers of a pass are coalesced as they stand.
constexpr int kDnTileW = 64, kDnTileH = kBlock / kDnTileW;
static_assert(kBlock == 256, "a block is a 64 x 4 tile");

template <class T>
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(DnParams<T> P, const T* __restrict__ rgb,
                                                            const double* __restrict__ feat,
                                                            const double* __restrict__ var, DnV4<T>* __restrict__ C,
                                                            DnV4<T>* __restrict__ N, DnV2<T>* __restrict__ G) {
  const int x = (int)(blockIdx.x * kDnTileW + (threadIdx.x & (kDnTileW - 1)));
  const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
  if (x >= P.W || y >= P.H) return;
  const size_t p = (size_t)y * P.W + x;
  DnV4<T> c, n;
  DnV2<T> g;
  dn_prepare_pixel(P, rgb, feat, var, x, y, c, n, g);
  C[p] = c;
  N[p] = n;
  G[p] = g;
}

// One pass with step s. LAST: the filtered colour goes, times the albedo factor, to the caller's image (3 T a pixel)
// instead of the other colour buffer.
template <class T, bool LAST>
__global__ __launch_bounds__(kBlock) void k_atrous(DnParams<T> P, const DnV4<T>* __restrict__ C,
                                                   const DnV4<T>* __restrict__ N, const DnV2<T>* __restrict__ G, int s,
                                                   DnV4<T>* __restrict__ C_out, const double* __restrict__ feat,
                                                   T* __restrict__ rgb_out) {
  const int x = (int)(blockIdx.x * kDnTileW + (threadIdx.x & (kDnTileW - 1)));
  const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
  if (x >= P.W || y >= P.H) return;
  const size_t p = (size_t)y * P.W + x;
  const DnV4<T> o = dn_atrous_pixel(P, C, N, G, x, y, s);
  if (LAST)
    dn_remodulate(P, feat + 8 * p, o, rgb_out + 3 * p);
  else
    C_out[p] = o;
}

}  // namespace

template <class T>
void launch_denoise(const rt_denoise_params& prm, const T* rgb_in, const double* feat, const double* var, T* scratch,
                    T* rgb_out, hipStream_t st) {
  const DnParams<T> P = dn_params<T>(prm);
  const size_t npix = (size_t)P.W * P.H;
  DnV4<T>* C[2] = {(DnV4<T>*)scratch, (DnV4<T>*)scratch + npix};
  DnV4<T>* N = (DnV4<T>*)scratch + 2 * npix;
  DnV2<T>* G = (DnV2<T>*)((DnV4<T>*)scratch + 3 * npix);
  const dim3 grid((uint32_t)((P.W + kDnTileW - 1) / kDnTileW), (uint32_t)((P.H + kDnTileH - 1) / kDnTileH));
  hipLaunchKernelGGL(k_denoise_prepare<T>, grid, dim3(kBlock), 0, st, P, rgb_in, feat, var, C[0], N, G);
  for (int k = 0; k < prm.iterations; k++) {
    if (k + 1 < prm.iterations)
      hipLaunchKernelGGL((k_atrous<T, false>), grid, dim3(kBlock), 0, st, P, C[k & 1], N, G, 1 << k, C[~k & 1],
                         (const double*)nullptr, (T*)nullptr);
    else
      hipLaunchKernelGGL((k_atrous<T, true>), grid, dim3(kBlock), 0, st, P, C[k & 1], N, G, 1 << k,
                         (DnV4<T>*)nullptr, feat, rgb_out);
  }
}
template void launch_denoise<float>(const rt_denoise_params&, const float*, const double*, const double*, float*,
                                    float*, hipStream_t);
template void launch_denoise<double>(const rt_denoise_params&, const double*, const double*, const double*, double*,
                                     double*, hipStream_t);

}  // namespace rtd

extern "C" {

rt_status rt_denoise_check(const rt_denoise_params* prm, char* why, size_t n) {
  const char* m = prm ? rtd::denoise_params_error(*prm) : "null parameters";
  if (why && n > 0) std::snprintf(why, n, "%s", m ? m : "");
  return m ? RT_ERR_INVALID_ARGUMENT : RT_OK;
}

// rt_denoise's passes as a host loop over the same functions (rt_denoise.h denoise_host), for tests: host pointers,
// no device, no stability promise.
rt_status rt_dev_denoise_host(const rt_denoise_params* prm, const void* rgb_in, const double* feat, const double* var,
                              void* rgb_out) {
  if (!prm || !rgb_in || !feat || !rgb_out || rtd::denoise_params_error(*prm)) return RT_ERR_INVALID_ARGUMENT;
  if (prm->precision == RT_PREC_F64)
    rtd::denoise_host<double>(*prm, (const double*)rgb_in, feat, var, (double*)rgb_out);
  else
    rtd::denoise_host<float>(*prm, (const float*)rgb_in, feat, var, (float*)rgb_out);
  return RT_OK;
}

}  // extern "C"
