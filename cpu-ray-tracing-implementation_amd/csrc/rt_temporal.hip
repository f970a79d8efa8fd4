// rt_temporal.hip -- the kernel of rt_temporal (include/rt_hip.h, "temporal accumulation"): one fused launch over
// rt_temporal.h's per-pixel step, its launch function, and the three host-only entry points (rt_temporal_check,
// rt_temporal_history_bytes, rt_dev_temporal_host). rt_temporal itself, which stages a host-pointer call in the
// context's buffers, is in rt_render.hip, which includes this file at its end: the two are one translation unit
// (Makefile).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/rt_hip.h"
#include "rt_launch.h"
#include "rt_temporal.h"

namespace rtd {

namespace {

// k_atrous' tile: a wave is 64 consecutive x of one row, a block a 64 x 4 tile. A wave's reads of the frame (feat
// rows of 64 B, rgb, var, ids) and its writes (two records, the count, the id, rgb, var) are contiguous runs. The
// reprojected position is smooth in p, so the wave's four taps are, away from a depth edge, four more runs of about
// 64 consecutive records in two adjacent rows of each history plane: each record is fetched whole (one 16-byte load
// in fp32, two in fp64) and neighbouring lanes share three of their four taps through the caches.
constexpr int kTpTileW = 64, kTpTileH = kBlock / kTpTileW;
static_assert(kBlock == 256, "a block is a 64 x 4 tile");

template <class T>
__global__ __launch_bounds__(kBlock) void k_temporal(TpParams<T> P, const T* rgb, const double* __restrict__ feat,
                                                     const int32_t* __restrict__ ids, const double* var,
                                                     TpHist<T> Hin, TpHist<T> Hout, T* rgb_out, double* var_out) {
  const int x = (int)(blockIdx.x * kTpTileW + (threadIdx.x & (kTpTileW - 1)));
  const int y = (int)(blockIdx.y * kTpTileH + threadIdx.x / kTpTileW);
  if (x >= P.W || y >= P.H) return;
  // (rgb_out may be rgb and var_out var: neither pair is __restrict__; a pixel reads its own entries before it writes)
  tp_store(tp_pixel(P, rgb, feat, ids, var, Hin, x, y), (size_t)y * P.W + x, Hout, rgb_out, var_out);
}

}  // namespace

template <class T>
void launch_temporal(const rt_temporal_params& prm, const rt_camera_desc* cam, const rt_camera_desc* prev,
                     const T* rgb_in, const double* feat, const int32_t* ids, const double* var, const void* hist_in,
                     void* hist_out, T* rgb_out, double* var_out, hipStream_t st) {
  const TpParams<T> P = tp_params<T>(prm, cam, prev, hist_in != nullptr);
  const size_t npix = (size_t)P.W * P.H;
  const dim3 grid((uint32_t)((P.W + kTpTileW - 1) / kTpTileW), (uint32_t)((P.H + kTpTileH - 1) / kTpTileH));
  hipLaunchKernelGGL(k_temporal<T>, grid, dim3(kBlock), 0, st, P, rgb_in, feat, ids, var,
                     tp_planes<T>((void*)hist_in, npix), tp_planes<T>(hist_out, npix), rgb_out, var_out);
}
template void launch_temporal<float>(const rt_temporal_params&, const rt_camera_desc*, const rt_camera_desc*,
                                     const float*, const double*, const int32_t*, const double*, const void*, void*,
                                     float*, double*, hipStream_t);
template void launch_temporal<double>(const rt_temporal_params&, const rt_camera_desc*, const rt_camera_desc*,
                                      const double*, const double*, const int32_t*, const double*, const void*, void*,
                                      double*, double*, hipStream_t);

}  // namespace rtd

extern "C" {

rt_status rt_temporal_check(const rt_temporal_params* prm, const rt_camera_desc* cam, const rt_camera_desc* prev_cam,
                            char* why, size_t n) {
  const char* m = nullptr;
  const rt_status s = rtd::temporal_check(prm, cam, prev_cam, &m);
  if (why && n > 0) std::snprintf(why, n, "%s", m ? m : "");
  return s;
}

size_t rt_temporal_history_bytes(int32_t width, int32_t height, int32_t precision) {
  rt_temporal_params p{};
  p.width = width;
  p.height = height;
  p.precision = precision;
  p.max_history = 1;
  p.depth_tol = 1.0;
  if (rtd::temporal_params_error(p)) return 0;
  return rtd::tp_history_bytes((size_t)width * (size_t)height, precision == RT_PREC_F64);
}

// rt_temporal as a host loop over the same functions (rt_temporal.h temporal_host), for tests: host pointers, no
// device, no stability promise. The history's address must be a multiple of 16, like a device call's.
rt_status rt_dev_temporal_host(const rt_temporal_params* prm, const rt_camera_desc* cam, const rt_camera_desc* prev_cam,
                               const void* rgb_in, const double* feat, const int32_t* ids, const double* var,
                               const void* hist_in, void* hist_out, void* rgb_out, double* var_out) {
  const char* m;
  if (!rgb_in || !feat || !hist_out || !rgb_out || (hist_in && !prev_cam)) return RT_ERR_INVALID_ARGUMENT;
  const rt_status s = rtd::temporal_check(prm, cam, hist_in ? prev_cam : nullptr, &m);
  if (s != RT_OK) return s;
  const size_t hb = rtd::tp_history_bytes((size_t)prm->width * (size_t)prm->height, prm->precision == RT_PREC_F64);
  if (hist_in && rtd::tp_overlap(hist_in, hist_out, hb)) return RT_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)hist_in | (uintptr_t)hist_out | (uintptr_t)feat) % 16 != 0) return RT_ERR_INVALID_ARGUMENT;
  if (prm->precision == RT_PREC_F64)
    rtd::temporal_host<double>(*prm, cam, prev_cam, (const double*)rgb_in, feat, ids, var, hist_in, hist_out,
                               (double*)rgb_out, var_out);
  else
    rtd::temporal_host<float>(*prm, cam, prev_cam, (const float*)rgb_in, feat, ids, var, hist_in, hist_out,
                              (float*)rgb_out, var_out);
  return RT_OK;
}

}  // extern "C"
