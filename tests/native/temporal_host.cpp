// Runs rt_temporal on the host (csrc/rt_temporal.h temporal_host: the function the kernel runs) over three generated
// frames of a moving camera whose arrays, the histories included, are exactly as long as the image needs, so that a
// tap that indexes outside the image is a heap overflow the address sanitizer sees (tests/test_temporal_abi.py).
//   temporal_host W H use_var use_ids f64  -> text: "finite_pixels npix pixels_with_history sum"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_temporal.h"

static rt_camera_desc camera(int W, int H, double x, double yaw) {
  rt_camera_desc c{};
  c.mode = RT_CAM_PERSPECTIVE;
  c.image_width = W;
  c.image_height = H;
  c.pos[0] = x;
  c.pos[1] = 1.0;
  c.dir[0] = std::sin(yaw);
  c.dir[2] = -std::cos(yaw);
  c.right[0] = std::cos(yaw);
  c.right[2] = std::sin(yaw);
  c.up[1] = 1.0;
  c.viewport_height = 1.4;
  c.viewport_width = 1.4 * W / H;
  c.focal_length = 1.0;
  return c;
}

template <class T>
int run(const rt_temporal_params& prm, bool use_var, bool use_ids) {
  const int W = prm.width, H = prm.height;
  const size_t npix = (size_t)W * H;
  const size_t hb = rtd::tp_history_bytes(npix, sizeof(T) == 8);
  std::vector<T> rgb(3 * npix), out(3 * npix);
  std::vector<double> feat(8 * npix), var(npix), var_out(npix);
  std::vector<int32_t> ids(4 * npix);
  // (operator new aligns to 16 bytes, what the records ask for)
  std::vector<unsigned char> h0(hb), h1(hb);
  uint32_t s = 4321u + (uint32_t)W * 977u + (uint32_t)H;
  auto rnd = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0;
  };
  rt_camera_desc prev{};
  unsigned char *hin = nullptr, *hout = h0.data();
  size_t fin = 0, with = 0;
  double sum = 0;
  for (int k = 0; k < 3; k++) {
    // a sideways step, then a yaw that sends part of the image outside; the third frame stands still
    const rt_camera_desc cam = camera(W, H, k == 0 ? 0.0 : 0.4, k == 0 ? 0.0 : 0.3);
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const size_t p = (size_t)y * W + x;
        const bool miss = npix > 2 && (x + 2 * y) % 7 == 3;
        const double hit = miss ? 0.0 : ((x + y) % 5 == 0 ? 0.5 : 1.0);
        double* f = &feat[8 * p];
        f[0] = 0.2 + 0.6 * rnd();
        f[1] = 0.5;
        f[2] = 0.7;
        f[3] = 0.0;
        f[4] = hit * (x < W / 2 ? 1.0 : 0.0);
        f[5] = hit * (x < W / 2 ? 0.0 : 1.0);
        f[6] = hit * (4.0 + 0.05 * x + 0.08 * y);
        f[7] = hit;
        for (int c = 0; c < 3; c++) rgb[3 * p + c] = (T)(f[c] * (0.8 + 0.4 * rnd()));
        var[p] = 0.01 * rnd();
        ids[4 * p] = miss ? -1 : (x < W / 2 ? 0 : 1);
      }
    if (npix > 4) rgb[3 * (npix / 2)] = (T)std::nan("");  // one broken pixel a frame
    const char* why = nullptr;
    if (rtd::temporal_check(&prm, &cam, hin ? &prev : nullptr, &why) != RT_OK) {
      std::fprintf(stderr, "%s\n", why);
      return 2;
    }
    rtd::temporal_host<T>(prm, &cam, &prev, rgb.data(), feat.data(), use_ids ? ids.data() : nullptr,
                          use_var ? var.data() : nullptr, hin, hout, out.data(), var_out.data());
    // in place: rgb_out = rgb_in and var_out = var give the same image and the same history
    std::vector<unsigned char> again(hb);
    std::vector<double> v2(var);
    rtd::temporal_host<T>(prm, &cam, &prev, rgb.data(), feat.data(), use_ids ? ids.data() : nullptr,
                          use_var ? v2.data() : nullptr, hin, again.data(), rgb.data(), use_var ? v2.data() : nullptr);
    const rtd::TpHist<T> a = rtd::tp_planes<T>(hout, npix), b = rtd::tp_planes<T>(again.data(), npix);
    for (size_t p = 0; p < npix; p++) {
      bool same = a.N[p] == b.N[p] && a.id[p] == b.id[p];
      for (int c = 0; c < 3; c++)
        same = same && (rgb[3 * p + c] == out[3 * p + c] || !(rtd::tp_finite(rgb[3 * p + c]) || rtd::tp_finite(out[3 * p + c])));
      if (use_var) same = same && (v2[p] == var_out[p] || !(rtd::tp_finite(v2[p]) || rtd::tp_finite(var_out[p])));
      if (!same) {
        std::fprintf(stderr, "in-place result differs at pixel %zu of frame %d\n", p, k);
        return 1;
      }
    }
    if (k == 2)
      for (size_t p = 0; p < npix; p++) {
        const bool ok = rtd::tp_finite(out[3 * p]) && rtd::tp_finite(out[3 * p + 1]) && rtd::tp_finite(out[3 * p + 2]);
        fin += ok;
        with += a.N[p] > (T)1;
        if (ok) sum += (double)out[3 * p] + (double)out[3 * p + 1] + (double)out[3 * p + 2];
      }
    prev = cam;
    hin = hout;
    hout = hout == h0.data() ? h1.data() : h0.data();
  }
  std::printf("%zu %zu %zu %.17g\n", fin, npix, with, sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: temporal_host W H use_var use_ids f64\n");
    return 2;
  }
  rt_temporal_params prm{};
  prm.width = std::atoi(argv[1]);
  prm.height = std::atoi(argv[2]);
  const bool use_var = std::atoi(argv[3]) != 0, use_ids = std::atoi(argv[4]) != 0, f64 = std::atoi(argv[5]) != 0;
  prm.precision = f64 ? RT_PREC_F64 : RT_PREC_F32;
  prm.flags = RT_TEMPORAL_DEMODULATE;
  prm.max_history = 64;
  prm.alpha_min = 0.05;
  prm.depth_tol = 0.1;
  prm.normal_cos = 0.9;
  prm.min_weight = 0.25;
  prm.albedo_eps = 1e-2;
  return f64 ? run<double>(prm, use_var, use_ids) : run<float>(prm, use_var, use_ids);
}
