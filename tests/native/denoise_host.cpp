// Runs rt_denoise's passes on the host (csrc/rt_denoise.h denoise_host: the functions the kernels run) over a
// generated frame whose arrays are exactly as long as the image needs, so that a border tap that indexes outside
// the image is a heap overflow the address sanitizer sees (tests/test_denoise_abi.py).
//   denoise_host W H iterations use_var f64  -> text: "finite_pixels npix sum"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_denoise.h"

template <class T>
int run(const rt_denoise_params& prm, bool use_var) {
  const int W = prm.width, H = prm.height;
  const size_t npix = (size_t)W * H;
  std::vector<T> rgb(3 * npix), out(3 * npix);
  std::vector<double> feat(8 * npix), var(npix);
  uint32_t s = 12345u + (uint32_t)W * 977u + (uint32_t)H;
  auto rnd = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0;
  };
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
      for (int k = 0; k < 3; k++) rgb[3 * p + k] = (T)(f[k] * (0.8 + 0.4 * rnd()));
      var[p] = 0.01 * rnd();
    }
  if (npix > 4) rgb[3 * (npix / 2)] = (T)std::nan("");  // one broken pixel
  rtd::denoise_host<T>(prm, rgb.data(), feat.data(), use_var ? var.data() : nullptr, out.data());
  size_t fin = 0;
  double sum = 0;
  for (size_t p = 0; p < npix; p++) {
    const bool ok = rtd::dn_finite(out[3 * p]) && rtd::dn_finite(out[3 * p + 1]) && rtd::dn_finite(out[3 * p + 2]);
    fin += ok;
    if (ok) sum += (double)out[3 * p] + (double)out[3 * p + 1] + (double)out[3 * p + 2];
  }
  // in place: rgb_out = rgb_in gives the same image
  rtd::denoise_host<T>(prm, rgb.data(), feat.data(), use_var ? var.data() : nullptr, rgb.data());
  for (size_t k = 0; k < 3 * npix; k++)
    if (!(rgb[k] == out[k]) && (rtd::dn_finite(rgb[k]) || rtd::dn_finite(out[k]))) {
      std::fprintf(stderr, "in-place result differs at %zu\n", k);
      return 1;
    }
  std::printf("%zu %zu %.17g\n", fin, npix, sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: denoise_host W H iterations use_var f64\n");
    return 2;
  }
  rt_denoise_params prm{};
  prm.width = std::atoi(argv[1]);
  prm.height = std::atoi(argv[2]);
  prm.iterations = std::atoi(argv[3]);
  const bool use_var = std::atoi(argv[4]) != 0, f64 = std::atoi(argv[5]) != 0;
  prm.precision = f64 ? RT_PREC_F64 : RT_PREC_F32;
  prm.flags = RT_DENOISE_DEMODULATE;
  prm.sigma_color = 2.0;
  prm.sigma_normal = 0.5;
  prm.sigma_depth = 1.0;
  prm.albedo_eps = 1e-2;
  prm.color_eps = 1e-8;
  prm.depth_eps = 1e-3;
  if (const char* m = rtd::denoise_params_error(prm)) {
    std::fprintf(stderr, "%s\n", m);
    return 2;
  }
  return f64 ? run<double>(prm, use_var) : run<float>(prm, use_var);
}
