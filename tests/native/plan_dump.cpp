// Answers questions about csrc/rt_plan.h (tests/test_plan.py), one per input line:
//   P spp samples_per_item flat full_pixels npix elem budget   -> the item plan (budget 0: the default)
//   D d n                                                       -> (n * m) >> k of div_magic(d)
//   F has_flat n_linear n_spheres n_tris has_volumes has_wide n_texdata has_cell_noise cam_mode persist ordered
//                                                               -> the kernel family and its name
#include <cinttypes>
#include <cstdio>

#include "rt_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[11] = {};
    const int n = std::sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3,
                              a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10);
    if (line[0] == 'P' && n == 7) {
      rtd::PlanKnobs kn;
      if (a[6]) kn.partial_budget = a[6];
      const rtd::ItemPlan p = rtd::plan_items((uint32_t)a[0], (int32_t)a[1], a[2] != 0, a[3], (uint32_t)a[4],
                                              (uint32_t)a[5], kn);
      std::printf("%u %u %u %u %u %u %" PRIu64 "\n", p.chunk, p.tail_chunk, p.k_bulk, p.nchunks, p.cpp, p.passes,
                  p.partial_bytes);
    } else if (line[0] == 'D' && n == 2) {
      uint64_t m;
      uint32_t k;
      rtd::div_magic((uint32_t)a[0], m, k);
      std::printf("%" PRIu64 "\n", (uint64_t)((a[1] * m) >> k));
    } else if (line[0] == 'F' && n == 11) {
      rtd::SceneHeader h{};
      h.has_flat = (uint32_t)a[0];
      h.n_linear = (uint32_t)a[1];
      h.n_spheres = (uint32_t)a[2];
      h.n_tris = (uint32_t)a[3];
      h.has_volumes = (int32_t)a[4];
      h.has_wide = (uint32_t)a[5];
      h.n_texdata = a[6];
      h.has_cell_noise = (int32_t)a[7];
      const rtd::KernelFamily f = rtd::kernel_family(h, (int32_t)a[8], a[9] != 0, a[10] != 0);
      std::printf("%d %s\n", (int)f, rtd::family_name(f));
    } else {
      std::fprintf(stderr, "bad line: %s", line);
      return 1;
    }
  }
  return 0;
}
