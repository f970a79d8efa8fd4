// Answers questions about csrc/rt_plan.h (tests/test_plan.py), one per input line:
//   P spp samples_per_item flat full_pixels npix elem budget   -> the item plan (budget 0: the default)
//   D d n                                                       -> (n * m) >> k of div_magic(d)
//   F has_flat n_linear n_spheres n_tris has_volumes has_wide n_texdata has_cell_noise cam_mode persist ordered
//                                                               -> the kernel family and its name
//   K has_flat n_linear n_spheres n_tris has_volumes has_wide n_texdata has_cell_noise
//     n_flat_quad n_flat_box n_flat_room n_mats n_nodes n_wnodes n_wprim_words wide_stack wide_kinds
//     mat_kinds tex_kinds light_kind light_aligned word_bytes cam_mode persist ordered stack_need
//                                                               -> the path kernel's tag (one line of input)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "rt_plan.h"

// the header fields kernel_family reads: a[0 .. 8)
static rtd::SceneHeader family_header(const unsigned long long* a) {
  rtd::SceneHeader h{};
  h.has_flat = (uint32_t)a[0];
  h.n_linear = (uint32_t)a[1];
  h.n_spheres = (uint32_t)a[2];
  h.n_tris = (uint32_t)a[3];
  h.has_volumes = (int32_t)a[4];
  h.has_wide = (uint32_t)a[5];
  h.n_texdata = a[6];
  h.has_cell_noise = (int32_t)a[7];
  return h;
}

int main() {
  char line[1024];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[26] = {};
    int n = 0;
    for (char *s = line + 1, *e = s; n < 26; s = e, n++) {
      a[n] = std::strtoull(s, &e, 10);
      if (e == s) break;
    }
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
      const rtd::SceneHeader h = family_header(a);
      const rtd::KernelFamily f = rtd::kernel_family(h, (int32_t)a[8], a[9] != 0, a[10] != 0);
      std::printf("%d %s\n", (int)f, rtd::family_name(f));
    } else if (line[0] == 'K' && n == 26) {
      rtd::SceneHeader h = family_header(a);
      h.n_flat_quad[0] = (uint32_t)a[8];  // (the choice reads the three axes' sum alone)
      h.n_flat_box = (uint32_t)a[9];
      h.n_flat_room = (uint32_t)a[10];
      h.n_mats = (uint32_t)a[11];
      h.n_nodes = (uint32_t)a[12];
      h.n_wnodes = (uint32_t)a[13];
      h.n_wprim_words = (uint32_t)a[14];
      h.wide_stack = (uint32_t)a[15];
      h.wide_kinds = (uint32_t)a[16];
      h.mat_kinds = (uint32_t)a[17];
      h.tex_kinds = (uint32_t)a[18];
      h.light_kind = (int32_t)a[19];
      h.light_aligned = (int32_t)a[20];
      const size_t word_bytes = (size_t)a[21];
      const rtd::PathKernel k = rtd::path_kernel(h, word_bytes, (int32_t)a[22], a[23] != 0, a[24] != 0, (int)a[25]);
      std::printf("%s\n", rtd::path_kernel_tag(k, word_bytes).c_str());
    } else {
      std::fprintf(stderr, "bad line: %s", line);
      return 1;
    }
  }
  return 0;
}
