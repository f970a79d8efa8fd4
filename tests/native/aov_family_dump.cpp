// Answers which traversal the feature-buffer pass takes (csrc/rt_plan.h aov_family; tests/test_aov_abi.py), one
// question per input line:
//   A has_flat n_linear has_wide n_wnodes n_wprim_words wide_stack tex_kinds ordered word_bytes
//     -> the pass's family, the query's family (trace_family) and the pass's family name
// tex_kinds: bit k set when the scene has a texture of rt_texture_kind k.
#include <cinttypes>
#include <cstdio>

#include "rt_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[9] = {};
    const int n = std::sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4,
                              a + 5, a + 6, a + 7, a + 8);
    if (line[0] != 'A' || n != 9) {
      std::fprintf(stderr, "bad line: %s", line);
      return 1;
    }
    rtd::SceneHeader h{};
    h.has_flat = (uint32_t)a[0];
    h.n_linear = (uint32_t)a[1];
    h.has_wide = (uint32_t)a[2];
    h.n_wnodes = (uint32_t)a[3];
    h.n_wprim_words = (uint32_t)a[4];
    h.wide_stack = (uint32_t)a[5];
    h.tex_kinds = (uint32_t)a[6];
    const rtd::TraceFamily f = rtd::aov_family(h, a[7] != 0, (size_t)a[8]);
    std::printf("%d %d %s\n", (int)f, (int)rtd::trace_family(h, a[7] != 0, (size_t)a[8]), rtd::trace_family_name(f));
  }
  return 0;
}
