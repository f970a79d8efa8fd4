// Answers how an occlusion query runs (csrc/rt_plan.h occlusion_early_exit; tests/test_occlusion_abi.py), one
// question per input line:
//   O has_flat n_linear has_wide n_wnodes n_wprim_words wide_stack n_volumes n_quads ordered word_bytes
//     -> the query's family (trace_family), 1 if it takes the any-hit kernel with early exit (0: the closest-hit
//        traversal, compared with tmax afterwards), and the family's name
// The header is the one of the blob rays of that word size read: the fp32 blob (word_bytes 16) of a scene with quads
// carries their fp64 records (has_quads64), the fp64 blob never does (scene_compile.cpp).
#include <cinttypes>
#include <cstdio>

#include "rt_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[10] = {};
    const int n = std::sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3,
                              a + 4, a + 5, a + 6, a + 7, a + 8, a + 9);
    if (line[0] != 'O' || n != 10) {
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
    h.has_volumes = a[6] != 0;
    h.n_volumes = (uint32_t)a[6];
    h.n_quads = (uint32_t)a[7];
    h.has_quads64 = a[7] != 0 && a[9] == 16;
    const rtd::TraceFamily f = rtd::trace_family(h, a[8] != 0, (size_t)a[9]);
    std::printf("%d %d %s\n", (int)f, (int)rtd::occlusion_early_exit(h, f, (size_t)a[9]), rtd::trace_family_name(f));
  }
  return 0;
}
