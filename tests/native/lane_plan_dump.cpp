// Answers how a persistent launch is ordered (csrc/rt_plan.h lane_plan; tests/test_lane_plan.py), one question per
// input line:
//   L knob device_out persist shared_scratch second_set n inputs_written prev_overlapped stale0 stale1 pending caller prev
//     -> overlap lane set sync_prev wait_resolve record_inputs wait_inputs
// caller and prev are stream names as small integers (0: the null stream).
#include <cinttypes>
#include <cstdio>

#include "rt_plan.h"

int main() {
  char line[512];
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[13] = {};
    const int n = std::sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2,
                              a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10, a + 11, a + 12);
    if (line[0] != 'L' || n != 13) {
      std::fprintf(stderr, "bad line: %s", line);
      return 1;
    }
    rtd::LaneQuery q{};
    q.knob = a[0] != 0;
    q.device_out = a[1] != 0;
    q.persist = a[2] != 0;
    q.shared_scratch = a[3] != 0;
    q.second_set = a[4] != 0;
    q.n = a[5];
    q.inputs_written = a[6] != 0;
    q.prev_overlapped = a[7] != 0;
    q.lane_stale[0] = a[8] != 0;
    q.lane_stale[1] = a[9] != 0;
    q.pending = a[10] != 0;
    q.caller = (const void*)(uintptr_t)a[11];
    q.prev = (const void*)(uintptr_t)a[12];
    const rtd::LanePlan p = rtd::lane_plan(q);
    std::printf("%d %d %d %d %d %d %d\n", (int)p.overlap, p.lane, p.set, (int)p.sync_prev, (int)p.wait_resolve,
                (int)p.record_inputs, (int)p.wait_inputs);
  }
  return 0;
}
