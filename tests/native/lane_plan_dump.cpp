// Answers how a persistent launch is ordered (csrc/rt_plan.h lane_plan, lane_advance; tests/test_lane_plan.py), one
// question per input line:
//   L knob device_out persist shared_scratch second_set n inputs_written prev_overlapped stale0 stale1 pending caller prev
//     -> overlap lane set sync_prev wait_resolve record_inputs wait_inputs
//   S knob device_out persist shared_scratch second_set pending caller prev write
//     -> overlap lane set sync_prev wait_resolve record_inputs wait_inputs  n inputs_written prev_overlapped stale0 stale1
// L is one question with the state given. S is the next launch of a context: the process holds a LaneState across the S
// lines (a new context's at first), `write` says whether an input was written since the launch before, and lane_advance
// is applied after the answer; the five numbers after the plan are the state it leaves.
// caller and prev are stream names as small integers (0: the null stream).
#include <cinttypes>
#include <cstdio>

#include "rt_plan.h"

int main() {
  char line[512];
  rtd::LaneState state{};
  while (std::fgets(line, sizeof line, stdin)) {
    unsigned long long a[13] = {};
    const int n = std::sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2,
                              a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10, a + 11, a + 12);
    const bool stateful = line[0] == 'S';
    if (!(stateful ? n == 9 : line[0] == 'L' && n == 13)) {
      std::fprintf(stderr, "bad line: %s", line);
      return 1;
    }
    rtd::LaneQuery q{};
    q.knob = a[0] != 0;
    q.device_out = a[1] != 0;
    q.persist = a[2] != 0;
    q.shared_scratch = a[3] != 0;
    q.second_set = a[4] != 0;
    const unsigned long long* rest = a + 5;  // pending caller prev
    if (stateful) {
      if (a[8]) state.inputs_written = true;
      q.set_state(state);
    } else {
      q.n = a[5];
      q.inputs_written = a[6] != 0;
      q.prev_overlapped = a[7] != 0;
      q.lane_stale[0] = a[8] != 0;
      q.lane_stale[1] = a[9] != 0;
      rest = a + 10;
    }
    q.pending = rest[0] != 0;
    q.caller = (const void*)(uintptr_t)rest[1];
    q.prev = (const void*)(uintptr_t)rest[2];
    const rtd::LanePlan p = rtd::lane_plan(q);
    std::printf("%d %d %d %d %d %d %d", (int)p.overlap, p.lane, p.set, (int)p.sync_prev, (int)p.wait_resolve,
                (int)p.record_inputs, (int)p.wait_inputs);
    if (stateful) {
      rtd::lane_advance(state, p);
      std::printf("  %" PRIu64 " %d %d %d %d", state.n, (int)state.inputs_written, (int)state.prev_overlapped,
                  (int)state.lane_stale[0], (int)state.lane_stale[1]);
    }
    std::printf("\n");
  }
  return 0;
}
