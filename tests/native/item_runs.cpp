// Walks the units of a persistent launch's queue as the kernels that take runs walk them (csrc/rt_plan.h RunPlan,
// plan_runs, unit_first_chunk, unit_first_item, run_goes_on, auto_run; tests/test_item_runs.py).
//   item_runs plan spp samples_per_item flat full_pixels npix elem budget run
//     -> text: "chunk tail_chunk k_bulk nchunks cpp passes", then per pass
//        "chunk0 pc run_log2 runs n_units run_samples run_mask run_cfg"  (budget 0: the default; run_cfg: the
//        kernels' packed word, then the runs and run_log2 read back from it)
//   item_runs walk spp samples_per_item flat full_pixels npix elem budget run pass
//     -> binary, three uint32 per unit of that pass in queue order: the unit's first item, the items the lane walks
//        before it asks the queue again, and the end of the last one's sample range
//   item_runs auto spp samples_per_item flat full_pixels npix elem budget takes_runs lanes overlapped
//     -> text: the automatic run length; takes_runs 1: the flat LL kernel on the persistent schedule, 0: the same
//        kernel's plan on the wavefront schedule (which takes the flat program's general kernel)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_plan.h"

int main(int argc, char** argv) {
  if (argc < 10) {
    std::fprintf(stderr, "usage: item_runs plan|walk|auto ...\n");
    return 2;
  }
  unsigned long long a[10] = {};
  for (int i = 2; i < argc && i < 12; i++) a[i - 2] = std::strtoull(argv[i], nullptr, 10);
  const uint32_t spp = (uint32_t)a[0], npix = (uint32_t)a[4];
  rtd::PlanKnobs kn;
  if (a[6]) kn.partial_budget = a[6];
  const rtd::ItemPlan pl = rtd::plan_items(spp, (int32_t)a[1], a[2] != 0, a[3], npix, (uint32_t)a[5], kn);
  const uint32_t run = (uint32_t)a[7];
  if (!std::strcmp(argv[1], "plan") && argc == 10) {
    std::printf("%u %u %u %u %u %u\n", pl.chunk, pl.tail_chunk, pl.k_bulk, pl.nchunks, pl.cpp, pl.passes);
    for (uint32_t c0 = 0; c0 < pl.nchunks; c0 += pl.cpp) {
      const uint32_t pc = std::min(pl.cpp, pl.nchunks - c0);
      const rtd::RunPlan r = rtd::plan_runs(pl, spp, c0, pc, npix, run);
      const uint32_t cfg = rtd::run_cfg_pack(r.runs, r.run_log2);
      std::printf("%u %u %u %u %u %u %u %u %u %u\n", c0, pc, r.run_log2, r.runs, r.n_units, r.run_samples, r.run_mask, cfg,
                  rtd::run_cfg_runs(cfg), rtd::run_cfg_log2(cfg));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "walk") && argc == 11) {
    const uint32_t c0 = (uint32_t)a[8] * pl.cpp;
    if (c0 >= pl.nchunks) return 2;
    const uint32_t pc = std::min(pl.cpp, pl.nchunks - c0);
    rtd::RunPlan r = rtd::plan_runs(pl, spp, c0, pc, npix, run);
    const uint32_t cfg = rtd::run_cfg_pack(r.runs, r.run_log2);  // the kernel sees the plan through this word
    r.runs = rtd::run_cfg_runs(cfg);
    r.run_log2 = rtd::run_cfg_log2(cfg);
    r.run_samples = (r.runs << r.run_log2) * pl.chunk;
    r.run_mask = (pl.chunk << r.run_log2) - 1;
    uint64_t m;
    uint32_t k;
    rtd::div_magic(npix, m, k);
    std::vector<uint32_t> out;
    out.reserve(3ull * r.n_units);
    for (uint32_t unit = 0; unit < r.n_units; unit++) {
      // begin_item RUNS
      const uint32_t q = (uint32_t)(((uint64_t)unit * m) >> k);
      const uint32_t lchunk = rtd::unit_first_chunk(q, r.runs, r.run_log2);
      uint32_t item = rtd::unit_first_item(unit, q * npix, npix, r.runs, r.run_log2);
      // chunk_range
      const uint32_t chunk = lchunk + c0;
      const bool bulk = chunk < pl.k_bulk;
      const uint32_t first = bulk ? chunk * pl.chunk : pl.k_bulk * pl.chunk + (chunk - pl.k_bulk) * pl.tail_chunk;
      uint32_t end = std::min(first + (bulk ? pl.chunk : pl.tail_chunk), spp);
      out.push_back(item);
      // shade's item end: the sample index is `end` when the chunk ends
      uint32_t walked = 1;
      while (rtd::run_goes_on(end, r.run_samples, r.run_mask)) {
        item += npix;
        end += pl.chunk;
        walked++;
        if (walked > pl.nchunks) return 3;  // (a run cannot be longer than the pixel's chunks)
      }
      out.push_back(walked);
      out.push_back(end);
    }
    std::fwrite(out.data(), 4, out.size(), stdout);
    return 0;
  }
  if (!std::strcmp(argv[1], "auto") && argc == 12) {
    rtd::PathKernel kern{};
    kern.fam = rtd::KF_FLAT;
    kern.persist = a[7] != 0;
    kern.lds = kern.persist;  // (path_kernel: the tables in LDS, and so the LL form, on the persistent schedule alone)
    kern.shade = kern.lds ? rtd::SH_LL : rtd::SH_GENERAL;
    std::printf("%u\n", rtd::auto_run(pl, kern, spp, npix, a[8], a[9] != 0));
    return 0;
  }
  std::fprintf(stderr, "bad arguments\n");
  return 2;
}
