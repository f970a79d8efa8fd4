// rt_context.h -- what a context is, for rt_render.hip alone (the C ABI's rt_context is opaque to everyone else): the
// struct and the device buffers it owns, the error text, and the few functions that say what of a context may still
// be running and wait for it (mark_pending, wait_pending, ensure, settle). No render, query or launch decision lives
// here. Everything has internal linkage: the library exports the C ABI only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_launch.h"
#include "rt_plan.h"
#include "scene_compile.h"

using namespace rtd;

// A device allocation a context owns: grown by ensure(), freed with the context (rt_context_destroy waits for the
// work that may still read it first).
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (ptr) (void)hipFree(ptr);
  }
};

struct rt_context {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  CompiledScene scene;
  bool has_scene = false;
  DevBuf scene32, scene64;
  DevBuf state, partial, pixmap, queue0, queue1, blk, out_tmp, counters, camx, heads, tiles;
  DevBuf wide_spill;  // the wide traversal's stack entries past wide_lds_stack (deep trees in HBM)
  CamDev cam_host;  // source of camx (kept alive for the async copy)
  uint32_t* total_host = nullptr;  // pinned: [0] live slots, [1] fault word, [16..] segment counter shards
  uint64_t samples = 0;
  rt_counters last{};  // host-known totals since rt_reset_counters; segments and step_ms settle in settle()
  int timing = 0;
  std::vector<hipEvent_t> events;
  // asynchronous renders (device output): what rt_stats / rt_reset_counters / a host-output render
  // settle with one sync -- the stream, the timing events recorded since the last settle
  hipStream_t pend_stream = nullptr;
  bool pending = false;
  size_t ev_used = 0;
  DevBuf fault;  // sticky internal-error word of the persistent kernel (zeroed by rt_reset_counters)
  // inputs kept on the device while they do not change between calls
  std::vector<uint4> tiles_dev;  // the tile list k_pixmap last expanded into pixmap
  void* pixmap_for = nullptr;    // pixmap buffer that expansion went to
  uint32_t pixmap_npix = 0;      // pixels it expanded: a tile entry {x0, y0, width, first} does not
                                 // hold the height, so the last tile can change with the list equal
  CamDev cam_dev{};              // the camera view in camx
  bool cam_valid = false;
  // the compiled scene is copied into scene32 / scene64 by the first render after rt_scene_upload,
  // on that render's stream: a copy made on another stream is not guaranteed visible to the kernels
  // of the render stream (their launch need not invalidate the L2 lines of the previous scene)
  bool scene_dirty32 = false, scene_dirty64 = false;
  // ray queries (rt_trace_rays): the compiled scene's (object, material) tables, copied like the scene by the first
  // query after rt_scene_upload on that query's stream; device copies of a host-pointer query's rays and outputs
  DevBuf ids, q_rays, q_geom, q_ids;
  bool ids_dirty = false;
  // the launch lanes (rt_plan.h lane_plan): lane 0 is `stream`, lane 1 a second internal stream; launch n of the
  // lanes runs on lane n & 1 and writes partial / heads (n even) or partial2 / heads2 (n odd). Made by the first
  // render that overlaps; a context that never does holds none of it.
  hipStream_t lane1 = nullptr;
  DevBuf partial2, heads2;
  hipEvent_t ev_done[2] = {nullptr, nullptr};     // launch on this lane finished (the caller's stream waits for it)
  hipEvent_t ev_resolved[2] = {nullptr, nullptr}; // this set's resolve finished, on the caller's stream
  hipEvent_t ev_inputs = nullptr;                 // the caller's stream, behind the inputs a call queued there
  bool lanes_failed = false;     // making them failed once (out of memory): the context stays serial
  bool lanes_live = false;       // a lane may still be running (cleared by wait_pending)
  LaneState lane_state;          // what lane_plan asks of the launches before (rt_plan.h; advanced by one_pass)
  int ncu = 1;                   // the device's compute units (device_max_lanes), read by rt_context_create
  std::vector<uint8_t> ev_lane;  // per pair of timing events: recorded on a lane (settle() clamps its start)
  // adaptive sampling (rt_render_adaptive): the pixels' moment records, the two pixel lists the rounds alternate
  // between (positions, and the pixels' slots in the outputs and records), the select's block counts, and device
  // copies of a host-pointer call's out_spp and out_err (out_rgb's is out_tmp)
  DevBuf ad_acc, ad_pix[2], ad_slot[2], ad_blk, ad_spp, ad_err;
  // denoising (rt_denoise): the working records, kDnScratchT T a pixel; a host-pointer call's inputs and output are
  // staged in out_tmp (rgb, in and out), q_rays (feat) and q_geom (var). A host-pointer rt_temporal stages the same way,
  // its ids in q_ids and its two histories in dn_scratch (it has no working records of its own)
  DevBuf dn_scratch;
};

namespace {

std::mutex g_err_mu;
std::string g_create_err;

rt_status set_err(rt_context* c, rt_status s, const std::string& m) {
  if (c) {
    c->err = m;
  } else {
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_create_err = m;
  }
  return s;
}

#define RT_HIP(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return set_err((ctx), RT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// The context has work outstanding on `st` from here on: a later call on another stream waits for st
// (wait_other_stream), and rt_stats, rt_reset_counters or a host-output call settle it.
void mark_pending(rt_context* c, hipStream_t st) {
  c->pending = true;
  c->pend_stream = st;
}

// The most lanes the device can hold: 32 waves of 64 per CU (the wide spill area's size, auto_run's bound)
uint32_t device_max_lanes(const rt_context* c) { return (uint32_t)std::max(c->ncu, 1) * 2048u; }

// Wait on the host for everything of this context that may still run. pend_stream alone covers the lanes in the
// normal course (it waits for every lane launch before that launch's resolve); the lanes are waited for too, so
// that a call which failed between a launch and that wait leaves nothing behind either. `pending` stays: the
// device-side results are still to be folded in by settle().
rt_status wait_pending(rt_context* c) {
  if (c->pending) RT_HIP(c, hipStreamSynchronize(c->pend_stream));
  if (c->lanes_live) {
    RT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->lane1) RT_HIP(c, hipStreamSynchronize(c->lane1));
    c->lanes_live = false;
  }
  return RT_OK;
}

// Grow a context buffer. The only work that can still read the old buffer is this context's
// outstanding device-output render (host-output renders return finished, and a render on another
// stream waits for pend_stream first): wait for that stream and the lanes, not for the whole device.
rt_status ensure(rt_context* c, DevBuf& b, size_t bytes) {
  if (b.ptr && b.bytes >= bytes) return RT_OK;
  if (b.ptr) {
    rt_status w;
    if ((w = wait_pending(c)) != RT_OK) return w;
    RT_HIP(c, hipFree(b.ptr));
    b.ptr = nullptr;
    b.bytes = 0;
  }
  size_t want = std::max<size_t>(bytes, 256);
  hipError_t e = hipMalloc(&b.ptr, want);
  if (e != hipSuccess) {
    b.ptr = nullptr;
    (void)hipGetLastError();
    return set_err(c, RT_ERR_OUT_OF_MEMORY,
                   "hipMalloc(" + std::to_string(want) + " bytes): " + hipGetErrorString(e));
  }
  b.bytes = want;
  return RT_OK;
}

hipEvent_t take_event(rt_context* c, size_t idx) {
  while (c->events.size() <= idx) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->events.push_back(e);
  }
  return c->events[idx];
}

// Wait for the context's outstanding renders and fold their device-side results into c->last:
// the cumulative segment count, the kernel time of the timing events, the fault word.
rt_status settle(rt_context* c) {
  if (!c->pending) return RT_OK;
  {
    rt_status w;
    if ((w = wait_pending(c)) != RT_OK) return w;
  }
  c->pending = false;
  unsigned long long* shards = (unsigned long long*)(c->total_host + 16);
  RT_HIP(c, hipMemcpy(shards, c->counters.ptr, sizeof(unsigned long long) * kSegShards, hipMemcpyDeviceToHost));
  uint64_t segs = 0;
  for (int k = 0; k < kSegShards; k++) segs += shards[k];
  c->last.segments = segs;
  double ms = 0;
  for (size_t k = 0; k + 1 < c->ev_used; k += 2) {
    float a = 0;
    RT_HIP(c, hipEventElapsedTime(&a, c->events[k], c->events[k + 1]));
    // A lane launch's start event fires when its lane reaches it, which with two lanes is while the launch before
    // still fills the chip. Its time counts from the later of its own start and that launch's end, so step_ms never
    // counts a moment twice: it stays below the wall time and in steady state is the frame period (rt_counters).
    if (k >= 2 && k / 2 < c->ev_lane.size() && c->ev_lane[k / 2]) {
      float lead = 0;  // own start -> previous end; positive: the previous launch was still running
      if (hipEventElapsedTime(&lead, c->events[k], c->events[k - 1]) == hipSuccess && lead > 0)
        a = std::max(0.0f, a - lead);
      else
        (void)hipGetLastError();
    }
    ms += a;
  }
  c->ev_used = 0;
  c->ev_lane.clear();
  c->last.step_ms += ms;
  uint32_t fault = 0;
  if (c->fault.ptr) RT_HIP(c, hipMemcpy(&fault, c->fault.ptr, 4, hipMemcpyDeviceToHost));
  if (fault) return set_err(c, RT_ERR_HIP, "a path did not finish (internal error)");
  return RT_OK;
}

}  // namespace
