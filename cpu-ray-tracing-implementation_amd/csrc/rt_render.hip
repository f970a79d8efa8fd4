// rt_render.hip -- the host side of librt_hip.so, in the order of the file:
//  - (rt_context.h: contexts and their device buffers -- rt_context, DevBuf, ensure, wait_pending, settle;)
//  - the two schedules of a path launch (run_persistent, run_wavefront);
//  - render<R>(): the path-traced pixels of one PixelSource -- a camera's tiles (rt_render_tiles), a ray batch
//    (rt_radiance) or a camera's pixel list (a round of rt_render_adaptive) -- as a list of named steps, of which
//    one_pass() is the only one that launches a path kernel;
//  - the query path (trace_rays<R>(), occluded<R>(), camera_rays(), render_aov<R>()), the round loop of
//    rt_render_adaptive (render_adaptive<R>()), denoise<T>() and temporal<T>();
//  - the C ABI of include/rt_hip.h with its argument checks.
// It contains no kernel of its own: what a render launches goes through rt_launch.h (rt_kernels.hip), and its item
// layout, kernel family and lane ordering come from rt_plan.h. (The denoiser's kernels, rt_denoise.hip, and the temporal
// accumulation's, rt_temporal.hip, are included at the end, so that the library stays four translation units.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_context.h"
#include "rt_launch.h"
#include "rt_plan.h"
#include "scene_compile.h"

using namespace rtd;

namespace {

// camera.h:137-141, 246, 253, 278-279 evaluated in double exactly as the reference orders them
CamDev make_view(const rt_camera_desc* c) {
  CamDev v{};
  v.mode = c->mode;
  double du[3], dv[3], dir00[3], pos00[3];
  for (int k = 0; k < 3; k++) {
    du[k] = (c->right[k] * c->viewport_width) / (double)c->image_width;
    dv[k] = (c->up[k] * -c->viewport_height) / (double)c->image_height;
  }
  for (int k = 0; k < 3; k++) {
    double a = c->dir[k] * c->focal_length;
    double b = c->right[k] * (c->viewport_width / 2.0);
    double u = c->up[k] * (c->viewport_height / 2.0);
    double e = (du[k] + dv[k]) * 0.5;
    dir00[k] = ((a - b) + u) + e;
    pos00[k] = ((c->pos[k] - b) + u) + e;
  }
  v.pos = {c->pos[0], c->pos[1], c->pos[2]};
  v.du = {du[0], du[1], du[2]};
  v.dv = {dv[0], dv[1], dv[2]};
  v.dir00 = {dir00[0], dir00[1], dir00[2]};
  v.pos00 = {pos00[0], pos00[1], pos00[2]};
  v.dir = {c->dir[0], c->dir[1], c->dir[2]};
  v.fdir = {c->focus_dist * c->dir[0], c->focus_dist * c->dir[1], c->focus_dist * c->dir[2]};
  v.disk_u = {c->defocus_u[0], c->defocus_u[1], c->defocus_u[2]};
  v.disk_v = {c->defocus_v[0], c->defocus_v[1], c->defocus_v[2]};
  v.focal = c->focal_length;
  return v;
}

// What a build without the kernels of a family (RT_DEV_ONLY) says when it refuses a scene or a call
std::string dev_only_lacks(const std::string& what) { return "this build (RT_DEV_ONLY) has no " + what; }
std::string dev_only_lacks(KernelFamily fam) { return dev_only_lacks(std::string(family_name(fam)) + " kernels"); }

template <class R>
DevScene<R> dev_scene(const SceneHeader& h, void* base) {
  auto at = [&](uint64_t off) { return (const unsigned char*)base + off; };
  DevScene<R> s{};
  s.quads = (const Quad<R>*)at(h.off_quads);
  s.spheres = (const Sphere<R>*)at(h.off_spheres);
  s.tris = (const Tri<R>*)at(h.off_tris);
  s.insts = (const Instance<R>*)at(h.off_instances);
  s.vols = (const Volume<R>*)at(h.off_volumes);
  s.nodes = (const Node<R>*)at(h.off_nodes);
  s.refs = (const uint32_t*)at(h.off_refs);
  s.mats = (const Material<R>*)at(h.off_mats);
  s.texs = (const Texture<R>*)at(h.off_texs);
  s.light = (const Light<R>*)at(h.off_light);
  s.lin = (const LinRec<R>*)at(h.off_linear);
  s.n_linear = h.n_linear;
  s.has_flat = (int32_t)h.has_flat;
  s.flatq = (const FlatQuadT<R>*)at(h.off_flat_quad);
  s.flatb = (const FlatBoxT<R>*)at(h.off_flat_box);
  for (int a = 0; a < 3; a++) s.n_flatq[a] = h.n_flat_quad[a];
  s.n_flatb = h.n_flat_box;
  s.n_flatr = h.n_flat_room;  // the records follow the boxes (flat_rooms)
  s.n_mats = h.n_mats;
  s.root = h.root;
  s.background = h.background;
  s.has_volumes = h.has_volumes;
  s.n_nodes = h.n_nodes;
  s.texdata = (const double*)at(h.off_texdata);
  s.images = (const uint8_t*)at(h.off_images);
  s.has_procedural = extended_form(h, RT_CAM_PERSPECTIVE);  // (by its textures alone)
  s.has_wide = (int32_t)h.has_wide;
  s.wnodes = (const WNode*)at(h.off_wnodes);
  s.wprims = (const typename WWord<R>::T*)at(h.off_wprims);
  s.n_wnodes = h.n_wnodes;
  s.n_wprim_words = h.n_wprim_words;
  s.wroot = h.wroot;
  s.wide_stack = h.wide_stack;
  s.wide_kinds = h.wide_kinds;
  s.wide_big = h.wide_big;
  s.wide_top = h.wide_top;
  s.wnodesh = h.has_wnodesh ? (const WNodeH*)at(h.off_wnodesh) : nullptr;
  s.quads64 = h.has_quads64 ? (const Quad<double>*)at(h.off_quads64) : nullptr;
  return s;
}

// A deep wide tree: a spill area of (need - wide_lds_stack) stack entries for every lane the chip can hold
// (trace_wide indexes it by lane: a launch over it has at most spill_lanes / kBlock blocks)
template <class R>
rt_status wide_spill_area(rt_context* c, const SceneHeader& hdr, DevScene<R>& sc) {
  const uint32_t wide_need = hdr.wide_stack;
  constexpr uint32_t kWideLdsStack = wide_lds_stack<R>();
  if (hdr.has_wide && wide_need > kWideLdsStack) {
    const uint32_t lanes = device_max_lanes(c);
    rt_status s;
    if ((s = ensure(c, c->wide_spill, 4ull * (wide_need - kWideLdsStack) * lanes)) != RT_OK) return s;
    sc.wide_spill = (uint32_t*)c->wide_spill.ptr;
    sc.spill_lanes = lanes;
  }
  return RT_OK;
}

constexpr int kBatch = 16;  // wavefront schedule: extend/shade rounds between live-slot counts
constexpr uint32_t kAutoPool32 = 1u << 21;
constexpr uint32_t kAutoPool64 = 1u << 19;
constexpr int kAutoSegments = 16;  // segments each slot advances per k_step launch
// persistent schedule: upper bound of the grid's lanes (launch_step cuts the grid to what the chip holds resident)
constexpr uint32_t kAutoPersistLanes = 1u << 22;

// The item layout's knobs (rt_plan.h): RT_ITEM_*, RT_ITEMS_TARGET and RT_PARTIAL_BUDGET in the environment override
// the defaults for A/B runs (scripts/dev_tail.py, tests/test_gpu_passes.py)
PlanKnobs env_knobs() {
  auto num = [](const char* name, double dflt) {
    const char* v = std::getenv(name);
    return (v && *v) ? std::strtod(v, nullptr) : dflt;
  };
  PlanKnobs k;
  k.chunk = (uint32_t)num("RT_ITEM_CHUNK", k.chunk);
  k.chunk_flat = (uint32_t)num("RT_ITEM_CHUNK_FLAT", k.chunk_flat);
  k.tail_chunk = (uint32_t)num("RT_ITEM_TAIL_CHUNK", k.tail_chunk);
  k.tail_chunk_flat = (uint32_t)num("RT_ITEM_TAIL_CHUNK_FLAT", k.tail_chunk_flat);
  k.tail_frac = num("RT_ITEM_TAIL_FRAC", k.tail_frac);
  k.tail_frac_flat = num("RT_ITEM_TAIL_FRAC_FLAT", k.tail_frac_flat);
  k.items_target = (uint64_t)num("RT_ITEMS_TARGET", (double)k.items_target);
  k.partial_budget = (uint64_t)num("RT_PARTIAL_BUDGET", (double)k.partial_budget);
  return k;
}

// RT_FRAME_OVERLAP=0: every launch on the caller's stream, the chain as it was before the lanes (for A/B runs and
// for profiles that need one kernel at a time). Read per call, as the knobs above.
bool env_frame_overlap() {
  const char* v = std::getenv("RT_FRAME_OVERLAP");
  return !(v && *v) || std::strtol(v, nullptr, 10) != 0;
}

// RT_ITEM_RUN=L: the run length of the kernels that take runs (rt_plan.h RunPlan), a power of two, for A/B runs and
// tests; 1: every unit is an item. 0 or unset: auto_run's choice. Read per call, as the knobs above.
uint32_t env_item_run() {
  const char* v = std::getenv("RT_ITEM_RUN");
  const long r = (v && *v) ? std::strtol(v, nullptr, 10) : 0;
  return r > 0 ? (uint32_t)std::min<long>(r, (long)kMaxItemsPerPixel) : 0;
}

// One launch_step, between two events when the context collects kernel times (settle() sums the pairs)
template <class R>
rt_status timed_step(rt_context* c, const LaunchParams<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st,
                     bool on_lane = false) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->timing) {
    e0 = take_event(c, c->ev_used);
    e1 = take_event(c, c->ev_used + 1);
    if (!e0 || !e1) return set_err(c, RT_ERR_HIP, "hipEventCreate failed");
    RT_HIP(c, hipEventRecord(e0, st));
  }
  launch_step<R>(p, k, grid, st);
  if (c->timing) {
    RT_HIP(c, hipEventRecord(e1, st));
    c->ev_lane.resize(c->ev_used / 2 + 1, 0);
    c->ev_lane[c->ev_used / 2] = on_lane;
    c->ev_used += 2;
  }
  c->last.launches++;
  c->last.iterations++;
  return RT_OK;
}

// The persistent schedule (the default): one launch of at most `grid` blocks renders the pass. A fault is
// reported by the settle after the call (rt_stats, or a host-output render).
template <class R>
rt_status run_persistent(rt_context* c, const LaunchParams<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st,
                         bool on_lane = false) {
  RT_HIP(c, hipMemsetAsync(p.heads, 0, 4ull * kHeads * kHeadStride, st));
  rt_status s;
  if ((s = timed_step(c, p, k, grid, st, on_lane)) != RT_OK) return s;
  RT_HIP(c, hipGetLastError());
  c->last.grid_lanes = last_grid_lanes();
  return RT_OK;
}

// The wavefront schedule (segments_per_launch = K > 0): P slots with their path state in HBM, one launch per K
// segments, the live slots counted every kBatch launches and compacted into a queue once half have finished.
template <class R>
rt_status run_wavefront(rt_context* c, LaunchParams<R> p, const PathKernel& k, uint32_t nblk_max, hipStream_t st) {
  const uint32_t P = p.P;
  p.queue = nullptr;
  p.n = P;
  launch_init<R>(p, k, nblk_max, st);
  c->last.launches++;
  uint32_t* qbuf[2] = {(uint32_t*)c->queue0.ptr, (uint32_t*)c->queue1.ptr};
  int qsel = 0;
  uint32_t* blk = (uint32_t*)c->blk.ptr;
  uint32_t* d_total = blk + nblk_max + 1;
  // every slot finishes within (items per slot) * chunk * max_depth segments; anything longer is a bug
  const uint64_t iter_cap =
      c->last.iterations + (((uint64_t)(p.n_items + P - 1) / P) * p.chunk * (uint64_t)p.max_depth + p.K - 1) / p.K + 4 * kBatch;
  for (;;) {
    if (c->last.iterations > iter_cap) return set_err(c, RT_ERR_HIP, "wavefront did not drain (internal error)");
    const uint32_t grid = (p.n + kBlock - 1) / kBlock;
    rt_status s;
    for (int b = 0; b < kBatch; b++)
      if ((s = timed_step(c, p, k, grid, st)) != RT_OK) return s;
    RT_HIP(c, hipGetLastError());
    // live-slot count; compact into a queue once half the pool has finished
    launch_count(p.D, sizeof(R) == 8, p.queue, p.n, blk, d_total, st);
    c->last.launches += 2;
    RT_HIP(c, hipMemcpyAsync(c->total_host, d_total, 4, hipMemcpyDeviceToHost, st));
    RT_HIP(c, hipStreamSynchronize(st));
    const uint32_t alive = *c->total_host;
    if (alive == 0) return RT_OK;
    if (p.queue || alive * 2 <= P) {
      uint32_t* nq = qbuf[qsel];
      qsel ^= 1;
      launch_compact(p.D, sizeof(R) == 8, p.queue, p.n, blk, nq, st);
      c->last.launches++;
      p.queue = nq;
      p.n = alive;
    }
  }
}

// The tile list of a call as k_pixmap takes it: {x0, y0, width, first packed pixel} of every tile that is not
// empty, in the given order; npix: the pixels of all of them.
std::vector<uint4> pack_tiles(const rt_tile* tiles, int32_t ntiles, uint64_t& npix) {
  std::vector<uint4> tl;
  tl.reserve(ntiles);
  npix = 0;
  for (int t = 0; t < ntiles; t++) {
    if (tiles[t].width == 0 || tiles[t].height == 0) continue;
    tl.push_back(make_uint4((uint32_t)tiles[t].x0, (uint32_t)tiles[t].y0, (uint32_t)tiles[t].width, (uint32_t)npix));
    npix += (uint64_t)tiles[t].width * (uint64_t)tiles[t].height;
  }
  return tl;
}

// The pixel map of the tile list in c->pixmap (tiles packed in order, row-major inside each tile), expanded by
// k_pixmap on `st` unless the map of the same list is still there.
rt_status pixel_map(rt_context* c, const std::vector<uint4>& tl, uint32_t npix, hipStream_t st) {
  rt_status s;
  const size_t pixmap_bytes = c->pixmap.bytes;
  if ((s = ensure(c, c->pixmap, 4ull * npix)) != RT_OK) return s;
  if (c->pixmap.bytes != pixmap_bytes) c->tiles_dev.clear();  // reallocated: the old map is gone
  const bool same_tiles = c->pixmap_for == c->pixmap.ptr && c->pixmap_npix == npix && c->tiles_dev.size() == tl.size() &&
                          std::memcmp(c->tiles_dev.data(), tl.data(), sizeof(uint4) * tl.size()) == 0;
  if (!same_tiles) {  // the pixel map of an unchanged tile list is still in pixmap
    if ((s = ensure(c, c->tiles, sizeof(uint4) * tl.size())) != RT_OK) return s;
    c->tiles_dev = tl;  // the copy's source outlives this call
    c->pixmap_for = c->pixmap.ptr;
    c->pixmap_npix = npix;
    c->lane_state.inputs_written = true;  // (whoever queues it: a feature-buffer call's map is a later render's input too)
    RT_HIP(c, hipMemcpyAsync(c->tiles.ptr, c->tiles_dev.data(), sizeof(uint4) * tl.size(), hipMemcpyHostToDevice, st));
    launch_pixmap((const uint4*)c->tiles.ptr, (uint32_t)tl.size(), npix, (uint32_t*)c->pixmap.ptr, st);
  }
  return RT_OK;
}

// The camera's view (make_view) in c->camx, copied on `st` when it differs from the one there.
rt_status camera_view(rt_context* c, const rt_camera_desc* cam, hipStream_t st) {
  rt_status s;
  c->cam_host = make_view(cam);
  if ((s = ensure(c, c->camx, sizeof(CamDev))) != RT_OK) return s;
  if (!c->cam_valid || std::memcmp(&c->cam_dev, &c->cam_host, sizeof(CamDev)) != 0) {
    c->lane_state.inputs_written = true;
    RT_HIP(c, hipMemcpyAsync(c->camx.ptr,&c->cam_host, sizeof(CamDev), hipMemcpyHostToDevice, st));
    c->cam_dev = c->cam_host;
    c->cam_valid = true;
  }
  return RT_OK;
}

// The second lane and buffer set (rt_plan.h lane_plan), made by the first render that overlaps and grown with the
// first set. False when something cannot be had (the second partial buffer doubles the largest allocation of a
// render): the render then takes the serial order, with no error. A stream or an event that cannot be made is not
// tried again; the buffer is, because a later, smaller render may fit.
bool lanes_ready(rt_context* c, size_t partial_bytes) {
  if (c->lanes_failed) return false;
  if (!c->lane1) {
    bool ok = hipStreamCreateWithFlags(&c->lane1, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t* e : {&c->ev_done[0], &c->ev_done[1], &c->ev_resolved[0], &c->ev_resolved[1], &c->ev_inputs})
      ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      c->lanes_failed = true;  // (what was made goes with the context)
      return false;
    }
  }
  const std::string err = c->err;
  const bool ok = ensure(c, c->heads2, 4ull * kHeads * kHeadStride) == RT_OK && ensure(c, c->partial2, partial_bytes) == RT_OK;
  if (!ok) c->err = err;
  return ok;
}

// Work of this context still pending on another stream than `st` reads the context's shared buffers (pixmap, tiles,
// camx, heads, partial, the scene): every call waits for it here before it writes any of them. lq: the three fields of
// the lane query that lane_plan's sync_prev depends on, as they stand for the launches of this call.
rt_status wait_other_stream(rt_context* c, hipStream_t st, LaneQuery* lq = nullptr) {
  LaneQuery q{};
  q.pending = c->pending;
  q.caller = (const void*)st;
  q.prev = (const void*)c->pend_stream;
  if (lane_plan(q).sync_prev) {
    rt_status w;
    if ((w = wait_pending(c)) != RT_OK) return w;
    q.pending = false;  // nothing is running any more: the launches below have no other stream to wait for
  }
  if (lq) *lq = q;
  return RT_OK;
}

// The opening of every call that reads the scene: wait_other_stream, then the scene blob of the precision copied on
// `st` if rt_scene_upload has replaced it since the last call of that precision, stream-ordered before the kernels.
rt_status scene_to_device(rt_context* c, bool f64, hipStream_t st, LaneQuery* lq = nullptr) {
  rt_status s;
  if ((s = wait_other_stream(c, st, lq)) != RT_OK) return s;
  bool& dirty = f64 ? c->scene_dirty64 : c->scene_dirty32;
  if (dirty) {
    const std::vector<unsigned char>& blob = f64 ? c->scene.blob64 : c->scene.blob32;
    void* sbase = f64 ? c->scene64.ptr : c->scene32.ptr;
    c->lane_state.inputs_written = true;
    RT_HIP(c, hipMemcpyAsync(sbase, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
    dirty = false;
    // outstanding from here on, whatever the call does next (an empty tile list or max_depth <= 0
    // launches nothing that reads the scene): a later call on another stream waits for st
    mark_pending(c, st);
  }
  return RT_OK;
}

// A ray batch in place of a camera and tiles (rt_radiance): `n` rays (0 < n < 2^31) at `rays`, device memory when
// on_device (else the call stages them in q_rays), ray i keyed as pixel ray_base + i. render() lays the batch out as the
// n "pixels" of its call -- item planner, passes, partial sums and resolve as for an image -- and the kernel reads ray
// i where a camera kernel would read pixel i of the pixel map.
struct RayBatch {
  const double* rays;
  uint32_t n, ray_base;
  bool on_device;
};

// A pixel list in place of tiles (a round of rt_render_adaptive): entry j of `n` (0 < n < 2^31) is the pixel at
// pixmap[j] (x | y << 16, device memory, as k_pixmap writes a tile list's), and slots[j] (null: j) is its place in
// the records at `acc`. render() takes the list as its pixel map as it stands -- no tiles, no pixel_map() and none of
// its cache -- and resolves every pass into the records' moments (launch_resolve_moments) instead of an image: there
// is no `out`. prm->samples_per_item is the batch, prm->spp a multiple of it.
struct PixelList {
  const uint32_t* pixmap;
  const uint32_t* slots;
  uint32_t n;
  AdaptiveAcc* acc;
};

// The pixels of one render<R>() call and where their result goes. Three kinds of source:
//  - SRC_TILES: `ntiles` tiles of the image of `cam`; the result is the tiles' packed image;
//  - SRC_RAYS: the ray batch `rays`, ray i the call's pixel i; the result is one value a ray;
//  - SRC_LIST: the pixel list `list` of the image of `cam`; no image, every pass goes into the records at list.acc.
// The result is written to `out`: device memory when out_dev, and the call returns with its work queued, else host
// memory, and the call returns finished. A list has no `out` and is a device-output call.
// Every rule of render<R>() that depends on the kind is a member here, written once; render<R>() and its steps ask
// the source and never its kind.
enum SourceKind { SRC_TILES, SRC_RAYS, SRC_LIST };
struct PixelSource {
  SourceKind kind;
  const rt_camera_desc* cam;  // SRC_TILES, SRC_LIST
  const rt_tile* tiles;       // SRC_TILES
  int32_t ntiles;
  RayBatch rays;              // SRC_RAYS
  PixelList list;             // SRC_LIST
  void* out;
  bool out_dev;

  static PixelSource of_tiles(const rt_camera_desc* cam, const rt_tile* tiles, int32_t ntiles, void* out, bool out_dev) {
    PixelSource s{};
    s.kind = SRC_TILES, s.cam = cam, s.tiles = tiles, s.ntiles = ntiles, s.out = out, s.out_dev = out_dev;
    return s;
  }
  static PixelSource of_rays(const RayBatch& rb, void* out, bool out_dev) {
    PixelSource s{};
    s.kind = SRC_RAYS, s.rays = rb, s.out = out, s.out_dev = out_dev;
    return s;
  }
  static PixelSource of_list(const rt_camera_desc* cam, const PixelList& pl) {
    PixelSource s{};
    s.kind = SRC_LIST, s.cam = cam, s.list = pl, s.out = nullptr, s.out_dev = true;
    return s;
  }

  // The call's pixels: their count and, for tiles, the packed list that expand_map() takes (else empty)
  std::vector<uint4> packed_tiles(uint64_t& npix) const {
    if (kind == SRC_TILES) return pack_tiles(tiles, ntiles, npix);
    npix = kind == SRC_RAYS ? rays.n : list.n;
    return {};
  }
  // The pixel map: tiles packed in order, row-major inside each tile (expanded by k_pixmap into c->pixmap); a list is
  // its own map as it stands, and a batch has none (the kernel reads ray i where it would read pixel i of the map)
  rt_status expand_map(rt_context* c, const std::vector<uint4>& tl, uint32_t npix, hipStream_t st) const {
    return kind == SRC_TILES ? pixel_map(c, tl, npix, st) : RT_OK;
  }
  const uint32_t* pixmap(const rt_context* c) const {
    return kind == SRC_LIST ? list.pixmap : (const uint32_t*)c->pixmap.ptr;
  }
  // What decides the item size (plan_items): the full image's pixels, not this call's tiles. A batch is its own full
  // image: with samples_per_item given, the layout depends on spp alone.
  uint64_t image_pixels(uint32_t npix) const {
    return kind == SRC_RAYS ? (uint64_t)npix : (uint64_t)cam->image_width * (uint64_t)cam->image_height;
  }
  PathKernel kernel(const CompiledScene& cs, const SceneHeader& hdr, size_t word_bytes, bool persist, bool ordered) const {
    return kind == SRC_RAYS ? radiance_kernel(hdr, word_bytes, ordered, cs.stack_need)
                            : path_kernel(hdr, word_bytes, cam->mode, persist, ordered, cs.stack_need);
  }
  // Whether the call's launches may go through the launch lanes (LaneQuery::knob, with RT_FRAME_OVERLAP).
  // A ray batch stays on the caller's stream: its rays are the caller's, written on that stream, and a lane would
  // have to wait for them before every launch -- there is no unchanged-input case for the lanes to overlap.
  // A pixel list stays there too: the list is written on that stream just before, and the host waits between rounds.
  bool may_use_lanes() const { return kind == SRC_TILES; }

  // The source's part of the launch parameters: the camera's view, or the batch's rays (staged in q_rays unless
  // they are on the device), queued on `st`
  template <class R>
  rt_status fill(rt_context* c, LaunchParams<R>& p, uint32_t npix, hipStream_t st) const {
    rt_status s;
    if (kind == SRC_RAYS) {  // no camera: cam64 stays null, so a near-edge quad re-decision (quad_edge64) takes the given ray, as a query's
      p.rays = rays.rays;
      p.ray_base = rays.ray_base;
      p.cam_mode = RT_CAM_PERSPECTIVE;
      if (!rays.on_device) {
        if ((s = ensure(c, c->q_rays, 64ull * npix)) != RT_OK) return s;
        p.rays = (const double*)c->q_rays.ptr;
        RT_HIP(c, hipMemcpyAsync(c->q_rays.ptr, rays.rays, 64ull * npix, hipMemcpyHostToDevice, st));
      }
    } else {
      p.W = (uint32_t)cam->image_width;
      if ((s = camera_view(c, cam, st)) != RT_OK) return s;
      p.cam_mode = c->cam_host.mode;
      p.camx = (const CamDev*)c->camx.ptr;
      if (p.cam_mode == RT_CAM_PERSPECTIVE) p.sc.cam64 = p.camx;
    }
    return RT_OK;
  }
  // The resolve of the pass of chunks [c0, c0 + pc) of plan.nchunks, on `st`: into the image at `dout`, or a list's
  // into its records' moments
  template <class R>
  void resolve(const R* partial, uint32_t npix, uint32_t c0, uint32_t pc, const ItemPlan& plan, uint32_t spp, void* dout,
               hipStream_t st) const {
    if (kind == SRC_LIST)
      launch_resolve_moments<R>(partial, list.slots, npix, pc, list.acc, st);
    else
      launch_resolve<R>(partial, npix, pc, spp, (R*)dout, c0 == 0, c0 + pc >= plan.nchunks, st);
  }
  // max_depth <= 0: ray_color(r, 0) is black for every sample (camera.h:194-195), so the image is zero; a list's
  // batches' sums are zero: the records count them and stay as they are
  template <class R>
  rt_status depth0(rt_context* c, const rt_render_params* prm, uint32_t npix, void* dout, hipStream_t st) const {
    if (kind != SRC_LIST) {
      launch_zero<R>((R*)dout, 3ull * npix, st);
      return RT_OK;
    }
    launch_resolve_moments<R>(nullptr, list.slots, npix, (uint32_t)(prm->spp / prm->samples_per_item), list.acc, st);
    c->last.launches++;
    RT_HIP(c, hipGetLastError());
    mark_pending(c, st);
    c->last.samples += (uint64_t)npix * (uint32_t)prm->spp;
    return RT_OK;
  }
};

// One render<R>() call, as its steps build it up (each step's comment says what it adds)
template <class R>
struct RenderCall {
  const PixelSource& src;
  const rt_render_params* prm;
  hipStream_t st;
  uint32_t npix = 0;
  void* dout = nullptr;  // the result on the device: src.out, or out_tmp behind a host `out`
  // plan_call
  uint32_t spp = 0;
  bool persist = true;
  PathKernel kind{};
  ItemPlan plan{};
  uint32_t P = 0, nblk_max = 0;
  // path_buffers
  size_t r4 = 0, sb = 0;  // the bytes of an R4 array and of the key array of the path state
  // fill_params
  LaunchParams<R> p{};
  // scene_to_device (pending, caller, prev), lane_setup (the rest)
  LaneQuery lq{};
  uint32_t forced_run = 0;
};

// Step: the kernel, the item layout and the pool of the call.
template <class R>
rt_status plan_call(rt_context* c, RenderCall<R>& rc) {
  const rt_render_params* prm = rc.prm;
  const CompiledScene& cs = c->scene;
  rc.spp = (uint32_t)prm->spp;
  // the default schedule is persistent (k_persist); an explicit segments_per_launch selects the
  // launch-per-K-segments wavefront with HBM path state and live-slot compaction
  rc.persist = prm->segments_per_launch <= 0;
  rc.kind = rc.src.kernel(cs, sizeof(R) == 8 ? cs.hdr64 : cs.hdr, sizeof(typename WWord<R>::T), rc.persist,
                          prm->traversal == RT_TRAV_ORDERED);
  if (!family_built(rc.kind.fam)) return set_err(c, RT_ERR_UNSUPPORTED, dev_only_lacks(rc.kind.fam));
  // the item layout and the passes
  rc.plan = plan_items(rc.spp, prm->samples_per_item, rc.kind.fam == KF_FLAT, rc.src.image_pixels(rc.npix), rc.npix,
                       sizeof(R), env_knobs());
  const uint32_t n_items = rc.npix * rc.plan.cpp;  // items of the largest pass
  uint32_t P = prm->pool_slots > 0 ? (uint32_t)prm->pool_slots
               : rc.persist       ? kAutoPersistLanes
                                  : (sizeof(R) == 8 ? kAutoPool64 : kAutoPool32);
  rc.P = std::max<uint32_t>(1, std::min(P, n_items));
  rc.nblk_max = (rc.P + kBlock - 1) / kBlock;
  return RT_OK;
}

// Step: the buffers a path launch writes, sized by the plan. (The persistent schedule's fault word and dequeue heads
// are ensured at the end of fill_params, behind the inputs the call queues, where they have always been.)
template <class R>
rt_status path_buffers(rt_context* c, RenderCall<R>& rc) {
  rt_status s;
  // path state: 5 R4 arrays (O, D, T, L, A) + uint4 keys (S) + uint4 exclusion/pixel (X), each P long
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t xb = al(16 * (size_t)rc.P);
  rc.r4 = al(sizeof(R4<R>) * (size_t)rc.P);
  rc.sb = al(16 * (size_t)rc.P);
  if (!rc.persist) {
    if ((s = ensure(c, c->state, 5 * rc.r4 + rc.sb + xb)) != RT_OK) return s;
    if ((s = ensure(c, c->queue0, 4ull * rc.P)) != RT_OK) return s;
    if ((s = ensure(c, c->queue1, 4ull * rc.P)) != RT_OK) return s;
  }
  if ((s = ensure(c, c->partial, rc.plan.partial_bytes)) != RT_OK) return s;
  c->last.passes += rc.plan.passes;
  c->last.partial_bytes = rc.plan.partial_bytes;
  return ensure(c, c->blk, 4ull * (rc.nblk_max + 2));
}

// Step: the launch parameters, everything that is fixed for the whole call -- from the scene, the plan and the source.
template <class R>
rt_status fill_params(rt_context* c, RenderCall<R>& rc) {
  const bool f64 = sizeof(R) == 8;
  const SceneHeader& hdr = f64 ? c->scene.hdr64 : c->scene.hdr;
  const rt_render_params* prm = rc.prm;
  const size_t r4 = rc.r4, sb = rc.sb;
  rt_status s;
  unsigned char* sp = (unsigned char*)c->state.ptr;
  LaunchParams<R>& p = rc.p;
  p.sc = dev_scene<R>(hdr, f64 ? c->scene64.ptr : c->scene32.ptr);
  if ((s = wide_spill_area<R>(c, hdr, p.sc)) != RT_OK) return s;
  if (prm->traversal == RT_TRAV_ORDERED) p.sc.has_flat = p.sc.has_wide = 0;
  p.sc.cam64 = nullptr;  // set with the camera below (perspective only)
  p.O = (R4<R>*)sp;
  p.D = (R4<R>*)(sp + r4);
  p.T = (R4<R>*)(sp + 2 * r4);
  p.L = (R4<R>*)(sp + 3 * r4);
  p.A = (R4<R>*)(sp + 4 * r4);
  p.S = (uint4*)(sp + 5 * r4);
  p.X = (uint4*)(sp + 5 * r4 + sb);
  p.partial = (R*)c->partial.ptr;
  p.pixmap = rc.src.pixmap(c);
  p.queue = nullptr;
  p.n = rc.P;
  p.P = rc.P;
  p.npix = rc.npix;
  div_magic(rc.npix, p.npix_m, p.npix_k);
  p.n_items = rc.npix * rc.plan.cpp;  // items of the largest pass
  p.chunk = rc.plan.chunk;
  p.k_bulk = rc.plan.k_bulk;
  p.tail_chunk = rc.plan.tail_chunk;
  p.spp = rc.spp;
  p.first_sample = (uint32_t)std::max(0, prm->first_sample);
  p.max_depth = prm->max_depth;
  p.seed = prm->seed;
  if ((s = rc.src.template fill<R>(c, p, rc.npix, rc.st)) != RT_OK) return s;
  p.seg_shards = (unsigned long long*)c->counters.ptr;
  p.K = prm->segments_per_launch > 0 ? std::min(prm->segments_per_launch, 64) : kAutoSegments;
  if (c->timing && c->ev_used > 4096 && (s = settle(c)) != RT_OK) return s;  // bound the pending events
  if (rc.persist) {
    if ((s = ensure(c, c->fault, 4)) != RT_OK) return s;
    p.persist = kPersist;
    p.fault = (uint32_t*)c->fault.ptr;
    if ((s = ensure(c, c->heads, 4ull * kHeads * kHeadStride)) != RT_OK) return s;
    p.heads = (uint32_t*)c->heads.ptr;
  }
  return RT_OK;
}

// Step: the launch lanes (rt_plan.h lane_plan) -- what of the lane query is fixed for the call, the second lane and
// buffer set if the call would use them, and the forced run length. The plan itself is asked per launch (one_pass),
// so the passes of a call alternate too.
template <class R>
void lane_setup(rt_context* c, RenderCall<R>& rc) {
  LaneQuery& lq = rc.lq;
  lq.knob = env_frame_overlap() && rc.src.may_use_lanes();
  lq.device_out = rc.src.out_dev;
  lq.persist = rc.persist;
  lq.shared_scratch = rc.p.sc.wide_spill != nullptr;
  lq.second_set = true;  // asked first whether the call would overlap at all; then whether the set can be had
  lq.second_set = lane_plan(lq).overlap && lanes_ready(c, rc.plan.partial_bytes);
  // the run length of the queue's units (rt_plan.h RunPlan) is the knob's for a kernel that takes runs, else
  // auto_run's (one_pass, per launch), against the most lanes the device can hold (device_max_lanes)
  rc.forced_run = kernel_takes_runs(rc.kind) ? env_item_run() : 1;
}

// Step: one pass, the chunks [c0, c0 + plan.cpp) of every pixel. The lane plan of this launch and the state it leaves
// (lane_plan, lane_advance); then, side by side, the overlapped launch on a lane between its events and the serial
// launch on the caller's stream; then the resolve, on the caller's stream either way.
template <class R>
rt_status one_pass(rt_context* c, RenderCall<R>& rc, uint32_t c0) {
  const ItemPlan& plan = rc.plan;
  LaunchParams<R>& p = rc.p;
  const hipStream_t st = rc.st;
  rt_status s;
  const uint32_t pc = std::min(plan.cpp, plan.nchunks - c0);
  p.chunk0 = c0;
  p.n_items = rc.npix * pc;
  rc.lq.set_state(c->lane_state);
  const LanePlan lp = lane_plan(rc.lq);
  lane_advance(c->lane_state, lp);
  // runs only in a stream of overlapped launches, where the next launch hides this one's longer end (auto_run)
  const uint32_t run = rc.forced_run ? rc.forced_run
                                     : auto_run(plan, rc.kind, rc.spp, rc.npix, device_max_lanes(c),
                                                lp.overlap && rc.lq.prev_overlapped);
  const RunPlan rp = plan_runs(plan, rc.spp, c0, pc, rc.npix, run);
  p.n_units = rp.n_units;
  p.run_cfg = run_cfg_pack(rp.runs, rp.run_log2);
  const R* partial = (const R*)c->partial.ptr;
  if (lp.overlap) {
    hipStream_t lane = lp.lane ? c->lane1 : c->stream;
    if (lp.set) {
      p.partial = (R*)c->partial2.ptr;
      p.heads = (uint32_t*)c->heads2.ptr;
    } else {
      p.partial = (R*)c->partial.ptr;
      p.heads = (uint32_t*)c->heads.ptr;
    }
    partial = p.partial;
    // outstanding from here on, the lanes included, whatever fails below
    mark_pending(c, st);
    c->lanes_live = true;
    if (lp.wait_resolve) RT_HIP(c, hipStreamWaitEvent(lane, c->ev_resolved[lp.set], 0));
    if (lp.record_inputs) RT_HIP(c, hipEventRecord(c->ev_inputs, st));
    if (lp.wait_inputs) RT_HIP(c, hipStreamWaitEvent(lane, c->ev_inputs, 0));
    if ((s = run_persistent(c, p, rc.kind, rc.nblk_max, lane, true)) != RT_OK) return s;
    RT_HIP(c, hipEventRecord(c->ev_done[lp.lane], lane));
    // The caller's stream takes the launch in here, before its resolve: `out` is written on the caller's stream
    // alone, in the order of the calls, and whatever the caller queues behind this call (the next call's uploads
    // among it) is behind every launch so far.
    RT_HIP(c, hipStreamWaitEvent(st, c->ev_done[lp.lane], 0));
  } else {
    s = rc.persist ? run_persistent(c, p, rc.kind, rc.nblk_max, st) : run_wavefront(c, p, rc.kind, rc.nblk_max, st);
    if (s != RT_OK) return s;
  }
  rc.src.template resolve<R>(partial, rc.npix, c0, pc, plan, rc.spp, rc.dout, st);
  if (lp.overlap) RT_HIP(c, hipEventRecord(c->ev_resolved[lp.set], st));
  c->last.launches++;
  RT_HIP(c, hipGetLastError());
  return RT_OK;
}

// Step: the end of a call. A host `out` is copied out and the call returns finished and settled.
template <class R>
rt_status finish_render(rt_context* c, const RenderCall<R>& rc, std::chrono::steady_clock::time_point t0) {
  if (!rc.src.out_dev) {
    RT_HIP(c, hipMemcpyAsync(rc.src.out, rc.dout, 3ull * rc.npix * sizeof(R), hipMemcpyDeviceToHost, rc.st));
    RT_HIP(c, hipStreamSynchronize(rc.st));
    rt_status s;
    if ((s = settle(c)) != RT_OK) return s;
  }
  c->last.last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RT_OK;
}

// The path-traced pixels of `src` with the parameters `prm`, queued on `st`.
template <class R>
rt_status render(rt_context* c, const PixelSource& src, const rt_render_params* prm, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  RenderCall<R> rc{src, prm, st};
  rt_status s;
  if ((s = scene_to_device(c, sizeof(R) == 8, st, &rc.lq)) != RT_OK) return s;
  uint64_t npix64 = 0;
  const std::vector<uint4> tl = src.packed_tiles(npix64);
  if (npix64 >= (1ull << 31)) return set_err(c, RT_ERR_INVALID_ARGUMENT, "too many pixels in one call");
  rc.npix = (uint32_t)npix64;
  if (rc.npix == 0) return RT_OK;
  rc.dout = src.out;
  if (!src.out_dev) {
    if ((s = ensure(c, c->out_tmp, 3ull * rc.npix * sizeof(R))) != RT_OK) return s;
    rc.dout = c->out_tmp.ptr;
  }
  if (prm->max_depth <= 0) {
    if ((s = src.template depth0<R>(c, prm, rc.npix, rc.dout, st)) != RT_OK) return s;
  } else {
    if ((s = plan_call(c, rc)) != RT_OK) return s;
    if ((s = path_buffers(c, rc)) != RT_OK) return s;
    if ((s = src.expand_map(c, tl, rc.npix, st)) != RT_OK) return s;
    if ((s = fill_params(c, rc)) != RT_OK) return s;
    lane_setup(c, rc);
    for (uint32_t c0 = 0; c0 < rc.plan.nchunks; c0 += rc.plan.cpp)  // the passes (one for every BASELINE config but C5)
      if ((s = one_pass(c, rc, c0)) != RT_OK) return s;
    // device output: nothing waits here -- the segment counters (cumulative on the device), the
    // timing events and the fault word are settled by rt_stats, rt_reset_counters or a host-output call
    mark_pending(c, st);
    c->last.samples += (uint64_t)rc.npix * rc.spp;
  }
  return finish_render(c, rc, t0);
}

// ---------------------------------------------------------------- the query path
// What rt_trace_rays, rt_occluded, rt_render_aov and (the staging and the end alone) rt_camera_rays share. Each call:
// query_kernel_built, query_scene, its staging on the host path (stage), query_dev_scene with its own flag rule, its
// kernel arguments and launch, query_done.

// A build without the kernel of family `fam` refuses the call; what: "query", "occlusion" or "feature-buffer"
rt_status query_kernel_built(rt_context* c, TraceFamily fam, const char* what) {
  if (family_built(trace_render_family(fam))) return RT_OK;
  return set_err(c, RT_ERR_UNSUPPORTED, dev_only_lacks(std::string(trace_family_name(fam)) + " " + what + " kernel"));
}

// What a query or feature-buffer launch on `st` reads of the scene, in place: scene_to_device, then the (object,
// material) tables copied if rt_scene_upload has replaced them since (a buffer of their own: the blobs stay the render
// kernels').
rt_status query_scene(rt_context* c, bool f64, hipStream_t st) {
  const CompiledScene& cs = c->scene;
  rt_status s;
  if ((s = scene_to_device(c, f64, st)) != RT_OK) return s;
  if (c->ids_dirty) {
    if (!cs.ids.empty())
      RT_HIP(c, hipMemcpyAsync(c->ids.ptr, cs.ids.data(), cs.ids.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    c->ids_dirty = false;
    mark_pending(c, st);
  }
  return RT_OK;
}

// The device scene of a launch of family `fam`, with the spill area of a deep wide tree. The caller clears has_flat and
// has_wide by its own rule.
template <class R>
rt_status query_dev_scene(rt_context* c, TraceFamily fam, DevScene<R>& sc) {
  const bool f64 = sizeof(R) == 8;
  const SceneHeader& hdr = f64 ? c->scene.hdr64 : c->scene.hdr;
  sc = dev_scene<R>(hdr, f64 ? c->scene64.ptr : c->scene32.ptr);
  rt_status s;
  if (fam == TF_WIDE_HBM && (s = wide_spill_area<R>(c, hdr, sc)) != RT_OK) return s;
  // no camera: a near-edge quad hit is re-decided on the given ray, or the lane's own camera ray (quad_edge64)
  sc.cam64 = nullptr;
  return RT_OK;
}

// Host path: the context buffer `b`, grown to `bytes`, stands in for the caller's array behind `p`
template <class T>
rt_status stage(rt_context* c, DevBuf& b, size_t bytes, T*& p) {
  rt_status s;
  if ((s = ensure(c, b, bytes)) != RT_OK) return s;
  p = (T*)b.ptr;
  return RT_OK;
}

// The end of a call after its launch on `st`. The context has work outstanding on st (the launch reads the context's
// buffers, and the segment counter on the device settles with rt_stats, as after a device-output render). Host path:
// the staged outputs are copied out and the call returns finished and settled. counted: the launch is one of
// rt_counters.launches (rt_camera_rays' is not).
struct HostOut {
  void* host;
  const void* dev;
  size_t bytes;
};
rt_status query_done(rt_context* c, hipStream_t st, bool counted, bool on_device, std::initializer_list<HostOut> outs) {
  RT_HIP(c, hipGetLastError());
  if (counted) c->last.launches++;
  mark_pending(c, st);
  if (on_device) return RT_OK;
  for (const HostOut& o : outs) RT_HIP(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, st));
  RT_HIP(c, hipStreamSynchronize(st));
  return settle(c);
}

// rt_trace_rays for one precision: n rays (0 < n < 2^31) through the family trace_family gives the scene.
template <class R>
rt_status trace_rays(rt_context* c, const rt_trace_params* prm, const double* rays, uint32_t n, double* geom,
                     int32_t* ids, hipStream_t st) {
  const bool f64 = sizeof(R) == 8;
  const CompiledScene& cs = c->scene;
  const bool ordered = prm->traversal == RT_TRAV_ORDERED;
  const TraceFamily fam = trace_family(f64 ? cs.hdr64 : cs.hdr, ordered, sizeof(typename WWord<R>::T));
  rt_status s;
  if ((s = query_kernel_built(c, fam, "query")) != RT_OK) return s;
  if ((s = query_scene(c, f64, st)) != RT_OK) return s;
  TraceParams<R> p{};
  p.rays = rays;
  p.geom = geom;
  p.ids = ids;
  if (!prm->on_device) {
    if ((s = stage(c, c->q_rays, 64ull * n, p.rays)) != RT_OK) return s;
    if ((s = stage(c, c->q_geom, 56ull * n, p.geom)) != RT_OK) return s;
    if ((s = stage(c, c->q_ids, 16ull * n, p.ids)) != RT_OK) return s;
    RT_HIP(c, hipMemcpyAsync(c->q_rays.ptr, rays, 64ull * n, hipMemcpyHostToDevice, st));
  }
  if ((s = query_dev_scene<R>(c, fam, p.sc)) != RT_OK) return s;
  // a query leaves the flat program and the wide tree only when asked to (trace_family), so `ordered` says it all
  if (ordered) p.sc.has_flat = p.sc.has_wide = 0;
  p.idtab = (const int2*)c->ids.ptr;
  for (int k = 0; k < 4; k++) p.id_off[k] = cs.ids_off[k];
  p.n = n;
  p.seed = prm->seed;
  p.seg_shards = (unsigned long long*)c->counters.ptr;
  launch_trace<R>(p, fam, st);
  return query_done(c, st, true, prm->on_device != 0, {{geom, p.geom, 56ull * n}, {ids, p.ids, 16ull * n}});
}

// rt_occluded for one precision: trace_rays' family, stream and counters; one byte a ray (host path: in q_ids).
template <class R>
rt_status occluded(rt_context* c, const rt_trace_params* prm, const double* rays, uint32_t n, uint8_t* out,
                   hipStream_t st) {
  const bool f64 = sizeof(R) == 8;
  const SceneHeader& hdr = f64 ? c->scene.hdr64 : c->scene.hdr;
  const bool ordered = prm->traversal == RT_TRAV_ORDERED;
  const TraceFamily fam = trace_family(hdr, ordered, sizeof(typename WWord<R>::T));
  rt_status s;
  if ((s = query_kernel_built(c, fam, "occlusion")) != RT_OK) return s;
  if ((s = query_scene(c, f64, st)) != RT_OK) return s;
  OcclParams<R> p{};
  p.rays = rays;
  p.out = out;
  if (!prm->on_device) {
    if ((s = stage(c, c->q_rays, 64ull * n, p.rays)) != RT_OK) return s;
    if ((s = stage(c, c->q_ids, n, p.out)) != RT_OK) return s;
    RT_HIP(c, hipMemcpyAsync(c->q_rays.ptr, rays, 64ull * n, hipMemcpyHostToDevice, st));
  }
  if ((s = query_dev_scene<R>(c, fam, p.sc)) != RT_OK) return s;
  if (ordered) p.sc.has_flat = p.sc.has_wide = 0;  // as trace_rays
  p.n = n;
  p.seed = prm->seed;
  p.seg_shards = (unsigned long long*)c->counters.ptr;
  launch_occluded<R>(p, fam, occlusion_early_exit(hdr, fam, sizeof(typename WWord<R>::T)), st);
  return query_done(c, st, true, prm->on_device != 0, {{out, p.out, n}});
}

// rt_camera_rays: the rays of samples [first_sample, first_sample + spp) of the tiles' pixels, n = npix * spp rows.
// No scene, and no launch counted: rt_counters counts what traces.
rt_status camera_rays(rt_context* c, const rt_camera_desc* cam, uint64_t seed, int32_t first_sample, uint32_t spp,
                      const std::vector<uint4>& tl, uint32_t npix, double* out, bool on_device, hipStream_t st) {
  rt_status s;
  if ((s = wait_other_stream(c, st)) != RT_OK) return s;  // (it reads the pixel map and the camera view)
  if ((s = pixel_map(c, tl, npix, st)) != RT_OK) return s;
  if ((s = camera_view(c, cam, st)) != RT_OK) return s;
  const uint64_t n = (uint64_t)npix * spp;
  CamRayParams p{};
  p.pixmap = (const uint32_t*)c->pixmap.ptr;
  p.camx = (const CamDev*)c->camx.ptr;
  p.rays = out;
  if (!on_device && (s = stage(c, c->q_rays, 64ull * n, p.rays)) != RT_OK) return s;
  p.npix = npix;
  p.spp = spp;
  p.first_sample = (uint32_t)std::max(0, first_sample);
  p.W = (uint32_t)cam->image_width;
  p.cam_mode = c->cam_host.mode;
  p.seed = seed;
  launch_camera_rays(p, st);
  return query_done(c, st, false, on_device, {{out, p.rays, 64ull * n}});
}

// rt_render_aov for one precision: npix pixels (0 < npix * spp < 2^31) through the family aov_family gives the scene.
template <class R>
rt_status render_aov(rt_context* c, const rt_camera_desc* cam, const rt_aov_params* prm, const std::vector<uint4>& tl,
                     uint32_t npix, double* feat, int32_t* ids, hipStream_t st) {
  const bool f64 = sizeof(R) == 8;
  const CompiledScene& cs = c->scene;
  const SceneHeader& hdr = f64 ? cs.hdr64 : cs.hdr;
  const bool ordered = prm->traversal == RT_TRAV_ORDERED;
  const TraceFamily fam = aov_family(hdr, ordered, sizeof(typename WWord<R>::T));
  rt_status s;
  if ((s = query_kernel_built(c, fam, "feature-buffer")) != RT_OK) return s;
  if ((s = query_scene(c, f64, st)) != RT_OK) return s;
  if ((s = pixel_map(c, tl, npix, st)) != RT_OK) return s;
  if ((s = camera_view(c, cam, st)) != RT_OK) return s;
  AovParams<R> p{};
  p.feat = feat;
  p.ids = ids;
  if (!prm->on_device) {
    if ((s = stage(c, c->q_geom, 64ull * npix, p.feat)) != RT_OK) return s;
    if ((s = stage(c, c->q_ids, 16ull * npix, p.ids)) != RT_OK) return s;
  }
  if ((s = query_dev_scene<R>(c, fam, p.sc)) != RT_OK) return s;
  // not the queries' rule: a scene with a picture texture leaves the flat program without being asked to (aov_family),
  // and only the flat program; the wide tree is left as in a query
  if (fam != TF_FLAT) p.sc.has_flat = 0;
  if (ordered) p.sc.has_wide = 0;
  p.pixmap = (const uint32_t*)c->pixmap.ptr;
  p.camx = (const CamDev*)c->camx.ptr;
  p.idtab = (const int2*)c->ids.ptr;
  for (int k = 0; k < 4; k++) p.id_off[k] = cs.ids_off[k];
  p.npix = npix;
  p.spp = (uint32_t)prm->spp;
  p.first_sample = (uint32_t)std::max(0, prm->first_sample);
  p.W = (uint32_t)cam->image_width;
  p.cam_mode = c->cam_host.mode;
  p.ext = aov_extended(hdr, p.cam_mode) ? 1 : 0;
  p.seed = prm->seed;
  p.seg_shards = (unsigned long long*)c->counters.ptr;
  launch_aov<R>(p, fam, st);
  return query_done(c, st, true, prm->on_device != 0, {{feat, p.feat, 64ull * npix}, {ids, p.ids, 16ull * npix}});
}

// ---------------------------------------------------------------- adaptive sampling
// rt_render_adaptive for one precision: the round loop around render()'s pixel-list source. The tiles' pixel map is
// expanded once, into c->pixmap like any render's (so it stays the cached map of these tiles), and is round 0's list;
// the later rounds' lists are the select's survivors, in ad_pix / ad_slot, alternating. Every round: render() the
// list's next samples into the moment records, select (estimate, decision, outputs of the pixels that stop, the next
// list), and -- unless the round was the last there can be -- read the survivor count back and go on while it is not 0.
template <class R>
rt_status render_adaptive(rt_context* c, const rt_camera_desc* cam, const rt_adaptive_params* prm,
                          const std::vector<uint4>& tl, uint32_t npix, void* out_rgb, int32_t* out_spp, double* out_err,
                          hipStream_t st) {
  const bool f64 = sizeof(R) == 8;
  const auto t0 = std::chrono::steady_clock::now();
  const PathKernel kind = path_kernel(f64 ? c->scene.hdr64 : c->scene.hdr, sizeof(typename WWord<R>::T), cam->mode, true,
                                      prm->traversal == RT_TRAV_ORDERED, c->scene.stack_need);
  if (prm->max_depth > 0 && !family_built(kind.fam))  // (render() would say so too, after the records were cleared)
    return set_err(c, RT_ERR_UNSUPPORTED, dev_only_lacks(kind.fam));
  rt_status s;
  if ((s = wait_other_stream(c, st)) != RT_OK) return s;  // (the call writes the context's buffers from here on)
  const uint32_t nb = (npix + kBlock - 1) / kBlock;
  const bool rounds = prm->min_spp < prm->max_spp;
  if ((s = ensure(c, c->ad_acc, sizeof(AdaptiveAcc) * (size_t)npix)) != RT_OK) return s;
  if ((s = ensure(c, c->ad_blk, 4ull * (nb + 2))) != RT_OK) return s;
  for (int k = 0; rounds && k < 2; k++) {
    if ((s = ensure(c, c->ad_pix[k], 4ull * npix)) != RT_OK) return s;
    if ((s = ensure(c, c->ad_slot[k], 4ull * npix)) != RT_OK) return s;
  }
  SelectParams sp{};
  sp.out_rgb = out_rgb;
  sp.out_spp = out_spp;
  sp.out_err = out_err;
  if (!prm->on_device) {
    if ((s = stage(c, c->out_tmp, 3 * sizeof(R) * (size_t)npix, sp.out_rgb)) != RT_OK) return s;
    if ((s = stage(c, c->ad_spp, 4ull * npix, sp.out_spp)) != RT_OK) return s;
    if ((s = stage(c, c->ad_err, 8ull * npix, sp.out_err)) != RT_OK) return s;
  }
  if ((s = pixel_map(c, tl, npix, st)) != RT_OK) return s;
  mark_pending(c, st);  // outstanding from here on, whatever fails below
  RT_HIP(c, hipMemsetAsync(c->ad_acc.ptr, 0, sizeof(AdaptiveAcc) * (size_t)npix, st));
  sp.acc = (AdaptiveAcc*)c->ad_acc.ptr;
  sp.blk = (uint32_t*)c->ad_blk.ptr;
  sp.batch = (uint32_t)prm->batch;
  sp.max_spp = (uint32_t)prm->max_spp;
  sp.threshold = prm->threshold;
  sp.floor = prm->floor;
  // a round's render: the persistent schedule (no segments_per_launch), the automatic grid, an item a batch
  rt_render_params rp{};
  rp.max_depth = prm->max_depth;
  rp.seed = prm->seed;
  rp.precision = prm->precision;
  rp.samples_per_item = prm->batch;
  rp.traversal = prm->traversal;
  PixelList pl{(const uint32_t*)c->pixmap.ptr, nullptr, npix, sp.acc};
  int next = 0;
  for (int32_t have = 0;;) {
    rp.spp = have == 0 ? prm->min_spp : prm->step_spp;
    rp.first_sample = have;
    if ((s = render<R>(c, PixelSource::of_list(cam, pl), &rp, st)) != RT_OK) return s;
    have += rp.spp;
    const bool last = have >= prm->max_spp;  // every pixel stops after this round: no next list, no count to wait for
    sp.pixmap = pl.pixmap;
    sp.slots = pl.slots;
    sp.n = pl.n;
    sp.next_pixmap = last ? nullptr : (uint32_t*)c->ad_pix[next].ptr;
    sp.next_slots = last ? nullptr : (uint32_t*)c->ad_slot[next].ptr;
    launch_adaptive_select<R>(sp, st);
    c->last.launches += last ? 1 : 3;
    RT_HIP(c, hipGetLastError());
    if (last) break;
    RT_HIP(c, hipMemcpyAsync(c->total_host, sp.blk + (pl.n + kBlock - 1) / kBlock + 1, 4, hipMemcpyDeviceToHost, st));
    RT_HIP(c, hipStreamSynchronize(st));
    const uint32_t alive = *c->total_host;
    if (alive == 0) break;
    pl = PixelList{sp.next_pixmap, sp.next_slots, alive, sp.acc};
    next ^= 1;
  }
  c->last.last_render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return query_done(c, st, false, prm->on_device != 0,
                    {{out_rgb, sp.out_rgb, 3 * sizeof(R) * (size_t)npix},
                     {out_spp, sp.out_spp, 4ull * npix},
                     {out_err, sp.out_err, 8ull * npix}});
}

// rt_denoise for one precision: checked parameters, whole image. The prepare pass has read rgb_in before the last
// pass writes rgb_out, on one stream, so the two may be the same array.
template <class T>
rt_status denoise(rt_context* c, const rt_denoise_params* prm, const void* rgb_in, const double* feat,
                  const double* var, void* rgb_out, hipStream_t st) {
  const size_t npix = (size_t)prm->width * (size_t)prm->height;
  rt_status s;
  if ((s = wait_other_stream(c, st)) != RT_OK) return s;  // (a call on another stream may still use the scratch)
  if ((s = ensure(c, c->dn_scratch, npix * kDnScratchT * sizeof(T))) != RT_OK) return s;
  const T* in = (const T*)rgb_in;
  T* out = (T*)rgb_out;
  if (!prm->on_device) {
    const double *host_feat = feat, *host_var = var;
    if ((s = stage(c, c->out_tmp, npix * 3 * sizeof(T), out)) != RT_OK) return s;
    if ((s = stage(c, c->q_rays, npix * 64, feat)) != RT_OK) return s;
    if (var && (s = stage(c, c->q_geom, npix * 8, var)) != RT_OK) return s;
    in = out;
    RT_HIP(c, hipMemcpyAsync(out, rgb_in, npix * 3 * sizeof(T), hipMemcpyHostToDevice, st));
    RT_HIP(c, hipMemcpyAsync((void*)feat, host_feat, npix * 64, hipMemcpyHostToDevice, st));
    if (var) RT_HIP(c, hipMemcpyAsync((void*)var, host_var, npix * 8, hipMemcpyHostToDevice, st));
  }
  launch_denoise<T>(*prm, in, feat, var, (T*)c->dn_scratch.ptr, out, st);
  c->last.launches += (uint64_t)prm->iterations + 1;
  return query_done(c, st, false, prm->on_device != 0, {{rgb_out, out, npix * 3 * sizeof(T)}});
}

// rt_temporal for one precision: checked parameters, cameras and pointers, whole image. A pixel reads its own rgb and
// var before it writes them, so rgb_out may be rgb_in and var_out var. A host-pointer call stages the frame in the
// buffers rt_denoise's stages it in, the ids in q_ids and the two histories, one after the other, in dn_scratch.
template <class T>
rt_status temporal(rt_context* c, const rt_temporal_params* prm, const rt_camera_desc* cam,
                   const rt_camera_desc* prev_cam, const void* rgb_in, const double* feat, const int32_t* ids,
                   const double* var, const void* hist_in, void* hist_out, void* rgb_out, double* var_out,
                   hipStream_t st) {
  const size_t npix = (size_t)prm->width * (size_t)prm->height;
  const size_t hb = tp_history_bytes(npix, sizeof(T) == 8), hb_step = (hb + 255) / 256 * 256;
  rt_status s;
  if ((s = wait_other_stream(c, st)) != RT_OK) return s;  // (a call on another stream may still use the staging buffers)
  if (prm->on_device) {
    launch_temporal<T>(*prm, cam, prev_cam, (const T*)rgb_in, feat, ids, var, hist_in, hist_out, (T*)rgb_out, var_out, st);
    return query_done(c, st, true, true, {});
  }
  T* d_rgb = nullptr;
  double *d_feat = nullptr, *d_var = nullptr;
  int32_t* d_ids = nullptr;
  unsigned char* d_hist = nullptr;
  if ((s = stage(c, c->out_tmp, npix * 3 * sizeof(T), d_rgb)) != RT_OK) return s;
  if ((s = stage(c, c->q_rays, npix * 64, d_feat)) != RT_OK) return s;
  if ((var || var_out) && (s = stage(c, c->q_geom, npix * 8, d_var)) != RT_OK) return s;
  if (ids && (s = stage(c, c->q_ids, npix * 16, d_ids)) != RT_OK) return s;
  if ((s = stage(c, c->dn_scratch, 2 * hb_step, d_hist)) != RT_OK) return s;
  RT_HIP(c, hipMemcpyAsync(d_rgb, rgb_in, npix * 3 * sizeof(T), hipMemcpyHostToDevice, st));
  RT_HIP(c, hipMemcpyAsync(d_feat, feat, npix * 64, hipMemcpyHostToDevice, st));
  if (var) RT_HIP(c, hipMemcpyAsync(d_var, var, npix * 8, hipMemcpyHostToDevice, st));
  if (ids) RT_HIP(c, hipMemcpyAsync(d_ids, ids, npix * 16, hipMemcpyHostToDevice, st));
  if (hist_in) RT_HIP(c, hipMemcpyAsync(d_hist, hist_in, hb, hipMemcpyHostToDevice, st));
  launch_temporal<T>(*prm, cam, prev_cam, d_rgb, d_feat, d_ids, var ? d_var : nullptr, hist_in ? d_hist : nullptr,
                     d_hist + hb_step, d_rgb, var_out ? d_var : nullptr, st);
  if (var_out)
    return query_done(c, st, true, false,
                      {{rgb_out, d_rgb, npix * 3 * sizeof(T)}, {var_out, d_var, npix * 8}, {hist_out, d_hist + hb_step, hb}});
  return query_done(c, st, true, false, {{rgb_out, d_rgb, npix * 3 * sizeof(T)}, {hist_out, d_hist + hb_step, hb}});
}

// ---------------------------------------------------------------- argument checks of the C entry points
// Each check is written once; every entry point calls the ones it has in its own order (which error wins when several
// apply differs between them, and stays: tests/test_gpu_query_contract.py).
rt_status check_camera(rt_context* c, const rt_camera_desc* cam) {
  if (cam->mode < RT_CAM_PERSPECTIVE || cam->mode > RT_CAM_LENS)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "unknown camera mode");
  if (cam->image_width <= 0 || cam->image_height <= 0) return set_err(c, RT_ERR_INVALID_ARGUMENT, "empty image");
  if (cam->image_width > 65535 || cam->image_height > 65535)  // pixel positions are packed x | y << 16
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "image wider or taller than 65535 pixels");
  return RT_OK;
}
rt_status check_tiles(rt_context* c, const rt_camera_desc* cam, const rt_tile* tiles, int32_t ntiles) {
  for (int t = 0; t < ntiles; t++) {
    const rt_tile& tl = tiles[t];
    if (tl.x0 < 0 || tl.y0 < 0 || tl.width < 0 || tl.height < 0 || tl.x0 + tl.width > cam->image_width ||
        tl.y0 + tl.height > cam->image_height)
      return set_err(c, RT_ERR_INVALID_ARGUMENT, "tile " + std::to_string(t) + " outside the image");
  }
  return RT_OK;
}
rt_status check_spp(rt_context* c, int32_t spp) {
  return spp < 1 ? set_err(c, RT_ERR_INVALID_ARGUMENT, "spp must be positive") : RT_OK;
}
rt_status check_precision(rt_context* c, int32_t precision) {
  if (precision != RT_PREC_F32 && precision != RT_PREC_F64)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "unknown precision");
  return RT_OK;
}
rt_status check_precision_traversal(rt_context* c, int32_t precision, int32_t traversal) {
  rt_status s;
  if ((s = check_precision(c, precision)) != RT_OK) return s;
  if (traversal != RT_TRAV_AUTO && traversal != RT_TRAV_ORDERED)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "unknown traversal");
  return RT_OK;
}
rt_status check_nrays(rt_context* c, int64_t nrays) {
  if (nrays < 0 || nrays >= (1ll << 31)) return set_err(c, RT_ERR_INVALID_ARGUMENT, "nrays outside [0, 2^31)");
  return RT_OK;
}
rt_status check_npix_spp(rt_context* c, uint64_t npix, int32_t spp) {
  if (npix * (uint64_t)spp >= (1ull << 31)) return set_err(c, RT_ERR_INVALID_ARGUMENT, "npix * spp outside [0, 2^31)");
  return RT_OK;
}
rt_status check_scene(rt_context* c) {
  return c->has_scene ? RT_OK : set_err(c, RT_ERR_NO_SCENE, "rt_scene_upload has not succeeded on this context");
}

// The stream of a call. Device pointers: NULL is the HIP null stream (torch's default stream), so work the caller
// queues after this call on that stream -- a clone, a gather -- is ordered after it. Host pointers (the call returns
// finished): NULL is the context's own non-blocking stream, so contexts driven from different host threads do not
// serialise on the null stream.
hipStream_t call_stream(rt_context* c, void* stream, bool on_device) {
  return (stream == nullptr && !on_device) ? c->stream : (hipStream_t)stream;
}

// f() with running out of host memory reported as a status; any_exception: every other exception too (render<R>())
template <class F>
rt_status guarded(rt_context* c, bool any_exception, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return set_err(c, RT_ERR_OUT_OF_MEMORY, "out of host memory");
  } catch (const std::exception& e) {
    if (!any_exception) throw;
    return set_err(c, RT_ERR_INVALID_ARGUMENT, e.what());
  }
}
// ... and f(R()) for the float type R of a (checked) precision
template <class F>
rt_status by_precision(rt_context* c, int32_t precision, bool any_exception, F&& f) {
  return guarded(c, any_exception, [&] { return precision == RT_PREC_F64 ? f(double()) : f(float()); });
}

// rt_dev_plan_kernel and rt_dev_plan_radiance: `desc` compiled on the host, and the tag of the kernel that
// kernel_of(header, word bytes, ordered, stack need) chooses for it in buf[n]; "" for a descriptor that does not compile
// or an unknown precision or traversal
template <class F>
void dev_plan_tag(const rt_scene_desc* desc, int32_t precision, int32_t traversal, char* buf, size_t n, F&& kernel_of) {
  if (!buf || n == 0) return;
  buf[0] = 0;
  CompiledScene cs;
  std::string err;
  if (!desc || (precision != RT_PREC_F32 && precision != RT_PREC_F64) ||
      (traversal != RT_TRAV_AUTO && traversal != RT_TRAV_ORDERED) || compile_scene(desc, &cs, &err) != RT_OK)
    return;
  const bool f64 = precision == RT_PREC_F64;
  const size_t word_bytes = f64 ? sizeof(WWord<double>::T) : sizeof(WWord<float>::T);
  const PathKernel k = kernel_of(f64 ? cs.hdr64 : cs.hdr, word_bytes, traversal == RT_TRAV_ORDERED, cs.stack_need);
  std::snprintf(buf, n, "%s", path_kernel_tag(k, word_bytes).c_str());
}

}  // namespace

// ====================================================================== C ABI

extern "C" {

int32_t rt_abi_version(void) { return RT_ABI_VERSION; }

#define RT_STR2(x) #x
#define RT_STR(x) RT_STR2(x)
const char* rt_build_info(void) {
  return "dev_only=" RT_STR(RT_DEV_ONLY) " wide_top_n=" RT_STR(RT_WIDE_TOP_N) " wide_lds_stack=" RT_STR(RT_WIDE_LDS_STACK) " wide_waves_global=" RT_STR(RT_WIDE_WAVES_GLOBAL)
#ifdef RT_SECTION_CLOCKS
      " sections=1"
#endif
#ifdef RT_DEBUG_TRACE
      " trace=1"
#endif
#ifdef RT_PRECISE_F32
      " precise_f32=1"
#endif
      ;
}
#undef RT_STR
#undef RT_STR2

rt_status rt_context_create(int32_t device, rt_context** out) {
  if (!out) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "out is null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    (void)hipGetLastError();
    return set_err(nullptr, RT_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  }
  if (device < 0 || device >= n) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "device index out of range");
  if ((e = hipSetDevice(device)) != hipSuccess) return set_err(nullptr, RT_ERR_HIP, hipGetErrorString(e));
  if ((e = upload_sincos_table()) != hipSuccess)
    return set_err(nullptr, RT_ERR_HIP, std::string("sin/cos table: ") + hipGetErrorString(e));
  int ncu = 0;
  if ((e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess)
    return set_err(nullptr, RT_ERR_HIP, hipGetErrorString(e));
  auto* c = new rt_context;
  c->device = device;
  c->ncu = ncu;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
    delete c;
    return set_err(nullptr, RT_ERR_HIP, hipGetErrorString(e));
  }
  if ((e = hipHostMalloc((void**)&c->total_host, 64 + 8 * kSegShards, hipHostMallocDefault)) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return set_err(nullptr, RT_ERR_HIP, hipGetErrorString(e));
  }
  if (ensure(c, c->counters, sizeof(unsigned long long) * kSegShards) != RT_OK || ensure(c, c->fault, 4) != RT_OK ||
      hipMemset(c->counters.ptr, 0, sizeof(unsigned long long) * kSegShards) != hipSuccess ||
      hipMemset(c->fault.ptr, 0, 4) != hipSuccess) {
    std::string m = c->err;
    rt_context_destroy(c);
    return set_err(nullptr, RT_ERR_OUT_OF_MEMORY, m);
  }
  *out = c;
  return RT_OK;
}

void rt_context_destroy(rt_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // an outstanding device-output render still reads the buffers freed with the context below (its fault word
  // is dropped with it: nobody is left to report it to)
  if (c->pending) (void)hipStreamSynchronize(c->pend_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->lane1) (void)hipStreamSynchronize(c->lane1);
  for (hipEvent_t e : {c->ev_done[0], c->ev_done[1], c->ev_resolved[0], c->ev_resolved[1], c->ev_inputs})
    if (e) (void)hipEventDestroy(e);
  if (c->lane1) (void)hipStreamDestroy(c->lane1);
  for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
  if (c->total_host) (void)hipHostFree(c->total_host);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // (every DevBuf frees its memory)
}

const char* rt_last_error(const rt_context* c) {
  if (c) return c->err.c_str();
  std::lock_guard<std::mutex> lk(g_err_mu);
  return g_create_err.c_str();
}

rt_status rt_scene_upload(rt_context* c, const rt_scene_desc* desc) {
  if (!c || !desc) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null context or descriptor");
  RT_HIP(c, hipSetDevice(c->device));
  CompiledScene cs;
  std::string err;
  rt_status s = compile_scene(desc, &cs, &err);
  if (s != RT_OK) return set_err(c, s, err);
  // renders still pending on any stream, and on the lanes, read the current scene buffers
  if ((s = wait_pending(c)) != RT_OK) return s;
  if ((s = ensure(c, c->scene32, cs.blob32.size())) != RT_OK) return s;
  if ((s = ensure(c, c->scene64, cs.blob64.size())) != RT_OK) return s;
  if ((s = ensure(c, c->ids, cs.ids.size() * sizeof(int32_t))) != RT_OK) return s;
  c->scene = std::move(cs);  // copied to the device by the next render, on its stream (render<R>)
  c->scene_dirty32 = c->scene_dirty64 = true;
  c->ids_dirty = true;
  c->has_scene = true;
  return RT_OK;
}

rt_status rt_scene_check(const rt_scene_desc* desc, rt_scene_info* info, char* err, int32_t errlen) {
  CompiledScene cs;
  std::string m;
  rt_status s = desc ? compile_scene(desc, &cs, &m) : RT_ERR_INVALID_ARGUMENT;
  if (!desc) m = "null descriptor";
  if (s == RT_OK) {  // the kernels a perspective render on the default (persistent) schedule would take
    const KernelFamily fam = kernel_family(cs.hdr, RT_CAM_PERSPECTIVE, true, false);
    if (!family_built(fam)) {
      s = RT_ERR_UNSUPPORTED;
      m = dev_only_lacks(fam);
    }
  }
  if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", m.c_str());
  if (s == RT_OK && info) {
    const SceneHeader& h = cs.hdr;
    info->quads = cs.desc_quads;
    info->flat_quads = cs.flat_quads;
    info->flat_boxes = cs.flat_boxes;
    info->wide_nodes = cs.hdr.has_wide ? (int32_t)cs.hdr.n_wnodes : 0;
    info->wide_stack = cs.hdr.has_wide ? (int32_t)cs.hdr.wide_stack : 0;
    info->wide_kinds = cs.hdr.has_wide ? (int32_t)cs.hdr.wide_kinds : 0;
    info->wide_prim_words = cs.hdr.has_wide ? (int32_t)cs.hdr.n_wprim_words : 0;
    info->wide_big = cs.hdr.has_wide ? (int32_t)cs.hdr.wide_big : 0;
    info->spheres = (int32_t)h.n_spheres;
    info->triangles = (int32_t)h.n_tris;
    info->instances = h.num_instances;
    info->volumes = (int32_t)h.n_volumes;
    info->bvh_nodes = (int32_t)h.n_nodes;
    info->linear_ops = (int32_t)h.n_linear;
    info->stack_need = cs.stack_need;
    info->bytes_f32 = cs.blob32.size();
    info->bytes_f64 = cs.blob64.size();
  }
  return s;
}

rt_status rt_render_tiles(rt_context* c, const rt_camera_desc* cam, const rt_render_params* prm, const rt_tile* tiles,
                          int32_t ntiles, void* out_rgb, int32_t out_is_device, void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!cam || !prm || (!tiles && ntiles > 0) || ntiles < 0 || (!out_rgb && ntiles > 0))
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if ((s = check_scene(c)) != RT_OK) return s;
  if ((s = check_camera(c, cam)) != RT_OK) return s;
  if ((s = check_spp(c, prm->spp)) != RT_OK) return s;
  if ((s = check_precision(c, prm->precision)) != RT_OK) return s;
  if ((s = check_tiles(c, cam, tiles, ntiles)) != RT_OK) return s;
  RT_HIP(c, hipSetDevice(c->device));
  hipStream_t st = call_stream(c, stream, out_is_device != 0);
  return by_precision(c, prm->precision, true, [&](auto r) {
    return render<decltype(r)>(c, PixelSource::of_tiles(cam, tiles, ntiles, out_rgb, out_is_device != 0), prm, st);
  });
}

rt_status rt_trace_rays(rt_context* c, const rt_trace_params* prm, const double* rays, int64_t nrays, double* out_geom,
                        int32_t* out_ids, void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!prm || !rays || !out_geom || !out_ids) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if ((s = check_nrays(c, nrays)) != RT_OK) return s;
  if ((s = check_precision_traversal(c, prm->precision, prm->traversal)) != RT_OK) return s;
  // the kernel reads a ray and writes its ids as 16-byte words
  if (prm->on_device && (((uintptr_t)rays | (uintptr_t)out_ids) % 16 != 0 || (uintptr_t)out_geom % 8 != 0))
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device rays and out_ids must be 16-byte aligned, out_geom 8-byte");
  if ((s = check_scene(c)) != RT_OK) return s;
  if (nrays == 0) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  hipStream_t st = call_stream(c, stream, prm->on_device != 0);
  return by_precision(c, prm->precision, false, [&](auto r) {
    return trace_rays<decltype(r)>(c, prm, rays, (uint32_t)nrays, out_geom, out_ids, st);
  });
}

rt_status rt_occluded(rt_context* c, const rt_trace_params* prm, const double* rays, int64_t nrays,
                      uint8_t* out_occluded, void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!prm || !rays || !out_occluded) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if ((s = check_nrays(c, nrays)) != RT_OK) return s;
  if ((s = check_precision_traversal(c, prm->precision, prm->traversal)) != RT_OK) return s;
  if (prm->on_device && (uintptr_t)rays % 16 != 0)  // the kernel reads a ray as 16-byte words
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device rays must be 16-byte aligned");
  if ((s = check_scene(c)) != RT_OK) return s;
  if (nrays == 0) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  hipStream_t st = call_stream(c, stream, prm->on_device != 0);
  return by_precision(c, prm->precision, false, [&](auto r) {
    return occluded<decltype(r)>(c, prm, rays, (uint32_t)nrays, out_occluded, st);
  });
}

rt_status rt_radiance(rt_context* c, const rt_radiance_params* prm, const double* rays, int64_t nrays, void* out_rgb,
                      void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!prm || !rays || !out_rgb) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if (nrays < 0 || (uint64_t)prm->ray_base + (uint64_t)nrays > (1ull << 32))
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "nrays negative, or ray_base + nrays above 2^32");
  if ((s = check_spp(c, prm->spp)) != RT_OK) return s;
  if (prm->max_depth < 0) return set_err(c, RT_ERR_INVALID_ARGUMENT, "max_depth must not be negative");
  // the item planner's limit: a call's pixels -- here its rays -- below 2^31 (any spp: the chunks then come in passes)
  if ((s = check_nrays(c, nrays)) != RT_OK) return s;
  if ((s = check_precision_traversal(c, prm->precision, prm->traversal)) != RT_OK) return s;
  if (prm->on_device && ((uintptr_t)rays | (uintptr_t)out_rgb) % 16 != 0)  // the kernel reads a ray as 16-byte words
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device rays and out_rgb must be 16-byte aligned");
  if ((s = check_scene(c)) != RT_OK) return s;
  if (nrays == 0) return RT_OK;
  RT_HIP(c, hipSetDevice(c->device));
  hipStream_t st = call_stream(c, stream, prm->on_device != 0);
  // a render's parameters: the persistent schedule (no segments_per_launch), the automatic grid
  rt_render_params rp{};
  rp.spp = prm->spp;
  rp.max_depth = prm->max_depth;
  rp.seed = prm->seed;
  rp.precision = prm->precision;
  rp.first_sample = prm->first_sample;
  rp.samples_per_item = prm->samples_per_item;
  rp.traversal = prm->traversal;
  const RayBatch rb{rays, (uint32_t)nrays, prm->ray_base, prm->on_device != 0};
  return by_precision(c, prm->precision, true, [&](auto r) {
    return render<decltype(r)>(c, PixelSource::of_rays(rb, out_rgb, prm->on_device != 0), &rp, st);
  });
}

rt_status rt_camera_rays(rt_context* c, const rt_camera_desc* cam, uint64_t seed, int32_t first_sample, int32_t spp,
                         const rt_tile* tiles, int32_t ntiles, double* out_rays, int32_t on_device, void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!cam || !tiles || !out_rays || ntiles < 0) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if ((s = check_spp(c, spp)) != RT_OK) return s;
  if (on_device && (uintptr_t)out_rays % 16 != 0)  // the kernel writes a ray as 16-byte words
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device out_rays must be 16-byte aligned");
  if ((s = check_camera(c, cam)) != RT_OK) return s;
  if ((s = check_tiles(c, cam, tiles, ntiles)) != RT_OK) return s;
  return guarded(c, false, [&]() -> rt_status {
    uint64_t npix = 0;
    const std::vector<uint4> tl = pack_tiles(tiles, ntiles, npix);
    if ((s = check_npix_spp(c, npix, spp)) != RT_OK) return s;
    if (npix == 0) return RT_OK;
    RT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, stream, on_device != 0);
    return camera_rays(c, cam, seed, first_sample, (uint32_t)spp, tl, (uint32_t)npix, out_rays, on_device != 0, st);
  });
}

rt_status rt_render_aov(rt_context* c, const rt_camera_desc* cam, const rt_aov_params* prm, const rt_tile* tiles,
                        int32_t ntiles, double* out_feat, int32_t* out_ids, void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!cam || !prm || !tiles || !out_feat || !out_ids || ntiles < 0)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  rt_status s;
  if ((s = check_spp(c, prm->spp)) != RT_OK) return s;
  if ((s = check_precision_traversal(c, prm->precision, prm->traversal)) != RT_OK) return s;
  if (prm->on_device && ((uintptr_t)out_feat | (uintptr_t)out_ids) % 16 != 0)  // both are written as 16-byte words
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device out_feat and out_ids must be 16-byte aligned");
  if ((s = check_camera(c, cam)) != RT_OK) return s;
  if ((s = check_tiles(c, cam, tiles, ntiles)) != RT_OK) return s;
  if ((s = check_scene(c)) != RT_OK) return s;
  return by_precision(c, prm->precision, false, [&](auto r) -> rt_status {
    uint64_t npix = 0;
    const std::vector<uint4> tl = pack_tiles(tiles, ntiles, npix);
    if ((s = check_npix_spp(c, npix, prm->spp)) != RT_OK) return s;
    if (npix == 0) return RT_OK;
    RT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, stream, prm->on_device != 0);
    return render_aov<decltype(r)>(c, cam, prm, tl, (uint32_t)npix, out_feat, out_ids, st);
  });
}

rt_status rt_adaptive_check(const rt_adaptive_params* prm, char* err, int32_t errlen) {
  const char* m = prm ? adaptive_params_error(*prm) : "null parameters";
  if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", m ? m : "");
  return m ? RT_ERR_INVALID_ARGUMENT : RT_OK;
}

rt_status rt_render_adaptive(rt_context* c, const rt_camera_desc* cam, const rt_adaptive_params* prm,
                             const rt_tile* tiles, int32_t ntiles, void* out_rgb, int32_t* out_spp, double* out_err,
                             void* stream) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (!cam || !prm || (!tiles && ntiles > 0) || ntiles < 0 || !out_rgb || !out_spp || !out_err)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* m = adaptive_params_error(*prm)) return set_err(c, RT_ERR_INVALID_ARGUMENT, m);
  if (prm->on_device && ((uintptr_t)out_rgb | (uintptr_t)out_spp | (uintptr_t)out_err) % 16 != 0)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device out_rgb, out_spp and out_err must be 16-byte aligned");
  rt_status s;
  if ((s = check_camera(c, cam)) != RT_OK) return s;
  if ((s = check_tiles(c, cam, tiles, ntiles)) != RT_OK) return s;
  if ((s = check_scene(c)) != RT_OK) return s;
  return by_precision(c, prm->precision, true, [&](auto r) -> rt_status {
    uint64_t npix = 0;
    const std::vector<uint4> tl = pack_tiles(tiles, ntiles, npix);
    if (npix >= (1ull << 31)) return set_err(c, RT_ERR_INVALID_ARGUMENT, "too many pixels in one call");
    if (npix == 0) return RT_OK;
    RT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, stream, prm->on_device != 0);
    return render_adaptive<decltype(r)>(c, cam, prm, tl, (uint32_t)npix, out_rgb, out_spp, out_err, st);
  });
}

// The estimator as the kernel runs it (rt_plan.h adaptive_error), for tests: no device, no stability promise.
void rt_dev_adaptive_error(int32_t K, int32_t batch, const double* S, const double* Q, double floor, double* mean3,
                           double* err) {
  adaptive_error((uint32_t)K, (uint32_t)batch, S, Q, floor, mean3, err);
}

// (rt_denoise_check and rt_dev_denoise_host, which need no context: rt_denoise.hip)
rt_status rt_denoise(rt_context* c, const rt_denoise_params* prm, const void* rgb_in, const double* feat,
                     const double* var, void* rgb_out, void* stream) {
  // (the context last: the checks before it need none, and rt_last_error(NULL) names the one that failed)
  if (!prm || !rgb_in || !feat || !rgb_out) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* m = denoise_params_error(*prm)) return set_err(c, RT_ERR_INVALID_ARGUMENT, m);
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (prm->on_device && ((uintptr_t)rgb_in | (uintptr_t)feat | (uintptr_t)var | (uintptr_t)rgb_out) % 16 != 0)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device rgb_in, feat, var and rgb_out must be 16-byte aligned");
  return by_precision(c, prm->precision, false, [&](auto r) -> rt_status {
    RT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, stream, prm->on_device != 0);
    return denoise<decltype(r)>(c, prm, rgb_in, feat, var, rgb_out, st);
  });
}

// (rt_temporal_check, rt_temporal_history_bytes and rt_dev_temporal_host, which need no context: rt_temporal.hip)
rt_status rt_temporal(rt_context* c, const rt_temporal_params* prm, const rt_camera_desc* cam,
                      const rt_camera_desc* prev_cam, const void* rgb_in, const double* feat, const int32_t* ids,
                      const double* var, const void* hist_in, void* hist_out, void* rgb_out, double* var_out,
                      void* stream) {
  // (the context last, as in rt_denoise)
  if (!prm || !cam || !rgb_in || !feat || !hist_out || !rgb_out || (hist_in && !prev_cam))
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  const char* m = nullptr;
  if (const rt_status s = temporal_check(prm, cam, hist_in ? prev_cam : nullptr, &m)) return set_err(c, s, m);
  if (hist_in && tp_overlap(hist_in, hist_out,
                            tp_history_bytes((size_t)prm->width * (size_t)prm->height, prm->precision == RT_PREC_F64)))
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "hist_in and hist_out overlap");
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  if (prm->on_device && ((uintptr_t)rgb_in | (uintptr_t)feat | (uintptr_t)ids | (uintptr_t)var | (uintptr_t)hist_in |
                         (uintptr_t)hist_out | (uintptr_t)rgb_out | (uintptr_t)var_out) % 16 != 0)
    return set_err(c, RT_ERR_INVALID_ARGUMENT, "device pointers must be 16-byte aligned");
  return by_precision(c, prm->precision, false, [&](auto r) -> rt_status {
    RT_HIP(c, hipSetDevice(c->device));
    hipStream_t st = call_stream(c, stream, prm->on_device != 0);
    return temporal<decltype(r)>(c, prm, cam, prev_cam, rgb_in, feat, ids, var, hist_in, hist_out, rgb_out, var_out, st);
  });
}

int32_t rt_trace_family(rt_context* c, int32_t precision, int32_t traversal) {
  if (!c || !c->has_scene || (precision != RT_PREC_F32 && precision != RT_PREC_F64) ||
      (traversal != RT_TRAV_AUTO && traversal != RT_TRAV_ORDERED))
    return -1;
  const bool f64 = precision == RT_PREC_F64;
  return (int32_t)trace_family(f64 ? c->scene.hdr64 : c->scene.hdr, traversal == RT_TRAV_ORDERED,
                               f64 ? sizeof(WWord<double>::T) : sizeof(WWord<float>::T));
}

rt_status rt_stats(rt_context* c, rt_counters* out) {
  if (!c || !out) return set_err(c, RT_ERR_INVALID_ARGUMENT, "null argument");
  RT_HIP(c, hipSetDevice(c->device));
  const rt_status s = settle(c);
  *out = c->last;
  return s;
}

rt_status rt_reset_counters(rt_context* c) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  RT_HIP(c, hipSetDevice(c->device));
  const rt_status s = settle(c);  // nothing of this context is outstanding after it
  RT_HIP(c, hipMemsetAsync(c->counters.ptr, 0, sizeof(unsigned long long) * kSegShards, c->stream));
  if (c->fault.ptr) RT_HIP(c, hipMemsetAsync(c->fault.ptr, 0, 4, c->stream));
  RT_HIP(c, hipStreamSynchronize(c->stream));
  c->last = rt_counters{};
  return s;
}

rt_status rt_set_timing(rt_context* c, int32_t enable) {
  if (!c) return set_err(nullptr, RT_ERR_INVALID_ARGUMENT, "null context");
  c->timing = enable ? 1 : 0;
  return RT_OK;
}

uint32_t rt_rng_u32(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t dim) {
  return draw_u32(key_path(key_pixel(seed, pixel), key_sample(seed, sample)), dim);
}

// The tag of the path kernel a render of `desc` with these arguments would launch (path_kernel, as render() asks it),
// in rt_dev_last_kernel's format; "" for a descriptor that does not compile or an unknown precision or traversal.
// Compiles the descriptor on the host as rt_scene_check does and touches no GPU. A development entry point beside
// rt_dev_last_kernel: for tests and scripts, not in rt_hip.h.
void rt_dev_plan_kernel(const rt_scene_desc* desc, int32_t cam_mode, int32_t precision, int32_t traversal,
                        int32_t segments_per_launch, char* buf, size_t n) {
  dev_plan_tag(desc, precision, traversal, buf, n, [&](const SceneHeader& h, size_t word_bytes, bool ordered, auto need) {
    return path_kernel(h, word_bytes, cam_mode, segments_per_launch <= 0, ordered, need);
  });
}
// The same for rt_radiance on a scene of `desc` (radiance_kernel): the tag a perspective render's kernel has, with
// "rays" before the schedule.
void rt_dev_plan_radiance(const rt_scene_desc* desc, int32_t precision, int32_t traversal, char* buf, size_t n) {
  dev_plan_tag(desc, precision, traversal, buf, n, [](const SceneHeader& h, size_t word_bytes, bool ordered, auto need) {
    return radiance_kernel(h, word_bytes, ordered, need);
  });
}

}  // extern "C"

// The denoiser's kernels, their launch function and its two host-only entry points: a file of their own, compiled as
// part of this translation unit, so that the library stays the four sources every build of it lists.
#include "rt_denoise.hip"
// ... and rt_temporal's kernel with its three host-only entry points, the same way.
#include "rt_temporal.hip"
