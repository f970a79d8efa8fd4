// rt_kernels.hip -- the kernels of the wavefront path tracer for MI355X (gfx950) and the functions that
// launch them (rt_launch.h). The host side -- contexts, render(), the C ABI -- is rt_render.hip.
//
// The reference's per-pixel/per-sample loop (camera.h:154-172) and recursive ray_color (camera.h:193-241)
// become P path slots (Schedules). Default schedule: k_persist, one launch of as many lanes as the
// chip holds resident, each keeping its path in registers and pulling work items (pixel, chunk of samples) from
// per-XCD dequeue heads. Wavefront schedule (segments_per_launch = K > 0): the slots' state lives in HBM between
// launches -- k_init, then k_step (every live slot advances up to K segments) with k_count / k_scan / k_compact
// rebuilding the live-slot queue. k_resolve: the per-pixel mean over the chunks, in chunk order. Each sample's
// random numbers are keyed by (seed, global pixel, sample), so the image is bit-identical for any pool size,
// tiling or GPU count. k_trace: closest hits of caller-given rays through the same traversals (rt_trace_rays).
// k_persist over RaysOf<policy>: the persistent kernels with a batch of caller-given rays as their ray source, radiance
// along those rays (rt_radiance).
// k_camera_rays: the rays a render draws (rt_camera_rays); k_aov: per pixel the first-hit albedo, normal, depth and
// ids over those rays, through k_trace's loop (rt_render_aov).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>

#include "../../include/rt_hip.h"
#include "rt_device.h"
#include "rt_launch.h"

using namespace rtd;

namespace {

#ifndef RT_LINEAR_WAVES
#define RT_LINEAR_WAVES 6
#endif
#ifndef RT_STACK_WAVES  // 4: the LDS limit of the LDS-node BVH kernel (32.8 KB per block); C3 151 -> 129 ms vs 3
#define RT_STACK_WAVES 4
#endif
#ifndef RT_LINEAR_WAVES_F64  // fp64 linear programs: waves per SIMD the register budget is cut for (C5 fp64:
#define RT_LINEAR_WAVES_F64 3   // none (2 waves) 3,605 ms/frame, 3: 2,865, 4: 3,885)
#endif
#ifndef RT_STACK_WAVES_F64  // fp64 binary BVH with its nodes in HBM (C4 fp64: none (2 waves) 2,019 ms/frame, 3: 1,964,
#define RT_STACK_WAVES_F64 4  // 4: 1,704); with the nodes in LDS (C3 fp64) none: 260 ms, 3: 295, 4: 276
#endif
#ifndef RT_LINEAR_VOL_WAVES  // fp32 quad + volume linear program (C5), with slab-tested box() volumes: 1 (4 waves at
                             // 128 VGPRs) 1661 ms/frame, 5: 1567, 6: 2594 (spills); round 4 (cold state in LDS,
#define RT_LINEAR_VOL_WAVES 6  // radiance folded, table sin/cos): 5: 1,326, 6: 1,247
#endif
// the LLI volume program (lambertian + isotropic + light scenes, shade LL, LLI: C5 fp32 1,189 -> 1,124 ms/frame,
// fp64 2,358 -> 2,262, r05y), its fp32 form at 7 waves per SIMD (72 VGPRs + 36 B spilled; 79 VGPRs at 6): 1,124 ->
// 1,097 ms/frame (r05y). 8 waves (64 VGPRs + 60 B spilled) was 1.6 % faster (r05v2; r06a 1,070 against 1,094 ms) but
// its scratch -- 60 B for each of 8,192 waves' 64 lanes, 31 MB, about the L2s' size -- went to memory: 78.6 GB of
// writes per launch (r06a PMC) against 2.2 GB at 7 waves, where the partial sums are ~1.2 GB. Round 6 keeps 7.
#ifndef RT_LINEAR_VOL_WAVES_LLI
#define RT_LINEAR_VOL_WAVES_LLI 7
#endif
#ifndef RT_LINEAR_VOL_WAVES_F64  // the fp64 volume program (round 4, cold state in LDS): 3 waves 2,672 ms/frame, 4: 2,400
#define RT_LINEAR_VOL_WAVES_F64 4
#endif
constexpr uint32_t kQBatch = 64;  // items a wave takes from a head at a time (rt_launch.h kHeads)
constexpr uint32_t kNoItem = 0xFFFFFFFFu;

// utility.h:46-52 random_in_unit_disk by rejection; attempt k draws dimensions kDimDisk + 2k
// and + 2k + 1 (far above the per-bounce dimensions); the origin after kDiskTries failures
// (probability (1 - pi/4)^64 ~ 1e-43). Same as the oracle.
constexpr uint32_t kDimDisk = 0x7FFF0000u, kDiskTries = 64;

// The kernels' argument: LaunchParams as a type of this translation unit, like the kernels themselves.
template <class R>
struct Params : LaunchParams<R> {};

// The per-lane words of the path state that only sample and item boundaries touch (LC paths,
// below), in LDS as [word][lane]: 32-bit words, then the fp64 pixel base as [component][lane].
constexpr int kColdWords = 8, kColdDoubles = 3;
__device__ __forceinline__ uint32_t* cold_words() {
  __shared__ uint32_t w[kColdWords * kBlock];
  return w + threadIdx.x;
}
__device__ __forceinline__ double* cold_doubles() {
  __shared__ double w[kColdDoubles * kBlock];
  return w + threadIdx.x;
}
// the throughput of an LT path ([component][lane])
template <class R>
__device__ __forceinline__ R* cold_thr() {
  __shared__ R w[3 * kBlock];
  return w + threadIdx.x;
}
// the fp64 item sum of an LC path ([component][lane]; fp32 keeps it in three of the cold words)
__device__ __forceinline__ __attribute__((unused)) double* cold_acc64() {
  __shared__ double w[3 * kBlock];
  return w + threadIdx.x;
}

// One path's state. The fields a segment reads stay in registers; the cold ones -- the item's
// running sum, its pixel and RNG key, the sample counter and range, the fp64 camera base -- are
// registers too unless LC, where they live in the lane's LDS words (cold_words) so the trace and
// shade code of the persistent loop gets their 14 VGPRs.
// LEAN: the pixel key, the end of the item's sample range and the camera base are not kept at all but
// recomputed where they are used (ka_of, send_of, begin_sample): 8 fewer registers for kernels whose
// traversal state competes with them (the wide BVH kernels), at a few integer and fp64 operations per
// sample.
// NORAD: no radiance register either (shade adds emission straight into the item's running sum).
// LT: the throughput in the lane's LDS words too (cold_thr; the fp32 LLI volume kernel, whose 72-VGPR budget
// otherwise spills it to scratch every segment)
template <class R, bool LC = false, bool LEAN = false, bool NORAD = LEAN, bool LT = false>
struct Path {
  static constexpr bool kLean = LEAN;
  static constexpr bool kNoRad = NORAD;
  V<R> o, d, thr_, rad;
  R tm;
  int32_t bounce;
  uint32_t ks;
  uint32_t xe;
  int32_t xi;
  // cold state (register copies: unused when LC)
  V<R> acc_;
  uint32_t ka_, item_, sample_, send_, xy_;
  V<double> cb_;  // (dir00 + x du) + y dv of the item's pixel (pixel_base)
#ifdef RT_ITEM_CLOCKS
  uint64_t t0_;  // development: wall clock at the item's start
#endif
  enum { kAcc = 0, kKa = 3, kItem, kSample, kSend, kXy };
  __device__ __forceinline__ V<R> thr() const {
    if constexpr (LT) return mkv(cold_thr<R>()[0], cold_thr<R>()[kBlock], cold_thr<R>()[2 * kBlock]);
    else return thr_;
  }
  __device__ __forceinline__ void set_thr(V<R> v) {
    if constexpr (LT) {
      cold_thr<R>()[0] = v.x;
      cold_thr<R>()[kBlock] = v.y;
      cold_thr<R>()[2 * kBlock] = v.z;
    } else {
      thr_ = v;
    }
  }
  __device__ __forceinline__ static uint32_t& w(int k) { return cold_words()[k * kBlock]; }
  __device__ __forceinline__ V<R> acc() const {
    if constexpr (LC && sizeof(R) == 8) {
      return mkv(cold_acc64()[0], cold_acc64()[kBlock], cold_acc64()[2 * kBlock]);
    } else if constexpr (LC) {
      return mkv(__uint_as_float(w(kAcc)), __uint_as_float(w(kAcc + 1)), __uint_as_float(w(kAcc + 2)));
    } else {
      return acc_;
    }
  }
  __device__ __forceinline__ void set_acc(V<R> v) {
    if constexpr (LC && sizeof(R) == 8) {
      cold_acc64()[0] = v.x;
      cold_acc64()[kBlock] = v.y;
      cold_acc64()[2 * kBlock] = v.z;
    } else if constexpr (LC) {
      w(kAcc) = __float_as_uint(v.x);
      w(kAcc + 1) = __float_as_uint(v.y);
      w(kAcc + 2) = __float_as_uint(v.z);
    } else {
      acc_ = v;
    }
  }
#define RT_COLD_U32(name, K)                                                        \
  __device__ __forceinline__ uint32_t name() const {                                \
    if constexpr (LC) return w(K); else return name##_;                             \
  }                                                                                 \
  __device__ __forceinline__ void set_##name(uint32_t v) {                          \
    if constexpr (LC) w(K) = v; else name##_ = v;                                   \
  }
  RT_COLD_U32(ka, kKa)
  RT_COLD_U32(item, kItem)
  RT_COLD_U32(sample, kSample)
  RT_COLD_U32(send, kSend)
  RT_COLD_U32(xy, kXy)
#undef RT_COLD_U32
  __device__ __forceinline__ V<double> cb() const {
    if constexpr (LC) return mkv(cold_doubles()[0], cold_doubles()[kBlock], cold_doubles()[2 * kBlock]);
    else return cb_;
  }
  __device__ __forceinline__ void set_cb(V<double> v) {
    if constexpr (LC) {
      cold_doubles()[0] = v.x;
      cold_doubles()[kBlock] = v.y;
      cold_doubles()[2 * kBlock] = v.z;
    } else {
      cb_ = v;
    }
  }
};
static_assert(Path<float>::kXy < kColdWords, "cold words");

// The pixel's part of the perspective camera ray: the same for every sample of a work item, so it is
// computed once per item (and once per k_step launch), not once per sample. persp_pixel's expression, written
// out so that each field is loaded where it is used (as a call, whose arguments are loaded first, the k_step
// kernels' schedule moves).
template <class R, class PS>
__device__ __forceinline__ void pixel_base(const Params<R>& p, PS& s, uint32_t xy) {
  if constexpr (!PS::kLean) {
    const double x = double(xy & 0xFFFFu), y = double(xy >> 16);
    s.set_cb((ld_here(&p.camx->dir00) + x * ld_here(&p.camx->du)) + y * ld_here(&p.camx->dv));
  }
}

template <class R>
__device__ __forceinline__ void load_path(const Params<R>& p, uint32_t slot, R4<R> Dv, Path<R>& s) {
  R4<R> Ov = p.O[slot], Tv = p.T[slot], Lv = p.L[slot], Av = p.A[slot];
  uint4 S = p.S[slot];
  uint4 X = p.X[slot];
  s.o = mkv(Ov.x, Ov.y, Ov.z);
  s.tm = Ov.w;
  s.d = mkv(Dv.x, Dv.y, Dv.z);
  s.bounce = (int32_t)Dv.w;
  s.set_thr(mkv(Tv.x, Tv.y, Tv.z));
  s.rad = mkv(Lv.x, Lv.y, Lv.z);
  s.set_acc(mkv(Av.x, Av.y, Av.z));
  s.set_ka(S.x);
  s.ks = S.y;
  s.set_item(S.z);
  s.set_sample(S.w);
  s.xe = X.x;
  s.xi = (int32_t)X.y;
  s.set_xy(X.z);
  s.set_send(X.w);
  pixel_base(p, s, X.z);
}

template <class R>
__device__ __forceinline__ void store_path(const Params<R>& p, uint32_t slot, const Path<R>& s) {
  p.D[slot] = {s.d.x, s.d.y, s.d.z, R(s.bounce)};
  if (s.bounce < 0) return;
  p.O[slot] = {s.o.x, s.o.y, s.o.z, s.tm};
  const V<R> thr = s.thr();
  p.T[slot] = {thr.x, thr.y, thr.z, R(0)};
  p.L[slot] = {s.rad.x, s.rad.y, s.rad.z, R(0)};
  const V<R> acc = s.acc();
  p.A[slot] = {acc.x, acc.y, acc.z, R(0)};
  p.S[slot] = make_uint4(s.ka(), s.ks, s.item(), s.sample());
  p.X[slot] = make_uint4(s.xe, (uint32_t)s.xi, s.xy(), s.send());
}

// The wave's local queue [next, end) of the dynamic schedule, in LDS (two words per wave).
__device__ __forceinline__ uint32_t* wave_queue() {
  __shared__ uint32_t wq[2 * (kBlock / 64)];
  return wq + 2 * (threadIdx.x >> 6);
}

// A batch of kQBatch items for the calling lane's wave: the block's own head first (blocks b and
// b + 8 share an XCD, so a head's counter stays in one XCD's traffic), then the others. Returns the
// first item, or kNoItem once every head has run past the item space.
// (Round 6 measured two ways of shortening the frame's end at one rank of eight, C2 fp64: the last 1-4 x the
// grid's lanes of items handed out in batches of 8 instead of 64 -- 0.856 / 0.855 / 0.854 / 0.856 of linear
// at 8 emulated ranks for 0 / 1 / 2 / 4 x; batches of 1, 0.699 -- and a third item tier, the last 1/64 - 1/16 of
// every pixel's samples in items of 1-4, 0.858 - 0.868 against 0.860 - 0.862, within the spread, and +8 B of
// spill in the C5 fp32 kernel (r06a, r06b; profiles/r06b_ab_summary.txt). Neither is kept.)
__device__ __forceinline__ uint32_t grab_batch(uint32_t* heads, uint32_t n_items) {
  const uint32_t g = blockIdx.x & (kHeads - 1);
  for (uint32_t t = 0; t < kHeads; t++) {
    const uint32_t h = (g + t) & (kHeads - 1);
    const uint32_t j = atomicAdd(heads + h * kHeadStride, 1u);
    const uint64_t first = ((uint64_t)j * kHeads + h) * kQBatch;
    if (first < n_items) return (uint32_t)first;
  }
  return kNoItem;
}

// The next item of each calling lane (the lanes of the wave that finished an item in this
// call, in divergent code): consecutive items from the wave's queue, refilled one batch at a
// time by the lowest calling lane. Every value below is identical in the calling lanes.
// kNoItem: the frame is exhausted and the lane retires (queue state [kNoItem, kNoItem)).
// RUNS: the queue hands out the p.n_units units of a kernel that takes runs (begin_item RUNS), not the p.n_items items
template <bool RUNS = false, class R>
__device__ __forceinline__ uint32_t next_item_dyn(const Params<R>& p) {
  uint32_t* wq = wave_queue();
  const uint64_t need = __ballot(1);
  const uint32_t lane = __lane_id();
  const uint32_t k = (uint32_t)__popcll(need);
  const uint32_t r = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
  const uint32_t leader = (uint32_t)__ffsll((unsigned long long)need) - 1;
  uint32_t qn = __hip_atomic_load(wq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  uint32_t qe = __hip_atomic_load(wq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  uint32_t item = kNoItem, off = 0;
  for (;;) {
    const uint32_t rem = qe - qn;
    if (r >= off && r - off < rem) item = qn + (r - off);
    const uint32_t take = min(rem, k - off);
    qn += take;
    off += take;
    if (off >= k || qe == kNoItem) break;  // served, or the wave already found every head dry
    uint32_t b = kNoItem;
    if (lane == leader) b = grab_batch(p.heads, RUNS ? p.n_units : p.n_items);
    b = __shfl(b, (int)leader);
    if (b == kNoItem) {  // remember it: a dry scan stalls the wave for kHeads atomics
      qn = qe = kNoItem;
      break;
    }
    qn = b;
    qe = min(b + kQBatch, RUNS ? p.n_units : p.n_items);
  }
  if (lane == leader) {
    __hip_atomic_store(wq, qn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    __hip_atomic_store(wq + 1, qe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  return item;
}

// An item's first sample and the end of its sample range: bulk items of p.chunk samples, then tail
// items of p.tail_chunk (the item layout, rt_plan.h). `lchunk`: the item's chunk within this pass (item =
// lchunk * npix + the pixel's index); the layout is decided by the frame's chunk, lchunk + chunk0.
template <class R>
__device__ __forceinline__ void chunk_range(const Params<R>& p, uint32_t lchunk, uint32_t& first, uint32_t& end) {
  const uint32_t chunk = lchunk + p.chunk0;
  // fp64 items are uniform (the host never gives them a tail): compiled out, the select costs
  // the fp64 Cornell kernel 10 VGPRs, 3 -> 2 waves per SIMD (C2 f64 5.22 -> 4.08 Gsamples/s)
  const bool bulk = chunk < p.k_bulk;
  first = bulk ? chunk * p.chunk : p.k_bulk * p.chunk + (chunk - p.k_bulk) * p.tail_chunk;
  end = min(first + (bulk ? p.chunk : p.tail_chunk), p.spp);
}
template <class R>
__device__ __forceinline__ void item_range(const Params<R>& p, uint32_t item, uint32_t& lchunk, uint32_t& first,
                                           uint32_t& end) {
  lchunk = (uint32_t)(((uint64_t)item * p.npix_m) >> p.npix_k);
  chunk_range(p, lchunk, first, end);
}
// the pixel's RNG key and the end of the item's samples: kept, or (LEAN) recomputed
// RAYS (here, begin_item, begin_sample): the kernel's paths start on the rays of a batch (rt_radiance), not on a
// camera's. The path state's pixel word (xy) is then the ray's index in the batch, and its key pixel is that index
// above p.ray_base.
template <bool RAYS = false, class R, class PS>
__device__ __forceinline__ uint32_t ka_of(const Params<R>& p, const PS& s) {
  if constexpr (PS::kLean && RAYS) {
    return key_pixel(p.seed, p.ray_base + s.xy());
  } else if constexpr (PS::kLean) {
    const uint32_t xy = s.xy();
    return key_pixel(p.seed, (xy >> 16) * p.W + (xy & 0xFFFFu));
  } else {
    return s.ka();
  }
}
template <class R, class PS>
__device__ __forceinline__ uint32_t send_of(const Params<R>& p, const PS& s) {
  if constexpr (PS::kLean) {
    uint32_t chunk, first, end;
    item_range(p, s.item(), chunk, first, end);
    return end;
  } else {
    return s.send();
  }
}

// A new work item for the slot: its pixel and that pixel's RNG key.
#ifdef RT_ITEM_CLOCKS
// development build (scripts/dev_item_clocks.py): each item's duration in wall-clock ticks (100 MHz), by item
__device__ uint32_t* g_item_clk;
#endif
// RUNS: `item` is a unit of the wave queue (rt_plan.h RunPlan): the slot takes the unit's first item, and shade
// walks the rest of a run.
template <bool RAYS = false, bool RUNS = false, class R, class PS>
__device__ __forceinline__ void begin_item(const Params<R>& p, PS& s, uint32_t item) {
#ifdef RT_ITEM_CLOCKS
  s.t0_ = wall_clock64();
#endif
  uint32_t lchunk, first, end;
  if constexpr (RUNS) {
    const uint32_t q = (uint32_t)(((uint64_t)item * p.npix_m) >> p.npix_k);
    const uint32_t runs = run_cfg_runs(p.run_cfg), lg = run_cfg_log2(p.run_cfg);
    lchunk = unit_first_chunk(q, runs, lg);
    item = unit_first_item(item, q * p.npix, p.npix, runs, lg);
    chunk_range(p, lchunk, first, end);
  } else {
    item_range(p, item, lchunk, first, end);
  }
  // a batch's "pixel" is the ray's index itself: no pixel map, and no per-item camera base below
  uint32_t xy = item - lchunk * p.npix;
  if constexpr (!RAYS) xy = p.pixmap[xy];
  s.set_item(item);
  s.set_sample(first);
  s.set_xy(xy);
  if constexpr (!PS::kLean) {
    s.set_send(end);
    s.set_ka(key_pixel(p.seed, RAYS ? p.ray_base + xy : (xy >> 16) * p.W + (xy & 0xFFFFu)));
  }
  if constexpr (!RAYS) pixel_base(p, s, xy);
}

// camera::generate_ray for the orthonormal, fisheye and lens models (camera.h:252-290), reading
// its fields from device memory. Only the CAMX kernel instantiations contain it, so the
// perspective kernels' registers are not shaped by it.
RT_EXT_FN void camera_ray(const CamDev* cp, uint32_t ks, uint32_t x, uint32_t y, double ox,
                                        double oy, V<double>& o, V<double>& d, double& tm) {
  const int32_t mode = ld_uniform(&cp->mode, 0);
  const V<double> du = ld_uniform(&cp->du, 0), dv = ld_uniform(&cp->dv, 0);
  o = ld_uniform(&cp->pos, 0);
  if (mode == RT_CAM_ORTHONORMAL) {  // camera.h:252-258
    const V<double> q = (ld_uniform(&cp->pos00, 0) + double(x) * du) + double(y) * dv;
    o = (q + ox * du) + oy * dv;
    d = ld_uniform(&cp->dir, 0);
    tm = to_unit<double>(draw_u32(ks, 2));
  } else if (mode == RT_CAM_LENS) {  // camera.h:276-283, 287-290
    d = ((((ld_uniform(&cp->pos00, 0) + double(x) * du) + double(y) * dv) + ox * du) + oy * dv) +
        ld_uniform(&cp->fdir, 0);
    double px = 0, py = 0;
    for (uint32_t k = 0; k < kDiskTries; k++) {
      const double ax = -1 + 2 * to_unit<double>(draw_u32(ks, kDimDisk + 2 * k));
      const double ay = -1 + 2 * to_unit<double>(draw_u32(ks, kDimDisk + 2 * k + 1));
      if (ax * ax + ay * ay + 0.0 * 0.0 < 1) {
        px = ax;
        py = ay;
        break;
      }
    }
    o = o + (px * ld_uniform(&cp->disk_u, 0) + py * ld_uniform(&cp->disk_v, 0));
    d = d - o;
    tm = 0;  // ray(origin, direction): time 0, no draw
  } else {  // fisheye (camera.h:259-275)
    const V<double> dir = ld_uniform(&cp->dir, 0);
    d = persp_sample(persp_pixel(ld_uniform(&cp->dir00, 0), du, dv, x, y), du, dv, ox, oy);
    const V<double> w = d - dir;
    const double r = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    const double theta = asin(r / ld_uniform(&cp->focal, 0));
    const V<double> v1 = unit(dir), v2 = unit(d);
    const double st = sin(theta);
    const double b = sqrt(st * st / (1 - dot(v1, v2) * dot(v1, v2)));
    const double a = cos(theta) - b * dot(v1, v2);
    d = a * v1 + b * v2;
    tm = to_unit<double>(draw_u32(ks, 2));
  }
}

// The first ray of a sample of a ray batch (RAYS): ray s.xy() of p.rays, 64 bytes as load_query reads them, o, d and the
// time in fp64, rounded to R below as a camera ray is. The path's key is a camera sample's, (seed, pixel, sample), and
// its draws keep their dimensions: 0 and 1, the pixel jitter, are never drawn; 2, the ray time, is drawn as
// camera::generate_ray draws it only where the stored time is NaN. tmax is not read: the first segment runs over
// interval(0.001, inf) like every other (camera.h:198).
template <class R, class PS>
__device__ __forceinline__ void batch_ray(const Params<R>& p, const PS& s, V<double>& o, V<double>& d, double& tm) {
  const double2* q = (const double2*)(p.rays + 8ull * s.xy());  // 16-byte aligned (rt_radiance checks)
  const double2 r0 = q[0], r1 = q[1], r2 = q[2];
  o = mkv(r0.x, r0.y, r1.x);
  d = mkv(r1.y, r2.x, r2.y);
  tm = q[3].x;
  if (tm != tm) tm = to_unit<double>(draw_u32(s.ks, 2));
}

// camera::generate_ray, perspective mode (camera.h:244-251,293): sample s.sample of the slot's pixel
template <class R, bool CAMX, class PS>
__device__ __forceinline__ void pixel_ray(const Params<R>& p, const PS& s, V<double>& o, V<double>& d, double& tm) {
  // In fp64 for both paths: fp32 gets the correctly rounded ray, a few ulp less error on every
  // camera ray, which otherwise shows up as paths crossing a checker line or edge differently.
  const double ox = to_unit<double>(draw_u32(s.ks, 0)) - 0.5;  // sample_square (camera.h:293)
  const double oy = to_unit<double>(draw_u32(s.ks, 1)) - 0.5;
  o = ld_here(&p.camx->pos);
  if (!CAMX || p.cam_mode == RT_CAM_PERSPECTIVE) {  // camera.h:245-251
    const V<double> du = ld_here(&p.camx->du), dv = ld_here(&p.camx->dv);
    if constexpr (!PS::kLean) {
      d = persp_sample(s.cb(), du, dv, ox, oy);
    } else {  // no kept pixel base: pixel_base's value, recomputed
      const uint32_t xy = s.xy(), x = xy & 0xFFFFu, y = xy >> 16;
      d = persp_sample(persp_pixel(ld_here(&p.camx->dir00), du, dv, x, y), du, dv, ox, oy);
    }
    tm = to_unit<double>(draw_u32(s.ks, 2));
  } else if constexpr (CAMX) {
    const uint32_t xy = s.xy();
    camera_ray(p.camx, s.ks, xy & 0xFFFFu, xy >> 16, ox, oy, o, d, tm);
  }
}
// A new sample for the slot: its key and its first ray, the camera's or (RAYS; CAMX is then the scene's textures
// alone) the batch's
template <class R, bool CAMX, bool RAYS = false, class PS>
__device__ __forceinline__ void begin_sample(const Params<R>& p, PS& s) {
  s.ks = key_path(ka_of<RAYS>(p, s), key_sample(p.seed, p.first_sample + s.sample()));
  V<double> o, d;
  double tm;
  if constexpr (RAYS)
    batch_ray(p, s, o, d, tm);
  else
    pixel_ray<R, CAMX>(p, s, o, d, tm);
  s.o = mkv(R(o.x), R(o.y), R(o.z));
  s.d = mkv(R(d.x), R(d.y), R(d.z));
  s.tm = R(tm);
  s.bounce = 0;
  s.set_thr(mkv(R(1), R(1), R(1)));
  if constexpr (!PS::kNoRad) s.rad = mkv(R(0), R(0), R(0));
  s.xe = kNoHit;
  s.xi = -1;
}


template <class R, bool CAMX>
__global__ __launch_bounds__(kBlock) void k_init(Params<R> p) {
  uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
  if (slot >= p.P) return;
  Path<R> s;
  s.set_acc(mkv(R(0), R(0), R(0)));
  if (slot >= p.n_items) {
    s.d = mkv(R(0), R(0), R(0));
    s.bounce = -1;
  } else {
    begin_item(p, s, slot);
    begin_sample<R, CAMX>(p, s);
  }
  store_path(p, slot, s);
}

// camera::ray_color for one segment (camera.h:193-241), iteratively: given the
// closest hit (t, e, inst) of s's ray, add emission, scatter (or finish the
// sample and regenerate the slot's next camera ray). Returns false once the slot
// has no work left.
// FLAT: the hit comes from the flat program (trace_flat): a quad whose outward normal (+-e_A)
// and material are packed in nm, so no primitive or instance record is read.
// MOVING = false: the kernel's scene has no moving sphere (the wide kernels without WK_MOVING), so the
// ray time is not read here. A LEAN path has no radiance register: emission goes straight into the
// item's running sum (the same terms, added one by one instead of per sample: a rounding-level
// regrouping of the pixel's sum).
// MLDS: `mats` is the kernel's LDS copy of the materials (FlatTrav tables), read with ds_read (a generic
// pointer that may be LDS or global compiled to flat loads, which wait on both counters).
// LL ("lambertian + light", round 5): the scene's materials are lambertian and diffuse_light with solid
// textures (the background's too), and the light an axis-aligned quad (the Cornell configs; host-checked,
// launch_step): the material is one LDS record lm[mat] = (colour, is_light), and the texture, metal,
// dielectric, gloss, isotropic and no-light code is compiled out.
// NL ("no light", round 5): the materials are lambertian, metal and dielectric (solid and checker textures)
// and there is no importance-sampling light (RTOW, C3; host-checked): the emission, gloss, isotropic and
// light-mixture code is compiled out.
// LLI (with LL): isotropic phase materials too (the lm record's w is 2; C5's smoke volumes)
// What shade compiles in comes as one configuration type. ShadeOf<Trav>: the form a traversal policy's persistent
// kernel takes; ShadeGeneral: every material and light, materials from global memory (k_step, whose register
// budget the special forms' LDS tables would squeeze).
template <class Trav>
struct ShadeOf {
  static constexpr bool kFlat = Trav::kFlat, kMoving = Trav::kMoving, kLL = Trav::kLL, kNL = Trav::kNL,
                        kLLI = Trav::kLLI;
  static constexpr bool kMatsLds = Trav::kTablesLds || Trav::kLL;
  static constexpr bool kRays = Trav::kRays;  // the next sample starts on a ray of the batch (begin_sample RAYS)
  static constexpr bool kRuns = Trav::kItemRuns && !Trav::kRays;  // the queue hands out runs of items (RunPlan)
};
template <bool FLAT>
struct ShadeGeneral {
  static constexpr bool kFlat = FLAT, kMoving = true, kLL = false, kNL = false, kLLI = false, kMatsLds = false;
  static constexpr bool kRays = false, kRuns = false;
};
template <class R, bool CAMX, class Cfg, class PS>
__device__ bool shade(const Params<R>& p, PS& s, R t, uint32_t e, int32_t inst, uint32_t nm = 0,
                      const Material<R>* mats = nullptr, const R4<R>* lm = nullptr) {
  constexpr bool FLAT = Cfg::kFlat, MOVING = Cfg::kMoving, MLDS = Cfg::kMatsLds, LL = Cfg::kLL, NL = Cfg::kNL,
                 LLI = Cfg::kLLI;
  const DevScene<R>& sc = p.sc;
  // the light / material halves of the mixture pdf (pdf.h:52-56) as one select path, in the flat program (C2 fp64
  // 28.33 -> 28.15 ms/frame, fp32 18.83 -> 18.49, r05e); in every kernel it lost on C5 (fp64 2,226 ms, r06c)
  constexpr bool kMixSel = FLAT;
  V<R> add = mkv(R(0), R(0), R(0));
  bool has_add = false, done = false;
  V<R> new_o = s.o, new_d = s.d;
  const V<R> o = s.o, d = s.d;
  // The fp64 flat LL kernel (round 7) updates the path state in place: the scatter writes the next ray into s and
  // returns from there, and every other lane -- its sample is finished -- goes on to begin_sample, which writes the
  // whole state. No lane then leaves shade with the origin, direction and throughput it entered with, and the
  // compiler keeps fewer copies of them: through new_o / new_d and the common `!done` exit below, every join of the
  // segment loop copied the nine values from one set of registers to another (C2 fp64 25.29 -> 24.49 ms/frame; the
  // fp32 twin lost, 18.34 -> 18.57, and keeps the code it had, as every other kernel).
  constexpr bool kInPlace = FLAT && LL && sizeof(R) == 8;

  if (e == kNoHit) {  // camera::miss (camera.h:180-190)
#ifdef RT_DEBUG_TRACE
    printf("[dev] bounce %d o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g) miss\n", s.bounce, (double)o.x, (double)o.y,
           (double)o.z, (double)d.x, (double)d.y, (double)d.z);
#endif
    // a solid black background (the Cornell configs' solid_color::black) adds thr * 0: the unit-sphere test
    // that decides whether it is sampled (camera.h:183-187) is skipped (a wave-uniform test of the record)
    const Texture<R>* bgt = sc.background >= 0 ? sc.texs + sc.background : nullptr;
    const bool bg_black = bgt != nullptr && ld_here(&bgt->kind) == T_SOLID &&
                          ld_here(&bgt->c0[0]) == R(0) && ld_here(&bgt->c0[1]) == R(0) && ld_here(&bgt->c0[2]) == R(0);
    // any other solid background: the unit sphere about the ray's origin has the root t = 1/|d|, inside
    // [0.001, inf) for |d| < 1000, and a solid colour does not depend on where it is hit -- so for |d| < 500
    // the colour is added without the test (RT_BG_SOLID_FAST; RTOW's sky, C3)
    // (0 < |d|^2: a zero direction has a = 0 in sphere.h:48-62, a NaN root and no hit -- nothing is added)
    const R dd2 = dot(d, d);
    const bool bg_solid = bgt != nullptr && !bg_black && ld_here(&bgt->kind) == T_SOLID &&
                          dd2 < R(250000) && dd2 > R(0);
    if (bg_solid) {
      add = s.thr() * mkv(ld_here(&bgt->c0[0]), ld_here(&bgt->c0[1]), ld_here(&bgt->c0[2]));
      has_add = true;
    } else if (sc.background >= 0 && !bg_black) {
      R tb;
      if (sphere_roots<R>(o.x, o.y, o.z, d.x, d.y, d.z, o.x, o.y, o.z, R(1), R(0.001), Num<R>::inf(), false, tb)) {
        double bu = 0, bv = 0;
        if constexpr (CAMX) sphere_uv(tb * d, bu, bv);  // the unit sphere about the origin (camera.h:184-187)
        add = s.thr() * tex_sample<R, CAMX>(sc, sc.texs[sc.background], o + tb * d, bu, bv);
        has_add = true;
      }
    }
    done = true;
  } else {
    uint32_t ty = etype(e), idx = epay(e);
    V<R> pw, n;
    bool front;
    int32_t mat;
    double hu = 0, hv = 0;  // hit_record u, v (EXT kernels: picture textures); 0 where the reference leaves them stale
    bool unit_n = true;  // false: a moving sphere's normal, (p - 0) / r (sphere.h:69), is not a unit vector
    [[maybe_unused]] uint32_t fA = 0;  // FLAT: n = fs e_fA
    [[maybe_unused]] R fs = R(1);
    if constexpr (FLAT) {  // quad.h:47-50 with n = +-e_A (translate leaves it alone, hittable.h:75-82)
      // outward = sg e_A (sg = -1 when bit 31 is set); hit_record::set_face_normal (hittable.h:26-29):
      // dot(d, outward) < 0 is exactly sg d_A < 0, and n = front ? outward : -outward, whose zero
      // components are -0 on a back face, as the negation gives them
      const uint32_t A = (nm >> 28) & 3u;
      const bool neg = (nm >> 31) != 0;
      const R dA = A == 0 ? d.x : (A == 1 ? d.y : d.z);
      mat = (int32_t)(nm & kNmMat);
      pw = o + t * d;
      front = neg ? dA > R(0) : dA < R(0);
      fA = A;
      fs = front != neg ? R(1) : R(-1);
      const R z = front ? R(0) : -R(0);
      n = mkv(A == 0 ? fs : z, A == 1 ? fs : z, A == 2 ? fs : z);
    } else if (ty == E_VOLUME) {  // volumne.h:40-44
      pw = o + t * d;
      n = mkv(R(1), R(0), R(0));
      front = true;
      mat = sc.vols[idx].phase_mat;
    } else {
      V<R> oo = o, dd = d;
      const Instance<R>* in = nullptr;
      if (inst >= 0) in = &sc.insts[inst];
      // fp32, planar primitives: instances are rigid, so the hit is o + t d in world space and
      // only the object-space normal needs rotating out (fp64 keeps the reference's
      // object-space point, hittable.h:75-82, 125-149)
      const bool world_space = sizeof(R) == 4 && ty != E_SPHERE && !CAMX;
      if (in && !world_space) chain_in(*in, oo, dd);
      V<R> po = oo + t * dd;
      V<R> outward;
      if (ty == E_QUAD) {
        const Quad<R>& q = sc.quads[idx];
        outward = ld3(q.n);
        mat = q.mat;
        if constexpr (CAMX) {  // quad.h:47-62: u, v = alpha, beta
          const V<R> rel = po - ld3(q.q);
          hu = (double)dot(rel, ld3(q.a));
          hv = (double)dot(rel, ld3(q.b));
        }
      } else if (ty == E_SPHERE) {  // sphere.h:69 (center_ member; (0,0,0) for moving spheres)
        const Sphere<R>& sp = sc.spheres[idx];
        unit_n = !MOVING || !sp.moving;
        if constexpr (sizeof(R) == 8) {
          outward = (po - ld3(sp.cn)) / sp.r;
        } else {
          // The hit refined in fp64 from the fp32 ray: one Newton step on the quadratic
          // g(t) = a t^2 + 2 b t + c from the fp32 root (which is ~1e-7 relative off: ~1e-6 along
          // the ray for t ~ 10, tilting a small sphere's normal by ~1e-5 -- enough for a chain of
          // mirror / glass bounces to leave the fp64 path a few times per million segments),
          // then the point and normal (sphere.h:67-69) from the refined root. A step that does
          // not land near the fp32 root (a grazing double root) keeps it.
          double cx = sp.c1[0], cy = sp.c1[1], cz = sp.c1[2];  // sphere.h:83 (a static sphere: dc = 0)
          if (!unit_n) {
            cx += (double)s.tm * sp.dc[0];
            cy += (double)s.tm * sp.dc[1];
            cz += (double)s.tm * sp.dc[2];
          }
          // g(t0) = |o + t0 d - c|^2 - r^2 needs fp64 (it cancels); the step g / g' is tiny next
          // to t0, so g' = 2 d.(o + t0 d - c) and the quotient are fp32
          const double ox = oo.x, oy = oo.y, oz = oo.z, dx = dd.x, dy = dd.y, dz = dd.z, t0 = t, rr = sp.r;
          const double qx = (ox + t0 * dx) - cx, qy = (oy + t0 * dy) - cy, qz = (oz + t0 * dz) - cz;
          const double g = (qx * qx + qy * qy + qz * qz) - rr * rr;
          const float gp = 2.0f * ((float)qx * dd.x + (float)qy * dd.y + (float)qz * dd.z);
          float step = fdiv((float)g, gp);
          if (!(fabsf(step) <= 1e-4f * fabsf(t))) step = 0.0f;
          const double td = t0 - (double)step;
          const double px = ox + td * dx, py = oy + td * dy, pz = oz + td * dz;
          po = mkv((float)px, (float)py, (float)pz);
          outward = mkv((float)(px - sp.cn[0]), (float)(py - sp.cn[1]), (float)(pz - sp.cn[2])) * fdiv(R(1), sp.r);
          // big spheres (the RTOW ground, r = 1000) in particular: o + t*d in fp32 is off the surface
          // by ~1e-7 absolute, enough to flip the sign of y near the top of the ground (y = 0 under the
          // glass sphere) and with it the checker parity (texture.h:51-55)
        }
        mat = sp.mat;
        if constexpr (CAMX) sphere_uv(outward, hu, hv);  // sphere.h:70
      } else {
        const Tri<R>& tr = sc.tris[idx];
        outward = ld3(tr.n);
        mat = tr.mat;
      }
      if (world_space) {
        if (in)
          for (int q = in->nops - 1; q >= 0; q--) outward = op_out(in->op[q], outward, false);
        front = dot(dd, outward) < R(0);  // hit_record::set_face_normal (hittable.h:26-29)
        n = front ? outward : -outward;
        pw = po;
      } else {
        front = dot(dd, outward) < R(0);  // hit_record::set_face_normal (hittable.h:26-29)
        n = front ? outward : -outward;
        pw = po;
        if (in) {
          for (int q = in->nops - 1; q >= 0; q--) {
            pw = op_out(in->op[q], pw, true);
            n = op_out(in->op[q], n, false);
          }
        }
      }
    }
#ifdef RT_DEBUG_TRACE  // development build (scripts/dev_sample_trace.py): one line per segment
    printf("[dev] bounce %d o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g) t=%.9g p=(%.9g %.9g %.9g) n=(%.9g %.9g %.9g) "
           "front=%d mat=%d ty=%u idx=%u\n", s.bounce, (double)o.x, (double)o.y, (double)o.z, (double)d.x, (double)d.y,
           (double)d.z, (double)t, (double)pw.x, (double)pw.y, (double)pw.z, (double)n.x, (double)n.y, (double)n.z,
           (int)front, sc.mats[mat].kind, ty, idx);
#endif
    using LMat = const __attribute__((address_space(3))) Material<R>;
    using LRec = const __attribute__((address_space(3))) R4<R>;
    const Material<R>& m = MLDS ? *(const Material<R>*)((LMat*)mats + mat) : sc.mats[mat];
    V<R> col{};
    bool is_light;
    [[maybe_unused]] bool ll_iso = false;
    if constexpr (LL) {
      LRec* mc = (LRec*)lm + mat;
      col = mkv(mc->x, mc->y, mc->z);
      const R w = mc->w;
      is_light = w == R(1);
      if constexpr (LLI) ll_iso = w == R(2);
    } else {
      is_light = !NL && m.kind == M_DIFFUSE_LIGHT;
    }
    if (is_light) {  // material.h:211-215; no scatter
      if (front) {
        add = s.thr() * (LL ? col : tex_sample<R, CAMX>(sc, m.tx, pw, hu, hv));
        has_add = true;
      }
      done = true;
    } else {
      V<R> att = LL ? col : tex_sample<R, CAMX>(sc, m.tx, pw, hu, hv);
      const uint32_t bounce = (uint32_t)s.bounce;
      uint32_t js = 0;
      auto U = [&]() { return to_unit<R>(draw_u32(s.ks, dim_scatter(bounce, js++))); };
      // NL (lambertian / metal / dielectric, no light): the scatter draws are pure functions of (path key,
      // dimension), and lambertian's cosine sample and metal's fuzz sample each need sin/cos(2 pi u) of one of the
      // first two draws -- so both draws and one sincos are computed by every lane before the material branches,
      // which then hold no trigonometry (the same operations on the same values: bit-identical)
      [[maybe_unused]] R nl_u1 = R(0), nl_u2 = R(0), nl_sp = R(0), nl_cp = R(0);
      constexpr bool kNlTrig = NL;  // C3 fp32 48.16 -> 47.60 ms/frame, fp64 64.70 -> 64.09 (r06b)
      if constexpr (kNlTrig) {
        nl_u1 = to_unit<R>(draw_u32(s.ks, dim_scatter(bounce, 0)));
        nl_u2 = to_unit<R>(draw_u32(s.ks, dim_scatter(bounce, 1)));
        sincos2pi(m.kind == M_METAL ? nl_u2 : nl_u1, nl_sp, nl_cp);  // on_sphere: phi = 2 pi u2; cosine: 2 pi u1
      }
      if (!LL && m.kind == M_METAL) {  // material.h:85-92
        V<R> dir = unit(reflect(d, n));
        if constexpr (kNlTrig) {
          new_d = dir + m.fuzz * unit(on_sphere_sc(nl_u1, nl_sp, nl_cp));
        } else {
          R u1 = U();
          R u2 = U();
          new_d = dir + m.fuzz * unit(on_sphere(u1, u2));
        }
        s.set_thr(s.thr() * att);
      } else if (!LL && m.kind == M_DIELECTRIC) {  // material.h:113-131
        R ri = front ? fdiv(R(1), m.refr) : m.refr;
        V<R> ud = unit(d);
        R cos_t = fmin(dot(-ud, n), R(1));
        R sin_t = fsqrt(R(1) - cos_t * cos_t);
        bool cant = ri * sin_t > R(1);
        R r0 = fdiv(R(1) - ri, R(1) + ri);
        r0 = r0 * r0;
        if (cant || (r0 + (R(1) - r0) * pow5(R(1) - cos_t)) > (kNlTrig ? nl_u1 : U()))
          new_d = reflect(ud, n);
        else
          new_d = refract(ud, n, ri);
        s.set_thr(s.thr() * att);
      } else if (!LL && !NL && m.kind == M_GLOSS && to_unit<R>(draw_u32(s.ks, dim_scatter(bounce, js))) <= m.spec) {
        // gloss, specular branch (material.h:158-167): kDetermined, attenuation 1,
        // direction unit(lerp(smoothness, cosine-hemisphere sample about n, reflect(d_in, n)))
        js++;
        const Onb<R> b = FLAT ? make_onb_axis(n) : make_onb(n);
        const R r1 = U();
        const R r2 = U();
        const V<R> diffuse = onb_transform(b, cosine_dir(r1, r2));
        const R tt = m.smooth;
        new_d = unit((R(1) - tt) * diffuse + tt * reflect(d, n));
      } else {  // lambertian (material.h:62-72) / isotropic (material.h:193-200) / gloss diffuse: kRandom
        if (!LL && !NL && m.kind == M_GLOSS) js++;  // the specular-choice draw above (material.h:161)
        const bool iso = LL ? (LLI && ll_iso) : (!NL && m.kind == M_ISOTROPIC);
        const R iso_pdf = R(1) / (R(4) * Num<R>::pi());
        Onb<R> b;
        if (!FLAT && !iso) b = make_onb(n);
        // FLAT: n = fs e_A, so make_onb_axis(n) is a signed permutation (b.y = n; A = 0: b.x = -e_z,
        // b.z = -fs e_y; A = 1, 2: b.x = -e_x, b.z = -fs e_z / fs e_y) and onb_transform(b, v) is
        // exact: (fs v.y, -fs v.z, -v.x), (-v.x, fs v.y, -fs v.z), (-v.x, fs v.z, fs v.y) -- the same
        // values without the cross products and the nine multiply-adds (signed zeros aside, which no
        // later test can tell apart); dot(u, n) is fs u_A
        auto cos_dir = [&](R u1, R u2) -> V<R> {
          // (the flat LL kernels: u2 is a draw, so sqrt(1 - u2) needs no zero check; fp64: fs v as a sign flip. Both
          // leave every bit as it was; the other kernels that shade with this code keep theirs)
          const V<R> v = cosine_dir<R, FLAT && LL>(u1, u2);
          if constexpr (FLAT && LL && sizeof(R) == 8) {
            const R sy = flip_sign(v.y, fs < R(0)), sz = flip_sign(v.z, fs < R(0));
            return fA == 0 ? mkv(sy, -sz, -v.x) : (fA == 1 ? mkv(-v.x, sy, -sz) : mkv(-v.x, sz, sy));
          } else if constexpr (FLAT) {
            const R sy = fs * v.y, sz = fs * v.z;
            return fA == 0 ? mkv(sy, -sz, -v.x) : (fA == 1 ? mkv(-v.x, sy, -sz) : mkv(-v.x, sz, sy));
          } else {
            return onb_transform(b, v);
          }
        };
        auto cos_n = [&](V<R> u) -> R {  // dot(u, n) (onb.h's w = n)
          if constexpr (FLAT) return fs * (fA == 0 ? u.x : (fA == 1 ? u.y : u.z));
          return dot(u, b.y);
        };
        const Light<R>* Lt = sc.light;  // read at the point of use (light_pdf, light_random)
        R pv = R(1);
        V<R> dir;
        // no light (camera.h:217-226): the direction is drawn from the material's own pdf, the one
        // p_scattered returns (cosine for lambertian, material.h:62-80; uniform for isotropic,
        // material.h:193-205), so (attenuation * p_scattered) / pdf_value is the attenuation: the two
        // pdfs (equal up to rounding) are not evaluated (C3 fp32 52.49 -> 52.17 ms/frame, fp64 75.8 ->
        // 73.0). Not for a moving sphere: p_scattered takes the cosine against its non-unit normal,
        // the pdf against the unit one, and the ratio |n| is the reference's (quirk kept)
        bool own_pdf = false;
        if (NL || (!LL && ld_here(&Lt->kind) == L_NONE)) {
          if constexpr (kNlTrig) {  // NL has no isotropic material
            dir = onb_transform(b, cosine_dir_sc(nl_u2, nl_sp, nl_cp));
          } else {
            R u1 = U();
            R u2 = U();
            dir = iso ? unit(on_sphere(u1, u2)) : cos_dir(u1, u2);
          }
          own_pdf = iso || unit_n;
          if (!own_pdf) pv = fmax(R(0), div_pi(cos_n(unit(dir))));
        } else {  // dual_pdf(hittable_pdf(light), material pdf) (camera.h:227-239, pdf.h:48-61)
          R c = U();
          R u1 = U();
          R u2 = U();
          const bool from_light = c < R(0.5);
          if constexpr (kMixSel) {  // both generators for every lane, one select (no divergent branch)
            const V<R> dl = light_random(Lt, pw, u1, u2);
            const V<R> dc = iso ? unit(on_sphere(u1, u2)) : cos_dir(u1, u2);
            dir = from_light ? dl : dc;
          } else if (from_light) {
            dir = light_random(Lt, pw, u1, u2);
          } else if constexpr (LLI) {  // (C5 fp64 2,200 -> 2,185 ms/frame, fp32 1,094 -> 1,091, r06c)
            // the isotropic (on_sphere: phi = 2 pi u2) and lambertian (cosine: phi = 2 pi u1) lanes share one sincos
            R sp, cp;
            sincos2pi(iso ? u2 : u1, sp, cp);
            dir = iso ? unit(on_sphere_sc(u1, sp, cp)) : onb_transform(b, cosine_dir_sc(u2, sp, cp));
          } else {
            dir = iso ? unit(on_sphere(u1, u2)) : cos_dir(u1, u2);
          }
          R mp = iso ? iso_pdf : fmax(R(0), div_pi(cos_n(unit(dir))));
          pv = R(0.5) * light_pdf<R, kMixSel>(Lt, pw, dir, from_light) + R(0.5) * mp;
        }
        if (own_pdf) {
          s.set_thr(s.thr() * att);
        } else {
          R ps;
          if (iso) {
            ps = iso_pdf;
          } else {
            R c = FLAT ? cos_n(unit(dir)) : dot(n, unit(dir));
            ps = c < R(0) ? R(0) : div_pi(c);
          }
          if constexpr (sizeof(R) == 8)
            s.set_thr(s.thr() * ((att * ps) / pv));  // camera.h:238 grouping on the parity path
          else  // a zero mixture pdf (the reference's 0/0 = NaN) ends the path
            s.set_thr(pv > R(0) ? s.thr() * (att * fdiv(ps, pv)) : mkv(R(0), R(0), R(0)));
        }
        new_d = dir;
      }
      new_o = pw;
      if (s.bounce + 1 >= p.max_depth) {  // ray_color(.., 0) returns 0 (camera.h:194) ...
        done = true;
        // ... which the caller multiplies by this bounce's weight (camera.h:238): 0, but NaN where the weight is the
        // 0 / 0 of a zero mixture pdf (a base-class light). fp64 keeps the reference's NaN; fp32 ended that path above.
        // Not in the LL and NL forms: their scenes have an axis-aligned quad light or none, where a zero mixture pdf
        // is a measure-zero event, and the three multiplies cost the flat LL kernel 0.5 % (C2 fp64 23.01 -> 23.13
        // ms/frame, four alternating runs each, spread 0.02).
        if constexpr (sizeof(R) == 8 && !LL && !NL) {
          add = s.thr() * R(0);
          has_add = true;
        }
      }
      {
        const V<R> thr = s.thr();
        if (thr.x == R(0) && thr.y == R(0) && thr.z == R(0)) done = true;
      }
      if constexpr (kInPlace) {  // (no emission on this branch: nothing below concerns a lane that goes on)
        s.o = new_o;
        s.d = new_d;
        if (!done) {
          s.bounce += 1;
          s.xe = e;
          s.xi = inst;
          return true;
        }
      }
    }
  }
  if (has_add) {
    if constexpr (PS::kNoRad)
      s.set_acc(s.acc() + add);
    else
      s.rad = s.rad + add;
  }
  if (!kInPlace && !done) {
    s.o = new_o;
    s.d = new_d;
    s.bounce += 1;
    s.xe = e;
    s.xi = inst;
    return true;
  }
  // the sample is finished (camera.h:167): add it to the item's running sum
  RT_WIDE_STAT(8);
  V<R> acc = s.acc();
  if constexpr (!PS::kNoRad) acc = acc + s.rad;
  [[maybe_unused]] bool retire = false;
  const uint32_t sample = s.sample() + 1;
  s.set_sample(sample);
  if (sample < send_of(p, s)) {
    s.set_acc(acc);
  } else {
    const uint32_t item = s.item();
#ifdef RT_ITEM_CLOCKS
    if (g_item_clk) g_item_clk[item] = (uint32_t)(wall_clock64() - s.t0_);
#endif
    R* dst = p.partial + 3ull * item;
    dst[0] = acc.x;
    dst[1] = acc.y;
    dst[2] = acc.z;
    s.set_acc(mkv(R(0), R(0), R(0)));
    // a chunk that is not the last of its run (rt_plan.h RunPlan): the same pixel's next bulk chunk, with the
    // pixel, its key and the camera base as they are -- no dequeue and no begin_item
    bool in_run = false;
    if constexpr (Cfg::kRuns) {
      const uint32_t runs = run_cfg_runs(p.run_cfg), lg = run_cfg_log2(p.run_cfg);
      in_run = run_goes_on(sample, (runs << lg) * p.chunk, (p.chunk << lg) - 1);
    }
    if (in_run) {
      s.set_item(item + p.npix);
      s.set_send(sample + p.chunk);  // (a chunk inside a run is a whole bulk chunk: plan_runs)
    } else {
      // persistent schedule: from the wave's queue; wavefront schedule: the slot's next item, P further on
      const uint32_t nx = p.persist == kPersist ? next_item_dyn<Cfg::kRuns>(p)
                                                : (item + p.P < p.n_items ? item + p.P : kNoItem);  // (never with runs)
      if (nx == kNoItem) {
        if constexpr (kInPlace) {
          retire = true;  // (below)
        } else {
          s.bounce = -1;
          return false;
        }
      } else {
        begin_item<Cfg::kRays, Cfg::kRuns>(p, s, nx);
      }
    }
  }
  // (round 5: regenerating the finished lanes of a wave in batches -- a lane waiting idle until 16 or 32 of
  // its wave's lanes had finished -- was slower, C2 fp64 28.33 -> 28.46 / 29.95 ms/frame, r05e: the lanes a
  // wait idles in trace and shade cost more than the regeneration's 41 % lane use)
  begin_sample<R, CAMX, Cfg::kRays>(p, s);
  // kInPlace: a retiring lane generated a ray too (of its last item: registers only, never traced), so that it also
  // leaves with a state written here
  if constexpr (kInPlace) {
    if (retire) {
      s.bounce = -1;
      return false;
    }
  }
  return true;
}

// ------------------------------------------------------------------ the fused wavefront step
// Each launch advances every live slot by up to K segments: closest hit
// (extend, camera.h:198), then shade. Traversal: the wave-uniform linear
// program (small scenes) or the BVH stack machine with a per-lane LDS stack.
// LLI: a lambertian + isotropic + light scene (shade LL, LLI; C5's Cornell box with smoke volumes)
// What the traversal policies below have in common; each declares only what differs.
struct TravDefaults {
  static constexpr bool kFlat = false;       // the flat program (trace_flat; shade FLAT)
  static constexpr bool kWide = false;       // the wide BVH (resumable traversal: Trav::steps)
  static constexpr bool kTablesLds = false;  // the flat program's records and materials in LDS (Trav::Tables)
  struct Tables {};
  static constexpr int kStack = 0;           // the binary BVH's LDS stack entries per lane
  static constexpr int kLdsNodes = 0;        // the binary BVH's nodes copied into LDS, at most
  static constexpr uint32_t kLdsMats = kLdsMatsLL;  // materials the LL kernels' LDS table holds (rt_plan.h)
  // the scene class shade is compiled for (ShadeOf): lambertian + light, no light, LL + isotropic; moving spheres
  [[maybe_unused]] static constexpr bool kLL = false, kNL = false, kLLI = false, kMoving = true;
  // the path state (Path): lean, no radiance register, cold fields in LDS, throughput in LDS
  [[maybe_unused]] static constexpr bool kLean = false, kNoRad = false, kColdLds = false, kThrLds = false;
  // the segment loop tests the segment cap between trace and shade, as every kernel did before round 9, instead of
  // after shade (persist_body)
  static constexpr bool kCapBeforeShade = false;
  // occlusion queries: the policy also has k_occluded's closest-hit form (EARLY = false), which launch_occluded takes
  // where occlusion_early_exit (rt_plan.h) refuses the any-hit form. A policy without it always takes the any-hit form.
  [[maybe_unused]] static constexpr bool kClosestOccl = false;
  static constexpr bool kRays = false;  // RaysOf: the paths start on the rays of a batch, not on a camera's
  // the persistent kernel's wave queue hands out runs of a pixel's bulk items (rt_plan.h RunPlan, kernel_takes_runs;
  // DESIGN.md §4, round 11), not single items. Opt-in, like kCapBeforeShade: a kernel without it is the code it was
  // (FlatTrav RUNS)
  static constexpr bool kItemRuns = false;
};
// The policy `Trav` for a ray batch (rt_radiance): the same traversal, tables, path state and shade form, in a kernel of
// its own whose begin_item / begin_sample read the batch (RAYS) -- so the camera kernels hold no trace of it.
template <class Trav>
struct RaysOf : Trav {
  static constexpr bool kRays = true;
};
template <class R, bool SPH, bool TRI, bool VOL, bool LLI = false>
struct LinearTrav : TravDefaults {
  static constexpr bool kClosestOccl = true;  // (volumes draw after their interval test: occlusion_early_exit)
  static constexpr bool kLL = LLI, kLLI = LLI;
  // waves per SIMD the register budget is cut for (occupancy hides the shading loads); the
  // lean quad-only program fits 96 VGPRs with a small spill, the others would spill heavily
  static constexpr int kWaves = sizeof(R) != 4 ? (VOL ? RT_LINEAR_VOL_WAVES_F64 : RT_LINEAR_WAVES_F64)
                                 : (!SPH && !TRI && !VOL) ? RT_LINEAR_WAVES
                                 : (!SPH && !TRI && VOL)  ? (LLI ? RT_LINEAR_VOL_WAVES_LLI : RT_LINEAR_VOL_WAVES)
                                                          : 1;
  // the volume program's registers (C5: 23 -> 6 VGPRs spilled at 96, 1563 -> 1498 ms/frame); not lean (LLI lean: 7
  // waves 1,094 -> 1,117 ms/frame; 8 waves 48 B spilled, r06a)
  static constexpr bool kNoRad = VOL;
  static constexpr bool kColdLds = VOL;
  static constexpr bool kThrLds = VOL && LLI && sizeof(R) == 4;  // (Path LT: C5 fp32 1,091 -> 1,072 ms/frame, r06d)
  // the fp32 LLI kernel keeps the cap test where it was: with it after shade the kernel spilled 24 B in place of 16
  // and C5 fp32 went 1,071 -> 1,078 ms/frame (round 9)
  static constexpr bool kCapBeforeShade = VOL && LLI && sizeof(R) == 4;
  // ANY (here and in the other policies): the any-hit form of the traversal, rt_occluded's (rt_device.h)
  template <bool ANY = false, class PS>
  __device__ __forceinline__ static void run(const DevScene<R>& sc, const Node<R>*, const PS& s, Keys k,
                                             uint32_t*, R& t, uint32_t& e, int32_t& i, uint32_t&) {
    trace_linear<R, SPH, TRI, VOL, ANY>(sc, s.o, s.d, s.tm, s.xe, s.xi, k, (uint32_t)s.bounce, t, e, i);
  }
};
// The flat program (quad/box scenes such as every Cornell config): rt_device.h trace_flat.
#ifndef RT_FLAT_WAVES
#define RT_FLAT_WAVES 8
#endif
#ifndef RT_FLAT_WAVES_F64  // fp64 flat program: waves per SIMD the register budget is cut for (1: none)
#define RT_FLAT_WAVES_F64 5
#endif
#ifndef RT_FLAT_WAVES_F64_LL  // the same for the lambertian + light kernel
#define RT_FLAT_WAVES_F64_LL 7  // C2 fp64: 5 waves 28.90 ms/frame, 6: 28.08 (r05c; the general kernel at 5: 31.28);
                                // 7 (72 VGPRs + 32 B spilled, from 80): 27.94 -> 27.79 (r05w7); 8 does not fit
#endif
// RUNS: the LL kernel's second form, whose wave queue hands out runs of items (kItemRuns). A kernel of its own, which
// launch_step takes only for a launch that has runs: a launch without them runs the code it always ran.
template <class R, bool TLDS = false, bool LL = false, bool RUNS = false>
struct FlatTrav : TravDefaults {
  static_assert(!RUNS || (TLDS && LL), "the runs form is the LL kernel's");
  static constexpr bool kFlat = true;
  static constexpr bool kTablesLds = TLDS;  // persistent kernel: Tables in LDS (fill, run_lds)
  static constexpr bool kLL = LL;           // lambertian + light scene (shade LL; the lm table)
  static constexpr bool kItemRuns = RUNS;  // (rt_plan.h kernel_takes_runs names the same kernels)
  static constexpr int kWaves = sizeof(R) == 4 ? RT_FLAT_WAVES : (LL ? RT_FLAT_WAVES_F64_LL : RT_FLAT_WAVES_F64);
  // not lean (fp32: 72 -> 64 VGPRs, but C2 23.5 -> 24.1 ms/frame)
  static constexpr bool kNoRad = true;  // 6 VGPRs in fp64 (its item sum is in LDS)
  static constexpr bool kColdLds = sizeof(R) == 8;
  template <bool ANY = false, class PS>
  __device__ __forceinline__ static void run(const DevScene<R>& sc, const Node<R>*, const PS& s, Keys, uint32_t*,
                                             R& t, uint32_t& e, int32_t& i, uint32_t& nm) {
    trace_flat<R, false, ANY>(sc, s.o, s.d, s.xe, s.xi, t, e, i, nm, sc.flatq, flat_rooms(sc), sc.flatb);
  }
  // the scene's small tables copied into LDS (persistent kernel): the hit's record and
  // material are then LDS reads instead of dependent global loads
  // (the LL kernel's tables are smaller, so a 256-lane block's LDS -- tables plus the fp64 cold path state,
  // ~27 KB with the general sizes -- leaves room for 6 blocks per CU)
  // (the fp64 LL kernel's 7 blocks per CU leave no whole 512-byte LDS granule: its one room record, 112 B, takes
  // the place of two of its 16 quad slots, 128 B -- a room stands for five or six quads)
  // The sizes are rt_plan.h's (kFlatLds, kFlatLdsLL): path_kernel gives this kernel only to a scene they hold.
  static constexpr FlatCaps kCaps = LL ? kFlatLdsLL : kFlatLds;
  static constexpr uint32_t kLdsQuads = kCaps.quads, kLdsBoxes = kCaps.boxes, kLdsMats = kCaps.mats;
  static constexpr uint32_t kLdsRooms = kCaps.rooms;
  struct Tables {
    FlatQuadT<R> q[kLdsQuads];
    FlatRoomT<R> r[kLdsRooms];
    FlatBoxT<R> b[kLdsBoxes];
    Material<R> m[LL ? 1 : kLdsMats];
    R4<R> lm[LL ? kLdsMats : 1];  // LL: (solid colour, 1 for diffuse_light)
  };
  __device__ __forceinline__ static void fill(const DevScene<R>& sc, Tables& tb) {
    const uint32_t nq = sc.n_flatq[0] + sc.n_flatq[1] + sc.n_flatq[2];
    for (uint32_t j = threadIdx.x; j < nq; j += kBlock) tb.q[j] = sc.flatq[j];
    if constexpr (sizeof(R) == 8 || kFlatRoomsF32)
      for (uint32_t j = threadIdx.x; j < sc.n_flatr; j += kBlock) tb.r[j] = flat_rooms(sc)[j];
    for (uint32_t j = threadIdx.x; j < sc.n_flatb; j += kBlock) tb.b[j] = sc.flatb[j];
    for (uint32_t j = threadIdx.x; j < sc.n_mats; j += kBlock) {
      if constexpr (LL) {
        const Material<R>& m = sc.mats[j];
        tb.lm[j] = R4<R>{m.tx.c0[0], m.tx.c0[1], m.tx.c0[2], m.kind == M_DIFFUSE_LIGHT ? R(1) : R(0)};
      } else {
        tb.m[j] = sc.mats[j];
      }
    }
  }
  template <class PS>
  __device__ __forceinline__ static void run_lds(const DevScene<R>& sc, const Tables& tb, const PS& s, R& t,
                                                 uint32_t& e, int32_t& i, uint32_t& nm) {
    trace_flat<R, sizeof(R) == 8>(sc, s.o, s.d, s.xe, s.xi, t, e, i, nm, tb.q, tb.r, tb.b);
  }
};
// LDSN: the scene's BVH nodes (at most kLdsNodeMax, rt_plan.h) are copied into LDS at kernel start, so
// every traversal step reads LDS instead of waiting on the memory hierarchy (RTOW: 117 nodes)
template <class R, int STACK, bool LDSN = false>
struct StackTrav : TravDefaults {  // (no cold state in LDS: its LDS holds the traversal stacks)
  static constexpr bool kClosestOccl = true;  // (fp32 rays re-decide near-edge quad hits in fp64: occlusion_early_exit)
  static constexpr int kStack = STACK;
  static constexpr int kLdsNodes = LDSN ? (int)kLdsNodeMax : 0;
  static constexpr int kWaves = sizeof(R) == 4 ? RT_STACK_WAVES : (LDSN ? 1 : RT_STACK_WAVES_F64);  // occupancy over a small spill
  template <bool ANY = false, class PS>
  __device__ __forceinline__ static void run(const DevScene<R>& sc, const Node<R>* nodes, const PS& s, Keys k,
                                             uint32_t* stk, R& t, uint32_t& e, int32_t& i, uint32_t&) {
    trace<R, STACK, kBlock, ANY>(sc, LDSN ? nodes : sc.nodes, s.o, s.d, s.tm, s.xe, s.xi, k, (uint32_t)s.bounce,
                                 s.xy(), stk, t, e, i);
  }
};

// The wide BVH (fp32, rt_device.h trace_wide). LDSN: the whole tree -- nodes and primitive
// words -- is copied into the block's dynamic LDS at kernel start; the per-lane stack follows it
// ([depth][lane], conflict-free). Otherwise nodes and primitives are read from global memory and
// only the stack is in LDS. Dynamic LDS is sized from the compiled scene (wide_lds_bytes).
#ifndef RT_WIDE_WAVES  // LDS-resident tree (C3: 4 waves 93.6 ms, 5: 86.2, 6: 83.0; with leaves of 6 spheres the
#define RT_WIDE_WAVES 7  // block needs ~21 KB, so 7 fit a CU: 64.0 -> 62.2 despite 22 spilled VGPRs; 8: 67.8)
#endif
#ifndef RT_SHADE_BATCH  // < 64: a wave stops traversing to shade once this many of its lanes have finished
#define RT_SHADE_BATCH 48  // (LDS-resident tree, C3 fp32 ms/frame: never 57.06, 48: 52.57, 52: 52.58, 56: 52.81, 60: 53.57; fp64 81.3 -> 75.8)
#endif
#ifndef RT_SHADE_BATCH_GLOBAL  // the same for trees in HBM (speculative traversal): C4 stand-in 413.6 ms/frame
#define RT_SHADE_BATCH_GLOBAL 48  // never pausing, 415.2 / 370.8 / 363.8 / 362.5 / 368.4 / 379.6 at 16/32/40/48/56/60
#endif
#ifndef RT_WIDE_WAVES_F64  // fp64 rays over the wide tree (round 3), tree in LDS (C3 fp64, ms/frame: 2 or 3 waves
#define RT_WIDE_WAVES_F64 4  // 99, 4 waves 90.2)
#endif
#ifndef RT_WIDE_WAVES_GLOBAL_F64  // tree in HBM (C4 fp64: 3 waves 599.8, 4: 555.0, 5: 567.3)
#define RT_WIDE_WAVES_GLOBAL_F64 4
#endif
#ifndef RT_WIDE_WAVES_GLOBAL_F64_LL  // the LL form (116 VGPRs at 4 waves): C4 fp64 at 4 waves 522.4 ms/frame, 5: 490.6
#define RT_WIDE_WAVES_GLOBAL_F64_LL 5  // (r05g; the general kernel at 4: 526.7)
#endif
#ifndef RT_WIDE_WAVES_F64_NL  // the NL form over an LDS tree, fp64 (116 VGPRs at 4 waves)
#define RT_WIDE_WAVES_F64_NL 5  // C3 fp64 at 4 waves 69.07 ms/frame, 5: 65.41 (r05q; the general kernel at 4: 70.23)
#endif
// LL: a lambertian + light scene (shade LL; the material table in static LDS); NL: no light (shade NL)
template <class R, bool SPH, bool TRI, bool QUAD, bool MOV, bool LDSN, bool LL = false, bool NL = false>
struct WideTrav : TravDefaults {  // (no cold state in LDS: its LDS holds the tree and the stacks)
  static constexpr bool kWide = true;
  static constexpr bool kLL = LL, kNL = NL, kMoving = MOV;
  static constexpr int kWaves = sizeof(R) == 4 ? (LDSN ? RT_WIDE_WAVES : RT_WIDE_WAVES_GLOBAL)
                                               : (LDSN ? (NL ? RT_WIDE_WAVES_F64_NL : RT_WIDE_WAVES_F64)
                                                       : (LL ? RT_WIDE_WAVES_GLOBAL_F64_LL : RT_WIDE_WAVES_GLOBAL_F64));
  // (Path LT) the fp64 LL kernel over a tree in HBM (C4): its throughput in LDS, 6 KB a block, for which its LDS stack
  // keeps 18 entries instead of 24: 339.2 -> 331.8 ms/frame, writes 16.4 -> 9.4 GB per launch (r06d). The fp64 NL
  // kernel over an LDS tree (C3) lost with it: 63.55 -> 68.08 ms/frame
  static constexpr bool kThrLds = sizeof(R) == 8 && !LDSN && LL;
  static constexpr bool kLean = true;  // registers for the traversal (fewer spills)
  static constexpr bool kNoRad = true;
  using StackT = WStackT<LDSN>;
  using WW = typename WWord<R>::T;
  // LDS layout: [nodes, kWNodeLdsStride each][primitive words][stack: entries x kBlock of StackT]
  __host__ __device__ static uint32_t stack_offset(uint32_t n_wnodes, uint32_t n_words) {
    return LDSN ? n_wnodes * kWNodeLdsStride + n_words * (uint32_t)sizeof(WW) : 0u;
  }
  // a tree in HBM, fp32 rays (RT_WIDE_TOP): [stack][the first wide_top nodes, WNode layout]
  static constexpr bool kTop = !LDSN && sizeof(R) == 4;
  static constexpr bool kTopH = !LDSN && sizeof(R) == 8;
  __host__ __device__ static uint32_t top_offset(uint32_t wide_stack) {
    return (wide_stack < wide_lds_stack<R>() ? wide_stack : wide_lds_stack<R>()) * kBlock * 4u;
  }
  __host__ __device__ static uint32_t root(const DevScene<R>& sc) {
    return LDSN ? wide_code16(sc.wroot) : sc.wroot;
  }
  __device__ __forceinline__ static StackT* fill(const DevScene<R>& sc, uint4* lds) {
    unsigned char* base = (unsigned char*)lds;
    if constexpr (LDSN) {
      const uint4* gn = (const uint4*)sc.wnodes;  // 8 words of 16 B per node, the last one padding
      for (uint32_t j = threadIdx.x; j < sc.n_wnodes * 7u; j += kBlock) {
        const uint32_t nd = j / 7u, f = j - nd * 7u;
        uint4 v = gn[nd * 8u + f];
        if (f == 6)  // four 16-bit codes in the first 8 bytes (trace_wide)
          v = make_uint4(wide_code16(v.x) | wide_code16(v.y) << 16, wide_code16(v.z) | wide_code16(v.w) << 16, 0u, 0u);
        *(uint4*)(base + nd * kWNodeLdsStride + f * 16u) = v;
      }
      uint4* pw = (uint4*)(base + sc.n_wnodes * kWNodeLdsStride);
      const uint4* gp = (const uint4*)sc.wprims;
      const uint32_t n16 = sc.n_wprim_words * (uint32_t)(sizeof(WW) / 16);
      for (uint32_t j = threadIdx.x; j < n16; j += kBlock) pw[j] = gp[j];
      __syncthreads();
    }
    if constexpr (kTop) {
      uint4* dst = (uint4*)(base + top_offset(sc.wide_stack));
      const uint4* gn = (const uint4*)sc.wnodes;
      const uint32_t ntop = min(sc.wide_top, (uint32_t)RT_WIDE_TOP_N);
      constexpr uint32_t kRows = kWTopStride / 16u;  // 7: the pad row of WNode is not copied
      for (uint32_t j = threadIdx.x; j < ntop * kRows; j += kBlock) {
        const uint32_t nd = j / kRows, r = j - nd * kRows;
        dst[j] = gn[nd * 8u + r];
      }
      __syncthreads();
    } else if constexpr (kTopH) {  // fp64 rays: the fp16 form, 5 words per node
      uint4* dst = (uint4*)(base + top_offset(sc.wide_stack));
      const uint4* gn = (const uint4*)sc.wnodesh;
      const uint32_t ntop = min(sc.wide_top, (uint32_t)RT_WIDE_TOP_N_F64);
      for (uint32_t j = threadIdx.x; j < ntop * 5u; j += kBlock) dst[j] = gn[j];
      __syncthreads();
    }
    return (StackT*)(base + stack_offset(sc.n_wnodes, sc.n_wprim_words));
  }
  // Advance the ray of s (false: paused, see trace_wide)
  template <bool ANY = false, class PS>
  __device__ __forceinline__ static bool steps(const DevScene<R>& sc, const Node<R>* lds, const PS& s, StackT* stk,
                                               WideRayT<R>& ry) {
    const unsigned char* base = (const unsigned char*)lds;
    // LDSN: the whole tree at the base; kTop: the copy of the tree's first levels after the stack
    return trace_wide<R, SPH, TRI, QUAD, MOV, LDSN, kBlock, LDSN ? RT_SHADE_BATCH : RT_SHADE_BATCH_GLOBAL, ANY>(
        sc, (kTop || kTopH) ? base + top_offset(sc.wide_stack) : base, (const WW*)(base + sc.n_wnodes * kWNodeLdsStride), s.o,
        s.d, s.tm, s.xe, stk, ry);
  }
};

template <int N>
struct Lds {
  uint32_t v[N];
};
template <>
struct Lds<0> {
  uint32_t v[1];
};

// RT_SECTION_CLOCKS (development build, scripts/dev_sections.py): RT_LANE_TIMED(sum, expr) and RT_WAVE_TIMED(k, expr)
// evaluate expr and add the shader-clock cycles it took to a lane's own sum, or -- by the first of the wave's lanes
// that evaluate it -- to count k of the block's wave-level counts (rt_device.h wide_stats_lds). The product build
// evaluates expr alone.
#ifdef RT_SECTION_CLOCKS
__device__ unsigned long long g_section_clocks[4];  // trace, shade, store, lanes
struct LaneTimer {
  uint64_t& sum;
  uint64_t c0;
  __device__ __forceinline__ explicit LaneTimer(uint64_t& s) : sum(s), c0(clock64()) {}
  __device__ __forceinline__ ~LaneTimer() { sum += clock64() - c0; }
};
struct WaveTimer {
  int k;
  uint64_t c0;
  __device__ __forceinline__ explicit WaveTimer(int k_) : k(k_), c0(clock64()) {}
  __device__ __forceinline__ ~WaveTimer() {
    if (__lane_id() == (uint32_t)__ffsll((unsigned long long)__ballot(1)) - 1)
      atomicAdd(wide_stats_lds() + k, (unsigned long long)(clock64() - c0));
  }
};
#define RT_LANE_TIMED(sum, ...) [&] { LaneTimer tm_(sum); return __VA_ARGS__; }()
#define RT_WAVE_TIMED(k, ...) [&] { WaveTimer tm_(k); return __VA_ARGS__; }()
#else
#define RT_LANE_TIMED(sum, ...) (__VA_ARGS__)
#define RT_WAVE_TIMED(k, ...) (__VA_ARGS__)
#endif

template <class R, class Trav, bool CAMX>
__device__ __forceinline__ void step_body(const Params<R>& p) {
  __shared__ Lds<Trav::kStack * kBlock> stk;
  __shared__ uint32_t wave_cnt[kBlock / 64];
  __shared__ Node<R> lds_nodes[Trav::kLdsNodes > 0 ? Trav::kLdsNodes : 1];
  if constexpr (Trav::kLdsNodes > 0) {
    for (uint32_t j = threadIdx.x; j < p.sc.n_nodes; j += kBlock) lds_nodes[j] = p.sc.nodes[j];
    __syncthreads();
  }
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t slot = 0, segs = 0;
  bool active = i < p.n;
  R4<R> Dv{};
  if (active) {
    slot = p.queue ? p.queue[i] : i;
    Dv = p.D[slot];
    active = Dv.w >= R(0);
  }
  if (active) {
    Path<R> s;
    load_path(p, slot, Dv, s);
#ifdef RT_SECTION_CLOCKS
    uint64_t c_trace = 0, c_shade = 0, c_store = 0;
#endif
#pragma unroll 1
    for (int k = 0; k < p.K; k++) {
      R t;
      uint32_t e, nm = 0;
      int32_t inst;
      RT_LANE_TIMED(c_trace, Trav::run(p.sc, lds_nodes, s, Keys{s.ks}, stk.v + threadIdx.x, t, e, inst, nm));
      segs++;
      if (!RT_LANE_TIMED(c_shade, shade<R, CAMX, ShadeGeneral<Trav::kFlat>>(p, s, t, e, inst, nm))) break;
    }
    RT_LANE_TIMED(c_store, store_path(p, slot, s));
#ifdef RT_SECTION_CLOCKS
    // shader-clock cycles per section, summed over lanes (divide by the lane count)
    atomicAdd(&g_section_clocks[0], (unsigned long long)c_trace);
    atomicAdd(&g_section_clocks[1], (unsigned long long)c_shade);
    atomicAdd(&g_section_clocks[2], (unsigned long long)c_store);
    atomicAdd(&g_section_clocks[3], 1ull);
#endif
  }
  // segments traced: wave sums, one atomic per block
  for (int off = 32; off > 0; off >>= 1) segs += __shfl_xor(segs, off);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = segs;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (c) atomicAdd(&p.seg_shards[blockIdx.x % kSegShards], (unsigned long long)c);
  }
}

// Persistent form of the same loop (the default schedule): the grid is what the chip holds
// resident, every lane keeps its path state in registers for the whole render. shade's path
// regeneration pulls the next item from the wave's queue, refilled a batch at a time from the
// per-XCD heads (one returning atomic per 64 items; per-lane atomics on one counter for the whole
// chip serialised across the 8 XCDs' L2s: measured 6x slower on C2). No state goes through HBM
// between segments, there is no launch per K segments and no live-slot compaction.
//
// The kernel's parameters, read from the kernarg segment afresh each segment (the asm hides the
// pointer from loop-invariant hoisting): hoisted, they outgrow the SGPR file and spill into VGPR
// lanes, one v_readlane per use (C2 flat program: 73 SGPR spills -> 0, 24.9 -> 23.9 ms/frame;
// scalar loads hit the constant cache. The wide kernels, with the lean path state: C3 fp32 51.9 ->
// 51.1 ms/frame, fp64 71.3 -> 70.7, C4 neutral)
template <class R>
__device__ __forceinline__ const Params<R>& reload_params() {
  using KP = const __attribute__((address_space(4))) Params<R>*;
  KP kp = (KP)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return *(const Params<R>*)kp;
}
// True (and the fault word set) once a lane has traced more segments than its cap, which cannot happen:
// every segment advances a bounce-capped path
template <class R>
__device__ __forceinline__ bool seg_cap_hit(const Params<R>& q, uint64_t segs) {
  if (segs > q.seg_cap) {
    atomicOr(q.fault, 1u);
    return true;
  }
  return false;
}
// The same for the loops that count in 32 bits (launch keeps seg_cap below 2^32): the count is the loop's iteration
// number, the same in every lane still in it, so the compare is one scalar instruction
// (p: the kernel's own parameter, for the fault word's address. The compiler sinks the store below the loop, and an
// address read through q, which is a new value every iteration, would be copied into a VGPR pair every iteration)
template <class R>
__device__ __forceinline__ bool seg_cap_hit(const Params<R>& p, const Params<R>& q, uint32_t segs) {
  if (segs > (uint32_t)q.seg_cap) {
    atomicOr(p.fault, 1u);
    return true;
  }
  return false;
}
template <class R, class Trav, bool CAMX>
__device__ __forceinline__ void persist_body(const Params<R>& p) {
  __shared__ Lds<Trav::kStack * kBlock> stk;
  __shared__ uint32_t wave_cnt[kBlock / 64];
  __shared__ Node<R> lds_nodes[Trav::kLdsNodes > 0 ? Trav::kLdsNodes : 1];
  if constexpr (Trav::kLdsNodes > 0) {
    for (uint32_t j = threadIdx.x; j < p.sc.n_nodes; j += kBlock) lds_nodes[j] = p.sc.nodes[j];
    __syncthreads();
  }
  uint32_t* stk_lane = stk.v + threadIdx.x;
  const Node<R>* trav_nodes = lds_nodes;
  [[maybe_unused]] void* wstk = nullptr;  // the wide traversal's lane stack (uint16 or uint32 entries)
#ifdef RT_SECTION_CLOCKS
  if (threadIdx.x < 10) wide_stats_lds()[threadIdx.x] = 0;
  __syncthreads();
#endif
  if constexpr (Trav::kWide) {
    extern __shared__ uint4 dyn_lds[];
    wstk = Trav::fill(p.sc, dyn_lds) + threadIdx.x;
    trav_nodes = (const Node<R>*)dyn_lds;
  }
  // shade's LDS tables (ShadeOf<Trav>::kMatsLds, kLL): the materials, and the LL kernels' (colour, kind) records
  const Material<R>* mats = nullptr;
  const R4<R>* lm = nullptr;
  [[maybe_unused]] const typename Trav::Tables* flat_tb = nullptr;
  if constexpr (Trav::kTablesLds) {  // path_kernel (rt_plan.h) gives this kernel only to a scene whose tables fit
    __shared__ typename Trav::Tables tb;
    Trav::fill(p.sc, tb);
    __syncthreads();
    flat_tb = &tb;
    mats = tb.m;
    lm = tb.lm;
  }
  // the wide and linear LL kernels: the materials as (colour, kind) records in LDS, kind 0 lambertian, 1
  // diffuse_light, 2 isotropic (shade LL, LLI)
  if constexpr (Trav::kLL && !Trav::kTablesLds) {  // (the flat program's table is in its Tables)
    __shared__ R4<R> wlm_tab[Trav::kLdsMats];
    for (uint32_t j = threadIdx.x; j < p.sc.n_mats; j += kBlock) {
      const Material<R>& m = p.sc.mats[j];
      wlm_tab[j] = R4<R>{m.tx.c0[0], m.tx.c0[1], m.tx.c0[2],
                         m.kind == M_DIFFUSE_LIGHT ? R(1) : (m.kind == M_ISOTROPIC ? R(2) : R(0))};
    }
    __syncthreads();
    lm = wlm_tab;
  }
  constexpr bool kRuns = ShadeOf<Trav>::kRuns;  // item0 is then a unit of the queue (begin_item RUNS)
  uint32_t item0 = blockIdx.x * kBlock + threadIdx.x;
  if (p.persist == kPersist) {
    if ((threadIdx.x & 63) == 0) {
      __hip_atomic_store(wave_queue(), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
      __hip_atomic_store(wave_queue() + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    item0 = next_item_dyn<kRuns>(p);
  }
  std::conditional_t<Trav::kWide || Trav::kCapBeforeShade, uint64_t, uint32_t> segs = 0;
  if (item0 < (kRuns ? p.n_units : p.n_items)) {
    Path<R, Trav::kColdLds, Trav::kLean, Trav::kNoRad, Trav::kThrLds> s;
    s.set_acc(mkv(R(0), R(0), R(0)));
    begin_item<Trav::kRays, kRuns>(p, s, item0);
    begin_sample<R, CAMX, Trav::kRays>(p, s);
    if constexpr (Trav::kWide) {
      // resumable traversal: a ray paused with the wave's laggards carries on after the others shade
      using StackT = typename Trav::StackT;
      const uint32_t root = Trav::root(p.sc);
      WideRayT<R> ry{root, 0, Num<R>::inf(), kNoHit, 1u};
#pragma unroll 1
      for (;;) {
        const Params<R>& q = reload_params<R>();
        if (!RT_WAVE_TIMED(6, Trav::steps(q.sc, trav_nodes, s, (StackT*)wstk, ry))) continue;
        if (seg_cap_hit(q, ++segs)) break;
        const R t = ry.tmax;
        const uint32_t e = ry.e;
        ry = WideRayT<R>{root, 0, Num<R>::inf(), kNoHit, 1u};
        RT_WIDE_STAT(4);
        if (!RT_WAVE_TIMED(7, shade<R, CAMX, ShadeOf<Trav>>(q, s, t, e, -1, 0, mats, lm))) break;
      }
    } else {
      // the flat program with its records and materials in LDS (Trav::Tables), or the scene in global memory
#pragma unroll 1
      for (;;) {
        const Params<R>& q = reload_params<R>();
        R t;
        uint32_t e, nm = 0;
        int32_t inst;
        RT_WIDE_STAT(0);
        if constexpr (Trav::kTablesLds)
          RT_WAVE_TIMED(6, Trav::run_lds(q.sc, *flat_tb, s, t, e, inst, nm));
        else
          RT_WAVE_TIMED(6, Trav::run(q.sc, trav_nodes, s, Keys{s.ks}, stk_lane, t, e, inst, nm));
        // The segment is counted before shade (a lane that shade retires has traced it) and the cap tested after:
        // tested between trace and shade, the cap's exit was a second edge out of the loop that carried the path state
        // the iteration began with, and the loop's latch copied the state shade wrote over it, every iteration
        // (DESIGN.md §4, round 9). A lane past its cap, which cannot happen, shades once more before it leaves
        // (Trav::kCapBeforeShade: the one kernel that was slower so keeps the earlier order, and its 64-bit count)
        ++segs;
        if constexpr (Trav::kCapBeforeShade)
          if (seg_cap_hit(q, segs)) break;
        if (!RT_WAVE_TIMED(7, shade<R, CAMX, ShadeOf<Trav>>(q, s, t, e, inst, nm, mats, lm))) break;
        if constexpr (!Trav::kCapBeforeShade)
          if (seg_cap_hit(p, q, segs)) break;
      }
    }
  }
  uint32_t sg = (uint32_t)segs;
  for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = sg;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t c = (uint64_t)wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (c) atomicAdd(&p.seg_shards[blockIdx.x % kSegShards], (unsigned long long)c);
  }
#ifdef RT_SECTION_CLOCKS
  if (threadIdx.x < 10) atomicAdd(&g_wide_stats[threadIdx.x], wide_stats_lds()[threadIdx.x]);
#endif
}
template <class R, class Trav, bool CAMX>
__global__ __launch_bounds__(kBlock) void k_persist(Params<R> p) {
  persist_body<R, Trav, CAMX>(p);
}
// CAMX kernels (non-perspective cameras, picture and procedural textures) take RT_CAMX_WAVES (fp32) and
// RT_CAMX_WAVES_F64 waves per SIMD. Round 4 left them unbudgeted: ~290 registers, 1 wave per SIMD. With the
// heavy code as calls (RT_EXT_FN) the §8(f) configs, ms/frame at 1 wave (round 4) / 2 / 3 / 4 waves (r05f,
// r05g): fisheye f64 14.8 / 11.0 / 13.5 / 16.2, f32 14.2 / 10.7 / 8.6 / 8.8; earth f64 10.5 / 6.6 / 8.9 /
// 11.1, f32 9.9 / 6.2 / 4.9 / 4.8; perlin f64 148 / 81 / 70 / 79, f32 128 / 69 / 50 / 43. The fp64 linear
// programs need ~144 registers without any CAMX code, so 4 waves spills there.
#ifndef RT_CAMX_WAVES
#define RT_CAMX_WAVES 4
#endif
#ifndef RT_CAMX_WAVES_F64
#define RT_CAMX_WAVES_F64 2
#endif
#define RT_CAMX_W(R) (sizeof(R) == 8 ? RT_CAMX_WAVES_F64 : RT_CAMX_WAVES)
template <class R, class Trav, bool CAMX>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(CAMX ? RT_CAMX_W(R) : Trav::kWaves))) void k_persist_occ(
    Params<R> p) {
  persist_body<R, Trav, CAMX>(p);
}

// The kernel; k_step_occ is the same body with the register budget cut for Trav::kWaves
// waves per SIMD (only where that does not spill much, see LinearTrav::kWaves).
// CAMX ("extended"): a non-perspective camera (camera_ray) or procedural textures (noise.h); the
// base kernels, which every BASELINE config except the noise scenes uses, contain neither.
template <class R, class Trav, bool CAMX>
__global__ __launch_bounds__(kBlock) void k_step(Params<R> p) {
  step_body<R, Trav, CAMX>(p);
}
template <class R, class Trav, bool CAMX>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(CAMX ? RT_CAMX_W(R) : Trav::kWaves))) void k_step_occ(Params<R> p) {
  step_body<R, Trav, CAMX>(p);
}

// ------------------------------------------------------------------ ray queries (rt_trace_rays)
// k_trace: world.hit(r, interval(0.001, inf), rec) (camera.h:198) for caller-given rays, through the traversal
// policies above -- the same trace_flat / trace_linear / trace_wide / trace the render kernels call -- and the hit
// record shade would compute, written out instead of shaded. A grid-stride kernel: the grid is resident lanes, not
// rays (a deep wide tree's spill area is indexed by lane, launch_trace).
template <class R>
struct KTrace : TraceParams<R> {};  // the kernel's argument as a type of this translation unit (as Params)

// The ray state the policies read: a camera ray (bounce 0) that leaves no surface (no self-exclusion).
template <class R>
struct QueryRay {
  V<R> o, d;
  R tm;
  int32_t bounce;
  uint32_t ks;
  uint32_t xe;
  int32_t xi;
  __device__ __forceinline__ uint32_t xy() const { return 0u; }  // read only to rebuild a camera ray (cam64 = 0: never)
};

// hit_record of the closest hit (t, e, inst, nm) of the ray (o, d, tm): the point, the face-forwarded normal and
// front_face as shade computes them before it reads the material -- a restatement of shade's geometry block for
// the base kernels (CAMX = false, MOVING = true), kept apart so that shade's code does not move.
// obj_n (the feature-buffer pass): where given, the object-space outward normal of a sphere, quad or triangle,
// before it is face-forwarded and rotated out -- what sphere.h:70 takes u, v from.
template <class R, bool FLAT>
__device__ __forceinline__ void hit_record(const DevScene<R>& sc, V<R> o, V<R> d, R tm, R t, uint32_t e, int32_t inst,
                                           uint32_t nm, V<R>& pw, V<R>& n, bool& front, V<R>* obj_n = nullptr) {
  const uint32_t ty = etype(e), idx = epay(e);
  if constexpr (FLAT) {  // quad.h:47-50 with n = +-e_A; hit_record::set_face_normal (hittable.h:26-29)
    const uint32_t A = (nm >> 28) & 3u;
    const bool neg = (nm >> 31) != 0;
    const R dA = A == 0 ? d.x : (A == 1 ? d.y : d.z);
    pw = o + t * d;
    front = neg ? dA > R(0) : dA < R(0);
    const R fs = front != neg ? R(1) : R(-1);
    const R z = front ? R(0) : -R(0);
    n = mkv(A == 0 ? fs : z, A == 1 ? fs : z, A == 2 ? fs : z);
    return;
  }
  if (ty == E_VOLUME) {  // volumne.h:40-44
    pw = o + t * d;
    n = mkv(R(1), R(0), R(0));
    front = true;
    return;
  }
  V<R> oo = o, dd = d;
  const Instance<R>* in = nullptr;
  if (inst >= 0) in = &sc.insts[inst];
  // fp32, planar primitives: the hit is o + t d in world space and only the normal is rotated out; fp64 keeps the
  // reference's object-space point (hittable.h:75-82, 125-149)
  const bool world_space = sizeof(R) == 4 && ty != E_SPHERE;
  if (in && !world_space) chain_in(*in, oo, dd);
  V<R> po = oo + t * dd;
  V<R> outward;
  if (ty == E_QUAD) {
    outward = ld3(sc.quads[idx].n);
  } else if (ty == E_SPHERE) {  // sphere.h:69 (center_ member; (0,0,0) for moving spheres)
    const Sphere<R>& sp = sc.spheres[idx];
    if constexpr (sizeof(R) == 8) {
      outward = (po - ld3(sp.cn)) / sp.r;
    } else {  // the point and normal from the root refined in fp64 by one Newton step (shade)
      double cx = sp.c1[0], cy = sp.c1[1], cz = sp.c1[2];
      if (sp.moving) {
        cx += (double)tm * sp.dc[0];
        cy += (double)tm * sp.dc[1];
        cz += (double)tm * sp.dc[2];
      }
      const double ox = oo.x, oy = oo.y, oz = oo.z, dx = dd.x, dy = dd.y, dz = dd.z, t0 = t, rr = sp.r;
      const double qx = (ox + t0 * dx) - cx, qy = (oy + t0 * dy) - cy, qz = (oz + t0 * dz) - cz;
      const double g = (qx * qx + qy * qy + qz * qz) - rr * rr;
      const float gp = 2.0f * ((float)qx * dd.x + (float)qy * dd.y + (float)qz * dd.z);
      float step = fdiv((float)g, gp);
      if (!(fabsf(step) <= 1e-4f * fabsf(t))) step = 0.0f;
      const double td = t0 - (double)step;
      const double px = ox + td * dx, py = oy + td * dy, pz = oz + td * dz;
      po = mkv((float)px, (float)py, (float)pz);
      outward = mkv((float)(px - sp.cn[0]), (float)(py - sp.cn[1]), (float)(pz - sp.cn[2])) * fdiv(R(1), sp.r);
    }
  } else {
    outward = ld3(sc.tris[idx].n);
  }
  if (obj_n) *obj_n = outward;
  if (world_space) {  // dd is the world ray: the object-space normal goes out first
    if (in)
      for (int q = in->nops - 1; q >= 0; q--) outward = op_out(in->op[q], outward, false);
    front = dot(dd, outward) < R(0);  // hit_record::set_face_normal (hittable.h:26-29)
    n = front ? outward : -outward;
    pw = po;
  } else {
    front = dot(dd, outward) < R(0);
    n = front ? outward : -outward;
    pw = po;
    if (in) {
      for (int q = in->nops - 1; q >= 0; q--) {
        pw = op_out(in->op[q], pw, true);
        n = op_out(in->op[q], n, false);
      }
    }
  }
}

template <class R, class A>  // A: KTrace<R> or KOccl<R> (rays, seed)
__device__ __forceinline__ void load_query(const A& a, uint32_t i, QueryRay<R>& s, double& tmax) {
  const double2* q = (const double2*)(a.rays + 8ull * i);  // 64 bytes, 16-byte aligned
  const double2 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3];
  s.o = mkv(R(r0.x), R(r0.y), R(r1.x));
  s.d = mkv(R(r1.y), R(r2.x), R(r2.y));
  s.tm = R(r3.x);
  tmax = r3.y;
  s.bounce = 0;
  s.ks = key_path(key_pixel(a.seed, i), key_sample(a.seed, 0u));  // the path key of (seed, pixel = i, sample = 0)
  s.xe = kNoHit;
  s.xi = -1;
}
template <class R, bool FLAT>
__device__ __forceinline__ void store_query(const KTrace<R>& a, uint32_t i, const QueryRay<R>& s, double tmax, R t,
                                            uint32_t e, int32_t inst, uint32_t nm) {
  double* g = a.geom + 7ull * i;
  int4 id = make_int4(-1, -1, -1, -1);
  double tv = __builtin_huge_val();
  V<R> pw = mkv(R(0), R(0), R(0)), n = pw;
  if (e != kNoHit && (double)t <= tmax) {
    bool front;
    hit_record<R, FLAT>(a.sc, s.o, s.d, s.tm, t, e, inst, nm, pw, n, front);
    // the descriptor's object behind the device record (the flat program's face copies are quad records too)
    const uint32_t ty = etype(e), tab = ty == E_VOLUME ? 3u : ty;
    const int2 om = a.idtab[a.id_off[tab] + epay(e)];
    const int32_t kind = ty == E_QUAD ? RT_OBJ_QUAD : ty == E_SPHERE ? RT_OBJ_SPHERE : ty == E_TRI ? RT_OBJ_TRIANGLE : RT_OBJ_VOLUME;
    id = make_int4(om.x, om.y, kind, front ? 1 : 0);
    tv = (double)t;
  }
  g[0] = tv;
  g[1] = (double)pw.x;
  g[2] = (double)pw.y;
  g[3] = (double)pw.z;
  g[4] = (double)n.x;
  g[5] = (double)n.y;
  g[6] = (double)n.z;
  *(int4*)(a.ids + 4ull * i) = id;
}

// The loop of the query kernels over a traversal policy, a grid-stride loop over resident lanes. A Job is the ray
// source and the hit sink: valid() says whether the lane has a first ray, load() builds the current one, hit() takes
// its closest hit, advance() moves on and says whether there is another. k_trace's job reads caller-given rays and
// writes one record a ray; k_aov's builds the camera rays of a pixel and sums their feature channels.
// Job::kAny (k_occluded's early-exit job): the traversals run in their any-hit form, the interval's upper end being
// the job's bound() of the current ray; hit() then takes e != kNoHit as "occluded" and nothing else of a hit.
template <class R, class Trav, class Job>
__device__ __forceinline__ void query_loop(const DevScene<R>& sc, Job& job) {
  __shared__ Lds<Trav::kStack * kBlock> stk;
  QueryRay<R> s;
  if constexpr (Trav::kWide) {
    // the resumable traversal, driven as persist_body drives it: a ray paused with the wave's laggards carries on
    // beside the rays the finished lanes take next
    using StackT = typename Trav::StackT;
    extern __shared__ uint4 dyn_lds[];
    StackT* wstk = Trav::fill(sc, dyn_lds) + threadIdx.x;  // (every lane of the block: it holds the barriers)
    if (!job.valid()) return;
    job.load(s);
    const uint32_t root = Trav::root(sc);
    R hi = Num<R>::inf();  // the interval's upper end: open unless the job bounds it
    if constexpr (Job::kAny) hi = job.bound();
    WideRayT<R> ry{root, 0, hi, kNoHit, 1u};
#pragma unroll 1
    for (;;) {
      if (!Trav::template steps<Job::kAny>(sc, (const Node<R>*)dyn_lds, s, wstk, ry)) continue;
      job.template hit<false>(s, ry.tmax, ry.e, -1, 0u);
      if (!job.advance()) break;
      job.load(s);
      if constexpr (Job::kAny) hi = job.bound();
      ry = WideRayT<R>{root, 0, hi, kNoHit, 1u};
    }
  } else {
#pragma unroll 1
    for (bool more = job.valid(); more; more = job.advance()) {
      job.load(s);
      R t;  // closest hit: an output alone
      if constexpr (Job::kAny) t = job.bound();
      uint32_t e, nm = 0;
      int32_t inst;
      Trav::template run<Job::kAny>(sc, sc.nodes, s, Keys{s.ks}, stk.v + threadIdx.x, t, e, inst, nm);
      job.template hit<Trav::kFlat>(s, t, e, inst, nm);
    }
  }
}

template <class R>
struct TraceJob {
  static constexpr bool kAny = false;
  const KTrace<R>& a;
  uint32_t i, stride;  // stride: at most the resident lanes, so i + stride stays below 2^32
  double tmax;
  __device__ __forceinline__ bool valid() const { return i < a.n; }
  __device__ __forceinline__ void load(QueryRay<R>& s) { load_query(a, i, s, tmax); }
  template <bool FLAT>
  __device__ __forceinline__ void hit(const QueryRay<R>& s, R t, uint32_t e, int32_t inst, uint32_t nm) {
    store_query<R, FLAT>(a, i, s, tmax, t, e, inst, nm);
  }
  __device__ __forceinline__ bool advance() {
    i += stride;
    return i < a.n;
  }
};

template <class R, class Trav>
__global__ __launch_bounds__(kBlock) void k_trace(KTrace<R> a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) atomicAdd(a.seg_shards, (unsigned long long)a.n);  // rt_counters.segments
  TraceJob<R> job{a, i, gridDim.x * kBlock, 0.0};
  query_loop<R, Trav>(a.sc, job);
}

// ------------------------------------------------------------------ occlusion queries (rt_occluded)
// k_occluded: out[i] = 1 exactly when k_trace reports a hit for ray i (finite t), one byte a ray.
// EARLY (rt_plan.h occlusion_early_exit): the traversal's interval is [0.001, bound] from the start, bound being the
// largest R value <= tmax, and the lane is done at the first primitive that accepts -- no hit record, no ids. For a
// t representable in R, t <= bound <=> (double)t <= tmax, k_trace's own comparison; a primitive's test returns its
// first root inside the closed interval, so some primitive accepts within [0.001, bound] exactly when the closest
// hit is <= bound. !EARLY: k_trace's traversal and draws unchanged, then (double)t <= tmax.
template <class R>
struct KOccl : OcclParams<R> {};

template <class R, bool EARLY>
struct OcclJob {
  static constexpr bool kAny = EARLY;
  const KOccl<R>& a;
  uint32_t i, stride;  // as TraceJob's
  double tmax;
  R bnd;      // EARLY: the interval's upper end, never below its lower one (the fp32 tests order bit patterns)
  bool live;  // EARLY: [0.001, tmax] holds an R value at all (false also for a NaN tmax): else the answer is 0
  __device__ __forceinline__ bool valid() const { return i < a.n; }
  __device__ __forceinline__ void load(QueryRay<R>& s) {
    load_query(a, i, s, tmax);
    if constexpr (EARLY) {
      R b = (R)tmax;  // fp32: to nearest, then down where that went up (+inf stays, a finite tmax above FLT_MAX
                      // becomes FLT_MAX; a negative or NaN tmax fails the comparison below whatever its bits)
      if constexpr (sizeof(R) == 4)
        if ((double)b > tmax) b = __uint_as_float(__float_as_uint(b) - 1u);
      live = b >= R(0.001);
      bnd = live ? b : R(0.001);
    }
  }
  __device__ __forceinline__ R bound() const { return bnd; }
  template <bool FLAT>
  __device__ __forceinline__ void hit(const QueryRay<R>&, R t, uint32_t e, int32_t, uint32_t) {
    bool occ;
    if constexpr (EARLY)
      occ = live & (e != kNoHit);
    else
      occ = e != kNoHit && (double)t <= tmax;  // store_query's test
    a.out[i] = occ ? (uint8_t)1 : (uint8_t)0;
  }
  __device__ __forceinline__ bool advance() {
    i += stride;
    return i < a.n;
  }
};

template <class R, class Trav, bool EARLY>
__global__ __launch_bounds__(kBlock) void k_occluded(KOccl<R> a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) atomicAdd(a.seg_shards, (unsigned long long)a.n);  // rt_counters.segments
  OcclJob<R, EARLY> job{a, i, gridDim.x * kBlock, 0.0, R(0), false};
  query_loop<R, Trav>(a.sc, job);
}

// ------------------------------------------------------------------ camera rays and feature buffers
// camera::generate_ray (camera.h:244-293) for the sample with path key ks of pixel (x, y), every camera model, in
// fp64: the ray begin_sample builds (its perspective branch and camera_ray, through the same persp_pixel /
// persp_sample and the same draws), with the camera read as wave-uniform scalars. The one helper of k_camera_rays
// and k_aov, so the rays the one writes are bit for bit the rays the other traces. EXT = false: the perspective
// camera only (k_aov's base form, which then calls nothing out of line).
template <bool EXT>
__device__ __forceinline__ void sample_ray(const CamDev* cp, int32_t mode, uint32_t ks, uint32_t x, uint32_t y,
                                           V<double>& o, V<double>& d, double& tm) {
  const double ox = to_unit<double>(draw_u32(ks, 0)) - 0.5;  // sample_square (camera.h:293)
  const double oy = to_unit<double>(draw_u32(ks, 1)) - 0.5;
  if (!EXT || mode == RT_CAM_PERSPECTIVE) {  // camera.h:245-251
    const V<double> du = ld_uniform(&cp->du, 0), dv = ld_uniform(&cp->dv, 0);
    o = ld_uniform(&cp->pos, 0);
    d = persp_sample(persp_pixel(ld_uniform(&cp->dir00, 0), du, dv, x, y), du, dv, ox, oy);
    tm = to_unit<double>(draw_u32(ks, 2));
  } else if constexpr (EXT) {
    camera_ray(cp, ks, x, y, ox, oy, o, d, tm);
  }
}

// rt_camera_rays: one lane per (pixel, sample), rows in rt_trace_rays' format
__global__ __launch_bounds__(kBlock) void k_camera_rays(CamRayParams a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= a.npix * a.spp) return;
  const uint32_t pix = r / a.spp, sidx = r - pix * a.spp;
  const uint32_t xy = a.pixmap[pix], x = xy & 0xFFFFu, y = xy >> 16;
  const uint32_t ks = key_path(key_pixel(a.seed, y * a.W + x), key_sample(a.seed, a.first_sample + sidx));
  V<double> o, d;
  double tm;
  sample_ray<true>(a.camx, a.cam_mode, ks, x, y, o, d, tm);
  double2* q = (double2*)(a.rays + 8ull * r);  // 64 bytes, 16-byte aligned
  q[0] = make_double2(o.x, o.y);
  q[1] = make_double2(o.z, d.x);
  q[2] = make_double2(d.y, d.z);
  q[3] = make_double2(tm, __builtin_huge_val());
}

// k_aov: the first-hit feature buffers of a frame (rt_render_aov). The work item is a pixel: the lane builds the
// pixel's camera rays one after the other, traces each through the query loop above and adds its albedo, normal,
// depth and hit flag to eight double sums, in sample order -- so a pixel's values depend on nothing but (seed,
// pixel, samples) -- and stores the means once.
// EXT, as the render kernels' CAMX: the form for a non-perspective camera or a texture other than solid and checker
// (rt_plan.h aov_extended). The base form holds the perspective camera and tex_sample's solid / checker branch only
// and calls no out-of-line function of the extended kernels, so it keeps the query kernels' register budget.
template <class R>
struct KAov : AovParams<R> {};

template <class R, bool EXT>
struct AovJob {
  static constexpr bool kAny = false;
  const KAov<R>& a;
  uint32_t pix, stride;
  uint32_t sidx, xy, ka;
  double dlen;  // |d| of the running sample's fp64 ray: depth = t |d|
  double ar, ag, ab, nx, ny, nz, depth, hits;
  int4 id;

  __device__ __forceinline__ void begin_pixel() {
    xy = a.pixmap[pix];
    ka = key_pixel(a.seed, (xy >> 16) * a.W + (xy & 0xFFFFu));
    sidx = 0;
    ar = ag = ab = nx = ny = nz = depth = hits = 0.0;
    id = make_int4(-1, -1, -1, -1);
  }
  __device__ __forceinline__ bool valid() {
    if (pix >= a.npix) return false;
    begin_pixel();
    return true;
  }
  __device__ __forceinline__ void load(QueryRay<R>& s) {
    s.ks = key_path(ka, key_sample(a.seed, a.first_sample + sidx));  // the pixel's own path key: volume draws too
    V<double> o, d;
    double tm;
    sample_ray<EXT>(a.camx, a.cam_mode, s.ks, xy & 0xFFFFu, xy >> 16, o, d, tm);
    dlen = sqrt(dot(d, d));
    s.o = mkv(R(o.x), R(o.y), R(o.z));
    s.d = mkv(R(d.x), R(d.y), R(d.z));
    s.tm = R(tm);
    s.bounce = 0;
    s.xe = kNoHit;
    s.xi = -1;
  }
  template <bool FLAT>
  __device__ __forceinline__ void hit(const QueryRay<R>& s, R t, uint32_t e, int32_t inst, uint32_t nm) {
    const DevScene<R>& sc = a.sc;
    V<R> alb = mkv(R(0), R(0), R(0));
    if (e == kNoHit) {  // camera::miss (camera.h:180-190): the background through its unit-sphere test
      if (sc.background >= 0) {
        const V<R> o = s.o, d = s.d;
        R tb;
        if (sphere_roots<R>(o.x, o.y, o.z, d.x, d.y, d.z, o.x, o.y, o.z, R(1), R(0.001), Num<R>::inf(), false, tb)) {
          const Texture<R>& bt = sc.texs[sc.background];
          double bu = 0, bv = 0;
          if constexpr (EXT)
            if (bt.kind == T_IMAGE) sphere_uv(tb * d, bu, bv);  // (only a picture reads u, v)
          alb = tex_sample<R, EXT>(sc, bt, o + tb * d, bu, bv);
        }
      }
    } else {
      V<R> pw, n, on;
      bool front;
      hit_record<R, FLAT>(sc, s.o, s.d, s.tm, t, e, inst, nm, pw, n, front, &on);
      const uint32_t ty = etype(e), idx = epay(e);
      int32_t mat;  // the material shade reads for this record
      if constexpr (FLAT)
        mat = (int32_t)(nm & kNmMat);
      else
        mat = ty == E_VOLUME ? sc.vols[idx].phase_mat
              : ty == E_QUAD ? sc.quads[idx].mat
                             : ty == E_SPHERE ? sc.spheres[idx].mat : sc.tris[idx].mat;
      const Material<R>& m = sc.mats[mat];
      double hu = 0, hv = 0;  // hit_record u, v as shade's extended branch has them; only a picture reads them
      if constexpr (EXT && !FLAT) {  // (aov_family: a scene with pictures never takes the flat program)
        if (m.tx.kind == T_IMAGE) {
          if (ty == E_QUAD) {  // quad.h:47-62: alpha, beta of the object-space point
            const Quad<R>& q = sc.quads[idx];
            V<R> oo = s.o, dd = s.d;
            if (inst >= 0) chain_in(sc.insts[inst], oo, dd);
            const V<R> rel = (oo + t * dd) - ld3(q.q);
            hu = (double)dot(rel, ld3(q.a));
            hv = (double)dot(rel, ld3(q.b));
          } else if (ty == E_SPHERE) {
            sphere_uv(on, hu, hv);  // sphere.h:70
          }
        }
      }
      alb = tex_sample<R, EXT>(sc, m.tx, pw, hu, hv);
      nx += (double)n.x;
      ny += (double)n.y;
      nz += (double)n.z;
      depth += (double)t * dlen;
      hits += 1.0;
      if (sidx == 0) {  // the ids of sample first_sample, as store_query reports them
        const uint32_t tab = ty == E_VOLUME ? 3u : ty;
        const int2 om = a.idtab[a.id_off[tab] + idx];
        const int32_t kind = ty == E_QUAD ? RT_OBJ_QUAD : ty == E_SPHERE ? RT_OBJ_SPHERE : ty == E_TRI ? RT_OBJ_TRIANGLE : RT_OBJ_VOLUME;
        id = make_int4(om.x, om.y, kind, front ? 1 : 0);
      }
    }
    ar += (double)alb.x;
    ag += (double)alb.y;
    ab += (double)alb.z;
  }
  __device__ __forceinline__ bool advance() {
    if (++sidx < a.spp) return true;
    const double n = (double)a.spp;
    double2* f = (double2*)(a.feat + 8ull * pix);  // 64 bytes, 16-byte aligned
    f[0] = make_double2(ar / n, ag / n);
    f[1] = make_double2(ab / n, nx / n);
    f[2] = make_double2(ny / n, nz / n);
    f[3] = make_double2(depth / n, hits / n);
    *(int4*)(a.ids + 4ull * pix) = id;
    pix += stride;  // at most the resident lanes: pix + stride stays below 2^32
    if (pix >= a.npix) return false;
    begin_pixel();
    return true;
  }
};

// waves per SIMD of the extended form: the extended render kernels' (RT_CAMX_W). It calls the same out-of-line functions they call
// (camera_ray, sphere_uv, the noise textures), and the compiler gives such a function the loosest register budget of
// its callers: without the attribute those functions grow to 248 VGPRs and every extended render kernel, which
// counts its callees' registers, falls to one wave per SIMD.
template <class R, class Trav, bool EXT>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(EXT ? RT_CAMX_W(R) : 1))) void k_aov(KAov<R> a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) atomicAdd(a.seg_shards, (unsigned long long)a.npix * a.spp);  // rt_counters.segments
  AovJob<R, EXT> job{a, i, gridDim.x * kBlock};
  query_loop<R, Trav>(a.sc, job);
}

// ------------------------------------------------------------------ live-slot compaction
__device__ __forceinline__ bool slot_alive(const void* Dp, int prec, uint32_t slot) {
  if (prec == RT_PREC_F32) return reinterpret_cast<const R4<float>*>(Dp)[slot].w >= 0.f;
  return reinterpret_cast<const R4<double>*>(Dp)[slot].w >= 0.0;
}

__global__ __launch_bounds__(kBlock) void k_count(const void* Dp, int prec, const uint32_t* queue, uint32_t n,
                                                  uint32_t* blk) {
  __shared__ uint32_t wc[kBlock / 64];
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool alive = false;
  if (i < n) alive = slot_alive(Dp, prec, queue ? queue[i] : i);
  unsigned long long m = __ballot(alive);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive scan of the per-block counts (one workgroup), total in *total
__global__ __launch_bounds__(1024) void k_scan(uint32_t* blk, uint32_t nb, uint32_t* total) {
  __shared__ uint32_t part[1024];
  uint32_t per = (nb + 1023) / 1024;
  uint32_t b = threadIdx.x * per, e = min(nb, b + per);
  uint32_t s = 0;
  for (uint32_t j = b; j < e; j++) s += blk[j];
  part[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - s;
  for (uint32_t j = b; j < e; j++) {
    uint32_t c = blk[j];
    blk[j] = run;
    run += c;
  }
  if (threadIdx.x == 1023) *total = part[1023];
}

__global__ __launch_bounds__(kBlock) void k_compact(const void* Dp, int prec, const uint32_t* queue, uint32_t n,
                                                    const uint32_t* blk_off, uint32_t* out) {
  __shared__ uint32_t wc[kBlock / 64];
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t slot = 0;
  bool alive = false;
  if (i < n) {
    slot = queue ? queue[i] : i;
    alive = slot_alive(Dp, prec, slot);
  }
  unsigned long long m = __ballot(alive);
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = blk_off[blockIdx.x];
  for (int w = 0; w < wave; w++) base += wc[w];
  if (alive) {
    unsigned long long below = lane ? (m & ((1ull << lane) - 1ull)) : 0ull;
    out[base + (uint32_t)__popcll(below)] = slot;
  }
}

// ------------------------------------------------------------------ resolve (camera.h:169-170)
// A render in passes (rt_plan.h ItemPlan): pass k adds its chunks to the running sums that the earlier passes left in
// `out` (first: from 0), in chunk order, and the last pass divides -- the same additions in the same order as
// one pass over every chunk, so the image does not depend on the pass split.
template <class R>
__global__ __launch_bounds__(kBlock) void k_resolve(const R* partial, uint32_t npix, uint32_t nchunks, uint32_t spp,
                                                    R* out, int first, int last) {
  uint32_t px = blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  R s0 = 0, s1 = 0, s2 = 0;
  if (!first) {
    s0 = out[3ull * px];
    s1 = out[3ull * px + 1];
    s2 = out[3ull * px + 2];
  }
  for (uint32_t c = 0; c < nchunks; c++) {
    const R* q = partial + 3ull * ((uint64_t)c * npix + px);
    s0 += q[0];
    s1 += q[1];
    s2 += q[2];
  }
  if (last) {
    R inv = R(spp);
    s0 = s0 / inv;
    s1 = s1 / inv;
    s2 = s2 / inv;
  }
  out[3ull * px] = s0;
  out[3ull * px + 1] = s1;
  out[3ull * px + 2] = s2;
}

// ------------------------------------------------------------------ adaptive sampling (rt_render_adaptive)
// The resolve of a pass over a pixel list (rt_launch.h): one thread per entry j adds the pass's batch sums, in chunk
// order and in double, to the first and second moments of the entry's pixel. The record (rt_plan.h AdaptiveAcc, one
// 64-byte line, read and written as four 16-byte words) runs on across passes and rounds, so neither the pass split
// nor the round a batch came in changes it; a pixel is one entry of one list at a time, so no atomics. Each product
// and sum is rounded on its own (no contraction), as the estimator's definition counts them.
template <class R>
__global__ __launch_bounds__(kBlock) void k_resolve_moments(const R* partial, const uint32_t* slots, uint32_t n,
                                                            uint32_t nchunks, AdaptiveAcc* acc) {
#pragma clang fp contract(off)
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  AdaptiveAcc* rec = acc + (slots ? slots[j] : j);
  AdaptiveAcc a = *rec;
  if (partial) {  // (null: a black frame's sums, which change neither S nor Q)
    for (uint32_t c = 0; c < nchunks; c++) {
      const R* q = partial + 3ull * ((uint64_t)c * n + j);
      for (int k = 0; k < 3; k++) {
        const double s = (double)q[k];
        a.S[k] += s;
        a.Q[k] += s * s;
      }
    }
  }
  a.K += nchunks;
  *rec = a;
}

// The select of a round, first step: one thread per entry computes the pixel's estimate from its record
// (adaptive_error, the host's own copy), decides whether it stops and leaves both in the record; a pixel that stops
// gets its three outputs (every pixel stops once, N >= max_spp at the latest). The block's survivors are counted by
// wave ballot and popcount, per-wave counts in LDS, as k_count counts live slots; k_scan turns the counts into offsets.
template <class R>
__global__ __launch_bounds__(kBlock) void k_adaptive_select(SelectParams p) {
  __shared__ uint32_t wc[kBlock / 64];
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  bool survives = false;
  if (j < p.n) {
    const uint32_t slot = p.slots ? p.slots[j] : j;
    AdaptiveAcc a = p.acc[slot];
    double mean[3], err;
    adaptive_error(a.K, p.batch, a.S, a.Q, p.floor, mean, &err);
    const uint32_t samples = a.K * p.batch;
    const bool stop = adaptive_stops(err, p.threshold, samples, p.max_spp);
    a.err = err;
    a.stop = stop ? 1u : 0u;
    p.acc[slot] = a;
    if (stop) {
      R* rgb = (R*)p.out_rgb + 3ull * slot;
      rgb[0] = (R)mean[0];
      rgb[1] = (R)mean[1];
      rgb[2] = (R)mean[2];
      p.out_spp[slot] = (int32_t)samples;
      p.out_err[slot] = err;
    }
    survives = !stop;
  }
  const unsigned long long m = __ballot(survives);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) p.blk[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
// ... second step: the survivors go to the next round's list at their block's offset plus their rank in the block, so
// the list keeps its order (as k_compact keeps the live slots'), whatever order the blocks run in.
__global__ __launch_bounds__(kBlock) void k_adaptive_compact(SelectParams p) {
  __shared__ uint32_t wc[kBlock / 64];
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  uint32_t slot = 0, xy = 0;
  bool survives = false;
  if (j < p.n) {
    slot = p.slots ? p.slots[j] : j;
    xy = p.pixmap[j];
    survives = p.acc[slot].stop == 0;
  }
  const unsigned long long m = __ballot(survives);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = p.blk[blockIdx.x];
  for (int w = 0; w < wave; w++) base += wc[w];
  if (survives) {
    const unsigned long long below = lane ? (m & ((1ull << lane) - 1ull)) : 0ull;
    const uint32_t at = base + (uint32_t)__popcll(below);
    p.next_pixmap[at] = xy;
    p.next_slots[at] = slot;
  }
}

template <class R>
__global__ void k_zero(R* out, uint64_t n) {
  uint64_t i = blockIdx.x * (uint64_t)kBlock + threadIdx.x;
  if (i < n) out[i] = R(0);
}

// The pixel map (tiles packed in order, row-major inside each tile, camera.h:154-158's pixel
// loop per tile) built on the device from the tile list: tl[t] = {x0, y0, width, first packed
// pixel}; pixel i belongs to the last tile whose first pixel is <= i.
__global__ __launch_bounds__(kBlock) void k_pixmap(const uint4* tl, uint32_t ntiles, uint32_t npix, uint32_t* pixmap) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= npix) return;
  uint32_t lo = 0, hi = ntiles - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (tl[mid].w <= i) lo = mid;
    else hi = mid - 1;
  }
  const uint4 t = tl[lo];
  const uint32_t k = i - t.w, y = k / t.z, x = k - y * t.z;
  pixmap[i] = (t.x + x) | (t.y + y) << 16;
}

// ====================================================================== launch selection

// Resident blocks of one kernel on one device (occupancy query x CU count), cached per (kernel,
// device): every persistent kernel has its own register budget, so one kernel's grid must not
// size another's. Guarded: contexts on different host threads launch concurrently.
std::mutex g_occ_mu;
std::map<std::tuple<const void*, int, size_t>, uint32_t> g_occ;

uint32_t resident_blocks(const void* kern, int dev, size_t lds) {
  std::lock_guard<std::mutex> lk(g_occ_mu);
  auto it = g_occ.find({kern, dev, lds});
  if (it != g_occ.end()) return it->second;
  int n = 0, b = 0;
  uint32_t r = 0;  // unknown: keep the host's grid
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kern, kBlock, lds) == hipSuccess && b > 0 && n > 0)
    r = (uint32_t)(b * n);
  g_occ[{kern, dev, lds}] = r;
  return r;
}

// lanes of the last persistent launch on this host thread (rt_counters.grid_lanes)
thread_local uint64_t t_grid_lanes = 0;

// The tag of a path kernel (rt_dev_last_kernel): its traversal policy with every template argument in order (the
// precision first, as f32 / f64; bools as 0 / 1), "camx" for the extended camera and texture form, and the schedule:
// "WideTrav<f64,0,1,1,0,1,1,0> persist", "LinearTrav<f32,1,1,1,0> camx step". Host code only. Built from the
// instantiated types, not from the plan: it is the evidence of what ran (rt_plan.h path_kernel_tag spells the plan's).
template <class R, class... A>
std::string trav_tag(const char* name, A... args) {
  std::string s = std::string(name) + (sizeof(R) == 8 ? "<f64" : "<f32");
  ((s += "," + std::to_string((int)args)), ...);
  return s + ">";
}
template <class Trav>
struct TravName;
template <class R, bool SPH, bool TRI, bool VOL, bool LLI>
struct TravName<LinearTrav<R, SPH, TRI, VOL, LLI>> {
  static std::string get() { return trav_tag<R>("LinearTrav", SPH, TRI, VOL, LLI); }
};
template <class R, bool TLDS, bool LL, bool RUNS>  // (the runs form is the LL kernel by name: rt_plan.h path_kernel_tag)
struct TravName<FlatTrav<R, TLDS, LL, RUNS>> {
  static std::string get() { return trav_tag<R>("FlatTrav", TLDS, LL); }
};
template <class R, int STACK, bool LDSN>
struct TravName<StackTrav<R, STACK, LDSN>> {
  static std::string get() { return trav_tag<R>("StackTrav", STACK, LDSN); }
};
template <class R, bool SPH, bool TRI, bool QUAD, bool MOV, bool LDSN, bool LL, bool NL>
struct TravName<WideTrav<R, SPH, TRI, QUAD, MOV, LDSN, LL, NL>> {
  static std::string get() { return trav_tag<R>("WideTrav", SPH, TRI, QUAD, MOV, LDSN, LL, NL); }
};
template <class Trav>
struct TravName<RaysOf<Trav>> {  // "... rays persist": the policy's name, then the ray source (kernel_tag)
  static std::string get() { return TravName<Trav>::get(); }
};
template <class Trav, bool CAMX>
const char* kernel_tag(bool persist) {  // built once per kernel: a wavefront render launches its kernel many times
  static const std::string form = std::string(CAMX ? " camx" : "") + (Trav::kRays ? " rays" : "");
  static const std::string tag[2] = {TravName<Trav>::get() + form + " step", TravName<Trav>::get() + form + " persist"};
  return tag[persist ? 1 : 0].c_str();
}
// tag of the last path kernel launched on this host thread
thread_local const char* t_kernel = "";
// run length of its queue's units (rt_dev_last_run): 1 for a kernel whose units are items
thread_local uint32_t t_run = 0;

template <class Trav, bool CAMX, class KernelT, class R>
void launch_one(KernelT kern, Params<R> p, uint32_t grid, hipStream_t st, size_t lds = 0) {
  t_kernel = kernel_tag<Trav, CAMX>(p.persist != 0);
  t_run = ShadeOf<Trav>::kRuns ? 1u << run_cfg_log2(p.run_cfg) : 1u;  // (from the instantiated type, as the tag)
  if (p.persist) {  // as many blocks as the chip holds resident; lanes pull items
    int dev = 0;
    const uint32_t res = hipGetDevice(&dev) == hipSuccess ? resident_blocks((const void*)kern, dev, lds) : 0;
    if (res > 0) grid = std::min<uint32_t>(grid, res);
    p.P = grid * kBlock;
    // (at most UINT32_MAX: the flat, linear and binary-BVH loops count a lane's segments in 32 bits)
    p.seg_cap = std::min<uint64_t>((uint64_t)p.n_items * p.chunk * (uint64_t)p.max_depth + 1, UINT32_MAX);
    t_grid_lanes = (uint64_t)grid * kBlock;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, p);
}

// Dynamic LDS of a wide-BVH launch: the whole tree when it fits the budget (LDSN; rt_plan.h wide_tree_in_lds), else
// the stack only.
// The fp32 kernel over a tree in HBM runs RT_WIDE_WAVES_GLOBAL blocks per CU only if that many blocks' LDS -- the
// stack entries kept in LDS, the top of the tree and the small static tables -- fit the CU's 160 KiB. A knob
// combination over it does not fail: the occupancy query quietly launches fewer blocks (the round-5 sweep's "24 /
// 21 / 6" point ran at 5 blocks per CU), so it is refused here.
static_assert(((size_t)RT_WIDE_LDS_STACK * kBlock * 4u + (size_t)RT_WIDE_TOP_N * kWTopStride + 1024u) *
                      RT_WIDE_WAVES_GLOBAL <= (160u << 10),
              "RT_WIDE_LDS_STACK / RT_WIDE_TOP_N do not fit RT_WIDE_WAVES_GLOBAL blocks per CU");
// the same for the fp64 LL kernel over a tree in HBM at RT_WIDE_WAVES_GLOBAL_F64_LL blocks per CU: its LDS stack
// entries, the fp16 top nodes and the lanes' throughput (Path LT)
static_assert(((size_t)RT_WIDE_LDS_STACK_F64 * kBlock * 4u + (size_t)RT_WIDE_TOP_N_F64 * sizeof(WNodeH) +
               3u * kBlock * sizeof(double) + 1024u) *
                      RT_WIDE_WAVES_GLOBAL_F64_LL <= (160u << 10),
              "RT_WIDE_LDS_STACK_F64 / RT_WIDE_TOP_N_F64 do not fit RT_WIDE_WAVES_GLOBAL_F64_LL blocks per CU");
static_assert(RT_WIDE_TOP_N <= kWideTopMax && RT_WIDE_TOP_N_F64 <= kWideTopMax,
              "the scene compiler orders at most kWideTopMax top nodes first");
template <class R>
inline size_t wide_lds_bytes(const DevScene<R>& sc, bool ldsn) {
  // an LDS tree: every entry in LDS, uint16; a tree in HBM: up to wide_lds_stack uint32 entries (the rest spill)
  const size_t stack = ldsn ? (size_t)sc.wide_stack * kBlock * 2u
                            : (size_t)std::min<uint32_t>(sc.wide_stack, wide_lds_stack<R>()) * kBlock * 4u;
  // fp32 rays over a tree in HBM: the copy of its first levels (RT_WIDE_TOP)
  const size_t top = (!ldsn && sizeof(R) == 4)
                         ? (size_t)std::min<uint32_t>(sc.wide_top, RT_WIDE_TOP_N) * kWTopStride
                     : (!ldsn && sizeof(R) == 8)
                         ? (size_t)std::min<uint32_t>(sc.wide_top, RT_WIDE_TOP_N_F64) * sizeof(WNodeH) : 0u;
  if (ldsn) return wide_lds_tree_bytes(sc.n_wnodes, sc.n_wprim_words, sc.wide_stack, sizeof(typename WWord<R>::T));
  return stack + top;
}
// A launch over a wide tree in HBM whose stack spills: the spill area holds spill_lanes lanes, never launch more
// (the resident grid is below it)
template <class R>
uint32_t spill_grid(const DevScene<R>& sc, uint32_t grid) {
  return sc.wide_spill ? std::min<uint32_t>(grid, sc.spill_lanes / kBlock) : grid;
}
// The wide kernel of the plan's primitive kinds and shade class, over a tree in LDS or in HBM
template <class R, class InLds, class InHbm>
void launch_wide_t(const Params<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st) {
  if (k.lds) {
    launch_one<InLds, false>(k_persist_occ<R, InLds, false>, p, grid, st, wide_lds_bytes(p.sc, true));
    return;
  }
  launch_one<InHbm, false>(k_persist_occ<R, InHbm, false>, p, spill_grid(p.sc, grid), st, wide_lds_bytes(p.sc, false));
}
template <class R, bool SPH, bool TRI, bool QUAD, bool MOV, bool LL = false, bool NL = false>
void launch_wide_k(const Params<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st) {
  using InLds = WideTrav<R, SPH, TRI, QUAD, MOV, true, LL, NL>;
  using InHbm = WideTrav<R, SPH, TRI, QUAD, MOV, false, LL, NL>;
  if (k.rays)
    launch_wide_t<R, RaysOf<InLds>, RaysOf<InHbm>>(p, k, grid, st);
  else
    launch_wide_t<R, InLds, InHbm>(p, k, grid, st);
}
// A flat, linear or binary-BVH kernel in the plan's form (base or extended) and schedule
template <class R, class Trav>
void launch_k(const Params<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st) {
  if constexpr (!Trav::kRays) {
    if (k.rays) {  // a ray batch: the same choices over the policy's RAYS form (persistent only: radiance_kernel)
      launch_k<R, RaysOf<Trav>>(p, k, grid, st);
      return;
    }
  }
  if (k.camx) {  // (the flat program has no CAMX form: path_kernel)
    if constexpr (!Trav::kFlat) {
      if (k.persist)
        launch_one<Trav, true>(k_persist_occ<R, Trav, true>, p, grid, st);
      else if constexpr (!Trav::kRays)
        launch_one<Trav, true>(k_step_occ<R, Trav, true>, p, grid, st);
    }
    return;
  }
  if (k.persist) {
    if constexpr (Trav::kWaves > 1)
      launch_one<Trav, false>(k_persist_occ<R, Trav, false>, p, grid, st);
    else
      launch_one<Trav, false>(k_persist<R, Trav, false>, p, grid, st);
  } else if constexpr (!Trav::kRays) {
    if constexpr (Trav::kWaves > 1)
      launch_one<Trav, false>(k_step_occ<R, Trav, false>, p, grid, st);
    else
      launch_one<Trav, false>(k_step<R, Trav, false>, p, grid, st);
  }
}

// One launch of a query kernel over n work items (k_trace: rays, k_aov: pixels): a block per 256 of them, at most what
// the chip holds resident of this kernel and `max_blocks`
template <class KernelT, class P>
void launch_resident(KernelT kern, const P& p, uint32_t n, uint32_t max_blocks, hipStream_t st, size_t lds) {
  int dev = 0;
  const uint32_t res = hipGetDevice(&dev) == hipSuccess ? resident_blocks((const void*)kern, dev, lds) : 0;
  uint32_t grid = std::min<uint32_t>((n + kBlock - 1) / kBlock, max_blocks);
  if (res > 0) grid = std::min(grid, res);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, p);
}

// The traversal of a query family: one instantiation per family and precision, the most general one -- every primitive
// kind (the linear program's volumes too), the deepest binary-BVH stack with its nodes in HBM, the flat program's
// records in global memory. The one list of them: launch_trace, launch_occluded and launch_aov name only their kernel.
// Calls f(TravTag of the family's policy, the most blocks a launch may have, its dynamic LDS bytes) if this build has
// the family (family_built), and nothing otherwise.
template <class Trav>
struct TravTag {
  using type = Trav;
};
template <class R, class F>
void with_query_family(const DevScene<R>& sc, TraceFamily fam, F&& f) {
  constexpr uint32_t kMaxBlocks = 1u << 14;  // (the resident grid is below it on every device so far)
  constexpr size_t kNoLds = 0;
  switch (fam) {
    case TF_FLAT:
      if constexpr (family_built(KF_FLAT)) f(TravTag<FlatTrav<R>>{}, kMaxBlocks, kNoLds);
      return;
    case TF_LINEAR:
      if constexpr (family_built(KF_LIN_ALL)) f(TravTag<LinearTrav<R, true, true, true>>{}, kMaxBlocks, kNoLds);
      return;
    case TF_WIDE_LDS:
      if constexpr (family_built(KF_WIDE))
        f(TravTag<WideTrav<R, true, true, true, true, true>>{}, kMaxBlocks, wide_lds_bytes(sc, true));
      return;
    case TF_WIDE_HBM:
      if constexpr (family_built(KF_WIDE))
        f(TravTag<WideTrav<R, true, true, true, true, false>>{}, spill_grid(sc, kMaxBlocks), wide_lds_bytes(sc, false));
      return;
    case TF_STACK:
      if constexpr (family_built(KF_STACK)) f(TravTag<StackTrav<R, kStackDepth>>{}, kMaxBlocks, kNoLds);
      return;
  }
}

}  // namespace

// ====================================================================== rt_launch.h
namespace rtd {

// The instantiation a PathKernel names, one line per policy. Nothing is decided here: which scene gets which kernel is
// path_kernel's (rt_plan.h), and the tag reported afterwards is the instantiated type's (launch_one).
template <class R>
void launch_step(const LaunchParams<R>& lp, const PathKernel& k, uint32_t grid, hipStream_t st) {
  const Params<R> p{lp};
  switch (k.fam) {
    case KF_FLAT:
      if constexpr (family_built(KF_FLAT)) {
        if (k.shade == SH_LL && p.run_cfg != 0 && kernel_takes_runs(k))  // (the host plans runs for these alone)
          launch_k<R, FlatTrav<R, true, true, true>>(p, k, grid, st);
        else if (k.shade == SH_LL)
          launch_k<R, FlatTrav<R, true, true>>(p, k, grid, st);
        else if (k.lds)
          launch_k<R, FlatTrav<R, true>>(p, k, grid, st);
        else
          launch_k<R, FlatTrav<R>>(p, k, grid, st);
      }
      return;
    case KF_LIN_QUAD:
      if constexpr (family_built(KF_LIN_QUAD)) launch_k<R, LinearTrav<R, false, false, false>>(p, k, grid, st);
      return;
    case KF_LIN_VOL:
      if constexpr (family_built(KF_LIN_VOL)) {
        if (k.shade == SH_LLI)
          launch_k<R, LinearTrav<R, false, false, true, true>>(p, k, grid, st);
        else
          launch_k<R, LinearTrav<R, false, false, true>>(p, k, grid, st);
      }
      return;
    case KF_LIN_SPH:
      if constexpr (family_built(KF_LIN_SPH)) launch_k<R, LinearTrav<R, true, false, false>>(p, k, grid, st);
      return;
    case KF_LIN_ALL:
      if constexpr (family_built(KF_LIN_ALL)) launch_k<R, LinearTrav<R, true, true, true>>(p, k, grid, st);
      return;
    case KF_WIDE:
      if constexpr (family_built(KF_WIDE)) {
        if (k.kinds == WK_SPHERE && k.shade == SH_NL)
          launch_wide_k<R, true, false, false, false, false, true>(p, k, grid, st);
        else if (k.kinds == WK_SPHERE)
          launch_wide_k<R, true, false, false, false>(p, k, grid, st);
        else if (k.kinds == WK_TRI)
          launch_wide_k<R, false, true, false, false>(p, k, grid, st);
        else if (k.kinds == (WK_TRI | WK_QUAD) && k.shade == SH_LL)
          launch_wide_k<R, false, true, true, false, true>(p, k, grid, st);
        else if (k.kinds == (WK_TRI | WK_QUAD))
          launch_wide_k<R, false, true, true, false>(p, k, grid, st);
        else
          launch_wide_k<R, true, true, true, true>(p, k, grid, st);
      }
      return;
    case KF_STACK:
      if constexpr (family_built(KF_STACK)) {
        if constexpr (sizeof(R) == 4) {  // nodes in LDS: fp32 only
          if (k.lds) {
            launch_k<R, StackTrav<R, kStackMid, true>>(p, k, grid, st);
            return;
          }
        }
        if (k.stack == kStackSmall)
          launch_k<R, StackTrav<R, kStackSmall>>(p, k, grid, st);
        else if (k.stack == kStackMid)
          launch_k<R, StackTrav<R, kStackMid>>(p, k, grid, st);
        else
          launch_k<R, StackTrav<R, kStackDepth>>(p, k, grid, st);
      }
      return;
  }
}

uint64_t last_grid_lanes() { return t_grid_lanes; }
const char* last_kernel() { return t_kernel; }
uint32_t last_run() { return t_run; }

// The three query launches: with_query_family's traversal of `fam`, each in its own kernel.
template <class R>
void launch_trace(const TraceParams<R>& tp, TraceFamily fam, hipStream_t st) {
  const KTrace<R> p{tp};
  with_query_family(p.sc, fam, [&](auto trav, uint32_t max_blocks, size_t lds) {
    launch_resident(k_trace<R, typename decltype(trav)::type>, p, p.n, max_blocks, st, lds);
  });
}

// Occlusion queries: the any-hit form, or the closest-hit form of the families occlusion_early_exit can refuse
// (Trav::kClosestOccl: decided per policy at compile time, so the others have no such kernel)
template <class R>
void launch_occluded(const OcclParams<R>& op, TraceFamily fam, bool early, hipStream_t st) {
  const KOccl<R> p{op};
  with_query_family(p.sc, fam, [&](auto trav, uint32_t max_blocks, size_t lds) {
    using Trav = typename decltype(trav)::type;
    if (early || !Trav::kClosestOccl)
      launch_resident(k_occluded<R, Trav, true>, p, p.n, max_blocks, st, lds);
    else if constexpr (Trav::kClosestOccl)
      launch_resident(k_occluded<R, Trav, false>, p, p.n, max_blocks, st, lds);
  });
}

// The feature-buffer pass: a lane per pixel, each traversal in its base and its extended form (rt_plan.h aov_extended)
template <class R>
void launch_aov(const AovParams<R>& ap, TraceFamily fam, hipStream_t st) {
  const KAov<R> p{ap};
  with_query_family(p.sc, fam, [&](auto trav, uint32_t max_blocks, size_t lds) {
    using Trav = typename decltype(trav)::type;
    if (p.ext)
      launch_resident(k_aov<R, Trav, true>, p, p.npix, max_blocks, st, lds);
    else
      launch_resident(k_aov<R, Trav, false>, p, p.npix, max_blocks, st, lds);
  });
}
void launch_camera_rays(const CamRayParams& p, hipStream_t st) {
  const uint32_t n = p.npix * p.spp;
  hipLaunchKernelGGL(k_camera_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, p);
}

template <class R>
void launch_init(const LaunchParams<R>& lp, const PathKernel& k, uint32_t blocks, hipStream_t st) {
  const Params<R> p{lp};
  if (k.camx)
    hipLaunchKernelGGL((k_init<R, true>), dim3(blocks), dim3(kBlock), 0, st, p);
  else
    hipLaunchKernelGGL((k_init<R, false>), dim3(blocks), dim3(kBlock), 0, st, p);
}
void launch_count(const void* D, int f64, const uint32_t* queue, uint32_t n, uint32_t* blk, uint32_t* total,
                  hipStream_t st) {
  const uint32_t nb = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(kBlock), 0, st, D, f64, queue, n, blk);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, blk, nb, total);
}
void launch_compact(const void* D, int f64, const uint32_t* queue, uint32_t n, const uint32_t* blk_off, uint32_t* out,
                    hipStream_t st) {
  hipLaunchKernelGGL(k_compact, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, D, f64, queue, n, blk_off, out);
}
template <class R>
void launch_resolve(const R* partial, uint32_t npix, uint32_t nchunks, uint32_t spp, R* out, bool first, bool last,
                    hipStream_t st) {
  hipLaunchKernelGGL(k_resolve<R>, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, partial, npix, nchunks, spp,
                     out, (int)first, (int)last);
}
template <class R>
void launch_resolve_moments(const R* partial, const uint32_t* slots, uint32_t n, uint32_t nchunks, AdaptiveAcc* acc,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_resolve_moments<R>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, partial, slots, n,
                     nchunks, acc);
}
template <class R>
void launch_adaptive_select(const SelectParams& p, hipStream_t st) {
  const uint32_t nb = (p.n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_adaptive_select<R>, dim3(nb), dim3(kBlock), 0, st, p);
  if (!p.next_pixmap) return;  // the last round: every pixel has stopped
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, p.blk, nb, p.blk + nb + 1);
  hipLaunchKernelGGL(k_adaptive_compact, dim3(nb), dim3(kBlock), 0, st, p);
}
template <class R>
void launch_zero(R* out, uint64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_zero<R>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, out, n);
}
void launch_pixmap(const uint4* tiles, uint32_t ntiles, uint32_t npix, uint32_t* pixmap, hipStream_t st) {
  hipLaunchKernelGGL(k_pixmap, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, tiles, ntiles, npix, pixmap);
}

#define RT_INSTANTIATE(R)                                                                                        \
  template void launch_zero<R>(R*, uint64_t, hipStream_t);                                                       \
  template void launch_step<R>(const LaunchParams<R>&, const PathKernel&, uint32_t, hipStream_t);                \
  template void launch_init<R>(const LaunchParams<R>&, const PathKernel&, uint32_t, hipStream_t);                \
  template void launch_trace<R>(const TraceParams<R>&, TraceFamily, hipStream_t);                                \
  template void launch_aov<R>(const AovParams<R>&, TraceFamily, hipStream_t);                                    \
  template void launch_occluded<R>(const OcclParams<R>&, TraceFamily, bool, hipStream_t);                        \
  template void launch_resolve<R>(const R*, uint32_t, uint32_t, uint32_t, R*, bool, bool, hipStream_t);          \
  template void launch_resolve_moments<R>(const R*, const uint32_t*, uint32_t, uint32_t, AdaptiveAcc*, hipStream_t); \
  template void launch_adaptive_select<R>(const SelectParams&, hipStream_t);
RT_INSTANTIATE(double)
RT_INSTANTIATE(float)
#undef RT_INSTANTIATE

// g_sincos_tab (rt_device.h sincos2pi, fp64): (sin, cos)(2 pi j / 1024) in long double, rounded once,
// copied to the device of the calling thread (every context's device; module globals are per device)
hipError_t upload_sincos_table() {
  static double2 tab[kSinCosTab];
  static std::once_flag once;
  std::call_once(once, [] {
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int j = 0; j < kSinCosTab; j++) {
      const long double a = 2.0L * pi * (long double)j / (long double)kSinCosTab;
      tab[j] = make_double2((double)sinl(a), (double)cosl(a));
    }
  });
  return hipMemcpyToSymbol(HIP_SYMBOL(g_sincos_tab), tab, sizeof(tab));
}

}  // namespace rtd

// ====================================================================== development entry points
extern "C" {

#ifdef RT_ITEM_CLOCKS
// development build only (scripts/dev_item_clocks.py): where the persistent kernels write item durations
int rt_dev_set_item_clocks(void* dev_ptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_item_clk), &dev_ptr, sizeof(void*)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef RT_SECTION_CLOCKS
// development build only (scripts/dev_sections.py): read and clear the section clocks
int rt_dev_section_clocks(unsigned long long out[7]) {
  const unsigned long long z[4] = {0, 0, 0, 0};
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_section_clocks), sizeof(unsigned long long) * 4);
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out + 4, HIP_SYMBOL(rtd::g_trace_totals), sizeof(unsigned long long) * 3);
  // each symbol is cleared with its own size (g_section_clocks: 4 entries, g_trace_totals: 3)
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_section_clocks), z, sizeof(unsigned long long) * 4);
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_trace_totals), z, sizeof(unsigned long long) * 3);
  return e == hipSuccess ? 0 : -1;
}
// the wide kernels' wave-level counts (rt_device.h g_wide_stats), read and cleared
void rt_dev_wide_stats(unsigned long long out[10]) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_wide_stats), sizeof(unsigned long long) * 10);
  unsigned long long z[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_wide_stats), z, sizeof(z));
}
#endif
// The tag of the last path kernel launch_step launched on the calling host thread (kernel_tag above), "" before the
// first; copied into buf[0, n) and always terminated. Host only; for tests and scripts, not in rt_hip.h.
void rt_dev_last_kernel(char* buf, size_t n) {
  if (!buf || n == 0) return;
  std::snprintf(buf, n, "%s", rtd::last_kernel());
}
// The run length of the units that kernel's queue handed out (rt_plan.h RunPlan): L where launch_step took the runs
// form of a kernel, 1 where the units were items, 0 before the first launch. For tests and scripts, not in rt_hip.h.
uint32_t rt_dev_last_run(void) { return rtd::last_run(); }

}  // extern "C"
