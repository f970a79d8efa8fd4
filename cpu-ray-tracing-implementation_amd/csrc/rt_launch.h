// rt_launch.h -- what the host code (rt_render.hip) needs to call the kernels (rt_kernels.hip): the launch
// parameters, the constants both sides size things by, and one launch function per kernel. Internal to
// librt_hip.so: nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_plan.h"
#include "rt_temporal.h"
#include "rt_types.h"

namespace rtd __attribute__((visibility("hidden"))) {

// (kBlock, the lanes of a block: rt_plan.h)
constexpr int kSegShards = 256;  // segment counter shards
// persistent schedule: items are handed out in batches; batch j of head h is batch j * kHeads + h of the
// item space, so the heads interleave over the frame and a head that runs dry steals from the others
constexpr uint32_t kHeads = 8;
constexpr uint32_t kHeadStride = 64;  // 256 B apart: one L2 line per head

template <class R>
struct alignas(4 * sizeof(R)) R4 {
  R x, y, z, w;
};

// Path state in HBM (wavefront schedule), one entry per slot, structure of arrays of 16-byte (fp32)
// or 32-byte (fp64) records so every access is a coalesced dwordx4:
//   O  origin, ray time            D  direction, bounce (-1: slot retired)
//   T  throughput                  L  radiance of the running sample
//   A  running sum of the item     S  key_pixel, key of the running sample, item, sample
//   X  the surface the ray leaves (entry, instance): self-intersection exclusion;
//      the pixel (x | y << 16) and the end of the sample range of the slot's item
template <class R>
struct LaunchParams {
  DevScene<R> sc;
  R4<R>* O;
  R4<R>* D;
  R4<R>* T;
  R4<R>* L;
  R4<R>* A;
  uint4* S;
  uint4* X;
  R* partial;              // per item: 3 sums
  const uint32_t* pixmap;  // local pixel -> its image position x | y << 16
  const uint32_t* queue;   // live slots, or null = slots [0, n)
  uint32_t n;
  uint32_t P, npix, n_items, chunk, spp, first_sample, W;
  // two item sizes: chunks [0, k_bulk) hold `chunk` samples, the later ones (the frame's last
  // items in dequeue order) `tail_chunk` <= chunk samples each (rt_plan.h ItemPlan)
  uint32_t k_bulk, tail_chunk;
  // the render's chunks come in passes (the partial sums of one pass fit a memory budget): this
  // launch's items are chunks [chunk0, chunk0 + n_items / npix) of every pixel
  uint32_t chunk0;
  // what the wave queue hands out (rt_plan.h RunPlan; read by the kernels that take runs alone, FlatTrav::kItemRuns):
  // the pass's units, n_items where the run length is 1. (This word and run_cfg below sit where the struct had
  // padding, so every other field keeps its place and the kernarg segment its size.)
  uint32_t n_units;
  uint64_t npix_m;  // item / npix = (item * npix_m) >> npix_k for every item < 2^31 (div_magic)
  uint32_t npix_k;
  int32_t max_depth;
  uint64_t seed;
  // camera rays are built in fp64 for both paths (fp32 rounds once), from CamDev in device
  // memory (scalar loads at the point of use)
  int32_t cam_mode;
  const CamDev* camx;
  unsigned long long* seg_shards;
  int32_t K;  // segments per launch
  // kPersist: the persistent schedule (k_persist), one launch whose grid is what the chip holds resident and
  // whose lanes pull items from the per-XCD heads. 0: the wavefront schedule (k_init, k_step), slot s owns
  // items s, s + P, ...
  int32_t persist;
  uint32_t* heads;  // kHeads dequeue counters, kHeadStride words apart (persistent schedule)
  uint64_t seg_cap;  // a lane never needs more segments than this (its items * chunk * max_depth)
  uint32_t* fault;   // set when a lane hits seg_cap (internal error, reported by the host)
  // A ray batch (rt_radiance; PathKernel::rays): the lanes' first segments are caller-given rays instead of camera
  // rays. rays: [npix][8] doubles o, d, time, tmax as TraceParams' (16-byte aligned); the batch is laid out as an
  // image W wide whose pixel y * W + x is ray y * W + x, keyed as pixel ray_base + y * W + x. Last in the struct: the
  // camera kernels read neither, and every field they read keeps its place in the kernarg segment.
  const double* rays;
  uint32_t ray_base;
  uint32_t run_cfg;  // rt_plan.h run_cfg_pack of the pass's RunPlan; 0: every unit is an item
};
constexpr int32_t kPersist = 2;

// RT_DEV_ONLY (development builds for register/spill iteration, scripts/kernel_usage.py): instantiate one
// kernel family only -- 1 the flat program, 2 the wide BVH, 3 the quad + volume linear program. 0:
// everything. A render (and rt_scene_check) that needs a family such a build omits fails with
// RT_ERR_UNSUPPORTED instead of launching nothing.
#ifndef RT_DEV_ONLY
#define RT_DEV_ONLY 0
#endif
constexpr bool family_built(KernelFamily f) {
  return RT_DEV_ONLY == 0 || (RT_DEV_ONLY == 1 && f == KF_FLAT) || (RT_DEV_ONLY == 2 && f == KF_WIDE) ||
         (RT_DEV_ONLY == 3 && f == KF_LIN_VOL);
}

// Waves per SIMD of the fp32 wide-BVH kernel over a tree in HBM (WideTrav::kWaves; here because rt_build_info
// reports it): 32-bit stack in LDS (C4 stand-in: 4 waves 519 ms, 5: 462; with the speculative traversal 5: 424,
// 6: 412.5 -- 7 blocks of 24 KB stacks do not fit the 160 KB LDS)
#ifndef RT_WIDE_WAVES_GLOBAL
#define RT_WIDE_WAVES_GLOBAL 8  // round 5, with 12 LDS stack entries and 55 top nodes in LDS (wide_lds_stack)
#endif

// One launch of the render's path kernel, the one `k` names (rt_plan.h path_kernel, of the header and the precision
// p.sc was made from): `grid` blocks at most (the persistent schedule cuts it to the resident blocks, a spilling wide
// tree to its spill area). Defined for float and double.
template <class R>
void launch_step(const LaunchParams<R>& p, const PathKernel& k, uint32_t grid, hipStream_t st);
uint64_t last_grid_lanes();  // lanes of the last persistent launch_step on this host thread
uint32_t last_run();         // run length of the units that launch's queue handed out (1: items; 0 before the first)
const char* last_kernel();   // tag of the kernel the last launch_step on this host thread launched ("" before the first)

// wavefront schedule: the first camera ray of every slot (in k's form, base or extended); live-slot count and compaction
template <class R>
void launch_init(const LaunchParams<R>& p, const PathKernel& k, uint32_t blocks, hipStream_t st);
void launch_count(const void* D, int f64, const uint32_t* queue, uint32_t n, uint32_t* blk, uint32_t* total,
                  hipStream_t st);  // k_count + k_scan: blk = exclusive block offsets, *total = live slots
void launch_compact(const void* D, int f64, const uint32_t* queue, uint32_t n, const uint32_t* blk_off, uint32_t* out,
                    hipStream_t st);

template <class R>
void launch_resolve(const R* partial, uint32_t npix, uint32_t nchunks, uint32_t spp, R* out, bool first, bool last,
                    hipStream_t st);
template <class R>
void launch_zero(R* out, uint64_t n, hipStream_t st);
void launch_pixmap(const uint4* tiles, uint32_t ntiles, uint32_t npix, uint32_t* pixmap, hipStream_t st);

// ---- adaptive sampling (rt_render_adaptive): a round's pixels are a list, entry j = (pixmap[j], the pixel's position
// slots[j] in the call's packed outputs and accumulator records; slots null: j itself, the first round's full list).
// The resolve of a pass over a pixel list: adds the pass's nchunks batch sums of entry j, partial[3 * (c * n + j)] in
// chunk order, to the record acc[slot of j] (k_resolve_moments). partial null: the sums are zero (max_depth = 0).
template <class R>
void launch_resolve_moments(const R* partial, const uint32_t* slots, uint32_t n, uint32_t nchunks, AdaptiveAcc* acc,
                            hipStream_t st);
// What the select of a round needs: the round's list, the next round's, the outputs and the stopping rule.
struct SelectParams {
  AdaptiveAcc* acc;
  const uint32_t* pixmap;  // the round's list, n entries
  const uint32_t* slots;   // (null: the identity)
  uint32_t n;
  uint32_t* next_pixmap;   // the survivors, in the list's order (null: the last round, nobody survives)
  uint32_t* next_slots;
  uint32_t* blk;           // ceil(n / kBlock) + 2 words: the blocks' survivor counts, then offsets; the total last
  void* out_rgb;           // 3 R a pixel
  int32_t* out_spp;
  double* out_err;
  uint32_t batch, max_spp;
  double threshold, floor;
};
// k_adaptive_select in its two steps with k_scan between them: every entry's estimate, decision and -- for a pixel
// that stops -- outputs, and the blocks' survivor counts; then the survivors compacted in order into the next list.
// The survivor count ends up in p.blk[ceil(n / kBlock) + 1].
template <class R>
void launch_adaptive_select(const SelectParams& p, hipStream_t st);

// ---- ray queries (rt_trace_rays): the argument of k_trace. Its own struct: LaunchParams and DevScene are the render
// kernels' kernarg, whose SGPR budget is tuned (reload_params), so what only a query needs lives here.
//   rays  [n][8] doubles  o, d, time, tmax           (64 B a ray, read as four 16-byte loads)
//   geom  [n][7] doubles  t, p, n                    ids  [n][4] int32  object, material, kind, front
//   idtab (object, material) of the descriptor per device record, the quads' entries first, then the spheres',
//         triangles' and volumes' from id_off[1], [2], [3] (CompiledScene::ids)
template <class R>
struct TraceParams {
  DevScene<R> sc;  // cam64 = nullptr: a near-edge quad re-decision (quad_edge64) takes the given ray
  const double* rays;
  double* geom;
  int32_t* ids;
  const int2* idtab;
  uint32_t id_off[4];
  uint32_t n;
  uint64_t seed;
  unsigned long long* seg_shards;  // [0] += n (rt_counters.segments)
};
// One query launch of family `fam` (built: family_built(trace_render_family(fam))); the grid is what the chip
// holds resident at most (and what the wide spill area holds), the lanes stride over the rays. The traversal of each
// family, the block cap and the LDS bytes of this launch, launch_occluded and launch_aov are listed once, in
// with_query_family (rt_kernels.hip).
template <class R>
void launch_trace(const TraceParams<R>& p, TraceFamily fam, hipStream_t st);

// ---- occlusion queries (rt_occluded): the argument of k_occluded, rays as TraceParams'.
//   out  [n] bytes  1: world.hit(r, interval(0.001, tmax)) is true, 0: it is not
template <class R>
struct OcclParams {
  DevScene<R> sc;  // cam64 = nullptr, as a query's
  const double* rays;
  uint8_t* out;
  uint32_t n;
  uint64_t seed;
  unsigned long long* seg_shards;  // [0] += n (rt_counters.segments)
};
// One occlusion launch of family `fam`: with_query_family's traversal, block cap and LDS bytes, as launch_trace. early:
// what occlusion_early_exit (rt_plan.h) says of the scene: the any-hit kernel, else the closest-hit traversal with
// k_trace's draws (only the policies with kClosestOccl, the linear program and the binary BVH, have that second form;
// the others ignore `early`).
template <class R>
void launch_occluded(const OcclParams<R>& p, TraceFamily fam, bool early, hipStream_t st);

// ---- feature buffers (rt_render_aov) and camera rays (rt_camera_rays). Their own kernargs, for the reason above.
//   pixmap  local pixel -> x | y << 16 (launch_pixmap), camx the camera view (make_view) in device memory
//   feat  [npix][8] doubles  albedo, normal, depth, hit: the means over the pixel's samples (four 16-byte stores)
//   ids   [npix][4] int32    object, material, kind, front of sample first_sample
template <class R>
struct AovParams {
  DevScene<R> sc;  // cam64 = nullptr, as a query's: the lane's ray is the fp64 camera ray rounded once
  const uint32_t* pixmap;
  const CamDev* camx;
  double* feat;
  int32_t* ids;
  const int2* idtab;
  uint32_t id_off[4];
  uint32_t npix, spp, first_sample, W;
  int32_t cam_mode;
  int32_t ext;  // aov_extended (rt_plan.h): the kernel form with every camera model and texture kind
  uint64_t seed;
  unsigned long long* seg_shards;  // [0] += npix * spp
};
// One feature-buffer launch of family `fam` (aov_family; built: family_built(trace_render_family(fam))): a lane per
// pixel, striding over the pixels when the chip (or the wide spill area) holds fewer lanes. with_query_family's
// traversal, block cap and LDS bytes, as launch_trace; p.ext chooses between the kernel's two forms.
template <class R>
void launch_aov(const AovParams<R>& p, TraceFamily fam, hipStream_t st);

//   rays  [npix * spp][8] doubles  o, d, time, +inf: row pix * spp + s is sample first_sample + s of pixel pix
struct CamRayParams {
  const uint32_t* pixmap;
  const CamDev* camx;
  double* rays;
  uint32_t npix, spp, first_sample, W;  // npix * spp < 2^31
  int32_t cam_mode;
  uint64_t seed;
};
void launch_camera_rays(const CamRayParams& p, hipStream_t st);

// ---- denoising (rt_denoise; the kernels are rt_denoise.hip's): the prepare pass and prm.iterations a-trous passes on
// `st`, iterations + 1 launches. scratch: kDnScratchT T a pixel; the other pointers as rt_denoise takes them, on the
// device (var may be null, rgb_out may be rgb_in).
template <class T>
void launch_denoise(const rt_denoise_params& prm, const T* rgb_in, const double* feat, const double* var, T* scratch,
                    T* rgb_out, hipStream_t st);

// ---- temporal accumulation (rt_temporal; the kernel is rt_temporal.hip's): one launch on `st`. Checked parameters and
// cameras; the pointers as rt_temporal takes them, on the device (ids, var, hist_in and var_out may be null, rgb_out
// may be rgb_in and var_out var).
template <class T>
void launch_temporal(const rt_temporal_params& prm, const rt_camera_desc* cam, const rt_camera_desc* prev,
                     const T* rgb_in, const double* feat, const int32_t* ids, const double* var, const void* hist_in,
                     void* hist_out, T* rgb_out, double* var_out, hipStream_t st);

// the fp64 sin/cos table (rt_device.h g_sincos_tab) copied to the calling thread's device
hipError_t upload_sincos_table();

}  // namespace rtd
