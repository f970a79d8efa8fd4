// rt_types.h -- the plain structs and constants the host code and the kernels share: the vector
// type, the counter RNG's key functions, the camera and scene views a launch carries. No device
// symbol is defined here, so any translation unit may include it (rt_device.h defines some).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_scene.h"

namespace rtd {

template <class R>
struct V {
  R x, y, z;
};

// ------------------------------------------------------------------ counter RNG
// 32-bit draw for (seed, pixel, sample, dim); identical to the oracle's
// (oracle/oracle.cpp) and to rt_rng_u32 on the host.
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0xd35a2d97u;
  x ^= x >> 15;
  return x;
}
__host__ __device__ __forceinline__ uint32_t key_pixel(uint64_t seed, uint32_t pixel) {
  return mix32(pixel ^ mix32((uint32_t)seed ^ 0x9E3779B9u));
}
__host__ __device__ __forceinline__ uint32_t key_sample(uint64_t seed, uint32_t sample) {
  return mix32(sample + mix32((uint32_t)(seed >> 32) + 0x7F4A7C15u));
}
// the key of one camera sample; each draw is then a single mix (two 32-bit multiplies)
__host__ __device__ __forceinline__ uint32_t key_path(uint32_t ka, uint32_t kb) { return mix32(ka ^ kb); }
__host__ __device__ __forceinline__ uint32_t draw_u32(uint32_t ks, uint32_t dim) {
  return mix32(ks + dim * 0x9E3779B9u);
}

// ------------------------------------------------------------------ scene view
// A word of the wide BVH's primitive stream (rt_scene.h WNode): 16 bytes of floats in the fp32
// blob, 32 bytes of doubles in the fp64 one (same word indices, so the leaf codes are shared); the
// primitive's entry is in the bits of w (the low 32 bits of the double).
template <class R>
struct WWord;
template <>
struct WWord<float> {
  using T = float4;
};
struct alignas(32) double4w {
  double x, y, z, w;
};
template <>
struct WWord<double> {
  using T = double4w;
};

// The camera as camera::render/generate_ray use it (camera.h:137-141, 244-290), in double.
struct CamDev {
  int32_t mode;  // rt_camera_mode
  int32_t pad;
  V<double> pos, du, dv;
  V<double> dir00;   // perspective / fisheye: f dir - vw/2 right + vh/2 up + (du + dv)/2 (camera.h:246, 260)
  V<double> pos00;   // orthonormal / lens: pos - vw/2 right + vh/2 up + (du + dv)/2 (camera.h:253, 278)
  V<double> dir;     // dir_, unit
  V<double> fdir;    // focus_dist_ * dir_ (camera.h:279)
  V<double> disk_u, disk_v;  // defocus_disk_u/v (camera.h:129-131)
  double focal;      // focal_length_ (camera.h:266)
};

template <class R>
struct DevScene {
  const Quad<R>* quads;
  const Sphere<R>* spheres;
  const Tri<R>* tris;
  const Instance<R>* insts;
  const Volume<R>* vols;
  const Node<R>* nodes;
  const uint32_t* refs;
  const Material<R>* mats;
  const Texture<R>* texs;
  const Light<R>* light;
  const LinRec<R>* lin;  // linear program (n_linear > 0)
  uint32_t n_linear;
  const FlatQuadT<R>* flatq;  // flat program (has_flat): quads grouped by plane axis, then boxes
  const FlatBoxT<R>* flatb;
  uint32_t n_flatq[3], n_flatb;
  uint32_t n_mats;
  int32_t has_flat;
  uint32_t root;
  int32_t background;
  int32_t has_volumes;
  uint32_t n_nodes;
  const double* texdata;  // procedural-texture tables (Texture::data)
  const uint8_t* images;  // picture-texture pixels (Texture::data)
  int32_t has_procedural; // any perlin / value / worley / voronoi texture: the EXT kernels
  uint32_t n_flatr;       // flat program: rooms, stored directly after the boxes (flat_rooms)
  // wide BVH (rt_scene.h WNode; float boxes in both blobs): nodes, primitive words, root code,
  // stack need, WK_* kinds
  const WNode* wnodes;
  const typename WWord<R>::T* wprims;
  uint32_t n_wnodes, n_wprim_words, wroot, wide_stack, wide_kinds;
  int32_t has_wide;
  uint32_t wide_big;  // primitives at the head of the word stream, tested before the tree
  uint32_t wide_top;  // nodes [0, wide_top): the tree's first levels (HBM trees: read from an LDS copy)
  const WNodeH* wnodesh;  // the fp16 form of the tree (rt_scene.h WNodeH; 0: none)
  const Quad<double>* quads64;  // fp32 scenes: the fp64 quads (quad_t_near; 0: none)
  // the render's camera when it is perspective (0: another model): near-edge quad hits of camera rays are re-decided
  // on the fp64 camera ray (quad_edge64)
  const CamDev* cam64;
  // a tree in HBM keeps at most wide_lds_stack<R>() stack entries per lane in LDS; deeper entries go to
  // wide_spill[(depth - wide_lds_stack<R>()) * spill_lanes + lane]
  uint32_t* wide_spill;
  uint32_t spill_lanes;
};
// The flat program's room records follow its boxes in the blob (no pointer of their own: the view keeps its size
// and the offsets of every other field, so kernels that use no flat program compile to the same code).
template <class R>
__host__ __device__ __forceinline__ const FlatRoomT<R>* flat_rooms(const DevScene<R>& sc) {
  return reinterpret_cast<const FlatRoomT<R>*>(sc.flatb + sc.n_flatb);
}
// Trees in HBM: the tree's first levels are read from an LDS copy (trace_wide), at most this many nodes
// (the builder orders up to kWideTopMax breadth-first); fp64 rays read them in the fp16 form (WNodeH)
#ifndef RT_WIDE_TOP_N
#define RT_WIDE_TOP_N 55
#endif
#ifndef RT_WIDE_TOP_N_F64
#define RT_WIDE_TOP_N_F64 85
#endif
#ifndef RT_WIDE_LDS_STACK
#define RT_WIDE_LDS_STACK 12
#endif
#ifndef RT_WIDE_LDS_STACK_F64  // 18 since round 6: the fp64 LL kernel's LDS also holds the throughput (Path LT)
#define RT_WIDE_LDS_STACK_F64 18
#endif
// stack entries per lane kept in LDS for a tree in HBM, by ray precision (fp32: fewer, so the LDS also holds
// the top of the tree and 8 blocks fit a CU; C4 fp32, stack / top nodes / waves: 24 / 0 / 6 309.4 ms/frame,
// 22 / 21 / 6 290.1, 16 / 47 / 7 268.8, 14 / 63 / 7 268.1, 12 / 55 / 8 265.2; r05r-r05u)
template <class R>
constexpr uint32_t wide_lds_stack() {
  return sizeof(R) == 4 ? RT_WIDE_LDS_STACK : RT_WIDE_LDS_STACK_F64;
}

// the fp64 sin/cos table's entries (rt_device.h sincos2pi; filled by upload_sincos_table)
constexpr int kSinCosTab = 1024;

}  // namespace rtd
