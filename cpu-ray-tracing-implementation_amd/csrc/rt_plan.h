// rt_plan.h -- the host's decisions about a render, as pure functions of the compiled scene's header and the
// call's sizes: which kernel family it takes and which path kernel of that family (path_kernel; which traversal a ray
// query takes, whether a wide tree lives in LDS), and how its samples are cut into work items and passes. No
// HIP and no environment access, so the decisions are testable without a GPU (tests/test_plan.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "../../include/rt_hip.h"
#include "rt_scene.h"

namespace rtd {

// Division by a launch constant d >= 1 as a multiply (Granlund-Montgomery): with
// k = 32 + ceil(log2 d) and m = floor(2^k / d) + 1, (n * m) >> k == n / d for every n < 2^31
// (m d - 2^k <= d, so the error n (m d - 2^k) / 2^k stays below 1/d; n m < 2^64).
inline void div_magic(uint32_t d, uint64_t& m, uint32_t& k) {
  uint32_t l = 0;
  while ((1ull << l) < d) l++;
  k = 32 + l;
  m = (uint64_t)((((unsigned __int128)1) << k) / d) + 1;
}

// Whether a render needs its kernels' extended form (CAMX: k_init, the linear program's and the binary BVH's path
// kernels): a camera model other than the perspective one, or a procedural or picture texture. The flat program and
// the wide tree have no such form: kernel_family keeps an extended render off them.
inline bool extended_form(const SceneHeader& h, int32_t cam_mode) {
  return cam_mode != RT_CAM_PERSPECTIVE || h.n_texdata > 0 || h.has_cell_noise;
}

// The kernel family a render takes, decided from the compiled scene, the camera model, the schedule and the
// traversal order (path_kernel chooses the kernel within it).
enum KernelFamily { KF_FLAT, KF_LIN_QUAD, KF_LIN_VOL, KF_LIN_SPH, KF_LIN_ALL, KF_WIDE, KF_STACK };
inline KernelFamily kernel_family(const SceneHeader& h, int32_t cam_mode, bool persist, bool ordered) {
  const bool ext = extended_form(h, cam_mode);
  const bool sph = h.n_spheres > 0, tri = h.n_tris > 0, vol = h.has_volumes != 0;
  // the flat program (world-space quads and boxes, fp32 and fp64); the extended kernels keep the linear one
  if (!ordered && h.has_flat && !ext) return KF_FLAT;
  if (h.n_linear > 0) {
    if (!sph && !tri) return vol ? KF_LIN_VOL : KF_LIN_QUAD;
    return (sph && !tri && !vol) ? KF_LIN_SPH : KF_LIN_ALL;
  }
  // the wide BVH (persistent schedule, base kernels; fp64 rays since round 3)
  if (!ordered && h.has_wide && persist && !ext) return KF_WIDE;
  return KF_STACK;
}
// Lanes of a block of every path and query kernel (the LDS sizes below count per-lane stack entries by it).
constexpr int kBlock = 256;

// Whether a wide-BVH launch keeps the whole tree in the block's LDS (else: the tree in HBM, the stack and the top
// of the tree in LDS). The one home of that decision: path_kernel and trace_family ask here.
// word_bytes: a primitive word of the blob the rays read, 16 (fp32) or 32 (fp64).
constexpr size_t kWideLdsBudget = 40u << 10;  // bytes per 256-lane block: 4 blocks per CU of 160 KiB
inline size_t wide_lds_tree_bytes(uint32_t n_wnodes, uint32_t n_wprim_words, uint32_t wide_stack, size_t word_bytes) {
  // nodes at their LDS stride, the primitive words, and every stack entry of every lane as uint16
  return (size_t)n_wnodes * kWNodeLdsStride + (size_t)n_wprim_words * word_bytes + (size_t)wide_stack * kBlock * 2u;
}
inline bool wide_tree_in_lds(uint32_t n_wnodes, uint32_t n_wprim_words, uint32_t wide_stack, size_t word_bytes) {
  // LDS-resident trees use 16-bit child codes (wide_code16): node offset (index x 9) < 2^15, first word < 2^12
  return wide_lds_tree_bytes(n_wnodes, n_wprim_words, wide_stack, word_bytes) <= kWideLdsBudget &&
         n_wnodes * kWNodeLdsUnits < 0x8000u && n_wprim_words <= 0x1000u;
}

// The traversal a ray query (rt_trace_rays) takes: kernel_family without the conditions that concern shading alone
// (the camera model, procedural textures, the schedule), and with the wide tree's LDS / HBM split, which is a
// different kernel. The values are rt_trace_family_kind's. h: the header of the blob the rays read (hdr or hdr64).
enum TraceFamily { TF_FLAT = 0, TF_LINEAR = 1, TF_WIDE_LDS = 2, TF_WIDE_HBM = 3, TF_STACK = 4 };
inline TraceFamily trace_family(const SceneHeader& h, bool ordered, size_t word_bytes) {
  if (!ordered && h.has_flat) return TF_FLAT;
  if (h.n_linear > 0) return TF_LINEAR;
  if (!ordered && h.has_wide)
    return wide_tree_in_lds(h.n_wnodes, h.n_wprim_words, h.wide_stack, word_bytes) ? TF_WIDE_LDS : TF_WIDE_HBM;
  return TF_STACK;
}
// The traversal the feature-buffer pass (rt_render_aov) takes: the query's, with one exception. The pass samples the
// hit material's texture, and a picture texture needs the hit's u, v; the flat program's record (a face's axis, sign
// and material) cannot supply them, so a scene with an RT_TEX_IMAGE texture leaves the flat program for the next
// family in trace_family's order (a flat-eligible scene always has a linear program).
inline TraceFamily aov_family(const SceneHeader& h, bool ordered, size_t word_bytes) {
  const bool pictures = (h.tex_kinds & (1u << T_IMAGE)) != 0;
  return trace_family(h, ordered || (pictures && h.has_flat), word_bytes);
}
// Whether the pass needs its kernel's extended form: a camera model other than the perspective one, or a texture
// other than solid and checker (the base form's tex_sample holds those two only).
inline bool aov_extended(const SceneHeader& h, int32_t cam_mode) {
  return cam_mode != RT_CAM_PERSPECTIVE || (h.tex_kinds & ~((1u << T_SOLID) | (1u << T_CHECKER))) != 0;
}
// Whether an occlusion query (rt_occluded) of family `f` may start its traversal bounded by the ray's tmax and leave
// at the first accepted hit, or has to walk rt_trace_rays' closest-hit traversal and compare its t with tmax. The one
// home of that decision ("Occlusion queries"). Two cases keep the closest-hit traversal:
//  - a scene with volumes: volumne::hit draws with a running slot counter after its interval test, so another
//    interval or an earlier exit shifts the later draws;
//  - fp32 rays (word_bytes 16) through the binary BVH of a scene with the fp64 quad records (has_quads64): a near-edge
//    quad hit is re-decided by a second, fp64 distance against the same interval (quad_edge64), so whether a quad
//    accepts depends on the interval's upper end and not only on whether its root lies inside.
// Both concern the linear program and the binary BVH alone: the flat program and the wide tree hold world-level
// quads, spheres and triangles only (scene_compile.cpp), and neither re-decides a quad in fp64.
// h: the header of the blob the rays read, as for trace_family.
inline bool occlusion_early_exit(const SceneHeader& h, TraceFamily f, size_t word_bytes) {
  if (f != TF_LINEAR && f != TF_STACK) return true;
  if (h.has_volumes != 0) return false;
  if (f == TF_STACK && word_bytes == 16 && h.has_quads64 != 0) return false;
  return true;
}
// the render family whose RT_DEV_ONLY switch decides whether a build has the query kernel of `f`
inline KernelFamily trace_render_family(TraceFamily f) {
  return f == TF_FLAT ? KF_FLAT : f == TF_LINEAR ? KF_LIN_ALL : f == TF_STACK ? KF_STACK : KF_WIDE;
}
inline const char* trace_family_name(TraceFamily f) {
  static const char* n[] = {"flat program", "linear program", "wide BVH in LDS", "wide BVH in HBM", "binary BVH"};
  return n[f];
}

inline const char* family_name(KernelFamily f) {
  static const char* n[] = {"flat program", "linear program (quads)", "linear program (quads + volumes)",
                            "linear program (spheres)", "linear program (all kinds)", "wide BVH", "binary BVH"};
  return n[f];
}

// a lambertian + diffuse_light scene with solid textures (a background too) and an axis-aligned quad light (the
// Cornell configs): the flat kernel's LL form (shade LL)
inline bool lamb_light_scene(const SceneHeader& h) {
  const uint32_t ok_m = (1u << M_LAMBERTIAN) | (1u << M_DIFFUSE_LIGHT);
  return (h.mat_kinds & ~ok_m) == 0 && (h.tex_kinds & ~(1u << T_SOLID)) == 0 && h.light_kind == L_QUAD &&
         h.light_aligned != 0;
}
// no light, lambertian / metal / dielectric materials with solid or checker textures (RTOW): shade NL
inline bool no_light_scene(const SceneHeader& h) {
  const uint32_t ok_m = (1u << M_LAMBERTIAN) | (1u << M_METAL) | (1u << M_DIELECTRIC);
  return (h.mat_kinds & ~ok_m) == 0 && (h.tex_kinds & ~((1u << T_SOLID) | (1u << T_CHECKER))) == 0 &&
         h.light_kind == L_NONE;
}
// lambertian, isotropic and diffuse_light materials with solid textures and an axis-aligned quad light (C5)
inline bool lamb_iso_light_scene(const SceneHeader& h) {
  const uint32_t ok_m = (1u << M_LAMBERTIAN) | (1u << M_DIFFUSE_LIGHT) | (1u << M_ISOTROPIC);
  return (h.mat_kinds & ~ok_m) == 0 && (h.tex_kinds & ~(1u << T_SOLID)) == 0 && h.light_kind == L_QUAD &&
         h.light_aligned != 0;
}

// ------------------------------------------------------------------ the path kernel
// What the kernels keep in fixed-size LDS tables, and so what a scene may have at most to be given such a kernel:
// the policies (rt_kernels.hip) size their tables by these names and path_kernel tests a scene against them.
// The flat program's records and materials (FlatTrav::Tables), in its general and its LL form:
struct FlatCaps {
  uint32_t quads, boxes, rooms, mats;
};
constexpr FlatCaps kFlatLds{64, 16, 2, 32}, kFlatLdsLL{14, 8, 1, 16};
inline bool flat_tables_fit(const SceneHeader& h, const FlatCaps& c) {
  return h.n_flat_quad[0] + h.n_flat_quad[1] + h.n_flat_quad[2] <= c.quads && h.n_flat_box <= c.boxes &&
         h.n_flat_room <= c.rooms && h.n_mats <= c.mats;
}
constexpr uint32_t kLdsNodeMax = 256;  // the binary BVH's nodes in LDS (StackTrav LDSN, fp32 only)
constexpr uint32_t kLdsMatsLL = 16;    // materials of the linear LLI and wide LL kernels' LDS table (wlm_tab)
constexpr int kStackSmall = 8, kStackMid = 16;  // the binary BVH's LDS stacks below kStackDepth entries

// One path kernel by name: what launch_step instantiates and path_kernel_tag spells.
enum ShadeClass { SH_GENERAL, SH_LL, SH_NL, SH_LLI };  // lamb_light_scene, no_light_scene, lamb_iso_light_scene
struct PathKernel {
  KernelFamily fam;
  ShadeClass shade;
  bool lds;        // in LDS: the flat program's tables, the binary BVH's nodes, the wide tree
  int stack;       // binary BVH: the LDS stack entries of a lane, kStackSmall, kStackMid or kStackDepth; else 0
  uint32_t kinds;  // wide tree: the WK_* primitive kinds the kernel tests, one of six sets; else 0
  bool camx;       // the extended form (the linear program and the binary BVH alone)
  bool persist;    // the persistent schedule, else the wavefront schedule
  bool rays;       // the first segments are caller-given rays (rt_radiance; radiance_kernel), not camera rays
};
// The path kernel a render launches. h: the header of the blob the precision reads (hdr or hdr64: an fp64 flat scene
// stores a room's walls as one room record, so the two can fall on different sides of the flat tables' limits);
// word_bytes: a primitive word of that blob, 16 (fp32) or 32 (fp64); stack_need: CompiledScene::stack_need.
inline PathKernel path_kernel(const SceneHeader& h, size_t word_bytes, int32_t cam_mode, bool persist, bool ordered,
                              int stack_need) {
  PathKernel k{};
  k.fam = kernel_family(h, cam_mode, persist, ordered);
  k.shade = SH_GENERAL;
  k.persist = persist;
  // (the flat program and the wide tree never see an extended render: kernel_family)
  k.camx = k.fam != KF_FLAT && k.fam != KF_WIDE && extended_form(h, cam_mode);
  const bool few_mats = h.n_mats <= kLdsMatsLL;
  switch (k.fam) {
    case KF_FLAT:
      // the tables in LDS: the persistent kernel alone; the LL form's tables are smaller
      k.lds = persist && flat_tables_fit(h, kFlatLds);
      if (k.lds && lamb_light_scene(h) && flat_tables_fit(h, kFlatLdsLL)) k.shade = SH_LL;
      break;
    case KF_LIN_VOL:
      // lambertian + isotropic + light (C5), persistent schedule only: the LLI form's shade and LDS material table
      // are persist_body's; step_body (segments_per_launch > 0) shades with the general program, which its
      // register budget would squeeze
      if (lamb_iso_light_scene(h) && persist && few_mats) k.shade = SH_LLI;
      break;
    case KF_WIDE:
      // the primitive kinds of the scene: spheres only (RTOW, C3: NL), triangles only, triangles and quads (a mesh
      // under a quad light; lambertian + light, the C4 stand-in: LL), or all, moving spheres among them
      k.kinds = (h.wide_kinds == WK_SPHERE || h.wide_kinds == WK_TRI || h.wide_kinds == (WK_TRI | WK_QUAD))
                    ? h.wide_kinds
                    : (WK_SPHERE | WK_TRI | WK_QUAD | WK_MOVING);
      if (k.kinds == WK_SPHERE && no_light_scene(h)) k.shade = SH_NL;
      if (k.kinds == (WK_TRI | WK_QUAD) && lamb_light_scene(h) && few_mats) k.shade = SH_LL;
      k.lds = wide_tree_in_lds(h.n_wnodes, h.n_wprim_words, h.wide_stack, word_bytes);
      break;
    case KF_STACK:
      k.lds = word_bytes == 16 && h.n_nodes <= kLdsNodeMax && stack_need <= kStackMid;  // nodes in LDS: fp32 only
      k.stack = stack_need <= kStackSmall ? kStackSmall : stack_need <= kStackMid ? kStackMid : kStackDepth;
      if (k.lds) k.stack = kStackMid;  // (the one kernel with its nodes in LDS)
      break;
    default:  // the other linear programs: one kernel each
      break;
  }
  return k;
}
// The path kernel a ray batch launches (rt_radiance): the one a perspective render of the scene takes on the persistent
// schedule -- the same family, shade form, LDS use and stack, the extended form by the scene's textures alone (a batch
// has no camera model) -- in its form whose first segments are the caller's rays.
inline PathKernel radiance_kernel(const SceneHeader& h, size_t word_bytes, bool ordered, int stack_need) {
  PathKernel k = path_kernel(h, word_bytes, RT_CAM_PERSPECTIVE, true, ordered, stack_need);
  k.rays = true;
  return k;
}
// The kernel's tag as rt_dev_last_kernel reports it (rt_kernels.hip kernel_tag): the traversal policy with every
// template argument in order (the precision first, bools as 0 / 1), "camx" for the extended form, and the schedule:
// "WideTrav<f64,0,1,1,0,1,1,0> persist", "LinearTrav<f32,1,1,1,0> camx step"; a ray batch's has "rays" before the
// schedule, "FlatTrav<f64,1,1> rays persist".
inline std::string path_kernel_tag(const PathKernel& k, size_t word_bytes) {
  auto trav = [&](const char* name, std::initializer_list<int> args) {
    std::string s = std::string(name) + (word_bytes == 32 ? "<f64" : "<f32");
    for (int a : args) s += "," + std::to_string(a);
    return s + ">" + (k.camx ? " camx" : "") + (k.rays ? " rays" : "") + (k.persist ? " persist" : " step");
  };
  const bool sph = k.fam == KF_LIN_SPH || k.fam == KF_LIN_ALL, all = k.fam == KF_LIN_ALL;
  switch (k.fam) {
    case KF_FLAT:
      return trav("FlatTrav", {k.lds, k.shade == SH_LL});
    case KF_WIDE:
      return trav("WideTrav", {(k.kinds & WK_SPHERE) != 0, (k.kinds & WK_TRI) != 0, (k.kinds & WK_QUAD) != 0,
                               (k.kinds & WK_MOVING) != 0, k.lds, k.shade == SH_LL, k.shade == SH_NL});
    case KF_STACK:
      return trav("StackTrav", {k.stack, k.lds});
    default:  // SPH, TRI, VOL, LLI
      return trav("LinearTrav", {sph, all, all || k.fam == KF_LIN_VOL, k.shade == SH_LLI});
  }
}

// ------------------------------------------------------------------ the item layout
// Work item = (pixel, chunk of consecutive samples). The layout decides the image's summation order (per
// pixel: samples within an item, then items in chunk order), the item count (below 2^31 per launch) and the
// partial-sum memory, so it depends on spp and the full image alone: the same for any tiling or rank count.
//
// The automatic sizes (rt_render_params.samples_per_item = 0); the caller may override them for A/B runs
// (RT_ITEM_*, RT_ITEMS_TARGET, RT_PARTIAL_BUDGET in the environment; scripts/dev_tail.py). `flat`: the flat
// program's, whose items are cheaper per sample, so its default items are longer (fewer item ends, dequeues
// and partial-sum stores; C2: 23.9 -> 23.5 ms/frame).
// Bulk items: 8 samples (32 for the flat program); at most kMaxItemsPerPixel items per pixel in all (both
// sizes doubled until they fit), so a high-spp frame (C5: 3840x2160 at 4096 spp) keeps its item count under
// 2^31 and its partial sums bounded.
constexpr uint32_t kMaxItemsPerPixel = 256;
constexpr uint32_t kMinAutoChunk = 2;
struct PlanKnobs {
  uint32_t chunk = 8, chunk_flat = 32;        // bulk item size
  uint32_t tail_chunk = 4, tail_chunk_flat = 8;  // size of the frame's last items
  double tail_frac = 0.5, tail_frac_flat = 0.125;  // share of every pixel's samples in tail items
  // items a frame should have at least. C1 (400x400, 64 spp), ms/frame by target (item size): fp64 none (16)
  // 0.918, 1 M (8) 0.792, 2.5 M (4) 0.735, 5 M (2) 0.710; fp32 none (32 + tail items of 8) 0.661, 1 M 0.589,
  // 2.5 M 0.525, 5 M 0.536. The BASELINE configs from C2 up have 40 M items or more and keep their sizes.
  uint64_t items_target = 4000000;
  // item partial sums of one pass at most (a call needing more renders its chunks in passes)
  uint64_t partial_budget = 2ull << 30;
};

// Chunks [0, k_bulk) of a pixel hold `chunk` samples, chunks [k_bulk, nchunks) `tail_chunk` <= chunk (the
// last one what is left of spp). The chunks come in `passes` launches of at most `cpp` chunks each.
struct ItemPlan {
  uint32_t chunk, tail_chunk, k_bulk, nchunks;
  uint32_t cpp;            // chunks per pass
  uint32_t passes;
  uint64_t partial_bytes;  // partial sums of the largest pass: 3 elements per item
};

// spp >= 1; samples_per_item <= 0: the automatic layout; full_pixels: the whole image's; npix >= 1: this
// call's (its tiles'), below 2^31; elem: bytes of a partial sum's element (4 or 8).
inline ItemPlan plan_items(uint32_t spp, int32_t samples_per_item, bool flat, uint64_t full_pixels, uint32_t npix,
                           uint32_t elem, const PlanKnobs& kn) {
  const bool automatic = samples_per_item <= 0;
  uint32_t chunk0 = std::min(spp, automatic ? std::max(1u, flat ? kn.chunk_flat : kn.chunk) : (uint32_t)samples_per_item);
  // a small frame (C1: 160,000 px x 64 spp is ~2 items of 16 per resident lane) takes smaller items, so
  // the lanes that finish early find work while the last items run: the automatic size is halved until
  // the whole frame has items_target items
  if (automatic)
    while (chunk0 > kMinAutoChunk && full_pixels * ((spp + chunk0 - 1) / chunk0) < kn.items_target) chunk0 /= 2;
  ItemPlan pl{};
  pl.chunk = pl.tail_chunk = chunk0;
  pl.k_bulk = pl.nchunks = (spp + chunk0 - 1) / chunk0;
  // The frame's last items are short (automatic layout only): a lane that takes a long item just
  // before the queue runs dry keeps its wave resident while the others idle, and a small frame
  // (one rank of eight) has few items per lane. The last tail_samples of every pixel come in
  // items of tail_chunk samples. (fp64 too since round 3: round 2 kept uniform items of 16 for it)
  if (automatic) {
    const double frac = std::min(1.0, std::max(0.0, flat ? kn.tail_frac_flat : kn.tail_frac));
    const uint32_t ts = std::min<uint32_t>(spp, (uint32_t)((double)spp * frac + 0.5));
    pl.tail_chunk = std::min(pl.chunk, std::max(1u, flat ? kn.tail_chunk_flat : kn.tail_chunk));
    for (;;) {
      pl.k_bulk = (spp - ts) / pl.chunk;  // bulk items cover [0, k_bulk * chunk)
      pl.nchunks = pl.k_bulk + (spp - pl.k_bulk * pl.chunk + pl.tail_chunk - 1) / pl.tail_chunk;
      if (pl.nchunks <= kMaxItemsPerPixel || pl.chunk >= spp) break;
      pl.chunk = std::min(spp, 2 * pl.chunk);
      pl.tail_chunk = std::min(pl.chunk, 2 * pl.tail_chunk);
    }
  }
  // Passes: the item partial sums of a call are 3 elements per (pixel, chunk) -- C5 fp64 (3840 x 2160 at
  // 4096 spp, 192 chunks) would need 38 GB. The chunks come in passes of `cpp` chunks whose partial sums fit
  // the budget (and whose items fit 31 bits); every pass is one launch, and its resolve adds its chunks to
  // the running per-pixel sums in chunk order (k_resolve), so the image is the same for any split.
  const uint64_t per_chunk = 3ull * elem * npix;
  pl.cpp = (uint32_t)std::max<uint64_t>(
      1, std::min<uint64_t>({(uint64_t)pl.nchunks, kn.partial_budget / per_chunk, ((1ull << 31) - 1) / npix}));
  pl.passes = (pl.nchunks + pl.cpp - 1) / pl.cpp;
  pl.partial_bytes = per_chunk * pl.cpp;
  return pl;
}

// ------------------------------------------------------------------ item runs (what the wave queue hands out)
// The item layout above fixes the image's rounding. What a persistent launch's queue hands out is a *unit*: a run
// of L = 1 << run_log2 consecutive bulk chunks of one pixel, or a single item. A lane that ends a chunk inside its
// run goes on with the same pixel's next chunk (item + npix) and skips the dequeue, the pixel map load, the pixel
// key and the camera base; every item still writes its own partial sum, so the image does not depend on L.
// Of a pass's local chunks [0, pc) the first runs * L -- whole runs of bulk chunks -- are run units, handed out
// first and run-major (unit = run * npix + pixel, as today's items are chunk-major); the bulk chunks that do not
// fill a run and the tail items follow as single units, so the launch ends on items as short as before.
// L = 1 (runs = 0): a unit is an item. (constexpr: the kernels call these too)
struct RunPlan {
  uint32_t run_log2;     // L = 1 << run_log2
  uint32_t runs;         // run units of a pixel
  uint32_t n_units;      // units of the pass: its items less (L - 1) for every run
  uint32_t run_samples;  // samples of a pixel's runs, runs * L * chunk
  uint32_t run_mask;     // L * chunk - 1 (bulk chunk sizes are powers of two where runs > 0)
};
// The pass over chunks [chunk0, chunk0 + pc) of every one of npix pixels, in runs of `run` (a power of two).
// Runs need a pass that begins at the pixel's first sample (chunk0 = 0: the test at a chunk end is then one on the
// sample index as it stands), a power-of-two bulk chunk, items * L below 2^32 (unit_first_item) and at most
// kRunCfgRunsMax runs a pixel (what run_cfg_pack holds: a caller-given item size puts no limit on a pixel's chunks,
// where the automatic layout stops at kMaxItemsPerPixel); a pass without them has L = 1.
constexpr uint32_t kRunCfgRunsMax = 0xFFFFu;
inline RunPlan plan_runs(const ItemPlan& pl, uint32_t spp, uint32_t chunk0, uint32_t pc, uint32_t npix, uint32_t run) {
  RunPlan r{};
  // the bulk chunks that hold `chunk` samples (a caller-given item size may leave the last one short: it stays
  // single, so a chunk inside a run always ends on a multiple of chunk)
  const uint32_t bulk = chunk0 == 0 ? std::min({pl.k_bulk, spp / pl.chunk, pc}) : 0;
  const bool pow2 = (pl.chunk & (pl.chunk - 1)) == 0;  // (a caller-given samples_per_item may be anything)
  while (r.run_log2 < 16 && (2u << r.run_log2) <= run) r.run_log2++;
  // no run longer than the bulk chunks; a shorter run has more runs a pixel, so over kRunCfgRunsMax ends at L = 1
  while (r.run_log2 && (!pow2 || (bulk >> r.run_log2) == 0 || (bulk >> r.run_log2) > kRunCfgRunsMax ||
                        (((uint64_t)npix * pc) << r.run_log2) >> 32))
    r.run_log2--;
  r.runs = r.run_log2 ? bulk >> r.run_log2 : 0;
  r.n_units = npix * (pc - r.runs * ((1u << r.run_log2) - 1));
  r.run_samples = (r.runs << r.run_log2) * pl.chunk;
  r.run_mask = (pl.chunk << r.run_log2) - 1;
  return r;
}
// The kernels' word for a pass's runs (LaunchParams::run_cfg): runs in the low 16 bits, run_log2 above; 0: every
// unit is an item. plan_runs keeps runs within kRunCfgRunsMax.
constexpr uint32_t run_cfg_pack(uint32_t runs, uint32_t run_log2) { return runs | run_log2 << 16; }
constexpr uint32_t run_cfg_runs(uint32_t cfg) { return cfg & kRunCfgRunsMax; }
constexpr uint32_t run_cfg_log2(uint32_t cfg) { return cfg >> 16; }
// Unit -> the local chunk of its first item, and that item. q = unit / npix (the kernel divides by div_magic) and
// qn = q * npix. Run unit q of a pixel starts at chunk q * L; the singles follow the runs * L chunks of the runs,
// runs * (L - 1) chunks further on than their unit. Both as a minimum, which is cheaper on the device than a
// select: q (L - 1) < runs (L - 1) exactly where q < runs. (qn << run_log2 stays below 2^32: plan_runs)
constexpr uint32_t unit_first_chunk(uint32_t q, uint32_t runs, uint32_t run_log2) {
  const uint32_t a = q << run_log2, b = q + runs * ((1u << run_log2) - 1);
  return a < b ? a : b;
}
constexpr uint32_t unit_first_item(uint32_t unit, uint32_t qn, uint32_t npix, uint32_t runs, uint32_t run_log2) {
  const uint32_t a = (qn << run_log2) - qn, b = runs * ((1u << run_log2) - 1) * npix;
  return unit + (a < b ? a : b);
}
// At a chunk end: does the lane's run go on? sample: the pixel's sample index that follows the chunk (without
// first_sample, as item_range counts). Inside the runs' samples, and not at a run's boundary.
constexpr bool run_goes_on(uint32_t sample, uint32_t run_samples, uint32_t run_mask) {
  return sample < run_samples && (sample & run_mask) != 0;
}

// The kernels that hand out runs (FlatTrav::kItemRuns): the flat program's LL kernels on a camera's rays. Every
// other kernel's units are items whatever the plan says, so the host plans L = 1 for them.
inline bool kernel_takes_runs(const PathKernel& k) {
  return k.fam == KF_FLAT && k.shade == SH_LL && k.lds && k.persist && !k.rays;
}
// The automatic run length. L is pure scheduling, so it may depend on how much work the call has, and it must: a
// run is one unit of L * chunk samples that no other lane can take over, and the launch ends when its last lane
// does. Two conditions (has the measurements):
//  - `overlapped`: the launch goes through the launch lanes and so did the context's launch before it (lane_plan:
//    a stream of device-output frames), so the next launch's blocks fill the SIMDs this launch's last runs leave
//    idle. Runs lengthen a launch's end -- C2 fp64 with one launch at a time (RT_FRAME_OVERLAP=0): 23.27 ms a frame
//    with items, 23.50 at L = 2, 23.9 at 4, 25.2 at 8 -- and shorten everything before it; only a launch whose end
//    is hidden gains (back to back: 22.98 -> 22.41 at L = 8). A lone frame, a host-output render and the first frame
//    of a stream keep items; the last frame of a stream pays the longer end once.
//  - every lane still receives many units, so that the dynamic queue still evens out the paths' lengths:
//    kMinUnitsPerMaxLane on average over `lanes`, which the caller gives as the most lanes the device can hold (2,048
//    a CU), not the kernel's resident grid (the headline kernel's is 1,792 a CU: 8 here is 9.1 per resident lane).
//    The largest L up to kMaxRun that keeps it. C2 fp64, units per such lane (23 a pixel at L = 4 and 8, 30 at 2):
//    the whole frame, 28, is fastest at L = 8 (16 is slower again: one run and 12 single bulk chunks a pixel); half
//    of it, 14, gains at L = 4; a quarter gains nothing at 7 (L = 4) and 0.2 % at 9 (L = 2); an eighth loses 0.5 %
//    at 4.6 (L = 2) and 3 % at 3.5 (L = 4). A C1-sized frame has 3 to 6 at any L > 1 and keeps items.
// L = 1 for the wavefront schedule, for a kernel that does not take runs, for a ray batch (kernel_takes_runs) and
// for a multi-pass call (plan_runs gives runs to the first pass alone, and every pass would end on long units).
constexpr uint32_t kMaxRun = 8, kMinUnitsPerMaxLane = 8;
inline uint32_t auto_run(const ItemPlan& pl, const PathKernel& k, uint32_t spp, uint32_t npix, uint64_t lanes,
                         bool overlapped) {
  if (!kernel_takes_runs(k) || pl.passes != 1 || !overlapped) return 1;
  for (uint32_t run = kMaxRun; run > 1; run /= 2) {
    const RunPlan r = plan_runs(pl, spp, 0, pl.nchunks, npix, run);
    if ((1u << r.run_log2) == run && (uint64_t)r.n_units >= kMinUnitsPerMaxLane * lanes) return run;
  }
  return 1;
}

// ------------------------------------------------------------------ adaptive sampling (rt_render_adaptive)
// A pixel's running moments over its batches (rt_hip.h, "adaptive sampling"): per channel the sum S of the batch sums
// and the sum Q of their squares, in double and in batch order, and the batch count K. One 64-byte record a pixel of
// the call, indexed by the pixel's packed position; k_resolve_moments adds a pass's batches to it, k_adaptive_select
// reads it and leaves the estimate and its decision in it.
struct alignas(64) AdaptiveAcc {
  double S[3], Q[3];
  double err;     // the estimate the last select computed
  uint32_t K;
  uint32_t stop;  // that select's decision: 1 the pixel has stopped, 0 it takes the next round
};
static_assert(sizeof(AdaptiveAcc) == 64, "one record is one 64-byte line");

// The estimator's arithmetic, the one copy the kernel and the host (rt_dev_adaptive_error) run: K >= 2 batches of
// `batch` samples with the moments S, Q -> the channel means (in double) and err. Every operation is rounded on its
// own (no contraction), in the order written, so a numpy transcription gives the same bits. max(0, d) is written as a
// select that keeps a NaN: a pixel with a NaN sample has a NaN err, fails err <= threshold and runs to max_spp.
__host__ __device__ inline void adaptive_error(uint32_t K, uint32_t batch, const double S[3], const double Q[3],
                                               double floor, double mean3[3], double* err) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double k = (double)K, b = (double)batch;
  const double n = k * b;
  double var[3];
  for (int c = 0; c < 3; c++) {
    mean3[c] = S[c] / n;
    const double sq = S[c] * S[c];
    const double d = Q[c] - sq / k;
    var[c] = (d < 0.0 ? 0.0 : d) / (k - 1.0);
  }
  const double se2 = ((var[0] + var[1]) + var[2]) / (k * (b * b));
  const double level = ((mean3[0] + mean3[1]) + mean3[2]) / 3.0;
  *err = __builtin_sqrt(se2 / 3.0) / (floor + level);
}
// after a round: does the pixel stop? (a NaN err fails the comparison)
__host__ __device__ inline bool adaptive_stops(double err, double threshold, uint32_t samples, uint32_t max_spp) {
  return err <= threshold || samples >= max_spp;
}
// The parameter rules of rt_adaptive_params (rt_adaptive_check): nullptr, or what is wrong with them.
inline const char* adaptive_params_error(const rt_adaptive_params& p) {
  if (p.batch < 1) return "batch must be positive";
  if (p.step_spp < p.batch || p.step_spp % p.batch != 0) return "step_spp must be a positive multiple of batch";
  if (p.min_spp % p.step_spp != 0 || p.max_spp % p.step_spp != 0) return "min_spp and max_spp must be multiples of step_spp";
  if ((int64_t)p.min_spp < 2 * (int64_t)p.batch) return "min_spp must hold at least two batches";
  if (p.min_spp > p.max_spp) return "min_spp above max_spp";
  if (p.max_depth < 0) return "max_depth must not be negative";
  if (p.precision != RT_PREC_F32 && p.precision != RT_PREC_F64) return "unknown precision";
  if (p.traversal != RT_TRAV_AUTO && p.traversal != RT_TRAV_ORDERED) return "unknown traversal";
  if (!(p.threshold >= 0.0)) return "threshold must be >= 0 and not NaN";
  if (!(p.floor > 0.0) || p.floor - p.floor != 0.0) return "floor must be positive and finite";
  return nullptr;
}

// ------------------------------------------------------------------ the launch lanes (frame overlap)
// A persistent launch ends with a tail: its last paths, up to max_depth dependent segments each, run on a chip
// that is nearly empty (a frame costs its work plus ~0.5 ms whatever its size). The next launch
// could fill those SIMDs, but on one stream it starts only after the tail and the resolve behind it. So the
// persistent launches of device-output renders alternate between two internal streams, the lanes, and each
// writes one of two sets of what a launch writes (the item partial sums, the dequeue heads): launch n + 1's blocks
// become resident as launch n's retire. k_persist never waits for another kernel, so two resident launches cannot
// deadlock. The resolves, and so everything the caller sees, stay on the caller's stream.
//
// The one home of the ordering: what a context remembers between the launches of its lanes (LaneState), for its next
// persistent launch which lane and buffer set it takes and what it waits for (lane_plan), and what the launch leaves
// behind for the one after it (lane_advance). rt_render.hip's one_pass() turns a plan into events and launches;
// tests/test_lane_plan.py drives the three through tests/native/lane_plan_dump.cpp.
struct LaneState {
  uint64_t n = 0;               // launches that went through the lanes on this context so far
  bool inputs_written = false;  // something the kernel reads (scene, camera view, pixel map) was queued on a caller's
                                // stream after the last lane launch that waited for that stream
  bool prev_overlapped = false;  // the context's last path launch went through the lanes
  bool lane_stale[2] = {false, false};  // the lane has not waited for the inputs event since it was last recorded
};
// The question of one launch: the context's state as it stands before the launch (the base, so q.n, q.inputs_written,
// q.prev_overlapped and q.lane_stale are the state's own fields, defined once) and what is known of the call.
struct LaneQuery : LaneState {
  void set_state(const LaneState& s) { static_cast<LaneState&>(*this) = s; }
  bool knob;             // RT_FRAME_OVERLAP (default on)
  bool device_out;       // a device-output render: the call returns before the image is there
  bool persist;          // the persistent schedule (the wavefront schedule syncs with the host between launches)
  bool shared_scratch;   // the launch writes the context's wide spill area, which is indexed by lane alone
  bool second_set;       // the second lane and buffer set exist (false: their allocation failed)
  bool pending;          // the context has work outstanding on `prev`
  const void* caller;    // the stream of this call
  const void* prev;      // the stream of the outstanding work
};
struct LanePlan {
  bool overlap;       // false: the serial chain on the caller's stream (set 0), as before the lanes
  int lane, set;      // lane 0 is the context's own stream; the sets alternate with the lanes
  bool sync_prev;     // the host waits for `prev` (and the lanes behind it) first: the caller's stream changed
  bool wait_resolve;  // the lane waits for the resolve of launch n - 2, the last reader of this set
  bool record_inputs; // the inputs event is recorded now on the caller's stream (both lanes become stale)
  bool wait_inputs;   // the lane waits for the inputs event as last recorded
};
inline LanePlan lane_plan(const LaneQuery& q) {
  LanePlan pl{};
  // a render on another stream than the outstanding work's: that work reads what this call is about to write
  pl.sync_prev = q.pending && q.prev != q.caller;
  pl.overlap = q.knob && q.device_out && q.persist && !q.shared_scratch && q.second_set;
  if (!pl.overlap) return pl;
  pl.lane = pl.set = (int)(q.n & 1);
  // Launch n - 2 ran on this lane, so the kernels are in order already; its resolve ran on a caller's stream
  // (after a host wait it has finished, and the wait for its event costs nothing).
  pl.wait_resolve = q.n >= 2;
  // Inputs queued on the caller's stream, or a serial launch there that wrote set 0: an event behind them. The
  // launch that records it waits for it, and so does the other lane's next launch, which reads the same inputs
  // and is ordered behind its own lane and the resolve of launch n - 1 alone, both older than the event.
  // Inputs a caller queues *later* need nothing here: the caller's stream waits for every launch before that
  // launch's resolve, so whatever follows on it is behind every earlier launch. A call that changes no input
  // waits for nothing on the caller's stream but the resolve of launch n - 2: that is the case that overlaps.
  pl.record_inputs = q.inputs_written || !q.prev_overlapped;
  pl.wait_inputs = pl.record_inputs || q.lane_stale[pl.lane];
  return pl;
}
// The state after the launch `pl` plans.
inline void lane_advance(LaneState& s, const LanePlan& pl) {
  if (!pl.overlap) {
    s.prev_overlapped = false;
    s.inputs_written = false;  // the launch runs on the stream the inputs were queued on
    return;
  }
  if (pl.record_inputs) {
    s.inputs_written = false;
    s.lane_stale[0] = s.lane_stale[1] = true;  // neither lane is behind this event yet
  }
  if (pl.wait_inputs) s.lane_stale[pl.lane] = false;
  s.prev_overlapped = true;
  s.n++;
}

}  // namespace rtd
