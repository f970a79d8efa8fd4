/*
 * rt_hip.h -- C ABI of the MI355X wavefront path tracer.
 *
 * This is the drop-in boundary for the reference's render hot path:
 *   camera::render(std::ofstream&, const hittable& world,
 *                  std::shared_ptr<const hittable> light)
 *     (/root/reference/src/camera.h:135-176)
 * and everything it reaches per sample: camera::generate_ray (camera.h:244-284),
 * camera::ray_color (camera.h:193-241), camera::miss (camera.h:180-190),
 * hittable::hit for every concrete hittable (hittable.h:32-293, sphere.h:40-74,
 * quad.h:30-52, triangle.h:27-40, volumne.h:18-46, hittable_list.h:20-31,
 * bvh_node.h:49-59), material::{scatter,p_scattered,emitted} (material.h:36-219),
 * pdf::{value,generate} (pdf.h:7-61, hittable_list.h:39-50) and texture::sample
 * (texture.h:6-63).
 *
 * The reference has no FFI of its own: its plugin surface is the C++ virtual
 * interfaces above. The C++ headers under
 * cpu-ray-tracing-implementation_amd/rt/ keep those class names and
 * constructors; each object serialises itself into an rt_scene_desc (a POD
 * image of the hittable DAG) and camera::render hands it to this library.
 *
 * Conventions
 *  - Every entry point returns rt_status; no C++ exception crosses the ABI.
 *  - One rt_context per HIP device. A context is not re-entrant; different
 *    contexts may be used from different host threads concurrently.
 *  - rt_render_tiles is stream-ordered on the caller's stream (hipStream_t
 *    passed as void*; NULL = the HIP null stream, which is also torch's
 *    default stream) when out_rgb is a device pointer: work queued on that
 *    stream after the call sees the finished image. With a host pointer it
 *    returns after the copy.
 *  - rt_multi_* drive several devices from one process (camera.h:154-172's
 *    row parallelism lifted to tiles over GPUs): one
 *    context per device and one RCCL communicator (ncclCommInitAll) whose
 *    ncclGather brings every device's tiles to the first device.
 *  - All geometry in the descriptor is double precision, as in the reference
 *    (vec3.h:7). The device computes in fp32 (RT_PREC_F32, the production
 *    path) or fp64 (RT_PREC_F64, the parity path).
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8

typedef enum rt_status {
  RT_OK = 0,
  RT_ERR_INVALID_ARGUMENT = 1,
  RT_ERR_UNSUPPORTED = 2, /* scene uses a hittable/material/texture the device path does not implement */
  RT_ERR_HIP = 3,         /* a HIP runtime call failed (message in rt_last_error) */
  RT_ERR_OUT_OF_MEMORY = 4,
  RT_ERR_NO_SCENE = 5,
  RT_ERR_NO_DEVICE = 6
} rt_status;

/* ---- scene description: a POD image of the reference's hittable DAG ---- */

typedef enum rt_object_kind {
  RT_OBJ_SPHERE = 1,    /* sphere.h:7-35      a = center1, b = center2, s0 = radius, moving */
  RT_OBJ_QUAD = 2,      /* quad.h:9-23        a = corner, b = u, c = v                     */
  RT_OBJ_TRIANGLE = 3,  /* triangle.h:19-25   a = p0, b = p1, c = p2                       */
  RT_OBJ_LIST = 4,      /* hittable_list.h:7-37  children[first_child .. +child_count)     */
  RT_OBJ_BVH = 5,       /* bvh_node.h:13-47   children = the list it was built from        */
  RT_OBJ_TRANSLATE = 6, /* hittable.h:67-89   child, a = offset                            */
  RT_OBJ_ROTATE_X = 7,  /* hittable.h:93-158  child, s0 = sin(theta), s1 = cos(theta)      */
  RT_OBJ_ROTATE_Y = 8,  /* hittable.h:160-225                                              */
  RT_OBJ_ROTATE_Z = 9,  /* hittable.h:227-293                                              */
  RT_OBJ_VOLUME = 10    /* volumne.h:9-46     child = boundary, s0 = density,
                           material = the isotropic phase function (volumne.h:14)          */
} rt_object_kind;

typedef struct rt_object {
  int32_t kind;        /* rt_object_kind */
  int32_t material;    /* index into materials, or -1 */
  int32_t child;       /* translate / rotate_* / volume: the wrapped object */
  int32_t first_child; /* list / bvh: first index into children[] */
  int32_t child_count; /* list / bvh: number of children */
  int32_t moving;      /* sphere: 1 = the moving-sphere constructor (sphere.h:25-35) */
  double a[3];
  double b[3];
  double c[3];
  double s0;
  double s1;
} rt_object;

typedef enum rt_material_kind {
  RT_MAT_LAMBERTIAN = 1,    /* material.h:57-76   */
  RT_MAT_METAL = 2,         /* material.h:78-97   fuzz (stored as float, material.h:96) */
  RT_MAT_DIELECTRIC = 3,    /* material.h:100-143 refraction (float, material.h:142)    */
  RT_MAT_ISOTROPIC = 4,     /* material.h:187-204 */
  RT_MAT_DIFFUSE_LIGHT = 5, /* material.h:206-219 */
  RT_MAT_GLOSS = 6          /* material.h:145-185  smoothness (clamped to [0,1]), specular_prob */
} rt_material_kind;

typedef struct rt_material {
  int32_t kind;    /* rt_material_kind */
  int32_t texture; /* albedo / emission texture index */
  float fuzz;
  float refraction;
  float smoothness;
  float specular_prob;
} rt_material;

typedef enum rt_texture_kind {
  RT_TEX_SOLID = 1,   /* texture.h:12-37 */
  RT_TEX_CHECKER = 2, /* texture.h:39-63 */
  RT_TEX_PERLIN = 3,  /* texture.h:80-92, noise.h:10-89. scale; tex_data[data ..]: rand_offset (256 x 3),
                         then perm_x, perm_y, perm_z (256 each) as the constructor drew them */
  RT_TEX_VALUE = 4,   /* texture.h:95-103, noise.h:95-137. scale = resolution n; tex_data[data ..]: n^3 values */
  RT_TEX_WORLEY = 5,  /* texture.h:105-111, noise.h:139-168 */
  RT_TEX_VORONOI = 6, /* texture.h:113-119, noise.h:170-201 */
  RT_TEX_IMAGE = 7    /* texture.h:65-78, image.h: color[0] = width, color[1] = height; the pixels are
                         width * height * 3 bytes (row 0 at the top, RGB) at image_data[data]. A 0 x 0
                         image samples as magenta, like a file the reference could not load. */
} rt_texture_kind;

typedef struct rt_texture {
  int32_t kind;
  int32_t data;    /* perlin / value: offset of the texture's tables in rt_scene_desc.tex_data;
                      image: byte offset of its pixels in rt_scene_desc.image_data */
  double color[3]; /* solid */
  double odd[3];   /* checker */
  double even[3];  /* checker */
  double scale;    /* checker, perlin; value: the resolution */
} rt_texture;

typedef struct rt_scene_desc {
  const rt_object* objects;
  int32_t num_objects;
  const int32_t* children;
  int32_t num_children;
  const rt_material* materials;
  int32_t num_materials;
  const rt_texture* textures;
  int32_t num_textures;
  int32_t world;      /* root object: the `world` argument of camera::render */
  int32_t light;      /* object used for importance sampling, or -1 (camera.h:135 `light`) */
  int32_t background; /* texture index of camera::background_, or -1 (camera.h:329) */
  int32_t pad_;
  const double* tex_data; /* procedural-texture tables (rt_texture.data), may be NULL */
  int64_t num_tex_data;
  const uint8_t* image_data; /* picture-texture pixels (rt_texture.data), may be NULL */
  int64_t num_image_data;
} rt_scene_desc;

/* ---- camera: the values camera::initialize_* computes (camera.h:21-132) ---- */

typedef enum rt_camera_mode {
  RT_CAM_PERSPECTIVE = 0, /* camera.h:245-251 */
  RT_CAM_ORTHONORMAL = 1, /* camera.h:252-258 */
  RT_CAM_FISHEYE = 2,     /* camera.h:259-275 */
  RT_CAM_LENS = 3         /* camera.h:276-290 (defocus disk by rejection sampling) */
} rt_camera_mode;

typedef struct rt_camera_desc {
  int32_t mode;
  int32_t image_width;
  int32_t image_height;
  int32_t pad_;
  double pos[3];
  double dir[3];
  double right[3];
  double up[3];
  double viewport_width;
  double viewport_height;
  double focal_length;
  double focus_dist;
  double defocus_u[3];
  double defocus_v[3];
} rt_camera_desc;

/* ---- rendering ---- */

typedef enum rt_precision { RT_PREC_F32 = 0, RT_PREC_F64 = 1 } rt_precision;

typedef struct rt_render_params {
  int32_t spp;              /* camera::samples_per_pixel_ */
  int32_t max_depth;        /* camera::max_recur_depth_ */
  uint64_t seed;            /* counter-RNG key; pixel (x, y) sample s is keyed by (seed, y*W+x, s) */
  int32_t precision;        /* rt_precision */
  int32_t first_sample;     /* render samples [first_sample, first_sample + spp) of each pixel */
  int32_t samples_per_item; /* samples one work item accumulates. 0 = auto, from spp alone: items of 8
                               samples (32 on the flat program), the last half (eighth) of each pixel's
                               samples in items of 4 (8), at most 256 items per pixel; fp64: items of 16.
                               The per-pixel sum is grouped by item, so this changes the image only by
                               rounding. */
  int32_t pool_slots;       /* path slots: lanes of the persistent kernel, or the wavefront pool
                               (0 = auto). Does not change the image. */
  int32_t segments_per_launch; /* 0 = the persistent schedule (one launch, path state in registers);
                                  K > 0 = the wavefront schedule: each path slot advances up to K
                                  segments per launch, state in HBM between launches, live-slot
                                  compaction. Does not change the image. */
  int32_t traversal;        /* rt_traversal: 0 = auto. RT_TRAV_ORDERED keeps the reference-ordered
                               linear program / BVH in fp32 too (the fp32 flat program of quad/box
                               scenes differs from it only in exact-t ties and rounding). */
} rt_render_params;

typedef enum rt_traversal {
  RT_TRAV_AUTO = 0,
  RT_TRAV_ORDERED = 1
} rt_traversal;

/* A framebuffer rectangle. Output of a render call is the tiles packed in the
 * given order, each row-major (top row first, camera.h:170), 3 channels per
 * pixel: float for RT_PREC_F32, double for RT_PREC_F64. The value of a pixel
 * is the mean over its samples (camera.h:169), identical for any tiling, any
 * pool size and any number of GPUs. */
typedef struct rt_tile {
  int32_t x0;
  int32_t y0;
  int32_t width;
  int32_t height;
} rt_tile;

typedef struct rt_counters {
  uint64_t segments;   /* ray segments traced (world.hit calls, camera.h:198) */
  uint64_t samples;    /* camera samples completed */
  uint64_t iterations; /* extend/shade rounds (k_persist launches, or k_step rounds) */
  uint64_t launches;   /* kernel launches */
  double last_render_ms; /* host time of the last rt_render_tiles call (enqueue time when asynchronous) */
  double step_ms; /* device time of the path-step kernels (when timing is enabled): the sum over launches of
                     (end event - start event). Consecutive device-output renders overlap (two launches may be
                     resident, INTEGRATION.md "Streams and ordering"); such a launch counts from the later of its
                     own start event and the end event of the launch before it, so no moment is counted twice:
                     step_ms <= wall time, and in steady state step_ms / iterations is the frame period */
  double aux_ms;  /* rt_multi_stats: device time of the gather + unpack; otherwise 0 */
  uint64_t grid_lanes; /* lanes of the last persistent-kernel launch: the resident grid the occupancy
                          query gave that kernel on this device */
  uint64_t passes;        /* (ABI 8) chunk passes the renders took: a call whose item partial sums exceed
                             the budget (2 GiB, RT_PARTIAL_BUDGET) renders its chunks in several launches */
  uint64_t partial_bytes; /* (ABI 8) the partial-sum buffer of the last render call, bytes */
} rt_counters;

/* What rt_scene_check / rt_scene_upload compiled a descriptor into. */
typedef struct rt_scene_info {
  int32_t quads, spheres, triangles, instances, volumes, bvh_nodes;
  int32_t linear_ops; /* > 0: small scene traversed as a wave-uniform linear program */
  int32_t stack_need; /* traversal stack entries a ray can need (BVH path) */
  uint64_t bytes_f32; /* device scene size, fp32 / fp64 paths */
  uint64_t bytes_f64;
  int32_t flat_quads; /* fp32 flat program (quad/box scenes): world-space axis-aligned quads */
  int32_t flat_boxes; /*   and lambertian boxes traced as one slab test each; 0/0 = none */
  int32_t wide_nodes; /* fp32 wide BVH (world-level primitives): 4-wide nodes; 0 = none */
  int32_t wide_stack; /*   stack entries a ray can need in it */
  int32_t wide_kinds; /*   primitive kinds present: 1 sphere, 2 triangle, 4 quad, 8 moving sphere */
  int32_t wide_prim_words; /* 16-byte words of its primitive records */
  int32_t wide_big;        /*   primitives with scene-sized boxes, tested before its tree (e.g. a ground sphere) */
} rt_scene_info;

typedef struct rt_context rt_context;

/* Library / ABI version, for the binding to check. */
int32_t rt_abi_version(void);

/* The build's compile-time configuration as "key=value" words (e.g. "dev_only=0 wide_top_n=55 ..."), so a
 * harness can tell a development variant (scripts/build_variant.sh) from the product library: a build with
 * dev_only != 0 instantiates one kernel family and answers RT_ERR_UNSUPPORTED for every other. No reference
 * counterpart (the reference has no build variants). */
const char* rt_build_info(void);

/* Create a context on HIP device `device`. */
rt_status rt_context_create(int32_t device, rt_context** out);
void rt_context_destroy(rt_context* ctx);
/* Message for the last failing call on ctx (or the last create failure when ctx == NULL). */
const char* rt_last_error(const rt_context* ctx);

/* Compile the hittable DAG (BVH build, instance transforms, volumes) and upload
 * it. The library copies everything it needs; desc may be freed afterwards. */
rt_status rt_scene_upload(rt_context* ctx, const rt_scene_desc* desc);

/* Host-only: compile the descriptor exactly as rt_scene_upload would, without a
 * device. Returns RT_OK, RT_ERR_INVALID_ARGUMENT or RT_ERR_UNSUPPORTED (message in err). */
rt_status rt_scene_check(const rt_scene_desc* desc, rt_scene_info* info, char* err, int32_t errlen);

/* Render `ntiles` rectangles of the image described by `cam`. With out_is_device = 1 the call
 * is stream-ordered and returns without waiting for the GPU (the output is ready for later work
 * on `stream`); a device-side failure is then reported by the next rt_stats, rt_reset_counters or
 * host-output render. With out_is_device = 0 it returns once out_rgb holds the image. */
rt_status rt_render_tiles(rt_context* ctx, const rt_camera_desc* cam, const rt_render_params* params,
                          const rt_tile* tiles, int32_t ntiles, void* out_rgb, int32_t out_is_device,
                          void* stream);

/* Counters since the last rt_reset_counters; waits for outstanding renders of the context. */
rt_status rt_stats(rt_context* ctx, rt_counters* out);
rt_status rt_reset_counters(rt_context* ctx);

/* 1 = record per-kernel device time with HIP events (slightly perturbs timing). */
rt_status rt_set_timing(rt_context* ctx, int32_t enable);

/* Counter-based RNG of the device path, evaluated on the host (for tests):
 * returns the 32-bit draw for (seed, pixel, sample, dim). */
uint32_t rt_rng_u32(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t dim);

/* ---- ray queries: closest hit of caller-given rays against the uploaded scene ----
 *
 * world.hit(r, interval(0.001, inf), rec) (camera.h:198) for a batch of rays, through the same traversals the
 * render kernels use. No reference counterpart as an entry point: the reference only calls hit from ray_color.
 *
 * rays: nrays x 8 doubles, o[3], d[3], time, tmax. d is not normalised (ray.h); time is the ray time of moving
 * spheres (sphere.h:83). A closest hit with t > tmax is reported as a miss (pass +inf for no limit).
 * RT_PREC_F32 rounds o, d and time to float once; the outputs are doubles for both precisions.
 * out_geom: nrays x 7 doubles, t, p[3], n[3] -- the hit_record values ray_color shades with: world space, the
 * face-forwarded normal (hittable.h:26-29), a moving sphere's normal about center_ (sphere.h:69). A volume hit has
 * n = (1, 0, 0) (volumne.h:40-44). A miss: t = +inf, p = n = 0.
 * out_ids: nrays x 4 int32, object, material, kind, front. object: the index in rt_scene_desc.objects of the
 * sphere, quad, triangle or volume hit; material: that object's rt_object.material; kind: its rt_object_kind;
 * front: hit_record::front_face (1 for a volume). A miss: all -1.
 * volumne::hit draws a random number (volumne.h:36): ray i draws as bounce 0 of the path (seed, pixel = i,
 * sample = 0), its first volume draw being rt_rng_u32(seed, i, 0, 3). */
typedef struct rt_trace_params {
  uint64_t seed;      /* counter-RNG key for volume boundaries */
  int32_t precision;  /* rt_precision */
  int32_t traversal;  /* rt_traversal: AUTO = the family a render of this scene takes, ORDERED = linear program / binary BVH */
  int32_t on_device;  /* 1: rays, out_geom, out_ids are device pointers, call is stream-ordered like rt_render_tiles;
                         0: host pointers, returns when the outputs are filled */
  int32_t pad_;
} rt_trace_params;

typedef enum rt_trace_family_kind {
  RT_TRACE_FLAT = 0,
  RT_TRACE_LINEAR = 1,
  RT_TRACE_WIDE_LDS = 2,
  RT_TRACE_WIDE_HBM = 3,
  RT_TRACE_STACK = 4
} rt_trace_family_kind;

/* RT_ERR_INVALID_ARGUMENT: a null pointer, nrays < 0 or >= 2^31, an unknown precision or traversal, device
 * pointers (on_device = 1) that are not aligned to 16 bytes (rays, out_ids) and 8 bytes (out_geom);
 * RT_ERR_NO_SCENE; RT_ERR_UNSUPPORTED: a family a development build omits. nrays == 0 launches nothing.
 * Adds nrays to rt_counters.segments and 1 to launches; with on_device = 1 the call joins the context's
 * outstanding work exactly as a device-output render does. */
rt_status rt_trace_rays(rt_context* ctx, const rt_trace_params* params, const double* rays, int64_t nrays,
                        double* out_geom, int32_t* out_ids, void* stream);
/* The traversal rt_trace_rays takes for the uploaded scene (rt_trace_family_kind), or -1 without a scene or
 * for an unknown precision or traversal. */
int32_t rt_trace_family(rt_context* ctx, int32_t precision, int32_t traversal);

/* ---- occlusion queries: is anything in the way? (shadow rays, ambient occlusion, line of sight) ----
 *
 * out_occluded[i] = 1 if world.hit(r_i, interval(0.001, tmax_i), rec) is true, else 0: an any-hit query with early
 * exit, one byte a ray. rays: rt_trace_rays' format (nrays x 8 doubles, o[3], d[3] not normalised, time, tmax), so
 * rt_camera_rays' output and existing ray buffers work unchanged; params: rt_trace_params as is. out_occluded needs
 * no alignment, and bytes outside [0, nrays) are never written.
 *
 * Contract: for every ray, out_occluded[i] == 1 exactly when rt_trace_rays, called with the same context, params and
 * ray, reports a hit (finite t) -- both precisions, every family, every traversal, no tolerance. rt_trace_family
 * names the traversal taken. A NaN tmax or one below 0.001 gives 0; tmax = +inf asks "does this ray hit anything".
 *
 * The traversal starts with the interval [0.001, bound] instead of [0.001, inf) and a ray ends at the first
 * primitive that accepts. bound is the largest value of the kernel's precision <= tmax: RT_PREC_F32 rounds tmax
 * toward -inf (+inf stays +inf), so that for a float t, t <= bound is rt_trace_rays' (double)t <= tmax.
 * Volume rule: volumne::hit draws its random numbers after its interval test, with a running slot counter, so a
 * scene with volumes runs rt_trace_rays' closest-hit traversal unchanged (unbounded, no early exit, the same draws:
 * ray i as path (seed, pixel = i, sample = 0)) and compares its t with tmax. RT_PREC_F32 rays through the binary
 * BVH (RT_TRACE_STACK) of a scene with quads do the same, because that traversal re-decides near-edge quad hits with
 * a second distance in fp64 against the interval's upper end.
 *
 * Errors and stream-ordering are rt_trace_rays': RT_ERR_INVALID_ARGUMENT for a null pointer, nrays < 0 or >= 2^31, an
 * unknown precision or traversal, a device rays pointer (on_device = 1) not aligned to 16 bytes; RT_ERR_NO_SCENE;
 * RT_ERR_UNSUPPORTED for a family a development build omits. nrays == 0 launches nothing. Adds nrays to
 * rt_counters.segments and 1 to launches; with on_device = 1 the call joins the context's outstanding work exactly as
 * a device-output render does. */
rt_status rt_occluded(rt_context* ctx, const rt_trace_params* params, const double* rays, int64_t nrays,
                      uint8_t* out_occluded, void* stream);

/* ---- radiance queries: path-traced radiance along caller-given rays (probes, lightmaps, gathers, relighting) ----
 *
 * out_rgb[i] = the mean over samples s in [first_sample, first_sample + spp) of camera::ray_color(ray_i, world,
 * max_depth, light) (camera.h:193-241): what rt_render_tiles computes per pixel, without the camera. No reference
 * counterpart as an entry point: the reference reaches ray_color through camera::render alone.
 *
 * rays: rt_trace_rays' format (nrays x 8 doubles, o[3], d[3] not normalised, time, tmax), so rt_camera_rays' output
 * and existing ray buffers work unchanged. RT_PREC_F32 rounds o, d and time to float once. tmax is not read: the first
 * segment runs over interval(0.001, inf) like every other (camera.h:198). A finite time is the ray time of every
 * sample; a NaN time makes each sample draw its own as camera::generate_ray does, so a moving-sphere scene is
 * motion-blurred per sample like a render.
 * out_rgb: nrays x 3 floats (RT_PREC_F32) or doubles (RT_PREC_F64).
 *
 * Keys: the path of sample s of ray i is keyed (seed, pixel = ray_base + i, sample = s) and draws the counter-RNG
 * dimensions a render's path with that key draws, except 0 and 1 (the pixel jitter), which are never drawn, and 2 (the
 * ray time), drawn only for a NaN time. So ray i with a NaN time equals pixel ray_base + i of an N x 1 image rendered
 * by rt_render_tiles through a perspective camera with pos = o_i, dir = d_i, focal_length = 1 and a zero viewport,
 * with the same seed, spp, first_sample and max_depth -- up to the grouping of the sum over the samples, which
 * follows the item layout (samples_per_item). With samples_per_item given, a ray's value depends on its key and
 * nothing else: a batch split over several calls with matching ray_base gives bit-identical values.
 *
 * The kernel is the persistent path kernel a perspective render of the scene takes (family, shade form, LDS use),
 * in its form that reads the batch; there is no wavefront schedule (no segments_per_launch) for it. */
typedef struct rt_radiance_params {
  uint64_t seed;
  int32_t spp, first_sample; /* samples [first_sample, first_sample + spp) of every ray, spp >= 1; a negative
                                first_sample counts as 0 */
  int32_t max_depth;         /* 0: every ray is black (camera.h:194-195) */
  int32_t precision;         /* rt_precision */
  int32_t traversal;         /* rt_traversal */
  int32_t samples_per_item;  /* as rt_render_params: 0 = automatic */
  uint32_t ray_base;         /* ray i is keyed as pixel ray_base + i */
  int32_t on_device;         /* 1: rays and out_rgb are device pointers, the call is stream-ordered */
} rt_radiance_params;
/* RT_ERR_INVALID_ARGUMENT: a null pointer, nrays < 0 or >= 2^31 (the item planner's limit for one call, whatever
 * spp), ray_base + nrays > 2^32, spp < 1, max_depth < 0, an unknown precision or traversal, device pointers
 * (on_device = 1) not aligned to 16 bytes; RT_ERR_NO_SCENE; RT_ERR_UNSUPPORTED: a family a development build omits.
 * On an error nothing is launched and out_rgb is not written. nrays == 0 launches nothing. Adds nrays * spp to
 * rt_counters.samples, the traced segments to segments and its launches (a path launch and a resolve per chunk pass)
 * to launches; chunk passes and the partial-sum budget are a render's; with on_device = 1 the call joins the
 * context's outstanding work exactly as a device-output render does (its launches stay on `stream`: consecutive
 * batches do not overlap as consecutive frames do). */
rt_status rt_radiance(rt_context* ctx, const rt_radiance_params* params, const double* rays, int64_t nrays,
                      void* out_rgb, void* stream);

/* ---- camera rays and feature buffers (AOVs): what a frame's pixels see first ----
 *
 * rt_camera_rays writes the rays camera::generate_ray (camera.h:244-293) draws for a render, in rt_trace_rays'
 * format: out_rays holds npix * spp rows of 8 doubles, o[3], d[3], time, tmax = +inf. Pixels are those of the tiles,
 * packed as rt_render_tiles packs them; row pix * spp + s is sample first_sample + s of pixel pix, keyed
 * (seed, y * W + x, first_sample + s) like the render's: the same draws (the lens disk's rejection draws and the
 * time draw included), built in fp64 as the render builds them for both precisions. A negative first_sample counts
 * as 0, as in rt_render_params. Needs no scene. on_device / stream: as rt_trace_params.on_device.
 * RT_ERR_INVALID_ARGUMENT: a null pointer, spp < 1, an unknown camera mode, an empty image or one wider or taller
 * than 65535, a tile outside the image, npix * spp >= 2^31, a device out_rays not aligned to 16 bytes. No tile with
 * pixels launches nothing. Does not touch rt_counters. */
rt_status rt_camera_rays(rt_context* ctx, const rt_camera_desc* cam, uint64_t seed, int32_t first_sample, int32_t spp,
                         const rt_tile* tiles, int32_t ntiles, double* out_rays, int32_t on_device, void* stream);

/* rt_render_aov: per pixel the albedo, shading normal, depth and hit share, the guide channels of a denoiser or a
 * compositor, over the same camera samples as the beauty image. No reference counterpart as an entry point: it is
 * the first segment of camera::ray_color (camera.h:193-200) with the hit record and the texture written out.
 *
 * out_feat: npix x 8 doubles, albedo[3], normal[3], depth, hit; tiles packed as in rt_render_tiles. Every channel
 * is (1 / spp) x the sum over samples [first_sample, first_sample + spp) of the pixel, added in increasing sample
 * order in double for both precisions: a pixel's value does not depend on the tiling, the tile order or the GPU.
 * A sample's ray is rt_camera_rays' and goes through world.hit(r, interval(0.001, inf)) as in rt_trace_rays. It adds
 *   albedo  on a hit the hit material's texture (rt_material.texture; a volume's phase material's) sampled at the
 *           hit's (u, v, p) -- the value ray_color uses as attenuation or emission; u, v a quad's alpha, beta
 *           (quad.h:58-62), a sphere's get_sphere_uv (sphere.h:70), 0 for triangles and volumes. On a miss what
 *           camera::miss returns (camera.h:180-190): the background texture through its unit-sphere test, or 0;
 *   normal  on a hit rt_trace_rays' n (face-forwarded, world space; a moving sphere's is not a unit vector, a
 *           volume's is (1, 0, 0)), 0 on a miss;
 *   depth   on a hit t |d|, the distance from the ray's origin, 0 on a miss;
 *   hit     1 on a hit, 0 on a miss (divide the other sums by it for means over the hits).
 * out_ids: npix x 4 int32, object, material, kind, front of sample first_sample as rt_trace_rays reports them
 * (a miss: all -1).
 * volumne::hit draws as bounce 0 of the pixel's own path (seed, y * W + x, sample). With spp = 1, first_sample = 0
 * and one tile that is the whole image, ray index equals pixel index and the pass equals rt_trace_rays on
 * rt_camera_rays' output, volume scenes included. */
typedef struct rt_aov_params {
  uint64_t seed;
  int32_t spp, first_sample; /* camera samples [first_sample, first_sample + spp) of each pixel, spp >= 1 */
  int32_t precision;         /* rt_precision: the traversal's arithmetic; the outputs are doubles either way */
  int32_t traversal;         /* rt_traversal */
  int32_t on_device, pad_;   /* 1: out_feat and out_ids are device pointers, the call is stream-ordered */
} rt_aov_params;
/* The errors of rt_camera_rays and rt_trace_rays (device out_feat and out_ids aligned to 16 bytes), and
 * RT_ERR_NO_SCENE. The traversal is rt_trace_family's, except that a scene with an RT_TEX_IMAGE texture leaves the
 * flat program for the linear one (the flat program's hit carries no u, v). Adds npix * spp to rt_counters.segments
 * and 1 to launches; with on_device = 1 the call joins the context's outstanding work as a device-output render. */
rt_status rt_render_aov(rt_context* ctx, const rt_camera_desc* cam, const rt_aov_params* params, const rt_tile* tiles,
                        int32_t ntiles, double* out_feat, int32_t* out_ids, void* stream);

/* ---- adaptive sampling: a per-pixel noise estimate, and samples only where they still help ----
 *
 * rt_render_adaptive renders the tiles' pixels in rounds and stops each pixel once its estimated error is small
 * enough. No reference counterpart: camera::render gives every pixel samples_per_pixel samples.
 *
 * Sampling. A pixel's samples come in batches of `batch` consecutive samples: batch k is samples
 * [k * batch, (k + 1) * batch) of the key (seed, y * W + x), the samples rt_render_tiles draws for that pixel. The
 * first round renders samples [0, min_spp) of every pixel; each later round the next step_spp samples of the pixels
 * still active. A round is a render with samples_per_item = batch and first_sample = the samples the active pixels
 * have, over the list of active pixels in place of tiles: an item is a batch, and chunk passes under the partial-sum
 * budget apply as for a render.
 *
 * Estimator (the method of batch means). s_k: the three sums batch k's item wrote (floats or doubles, by the
 * precision), converted to double. Per channel, in double and in batch order, S_c = sum s_k,c and Q_c = sum s_k,c^2
 * over the K batches so far. With N = K * batch:
 *   mean_c = S_c / N                                     (rounded once to the precision for out_rgb)
 *   var_c  = max(0, Q_c - S_c^2 / K) / (K - 1)           (a NaN stays a NaN)
 *   se2    = (var_r + var_g + var_b) / (K * batch^2)     the summed variance of the three channel means
 *   err    = sqrt(se2 / 3) / (floor + (mean_r + mean_g + mean_b) / 3)
 * err is the RMS standard error of the channels relative to the pixel's level; `floor` makes it absolute in dark
 * pixels. A pixel stops after a round when err <= threshold or N >= max_spp. A NaN err fails the comparison, so such
 * a pixel runs to max_spp. threshold = 0 takes every pixel with any variance to max_spp (a fixed-spp render with a
 * noise map); threshold = +inf stops every pixel at min_spp. max_depth = 0 gives black pixels with err = 0 that stop
 * at min_spp.
 *
 * Outputs, packed by tile exactly as rt_render_tiles packs them: out_rgb npix x 3 floats (RT_PREC_F32) or doubles
 * (RT_PREC_F64), out_spp the samples each pixel took, out_err each pixel's final err. None may be NULL.
 *
 * A pixel's three outputs depend on (seed, pixel) and the parameters alone: not on the tiling, the tile order, the
 * other pixels of the call, the partial-sum budget or the device. The image is bit-identical for any split of the
 * frame. Only the persistent schedule is used, as for rt_radiance, and the kernel is the one a render of that scene
 * and camera takes, unchanged.
 *
 * Stream and ordering. The host must know each round's count of active pixels: the call waits on `stream` once per
 * round (a 4-byte read), but not after the last round when on_device = 1. The outputs are ordered on `stream` like a
 * device-output render's, and the call joins the context's outstanding work the same way; its launches stay on
 * `stream` (they do not overlap as consecutive frames do). */
typedef struct rt_adaptive_params {
  uint64_t seed;
  int32_t min_spp, max_spp, step_spp, batch; /* batch >= 1; step_spp a multiple of batch; min_spp and max_spp
                                                multiples of step_spp; 2 * batch <= min_spp <= max_spp */
  int32_t max_depth;                         /* >= 0 */
  int32_t precision;                         /* rt_precision */
  int32_t traversal;                         /* rt_traversal */
  int32_t on_device;         /* 1: the three outputs are device pointers (16-byte aligned), the call is stream-ordered */
  double threshold, floor;   /* threshold >= 0 (+inf allowed), not NaN; floor > 0 and finite */
} rt_adaptive_params;        /* 56 bytes, no padding */
/* RT_ERR_INVALID_ARGUMENT: a null pointer, parameters that break the rules above (rt_adaptive_check), rt_render_tiles'
 * errors for the camera and the tiles, device pointers (on_device = 1) not aligned to 16 bytes; RT_ERR_NO_SCENE;
 * RT_ERR_UNSUPPORTED: a family a development build omits. On an error nothing is launched and nothing is written. No
 * pixels: nothing is launched. Adds the sum of out_spp to rt_counters.samples; segments, launches and passes grow as
 * the rounds' launches and resolves add them. */
rt_status rt_render_adaptive(rt_context* ctx, const rt_camera_desc* cam, const rt_adaptive_params* params,
                             const rt_tile* tiles, int32_t ntiles, void* out_rgb, int32_t* out_spp, double* out_err,
                             void* stream);
/* The parameter rules alone, on the host (no device): RT_OK, or RT_ERR_INVALID_ARGUMENT with the message in err. */
rt_status rt_adaptive_check(const rt_adaptive_params* params, char* err, int32_t errlen);
/* The estimator's arithmetic as the kernel runs it, on the host, for tests: from K batches of `batch` samples with the
 * sums S[3] and Q[3] to mean3[3] (in double) and *err. A development helper with no stability promise. */
void rt_dev_adaptive_error(int32_t K, int32_t batch, const double* S, const double* Q, double floor, double* mean3,
                           double* err);

/* ---- denoising: a variance-guided a-trous filter over the guide channels ----
 *
 * rt_denoise filters a whole row-major width x height image with an edge-avoiding a-trous wavelet filter (Dammertz et
 * al. 2010) whose colour edge-stop scales with each pixel's own variance and which carries that variance from pass to
 * pass (Schied et al. 2017, SVGF). It is spatial and single-frame: no history, no motion vectors (the temporal half,
 * reprojected accumulation over frames, is rt_temporal below, whose outputs feed this call). No reference
 * counterpart. It needs no scene.
 *
 * rgb_in: npix x 3 floats (RT_PREC_F32) or doubles (RT_PREC_F64), e.g. rt_render_tiles' or rt_render_adaptive's image.
 * feat:   npix x 8 doubles, rt_render_aov's rows: albedo[3], normal[3], depth, hit (depth a distance, >= 0).
 * var:    npix doubles or NULL: the summed variance of the three channel means, the estimator's se2 above; from
 *         rt_render_adaptive's out_err it is (err * (floor + level))^2 * 3 with level the mean of the pixel's channels.
 * rgb_out: npix x 3 of the precision's type; may be rgb_in.
 *
 * All arithmetic is in T, float or double by the precision.
 * Prepare, per pixel p. hit > 0: n = normal / hit, z = depth / hit; else n = 0, z = -1, a "miss pixel".
 *   a = albedo + albedo_eps per channel with RT_DENOISE_DEMODULATE, else 1; c = rgb / a.
 *   v0 = var / 3 / mean(a)^2 and v = the 3 x 3 binomial ([1 2 1] / 4 per axis) mean of v0, taps outside the image
 *   skipped and the weights renormalised. var == NULL: v = 1, and sigma_color is an absolute colour distance.
 *   g = (gx, gy), the depth gradient in depth per pixel, per axis: the mean of the forward and the backward difference
 *   where both exist, the one that exists, or 0; a difference exists when both pixels are inside the image and
 *   neither is a miss pixel.
 * Pass k = 0 .. iterations - 1 with step s = 2^k, over the taps q = p + s (i, j), i, j in -2 .. 2 (j outer, i inner),
 * taps outside the image skipped, h = [1 4 6 4 1] / 16:
 *   d_c = mean over channels of (c_p - c_q)^2 / (sigma_color^2 v_p + color_eps)
 *   d_n = |n_p - n_q|^2 / sigma_normal^2
 *   d_z = 0 for two miss pixels; the tap is skipped when exactly one is a miss pixel; 0 when z_p == z_q; otherwise
 *         |z_p - z_q| / (sigma_depth |gx s i + gy s j| + depth_eps |z_p|)
 *   w = h_i h_j exp(-(d_c + d_n + d_z));   c'_p = sum w c_q / sum w;   v'_p = sum w^2 v_q / (sum w)^2
 * A tap whose c_q or v_q is not finite is skipped; a pixel whose c_p or v_p is not finite has d_c = 0 for every tap
 * (it is rebuilt from its neighbours); with no tap left c' = v' = 0. The last pass writes c' a to rgb_out.
 *
 * on_device = 1: the four pointers are device pointers aligned to 16 bytes and the call is ordered on `stream` like
 * rt_trace_rays; 0: host pointers, the call returns when rgb_out is filled. The launches stay on the caller's stream.
 * Whole images only (a filter needs its neighbours): with several GPUs, denoise the gathered frame. The scratch,
 * 14 T a pixel, belongs to the context, grows on demand and is no part of the partial-sum budget.
 * Adds iterations + 1 to rt_counters.launches and nothing else. */
#define RT_DENOISE_DEMODULATE 1
typedef struct rt_denoise_params {
  int32_t width, height, iterations, precision, on_device, flags;
  double sigma_color, sigma_normal, sigma_depth, albedo_eps, color_eps, depth_eps;
} rt_denoise_params; /* 72 bytes, no padding */
/* The parameter rules alone, on the host (no device): sides in [1, 65535] with width * height < 2^31, iterations in
 * [1, 8], a known precision, flags within RT_DENOISE_DEMODULATE, the sigmas finite and > 0, the eps finite and >= 0,
 * albedo_eps > 0 when demodulating. RT_OK, or RT_ERR_INVALID_ARGUMENT with the reason in why (n bytes). */
rt_status rt_denoise_check(const rt_denoise_params* params, char* why, size_t n);
/* RT_ERR_INVALID_ARGUMENT: a null pointer (var excepted), parameters rt_denoise_check refuses, device pointers not
 * aligned to 16 bytes. On an error nothing is launched and nothing is written. */
rt_status rt_denoise(rt_context* ctx, const rt_denoise_params* params, const void* rgb_in, const double* feat,
                     const double* var, void* rgb_out, void* stream);

/* ---- temporal accumulation: last frame's accumulated image reprojected into this frame ----
 *
 * rt_temporal is the temporal half of SVGF (Schied et al. 2017): it reprojects the accumulated image of the frame
 * before into this frame through the two cameras and this frame's depth, rejects history that no longer shows the
 * same surface, blends, and hands on a variance that has shrunk accordingly. Static scenes only: between the frames
 * the camera moves, the objects do not. No reference counterpart. It needs no scene. Whole row-major width x height
 * images, as for rt_denoise; T is float (RT_PREC_F32) or double (RT_PREC_F64).
 *
 * Inputs of this frame: rgb_in npix x 3 T; feat npix x 8 doubles, rt_render_aov's rows; ids npix x 4 int32,
 * rt_render_aov's out_ids, of which only `object` is read, or NULL; var npix doubles, rt_denoise's var (the summed
 * variance of the three channel means), or NULL.
 * History: caller-owned, rt_temporal_history_bytes bytes, four planes in this order:
 *   npix records {c.r, c.g, c.b, v}  4 T   the accumulated demodulated colour and the variance of a channel of it
 *   npix records {n.x, n.y, n.z, z}  4 T   the guides of the frame that wrote it (a miss pixel: n = 0, z = -1)
 *   npix counts N                    T     the frames accumulated, 0 = no usable history
 *   npix object ids                  int32 (-2 = unknown: ids was NULL)
 * hist_in == NULL is a first frame: no pixel has history, and prev_cam may be NULL. hist_in and hist_out must not
 * overlap (the call gathers from one while it writes the other). The caller swaps the two between frames.
 * Outputs: rgb_out npix x 3 T, may be rgb_in; var_out npix doubles or NULL, may be var.
 *
 * Per pixel p = (x, y). Steps 1 and 4 and the sums of step 3 are in T; step 2, the bilinear weights and the tests
 * of step 3 are in double for both precisions.
 * 1. The current sample. a = rt_denoise's albedo factor (albedo + albedo_eps per channel with
 *    RT_TEMPORAL_DEMODULATE, else 1); c_cur = rgb / a; v_cur = var / 3 / mean(a)^2, or 1 with var == NULL; n, z as
 *    rt_denoise prepares them: hit > 0: n = normal / hit, z = depth / hit; else n = 0, z = -1, a miss pixel. The
 *    pixel's id is ids' object, or -2 with ids == NULL.
 * 2. Where p was. If *cam and *prev_cam are byte-equal: (fx, fy) = (x, y) and z' = z exactly, for every camera mode.
 *    Otherwise both are RT_CAM_PERSPECTIVE with the image size of params (anything else: RT_ERR_UNSUPPORTED), and
 *      d_c = focal_length dir + ((x + 0.5) / W - 0.5) viewport_width right + (0.5 - (y + 0.5) / H) viewport_height up
 *    (the direction of the pixel's camera ray with a zero jitter). A hit pixel sees X = pos + d_c / |d_c| z (the depth
 *    is a distance); r = X - prev.pos and z' = |r|. A miss pixel sees the point at infinity: r = d_c. With
 *    A = r . dir' / |dir'|^2 and B, C the same against right' and up' of prev_cam: A <= 0, or an fx or fy that is not
 *    finite: no history. Otherwise
 *      fx = (B f' / A / vw' + 0.5) W - 0.5,   fy = (0.5 - C f' / A / vh') H - 0.5.
 * 3. The taps: the four pixels q = (floor(fx) + i, floor(fy) + j), i, j in 0 .. 1 (j outer, i inner), with their
 *    bilinear weights w_q; a tap with w_q == 0 or outside the image is skipped. A tap is valid when its {c, v} is
 *    finite, N_q > 0 and: for a miss pixel p, q is a miss pixel (z_q < 0); for a hit pixel p, q is a hit pixel with
 *    |z_q - z'| <= depth_tol z', n_p . n_q >= normal_cos, and an equal object id or either id unknown.
 *    Wv = sum of w_q over the valid taps. History exists when Wv >= min_weight and Wv > 0; then
 *      c_h = sum w_q c_q / Wv,   v_h = sum w_q^2 v_q / Wv^2 (rt_denoise's rule),   N_h = sum w_q N_q / Wv.
 * 4. The blend. With history: alpha = max(alpha_min, 1 / (N_h + 1)), c = (1 - alpha) c_h + alpha c_cur,
 *    v = (1 - alpha)^2 v_h + alpha^2 v_cur, N = min(N_h + 1, max_history). Without: c = c_cur, v = v_cur, N = 1.
 *    If c_cur or v_cur is not finite the frame contributes nothing: with history c, v, N = c_h, v_h, N_h; without,
 *    the record is stored as it is with N = 0, so it is never a valid tap later.
 * 5. The history record of p in hist_out is {c, v}, {n, z} of this frame, N and the pixel's id;
 *    rgb_out = c a; var_out = 3 mean(a)^2 v.
 *
 * Consequences. With byte-equal cameras, the same feat, alpha_min = 0, normal_cos = -1 and max_history above the
 * frame count, the output of frame k is the running mean of the k inputs and N = k (progressive rendering over
 * first_sample), and var_out is the exact variance of that mean under independence: the mean of the k var divided by
 * k. var_out has var's meaning and feeds rt_denoise unchanged. (normal_cos = -1 because n is rt_render_aov's mean
 * over the pixel's samples, not a unit vector: where a pixel straddles an edge n . n < 1, and a normal_cos near 1
 * rejects such a pixel's own history. On a moving camera that costs the edge pixels their history and nothing else.)
 *
 * on_device = 1: every pointer is a device pointer aligned to 16 bytes and the call is ordered on `stream` like
 * rt_denoise; 0: host pointers, the call returns when the outputs and hist_out are filled. The launch stays on the
 * caller's stream. Whole images only: with several GPUs, accumulate the gathered frame.
 * Adds exactly 1 to rt_counters.launches and nothing else. */
#define RT_TEMPORAL_DEMODULATE 1
typedef struct rt_temporal_params {
  int32_t width, height, precision, on_device, flags, max_history;
  double alpha_min, depth_tol, normal_cos, min_weight, albedo_eps;
} rt_temporal_params; /* 64 bytes, no padding */
/* The rules alone, on the host (no device). The parameters: sides in [1, 65535] with width * height < 2^31, a known
 * precision, flags within RT_TEMPORAL_DEMODULATE, max_history >= 1, alpha_min in [0, 1], depth_tol finite and > 0,
 * normal_cos in [-1, 1], min_weight in [0, 1), albedo_eps finite and >= 0, > 0 when demodulating: else
 * RT_ERR_INVALID_ARGUMENT, as for a null params or cam. The cameras, when prev_cam is not NULL: step 2's rule, else
 * RT_ERR_UNSUPPORTED. The reason goes to why (n bytes). */
rt_status rt_temporal_check(const rt_temporal_params* params, const rt_camera_desc* cam, const rt_camera_desc* prev_cam,
                            char* why, size_t n);
/* The bytes of a history of that size and precision, width * height * (9 sizeof(T) + 4); 0 for sides or a precision
 * rt_temporal_check refuses. */
size_t rt_temporal_history_bytes(int32_t width, int32_t height, int32_t precision);
/* RT_ERR_INVALID_ARGUMENT: a null pointer (ids, var, hist_in, var_out excepted; prev_cam only with hist_in == NULL),
 * parameters rt_temporal_check refuses, hist_in and hist_out that overlap, device pointers not aligned to 16 bytes;
 * RT_ERR_UNSUPPORTED: cameras that differ and are not both perspective cameras of the image's size. On an error
 * nothing is launched and nothing is written. */
rt_status rt_temporal(rt_context* ctx, const rt_temporal_params* params, const rt_camera_desc* cam,
                      const rt_camera_desc* prev_cam, const void* rgb_in, const double* feat, const int32_t* ids,
                      const double* var, const void* hist_in, void* hist_out, void* rgb_out, double* var_out,
                      void* stream);

/* ---- multi-GPU driver: the framebuffer tiled over the devices of one node ----
 *
 * Replaces camera::render's per-row std::for_each(par_unseq) (camera.h:154-172) when a
 * scene is rendered on several GPUs. Tiles of tile_size x tile_size pixels (row-major
 * over the image) are dealt round-robin: device k renders tiles k, k + n, k + 2n, ...
 * packed in that order into a buffer padded to the largest device's pixel count; one
 * ncclGather (RCCL over xGMI) brings the n buffers to devices[0], which unpacks them into
 * the linear framebuffer (row 0 at the top, camera.h:170) and copies it to the host.
 * Every pixel's samples are keyed by (seed, pixel, sample), so the image is bit-identical
 * for any device count. A device list that repeats a device (tests on a one-GPU box)
 * renders those ranks on the same device one after another and gathers with device copies
 * instead of RCCL (rt_multi_uses_rccl says which). */
typedef struct rt_multi rt_multi;

rt_status rt_multi_create(const int32_t* devices, int32_t ndev, rt_multi** out);
void rt_multi_destroy(rt_multi* m);
/* Message of the last failing call on m (or the last create failure when m == NULL). */
const char* rt_multi_last_error(const rt_multi* m);
/* 1 when the gather runs through an RCCL communicator, 0 for the device-copy gather. */
int32_t rt_multi_uses_rccl(const rt_multi* m);
/* rt_scene_upload on every device. */
rt_status rt_multi_scene_upload(rt_multi* m, const rt_scene_desc* desc);
/* The whole image into out_rgb: host memory, W * H * 3 floats (RT_PREC_F32) or doubles (RT_PREC_F64),
 * row-major, top row first. tile_size <= 0 selects 16. */
rt_status rt_multi_render(rt_multi* m, const rt_camera_desc* cam, const rt_render_params* params,
                          int32_t tile_size, void* out_rgb);
/* Counters of rank `rank` (0 <= rank < ndev) since rt_multi_create; aux_ms of rank 0 holds the
 * device time of the last gather + unpack. */
rt_status rt_multi_stats(rt_multi* m, int32_t rank, rt_counters* out);
/* Host-only tile plan: writes rank `rank`'s tiles (at most cap; tiles_out may be NULL) and returns
 * how many it has, or -1 for invalid arguments. */
int32_t rt_multi_plan(int32_t width, int32_t height, int32_t ndev, int32_t tile_size, int32_t rank,
                      rt_tile* tiles_out, int32_t cap);
/* RCCL communicators this process has created (ncclCommInitAll calls by rt_multi_create): a
 * camera that renders again on the same devices_ keeps its rt_multi, so the count stays put. */
uint64_t rt_multi_comm_inits(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */
