// scene_compile.h -- compile an rt_scene_desc (the reference's hittable DAG)
// into the device layout of rt_scene.h. Host-only C++; no HIP calls.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_scene.h"

namespace rtd {

struct CompiledScene {
  SceneHeader hdr{};
  std::vector<unsigned char> blob32;  // fp32 records, offsets in hdr
  std::vector<unsigned char> blob64;  // fp64 records, same offsets scaled (hdr64)
  SceneHeader hdr64{};
  int stack_need = 0;  // traversal stack entries a lane can need
  int bvh_depth = 0;
  int num_items = 0;
  int desc_quads = 0;  // quads of the descriptor (the flat program adds face copies)
  int flat_quads = 0, flat_boxes = 0;  // flat_quads counts the faces of rooms too (they are the scene's quads)
  int flat_rooms = 0;                  // rooms of the fp64 flat program (rt_scene.h FlatRoomT)
  std::vector<uint32_t> room_masks;    // their present masks
  // For ray queries (rt_trace_rays), outside the blobs (the render kernels never read it): the descriptor object
  // behind every device record and that object's rt_object.material, as (object, material) pairs -- the quad
  // records first (the flat program's face copies and its alignment padding included: same indices as the blob),
  // then the sphere, triangle and volume records from ids_off[1], [2], [3] (pairs; ids_off[0] = 0).
  std::vector<int32_t> ids;
  uint32_t ids_off[4] = {0, 0, 0, 0};
};

// Returns RT_OK or an error with a message.
rt_status compile_scene(const rt_scene_desc* desc, CompiledScene* out, std::string* err);

}  // namespace rtd
