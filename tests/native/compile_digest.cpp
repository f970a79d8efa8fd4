// Digests of everything the scene compiler emits (tests/test_compile_digest.py): compiled with csrc/scene_compile.cpp
// by a plain C++ compiler. Each argument is a file holding one serialised rt_scene_desc:
//   "RTDESC1\0", then 12 int64: sizeof(rt_object), sizeof(rt_material), sizeof(rt_texture), num_objects, num_children,
//   num_materials, num_textures, num_tex_data, num_image_data, world, light, background,
//   then the arrays as they lie in memory: objects, children, materials, textures, tex_data, image_data.
// Prints one line per file:
//   <file stem> status <s> hdr <fnv>:<bytes> hdr64 .. blob32 .. blob64 .. ids .. room_masks .. ids_off <4> stack_need <n>
//   bvh_depth <n> num_items <n> desc_quads <n> flat_quads <n> flat_boxes <n> flat_rooms <n>
// or, when the compile fails, <file stem> status <s> error <text>. fnv: 64-bit FNV-1a of the bytes, in hex.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scene_compile.h"

namespace {

uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

template <class T>
bool read_array(std::FILE* f, std::vector<T>& v, int64_t n) {
  if (n < 0) return false;
  v.resize((size_t)n);
  return n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

int digest(const char* path) {
  std::string stem = path;
  stem = stem.substr(stem.find_last_of('/') + 1);
  stem = stem.substr(0, stem.find_last_of('.'));
  std::FILE* f = std::fopen(path, "rb");
  char magic[8];
  int64_t h[12];
  if (!f || std::fread(magic, 1, 8, f) != 8 || std::memcmp(magic, "RTDESC1", 8) != 0 || std::fread(h, 8, 12, f) != 12 ||
      h[0] != (int64_t)sizeof(rt_object) || h[1] != (int64_t)sizeof(rt_material) || h[2] != (int64_t)sizeof(rt_texture)) {
    std::fprintf(stderr, "%s: not a descriptor dump of this ABI\n", path);
    return 1;
  }
  std::vector<rt_object> objects;
  std::vector<int32_t> children;
  std::vector<rt_material> materials;
  std::vector<rt_texture> textures;
  std::vector<double> tex_data;
  std::vector<uint8_t> image_data;
  const bool ok = read_array(f, objects, h[3]) && read_array(f, children, h[4]) && read_array(f, materials, h[5]) &&
                  read_array(f, textures, h[6]) && read_array(f, tex_data, h[7]) && read_array(f, image_data, h[8]) &&
                  std::fgetc(f) == EOF;
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "%s: arrays do not match their counts\n", path);
    return 1;
  }
  rt_scene_desc d{};
  d.objects = objects.data();
  d.num_objects = (int32_t)objects.size();
  d.children = children.data();
  d.num_children = (int32_t)children.size();
  d.materials = materials.data();
  d.num_materials = (int32_t)materials.size();
  d.textures = textures.data();
  d.num_textures = (int32_t)textures.size();
  d.tex_data = tex_data.empty() ? nullptr : tex_data.data();
  d.num_tex_data = (int64_t)tex_data.size();
  d.image_data = image_data.empty() ? nullptr : image_data.data();
  d.num_image_data = (int64_t)image_data.size();
  d.world = (int32_t)h[9];
  d.light = (int32_t)h[10];
  d.background = (int32_t)h[11];
  rtd::CompiledScene cs;
  std::string err;
  const rt_status st = rtd::compile_scene(&d, &cs, &err);
  if (st != RT_OK) {
    std::printf("%s status %d error %s\n", stem.c_str(), (int)st, err.c_str());
    return 0;
  }
  std::printf("%s status %d", stem.c_str(), (int)st);
  auto put = [](const char* name, const void* p, size_t n) {
    std::printf(" %s %016llx:%zu", name, (unsigned long long)fnv1a(p, n), n);
  };
  put("hdr", &cs.hdr, sizeof cs.hdr);
  put("hdr64", &cs.hdr64, sizeof cs.hdr64);
  put("blob32", cs.blob32.data(), cs.blob32.size());
  put("blob64", cs.blob64.data(), cs.blob64.size());
  put("ids", cs.ids.data(), cs.ids.size() * sizeof(int32_t));
  put("room_masks", cs.room_masks.data(), cs.room_masks.size() * sizeof(uint32_t));
  std::printf(" ids_off %u %u %u %u stack_need %d bvh_depth %d num_items %d desc_quads %d flat_quads %d flat_boxes %d "
              "flat_rooms %d\n",
              cs.ids_off[0], cs.ids_off[1], cs.ids_off[2], cs.ids_off[3], cs.stack_need, cs.bvh_depth, cs.num_items,
              cs.desc_quads, cs.flat_quads, cs.flat_boxes, cs.flat_rooms);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++)
    if (digest(argv[i])) return 1;
  return 0;
}
