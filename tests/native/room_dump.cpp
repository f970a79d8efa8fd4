// What the scene compiler's flat program makes of a scene's walls (tests/test_room_compile.py): compiled with
// csrc/scene_compile.cpp by a plain C++ compiler, prints one line per scene
//   <name> flat <0|1> quads <x> <y> <z> boxes <n> rooms <n> masks <m,...|-> inst <i,...|-> info <flat_quads> <flat_boxes> <quad records>
// (quads per plane axis, boxes and rooms of the fp64 blob's header; inst: each room's instance, -1 = world)
#include <cstdio>
#include <string>
#include <vector>

#include "scene_compile.h"

namespace {

struct Scene {
  std::vector<rt_object> objs;
  std::vector<int32_t> children;
  std::vector<rt_material> mats;
  std::vector<rt_texture> texs;
  int mat(int kind, double r, double g, double b) {
    rt_texture t{};
    t.kind = RT_TEX_SOLID;
    t.color[0] = r, t.color[1] = g, t.color[2] = b;
    texs.push_back(t);
    rt_material m{};
    m.kind = kind;
    m.texture = (int)texs.size() - 1;
    mats.push_back(m);
    return (int)mats.size() - 1;
  }
  int quad(double qx, double qy, double qz, double ux, double uy, double uz, double vx, double vy, double vz, int m) {
    rt_object o{};
    o.kind = RT_OBJ_QUAD;
    o.material = m;
    o.child = -1;
    o.a[0] = qx, o.a[1] = qy, o.a[2] = qz;
    o.b[0] = ux, o.b[1] = uy, o.b[2] = uz;
    o.c[0] = vx, o.c[1] = vy, o.c[2] = vz;
    objs.push_back(o);
    return (int)objs.size() - 1;
  }
  int list(const std::vector<int>& kids, int kind = RT_OBJ_LIST) {
    rt_object o{};
    o.kind = kind;
    o.material = -1;
    o.child = -1;
    o.first_child = (int)children.size();
    o.child_count = (int)kids.size();
    for (int k : kids) children.push_back(k);
    objs.push_back(o);
    return (int)objs.size() - 1;
  }
  int translate(int child, double x, double y, double z) {
    rt_object o{};
    o.kind = RT_OBJ_TRANSLATE;
    o.material = -1;
    o.child = child;
    o.a[0] = x, o.a[1] = y, o.a[2] = z;
    objs.push_back(o);
    return (int)objs.size() - 1;
  }
  // the faces of [0, s]^3 (wall f on plane lo (even f) or hi (odd f) of axis f / 2), each with its material
  std::vector<int> walls(double sx, double sy, double sz, const std::vector<int>& faces, const int* m) {
    std::vector<int> out;
    for (int f : faces) {
      switch (f) {
        case 0: out.push_back(quad(0, 0, 0, 0, sy, 0, 0, 0, sz, m[f])); break;
        case 1: out.push_back(quad(sx, 0, 0, 0, sy, 0, 0, 0, sz, m[f])); break;
        case 2: out.push_back(quad(0, 0, 0, sx, 0, 0, 0, 0, sz, m[f])); break;
        case 3: out.push_back(quad(sx, sy, sz, -sx, 0, 0, 0, 0, -sz, m[f])); break;
        case 4: out.push_back(quad(0, 0, 0, sx, 0, 0, 0, sy, 0, m[f])); break;
        default: out.push_back(quad(0, 0, sz, sx, 0, 0, 0, sy, 0, m[f])); break;
      }
    }
    return out;
  }
  // box() of the reference's quad.h: six quads in a list, one material
  int box(double ax, double ay, double az, double bx, double by, double bz, int m) {
    const double dx = bx - ax, dy = by - ay, dz = bz - az;
    return list({quad(ax, ay, bz, dx, 0, 0, 0, dy, 0, m), quad(bx, ay, bz, 0, 0, -dz, 0, dy, 0, m),
                 quad(bx, ay, az, -dx, 0, 0, 0, dy, 0, m), quad(ax, ay, az, 0, 0, dz, 0, dy, 0, m),
                 quad(ax, by, bz, dx, 0, 0, 0, 0, -dz, m), quad(ax, ay, az, dx, 0, 0, 0, 0, dz, m)});
  }
  void dump(const char* name, int world, int light) {
    rt_scene_desc d{};
    d.objects = objs.data();
    d.num_objects = (int)objs.size();
    d.children = children.data();
    d.num_children = (int)children.size();
    d.materials = mats.data();
    d.num_materials = (int)mats.size();
    d.textures = texs.data();
    d.num_textures = (int)texs.size();
    d.world = world;
    d.light = light;
    d.background = -1;
    rtd::CompiledScene cs;
    std::string err;
    if (rtd::compile_scene(&d, &cs, &err) != RT_OK) {
      std::printf("%s error %s\n", name, err.c_str());
      return;
    }
    const rtd::SceneHeader& h = cs.hdr64;
    std::printf("%s flat %u quads %u %u %u boxes %u rooms %u masks ", name, h.has_flat, h.n_flat_quad[0], h.n_flat_quad[1],
                h.n_flat_quad[2], h.n_flat_box, h.n_flat_room);
    const rtd::FlatRoomT<double>* r = (const rtd::FlatRoomT<double>*)(cs.blob64.data() + h.off_flat_room);
    for (uint32_t k = 0; k < h.n_flat_room; k++) std::printf("%s%u", k ? "," : "", r[k].present);
    std::printf("%s inst ", h.n_flat_room ? "" : "-");
    for (uint32_t k = 0; k < h.n_flat_room; k++) std::printf("%s%d", k ? "," : "", r[k].inst);
    std::printf("%s info %d %d %u\n", h.n_flat_room ? "" : "-", cs.flat_quads, cs.flat_boxes, h.n_quads);
  }
};

}  // namespace

int main() {
  const std::vector<int> all = {0, 1, 2, 3, 4, 5};
  {  // the Cornell box of the reference's main.cc: five walls (z = 0 open), two boxes, the light
    Scene s;
    const int red = s.mat(RT_MAT_LAMBERTIAN, .65, .05, .05), white = s.mat(RT_MAT_LAMBERTIAN, .73, .73, .73);
    const int green = s.mat(RT_MAT_LAMBERTIAN, .12, .45, .15), light = s.mat(RT_MAT_DIFFUSE_LIGHT, 15, 15, 15);
    const int m[6] = {red, green, white, white, white, white};
    std::vector<int> w = s.walls(555, 555, 555, {1, 0, 2, 3, 5}, m);
    w.push_back(s.translate(s.box(0, 0, 0, 165, 330, 165, white), 100, 0, 200));
    w.push_back(s.translate(s.box(0, 0, 0, 165, 165, 165, white), 50, 0, 100));
    const int lq = s.quad(343, 554, 332, -130, 0, 0, 0, 0, -105, light);
    w.push_back(lq);
    s.dump("cornell", s.list(w, RT_OBJ_BVH), lq);
  }
  auto room = [&](const char* name, const std::vector<int>& faces, double sx, double sy, double sz, int variant) {
    Scene s;
    const int a = s.mat(RT_MAT_LAMBERTIAN, .6, .2, .2), b = s.mat(RT_MAT_LAMBERTIAN, .7, .7, .7);
    const int metal = s.mat(RT_MAT_METAL, .8, .8, .9), light = s.mat(RT_MAT_DIFFUSE_LIGHT, 9, 9, 9);
    const int m[6] = {a, b, b, variant == 4 ? metal : b, a, b};
    std::vector<int> w = s.walls(sx, sy, sz, faces, m);
    if (variant == 1) s.objs[w[2]].c[2] *= 0.5;   // a wall that is shorter
    if (variant == 2) s.objs[w[2]].a[0] += 1e-9;  // a wall shifted by the smallest amount
    const int lq = s.quad(sx * 0.3, sy - 1, sz * 0.3, sx * 0.4, 0, 0, 0, 0, sz * 0.4, light);
    std::vector<int> top;
    if (variant == 3) {  // under a translate (five quads of mixed materials: not a box() record)
      top.push_back(s.translate(s.list(w), 40, -10, 25));
    } else {
      top = w;
    }
    top.push_back(lq);
    s.dump(name, s.list(top), lq);
  };
  room("open_px", {0, 2, 3, 4, 5}, 400, 300, 500, 0);
  room("closed", all, 400, 300, 500, 0);
  room("translated", {0, 1, 2, 3, 5}, 400, 300, 500, 3);
  room("metal_wall", {0, 1, 2, 3, 5}, 400, 300, 500, 4);
  room("four_walls", {0, 1, 2, 3}, 400, 300, 500, 0);
  room("short_wall", {0, 1, 2, 3, 5}, 400, 300, 500, 1);
  room("shifted_wall", {0, 1, 2, 3, 5}, 400, 300, 500, 2);
  return 0;
}
