"""The generators of material_scenes.py, pinned without a GPU, so that test_gpu_materials.py cannot hide a gap. For every
(scene, camera) of CASES:
 - the scene compiler (abi.scene_check) makes of it the program its GPU rows count on: the rt_scene_info fields are
   the ones written out here, and put the scene on its side of each limit (the flat tables, 96 linear ops, 256 BVH
   nodes, 8 / 16 stack entries, the wide tree's LDS budget, 32 materials);
 - the oracle's event counters (oracle.render_events, oracle.h ORC_EV_*) show that a frame of the GPU rows' own size,
   spp, depth and seed takes each branch the scene is listed with at least FLOOR times: a condition on the scenes, met
   by the oracle alone. The counts in CASES are those of the time of writing (their minimum is 102); an event a scene
   reaches fewer than FLOOR times is not listed, and no GPU row counts on it there;
 - the oracle's frame is lit and finite.
"""
import numpy as np
import pytest

import material_scenes as S
import oracle
from rt_amd import abi

SPP, DEPTH, SEED = 16, 8, 11  # test_gpu_materials.py's
FLOOR = 100                   # of at most 131,072 segments a frame (32 x 32 x 16 x 8)
FIELDS = ("flat_quads", "flat_boxes", "linear_ops", "volumes", "bvh_nodes", "stack_need", "wide_nodes", "wide_kinds",
          "wide_prim_words")

# (scene, camera, the rt_scene_info FIELDS, the events the scene is counted on with their counts)
CASES = [
    ("glass", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8471, emit_front=6269, emit_back=1563, lamb_light_half=7845, lamb_cosine_half=7813,
          diel_cant=558, diel_schlick=160, diel_refract_front=798, diel_refract_back=799, instance=2315,
          tex_solid=32713)),
    ("glass_neg", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8542, emit_front=6238, emit_back=1522, lamb_light_half=7780, lamb_cosine_half=7803,
          diel_cant=546, diel_schlick=154, diel_refract_front=801, diel_refract_back=804, instance=2305,
          tex_solid=32668)),
    ("glass067", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8490, emit_front=6250, emit_back=1472, lamb_light_half=7775, lamb_cosine_half=7817,
          diel_cant=537, diel_schlick=157, diel_refract_front=1265, diel_refract_back=1289, instance=3248,
          tex_solid=33580)),
    ("gloss", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8708, emit_front=6001, emit_back=1496, lamb_light_half=6332, lamb_cosine_half=6342,
          gloss_specular=2293, gloss_diffuse=3240, instance=2584, tex_solid=30623)),
    ("metal", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=11390, emit_front=3144, emit_back=1627, lamb_light_half=4564, lamb_cosine_half=4557,
          metal_mirror=4993, metal_fuzz=4916, metal_below=747, instance=1629, tex_solid=33564)),
    ("nolight", "perspective", (11, 0, 13, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=13968, lamb_no_light=28674, metal_fuzz=8372, metal_below=718, diel_cant=1237,
          diel_schlick=253, diel_refract_front=1585, diel_refract_back=1655, instance=4730, tex_solid=55744)),
    ("nolight_checker", "perspective", (5, 1, 13, 0, 0, 3, 0, 0, 0),
     dict(miss_textured=13553, lamb_no_light=33891, gloss_specular=2649, gloss_diffuse=6225, instance=3050,
          tex_solid=40116, tex_checker=13553)),
    ("dark", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_black=8471, emit_front=6269, emit_back=1563, lamb_light_half=7845, lamb_cosine_half=7813,
          diel_cant=558, diel_schlick=160, diel_refract_front=798, diel_refract_back=799, instance=2315,
          tex_solid=32713)),
    ("nobg", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_none=9062, emit_front=5673, emit_back=1487, lamb_light_half=7732, lamb_cosine_half=7739,
          metal_fuzz=2927, metal_below=476, instance=2659, tex_solid=24071)),
    ("backlight", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8800, emit_front=3995, emit_back=3162, lamb_light_half=12814, lamb_cosine_half=12675,
          instance=8601, tex_solid=38284)),
    ("backlight_metal", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=9853, emit_front=2650, emit_back=3403, lamb_light_half=10700, lamb_cosine_half=10556,
          metal_fuzz=4531, instance=7434, tex_solid=38290)),
    ("checker_light", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8415, emit_front=6418, emit_back=1418, lamb_light_half=8658, lamb_cosine_half=8626,
          instance=2749, tex_solid=25699, tex_checker=6418)),
    ("mats32", "perspective", (30, 1, 38, 0, 10, 6, 0, 0, 0),
     dict(miss_solid=9034, emit_front=5703, emit_back=1481, lamb_light_half=7756, lamb_cosine_half=7772,
          metal_fuzz=2886, metal_below=466, instance=2638, tex_solid=33151)),
    ("mats33", "perspective", (31, 1, 39, 0, 10, 6, 0, 0, 0),
     dict(miss_solid=9031, emit_front=5706, emit_back=1481, lamb_light_half=7760, lamb_cosine_half=7776,
          metal_fuzz=2888, metal_below=466, instance=2640, tex_solid=33161)),
    ("quads64", "perspective", (64, 0, 64, 0, 18, 6, 14, 4, 258),
     dict(miss_solid=9154, emit_front=5635, emit_back=1540, lamb_light_half=6960, lamb_cosine_half=6934,
          metal_fuzz=3134, metal_below=484, tex_solid=31817)),
    ("quads65", "perspective", (65, 0, 65, 0, 18, 6, 14, 4, 262),
     dict(miss_solid=9153, emit_front=5637, emit_back=1539, lamb_light_half=6961, lamb_cosine_half=6934,
          metal_fuzz=3130, metal_below=483, tex_solid=31815)),
    ("quads69", "perspective", (69, 0, 69, 0, 20, 7, 16, 4, 278),
     dict(miss_solid=9152, emit_front=5637, emit_back=1540, lamb_light_half=6962, lamb_cosine_half=6941,
          metal_fuzz=3119, metal_below=480, tex_solid=31811)),
    ("quads70", "perspective", (70, 0, 70, 0, 20, 7, 16, 4, 282),
     dict(miss_solid=9152, emit_front=5637, emit_back=1540, lamb_light_half=6962, lamb_cosine_half=6940,
          metal_fuzz=3118, metal_below=480, tex_solid=31809)),
    ("glass_rot", "perspective", (0, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8438, emit_front=6302, emit_back=1572, lamb_light_half=7873, lamb_cosine_half=7877,
          diel_cant=735, diel_refract_front=740, diel_refract_back=742, instance=2314, tex_solid=32804)),
    ("glass067_rot", "perspective", (0, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8516, emit_front=6201, emit_back=1479, lamb_light_half=7744, lamb_cosine_half=7820,
          diel_cant=750, diel_schlick=220, diel_refract_front=1338, diel_refract_back=1365, instance=3673,
          tex_solid=33954)),
    ("gloss_rot", "perspective", (0, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8663, emit_front=6013, emit_back=1520, lamb_light_half=6333, lamb_cosine_half=6345,
          gloss_specular=2372, gloss_diffuse=3444, instance=2839, tex_solid=30798)),
    ("chain", "perspective", (0, 0, 17, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8684, emit_front=5820, emit_back=1712, lamb_light_half=8075, lamb_cosine_half=8063,
          metal_fuzz=1055, diel_cant=1074, diel_schlick=102, diel_refract_front=896, diel_refract_back=903,
          instance=4030, tex_solid=34672)),
    ("chain_image", "perspective", (0, 0, 17, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8684, emit_front=5820, emit_back=1712, lamb_light_half=8075, lamb_cosine_half=8063,
          metal_fuzz=1055, diel_cant=1074, diel_schlick=102, diel_refract_front=896, diel_refract_back=903,
          instance=4030, tex_solid=30600, tex_image=4072)),
    ("smoke_thick", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=8359, emit_front=6201, emit_back=1418, lamb_light_half=7277, lamb_cosine_half=7269,
          iso_light=4615, tex_solid=33721)),
    ("smoke_thin", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=8397, emit_front=6509, emit_back=1458, lamb_light_half=7673, lamb_cosine_half=7661,
          iso_light=248, tex_solid=30488)),
    ("smoke_chain", "perspective", (0, 0, 12, 1, 0, 3, 0, 0, 0),
     dict(miss_solid=8540, emit_front=6171, emit_back=1494, lamb_light_half=7529, lamb_cosine_half=7503,
          metal_fuzz=1059, iso_light=2742, instance=3801, tex_solid=33544)),
    ("smoke_ball", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=8349, emit_front=6492, emit_back=1420, lamb_light_half=7420, lamb_cosine_half=7440,
          iso_light=2501, tex_solid=32202)),
    ("smoke_nolight", "perspective", (0, 0, 6, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=13479, lamb_no_light=39251, iso_no_light=4348, tex_solid=57078)),
    ("glass_image", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8471, emit_front=6269, emit_back=1563, lamb_light_half=7845, lamb_cosine_half=7813,
          diel_cant=558, diel_schlick=160, diel_refract_front=798, diel_refract_back=799, instance=2315,
          tex_solid=27909, tex_image=4804)),
    ("metal_perlin", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=9447, emit_front=5246, emit_back=1535, lamb_light_half=6567, lamb_cosine_half=6557,
          metal_fuzz=4921, metal_below=660, instance=1768, tex_solid=27818, tex_perlin=4920)),
    ("gloss_value", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8708, emit_front=6001, emit_back=1496, lamb_light_half=6332, lamb_cosine_half=6342,
          gloss_specular=2293, gloss_diffuse=3240, instance=2584, tex_solid=25829, tex_value=4794)),
    ("smoke_value", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=8364, emit_front=6455, emit_back=1444, lamb_light_half=7472, lamb_cosine_half=7443,
          iso_light=2444, tex_solid=27752, tex_value=4426)),
    ("glass_worley", "perspective", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8471, emit_front=6269, emit_back=1563, lamb_light_half=7845, lamb_cosine_half=7813,
          diel_cant=558, diel_schlick=160, diel_refract_front=798, diel_refract_back=799, instance=2315,
          tex_solid=27909, tex_worley=4804)),
    ("spheres_list", "perspective", (0, 0, 62, 0, 20, 7, 5, 1, 126),
     dict(miss_solid=14831, emit_front=749, lamb_light_half=8781, lamb_cosine_half=8767, metal_mirror=1141,
          metal_fuzz=5990, metal_below=637, diel_cant=1069, diel_schlick=325, diel_refract_front=2336,
          diel_refract_back=2322, tex_solid=46311)),
    ("spheres_nl", "perspective", (0, 0, 0, 0, 52, 9, 17, 1, 304),
     dict(miss_solid=62052, lamb_no_light=48876, metal_mirror=14640, metal_fuzz=29030, metal_below=4272,
          diel_cant=7128, diel_schlick=1912, diel_refract_front=14118, diel_refract_back=13417, tex_solid=152217,
          tex_checker=38956)),
    ("spheres_light", "perspective", (0, 0, 0, 0, 50, 9, 17, 1, 306),
     dict(miss_solid=56657, emit_front=3253, lamb_light_half=39092, lamb_cosine_half=38906, metal_mirror=13186,
          metal_fuzz=24958, metal_below=3634, diel_cant=6495, diel_schlick=1714, diel_refract_front=12571,
          diel_refract_back=12015, tex_solid=208847)),
    ("spheres_nl_hbm", "perspective", (0, 0, 0, 0, 1018, 15, 323, 1, 6084),
     dict(miss_solid=65064, lamb_no_light=43715, metal_mirror=1781, metal_fuzz=14421, metal_below=2225,
          diel_cant=1568, diel_schlick=281, diel_refract_front=2048, diel_refract_back=2025, tex_solid=130903)),
    ("spheres_light_hbm", "perspective", (0, 0, 0, 0, 1018, 15, 324, 1, 6086),
     dict(miss_solid=59781, emit_front=3145, lamb_light_half=38725, lamb_cosine_half=38781, metal_mirror=1627,
          metal_fuzz=12928, metal_below=2016, diel_cant=1433, diel_schlick=259, diel_refract_front=1805,
          diel_refract_back=1790, tex_solid=160274)),
    ("mesh", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=156775)),
    ("mesh_tris", "perspective", (0, 0, 0, 0, 77, 9, 48, 2, 668),
     dict(miss_solid=64708, lamb_no_light=48886, metal_mirror=4552, metal_fuzz=6949, metal_below=738,
          diel_cant=6689, diel_schlick=1064, diel_refract_front=8695, diel_refract_back=8595, gloss_specular=3001,
          gloss_diffuse=5151, tex_solid=155289)),
    ("mesh_small", "perspective", (0, 0, 0, 0, 37, 10, 23, 6, 316),
     dict(miss_solid=45272, emit_front=20029, lamb_light_half=22285, lamb_cosine_half=22213, metal_mirror=1758,
          metal_fuzz=3358, metal_below=405, diel_cant=6371, diel_schlick=1100, diel_refract_front=8714,
          diel_refract_back=8661, gloss_specular=1383, gloss_diffuse=2430, tex_solid=142191)),
    ("mesh_deep", "perspective", (0, 0, 0, 0, 88, 19, 55, 6, 697),
     dict(miss_solid=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=156775)),
    ("terrain", "perspective", (0, 0, 0, 0, 2738, 16, 1819, 2, 24578),
     dict(miss_solid=62856, lamb_no_light=115028, metal_fuzz=11468, metal_below=519, tex_solid=189352)),
    ("terrain_ll", "perspective", (0, 0, 0, 0, 2717, 17, 1885, 6, 24582),
     dict(miss_solid=35237, emit_front=26012, emit_back=1300, lamb_light_half=68276, lamb_cosine_half=67949,
          tex_solid=197474)),
    ("mesh_ll", "perspective", (0, 0, 0, 0, 72, 10, 42, 6, 634),
     dict(miss_solid=40639, emit_front=24487, lamb_light_half=37307, lamb_cosine_half=37024, tex_solid=139457)),
    ("mesh_checker_light", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=137632, tex_checker=19143)),
    ("mesh_extras", "perspective", (0, 0, 0, 1, 78, 11, 0, 0, 0),
     dict(miss_solid=45269, emit_front=18952, lamb_light_half=23141, lamb_cosine_half=23014, metal_mirror=4808,
          metal_fuzz=7627, metal_below=881, diel_cant=9079, diel_schlick=1742, diel_refract_front=13610,
          diel_refract_back=13588, gloss_specular=3552, gloss_diffuse=6058, iso_light=4712, instance=12548,
          tex_solid=171600)),
    ("mesh_tris_extras", "perspective", (0, 0, 0, 1, 78, 10, 0, 0, 0),
     dict(miss_solid=63917, lamb_no_light=48019, metal_mirror=4719, metal_fuzz=6943, metal_below=738,
          diel_cant=9629, diel_schlick=1665, diel_refract_front=13524, diel_refract_back=13501, gloss_specular=3026,
          gloss_diffuse=5142, iso_no_light=5521, instance=13356, tex_solid=172580)),
    ("mesh_image", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=116206, tex_image=40569)),
    ("mesh_perlin", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=116206, tex_perlin=40569)),
    ("spheres_small", "perspective", (0, 0, 0, 0, 34, 8, 11, 1, 206),
     dict(miss_solid=57873, emit_front=3250, lamb_light_half=38387, lamb_cosine_half=38283, metal_mirror=7435,
          metal_fuzz=29525, metal_below=3956, diel_cant=3698, diel_schlick=1144, diel_refract_front=7991,
          diel_refract_back=7733, tex_solid=195319)),
    ("spheres_nl_small", "perspective", (0, 0, 0, 0, 34, 8, 12, 1, 204),
     dict(miss_solid=63456, lamb_no_light=46169, metal_mirror=8481, metal_fuzz=33531, metal_below=4416,
          diel_cant=4144, diel_schlick=1223, diel_refract_front=8944, diel_refract_back=8630, tex_solid=136770,
          tex_checker=37808)),
    ("instanced", "perspective", (0, 0, 0, 0, 401, 8, 0, 0, 0),
     dict(miss_solid=60100, emit_front=3225, lamb_light_half=37611, lamb_cosine_half=37460, metal_mirror=1412,
          metal_fuzz=3797, metal_below=422, diel_cant=3877, diel_schlick=677, diel_refract_front=4445,
          diel_refract_back=4429, instance=96933, tex_solid=157033)),
    ("mixed", "perspective", (0, 0, 0, 0, 43, 8, 23, 15, 368),
     dict(miss_solid=44724, emit_front=18214, emit_back=1312, lamb_light_half=29957, lamb_cosine_half=30089,
          metal_fuzz=11852, metal_below=432, diel_cant=2008, diel_schlick=784, diel_refract_front=6384,
          diel_refract_back=4166, gloss_specular=2045, gloss_diffuse=4705, moving_sphere=4162, tex_solid=152883)),
    ("mixed_hbm", "perspective", (0, 0, 0, 0, 1025, 14, 635, 15, 8510),
     dict(miss_solid=44404, miss_short=1039, emit_front=17955, emit_back=954, lamb_light_half=26737,
          lamb_cosine_half=26660, metal_fuzz=12275, metal_below=425, diel_cant=1452, diel_schlick=823,
          diel_refract_front=6765, diel_refract_back=5275, gloss_specular=2312, gloss_diffuse=5446,
          moving_sphere=5566, tex_solid=147792)),
    ("mixed_static", "perspective", (0, 0, 0, 0, 42, 8, 23, 7, 368),
     dict(miss_solid=44873, emit_front=18209, emit_back=1308, lamb_light_half=29896, lamb_cosine_half=30126,
          metal_fuzz=10341, metal_below=503, diel_cant=1989, diel_schlick=856, diel_refract_front=6524,
          diel_refract_back=4484, gloss_specular=1994, gloss_diffuse=4583, tex_solid=151881)),
    ("mixed_static_hbm", "perspective", (0, 0, 0, 0, 1032, 14, 633, 7, 8510),
     dict(miss_solid=45313, emit_front=18166, emit_back=982, lamb_light_half=26790, lamb_cosine_half=26857,
          metal_fuzz=10747, metal_below=570, diel_cant=1509, diel_schlick=985, diel_refract_front=7518,
          diel_refract_back=6482, gloss_specular=2328, gloss_diffuse=5550, tex_solid=149917)),
    ("backlight@black", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_black=8800, emit_front=3995, emit_back=3162, lamb_light_half=12814, lamb_cosine_half=12675,
          instance=8601, tex_solid=38284)),
    ("backlight@none", "perspective", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_none=8800, emit_front=3995, emit_back=3162, lamb_light_half=12814, lamb_cosine_half=12675,
          instance=8601, tex_solid=29484)),
    ("chain", "lens", (0, 0, 17, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=8564, miss_short=119, emit_front=5812, emit_back=1713, lamb_light_half=8075,
          lamb_cosine_half=8046, metal_fuzz=1070, diel_cant=1082, diel_schlick=103, diel_refract_front=895,
          diel_refract_back=902, instance=4052, tex_solid=34549)),
    ("checker_light", "fisheye", (6, 1, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=9225, emit_front=5769, emit_back=1265, lamb_light_half=7812, lamb_cosine_half=7783,
          instance=2586, tex_solid=24820, tex_checker=5769)),
    ("glass", "orthonormal", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=3389, emit_front=11187, emit_back=1668, lamb_light_half=12883, lamb_cosine_half=12985,
          diel_cant=772, diel_schlick=247, diel_refract_front=2750, diel_refract_back=2753, instance=6522,
          tex_solid=46966)),
    ("glass@black", "orthonormal", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_black=3389, emit_front=11187, emit_back=1668, lamb_light_half=12883, lamb_cosine_half=12985,
          diel_cant=772, diel_schlick=247, diel_refract_front=2750, diel_refract_back=2753, instance=6522,
          tex_solid=46966)),
    ("glass@checker", "fisheye", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_textured=9277, emit_front=5639, emit_back=1401, lamb_light_half=7049, lamb_cosine_half=7023,
          diel_cant=509, diel_schlick=150, diel_refract_front=781, diel_refract_back=783, instance=2223,
          tex_solid=21934, tex_checker=9277)),
    ("glass@none", "lens", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_none=8463, emit_front=6271, emit_back=1565, lamb_light_half=7857, lamb_cosine_half=7810,
          diel_cant=571, diel_schlick=159, diel_refract_front=797, diel_refract_back=798, instance=2325,
          tex_solid=24263)),
    ("gloss", "fisheye", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=9527, emit_front=5351, emit_back=1335, lamb_light_half=5641, lamb_cosine_half=5717,
          gloss_specular=2128, gloss_diffuse=2986, instance=2440, tex_solid=29222)),
    ("instanced", "fisheye", (0, 0, 0, 0, 401, 8, 0, 0, 0),
     dict(miss_solid=60655, emit_front=2703, lamb_light_half=37219, lamb_cosine_half=37275, metal_mirror=1219,
          metal_fuzz=4204, metal_below=434, diel_cant=3825, diel_schlick=608, diel_refract_front=4157,
          diel_refract_back=4151, instance=95361, tex_solid=156016)),
    ("mesh", "fisheye", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848, metal_mirror=4534,
          metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138, diel_refract_front=8611,
          diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=154546)),
    ("mesh@black", "fisheye", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_black=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848, metal_mirror=4534,
          metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138, diel_refract_front=8611,
          diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=154546)),
    ("mesh@black", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_black=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=156775)),
    ("mesh@checker", "fisheye", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_textured=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848,
          metal_mirror=4534, metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138,
          diel_refract_front=8611, diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=108819,
          tex_checker=45727)),
    ("mesh@checker", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_textured=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093,
          metal_mirror=4668, metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122,
          diel_refract_front=8939, diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=111182,
          tex_checker=45593)),
    ("mesh@none", "fisheye", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_none=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848, metal_mirror=4534,
          metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138, diel_refract_front=8611,
          diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=108819)),
    ("mesh@none", "perspective", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_none=45593, emit_front=19143, lamb_light_half=24113, lamb_cosine_half=24093, metal_mirror=4668,
          metal_fuzz=7648, metal_below=894, diel_cant=6479, diel_schlick=1122, diel_refract_front=8939,
          diel_refract_back=8868, gloss_specular=3586, gloss_diffuse=6109, tex_solid=111182)),
    ("mesh_checker_light", "fisheye", (0, 0, 0, 0, 76, 11, 49, 6, 670),
     dict(miss_solid=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848, metal_mirror=4534,
          metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138, diel_refract_front=8611,
          diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=135540, tex_checker=19006)),
    ("mesh_deep", "fisheye", (0, 0, 0, 0, 88, 19, 55, 6, 697),
     dict(miss_solid=45727, emit_front=19006, lamb_light_half=23885, lamb_cosine_half=23848, metal_mirror=4534,
          metal_fuzz=7223, metal_below=839, diel_cant=6275, diel_schlick=1138, diel_refract_front=8611,
          diel_refract_back=8532, gloss_specular=3400, gloss_diffuse=5767, tex_solid=154546)),
    ("mesh_extras", "fisheye", (0, 0, 0, 1, 78, 11, 0, 0, 0),
     dict(miss_solid=45465, emit_front=18741, lamb_light_half=23072, lamb_cosine_half=23070, metal_mirror=4606,
          metal_fuzz=7139, metal_below=808, diel_cant=8892, diel_schlick=1693, diel_refract_front=12999,
          diel_refract_back=12958, gloss_specular=3379, gloss_diffuse=5711, iso_light=4244, instance=11852,
          tex_solid=168590)),
    ("mesh_ll@black", "perspective", (0, 0, 0, 0, 72, 10, 42, 6, 634),
     dict(miss_black=40639, emit_front=24487, lamb_light_half=37307, lamb_cosine_half=37024, tex_solid=139457)),
    ("mesh_ll@none", "perspective", (0, 0, 0, 0, 72, 10, 42, 6, 634),
     dict(miss_none=40639, emit_front=24487, lamb_light_half=37307, lamb_cosine_half=37024, tex_solid=98818)),
    ("mesh_tris", "fisheye", (0, 0, 0, 0, 77, 9, 48, 2, 668),
     dict(miss_solid=64740, lamb_no_light=48324, metal_mirror=4406, metal_fuzz=6600, metal_below=735,
          diel_cant=6305, diel_schlick=1031, diel_refract_front=8325, diel_refract_back=8231, gloss_specular=2946,
          gloss_diffuse=4876, tex_solid=152838)),
    ("mesh_tris_extras", "fisheye", (0, 0, 0, 1, 78, 10, 0, 0, 0),
     dict(miss_solid=64040, lamb_no_light=47458, metal_mirror=4488, metal_fuzz=6576, metal_below=723,
          diel_cant=9034, diel_schlick=1563, diel_refract_front=12740, diel_refract_back=12712, gloss_specular=2948,
          gloss_diffuse=4861, iso_no_light=4853, instance=12266, tex_solid=168325)),
    ("metal", "lens", (12, 0, 14, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=11270, miss_short=119, emit_front=3147, emit_back=1618, lamb_light_half=4557,
          lamb_cosine_half=4564, metal_mirror=4998, metal_fuzz=4953, metal_below=744, instance=1651,
          tex_solid=33489)),
    ("mixed_static", "fisheye", (0, 0, 0, 0, 42, 8, 23, 7, 368),
     dict(miss_solid=45410, emit_front=17851, emit_back=1157, lamb_light_half=29063, lamb_cosine_half=29412,
          metal_fuzz=9666, metal_below=505, diel_cant=1881, diel_schlick=830, diel_refract_front=6088,
          diel_refract_back=4246, gloss_specular=1706, gloss_diffuse=4075, tex_solid=148522)),
    ("nolight", "fisheye", (11, 0, 13, 0, 0, 3, 0, 0, 0),
     dict(miss_solid=14188, lamb_no_light=25778, metal_fuzz=7520, metal_below=645, diel_cant=1132,
          diel_schlick=227, diel_refract_front=1437, diel_refract_back=1508, instance=4304, tex_solid=51790)),
    ("smoke_ball", "lens", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=8225, miss_short=119, emit_front=6496, emit_back=1424, lamb_light_half=7426,
          lamb_cosine_half=7434, iso_light=2495, tex_solid=32076)),
    ("smoke_chain", "fisheye", (0, 0, 12, 1, 0, 3, 0, 0, 0),
     dict(miss_solid=9324, emit_front=5569, emit_back=1339, lamb_light_half=6740, lamb_cosine_half=6730,
          metal_fuzz=926, iso_light=2650, instance=3576, tex_solid=31939)),
    ("smoke_nolight", "lens", (0, 0, 6, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=13361, miss_short=119, lamb_no_light=39253, iso_no_light=4329, tex_solid=56943)),
    ("smoke_thick", "orthonormal", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_solid=3058, emit_front=10792, emit_back=1453, lamb_light_half=11392, lamb_cosine_half=11468,
          iso_light=13214, tex_solid=49924)),
    ("smoke_thick@black", "orthonormal", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_black=3058, emit_front=10792, emit_back=1453, lamb_light_half=11392, lamb_cosine_half=11468,
          iso_light=13214, tex_solid=49924)),
    ("smoke_thick@black", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_black=8359, emit_front=6201, emit_back=1418, lamb_light_half=7277, lamb_cosine_half=7269,
          iso_light=4615, tex_solid=33721)),
    ("smoke_thick@none", "orthonormal", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_none=3058, emit_front=10792, emit_back=1453, lamb_light_half=11392, lamb_cosine_half=11468,
          iso_light=13214, tex_solid=46866)),
    ("smoke_thick@none", "perspective", (0, 0, 7, 1, 0, 1, 0, 0, 0),
     dict(miss_none=8359, emit_front=6201, emit_back=1418, lamb_light_half=7277, lamb_cosine_half=7269,
          iso_light=4615, tex_solid=25362)),
    ("spheres_list", "fisheye", (0, 0, 62, 0, 20, 7, 5, 1, 126),
     dict(miss_solid=14974, emit_front=619, lamb_light_half=8725, lamb_cosine_half=8585, metal_mirror=1202,
          metal_fuzz=5745, metal_below=662, diel_cant=954, diel_schlick=305, diel_refract_front=2139,
          diel_refract_back=2122, tex_solid=45370)),
    ("spheres_nl_hbm", "fisheye", (0, 0, 0, 0, 1018, 15, 323, 1, 6084),
     dict(miss_solid=65110, lamb_no_light=43224, metal_mirror=2122, metal_fuzz=13258, metal_below=1997,
          diel_cant=1340, diel_schlick=265, diel_refract_front=1873, diel_refract_back=1855, tex_solid=129047)),
    ("spheres_nl_small@checker", "perspective", (0, 0, 0, 0, 34, 8, 12, 1, 204),
     dict(miss_textured=63456, lamb_no_light=46169, metal_mirror=8481, metal_fuzz=33531, metal_below=4416,
          diel_cant=4144, diel_schlick=1223, diel_refract_front=8944, diel_refract_back=8630, tex_solid=73314,
          tex_checker=101264)),
    ("spheres_small", "fisheye", (0, 0, 0, 0, 34, 8, 11, 1, 206),
     dict(miss_solid=58542, emit_front=2699, lamb_light_half=37921, lamb_cosine_half=38272, metal_mirror=7748,
          metal_fuzz=27805, metal_below=3596, diel_cant=3525, diel_schlick=1161, diel_refract_front=7835,
          diel_refract_back=7586, tex_solid=193094)),
]
EVENTS = {(c[0], c[1]): c[3] for c in CASES}
INFO = {c[0]: dict(zip(FIELDS, c[2])) for c in CASES}


def family(name):
    """The traversal family the default path gives the scene, from the pinned rt_scene_info (rt_plan.h
    kernel_family): flat, linear, wide_lds, wide_hbm, stack."""
    i = INFO[name]
    if i["flat_quads"] + i["flat_boxes"] > 0:
        return "flat"
    if i["linear_ops"] > 0:
        return "linear"
    if i["wide_nodes"] == 0:
        return "stack"  # an instance or a volume under the bvh_node: no wide tree, the binary BVH on every path
    return "wide_hbm" if i["wide_prim_words"] > 4096 else "wide_lds"


def test_every_scene_has_a_case_and_the_frames_are_small():
    assert {c[0] for c in CASES if c[1] == "perspective" and "@" not in c[0]} == set(S.SCENES)
    assert {c[0].partition("@")[0] for c in CASES} == set(S.SCENES)
    assert len(EVENTS) == len(CASES)
    for name in S.SCENES:
        _, cam = S.SCENES[name]()
        assert cam.image_width == cam.image_height == (64 if name in S.BVH_SCENES else 32), name
        assert (family(name) in ("wide_lds", "wide_hbm", "stack")) == (name in S.BVH_SCENES), name


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_scene_compiles_as_its_rows_expect_and_reaches_its_events(case):
    name, cam_kind, fields, events = case
    desc, cam = S.build(name, cam_kind)
    st, info, msg = abi.scene_check(desc)
    assert st == abi.RT_OK, msg
    assert tuple(getattr(info, f) for f in FIELDS) == fields
    ref, segs, ev = oracle.render_events(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
    assert np.isfinite(ref).all() and ref.mean() > 0.05, ref.mean()
    plain, segs_plain = oracle.render(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
    assert segs == segs_plain and np.array_equal(ref, plain)  # counting changes neither the image nor the segments
    assert 0 < segs <= cam.image_width * cam.image_height * SPP * DEPTH
    print(name, cam_kind, {k: ev[k] for k in events})
    for k in events:
        assert ev[k] >= FLOOR, (k, ev[k])
    # every traced segment is a miss, an emitter or a scatter: the counters leave none out
    scatters = ("lamb_light_half", "lamb_cosine_half", "lamb_no_light", "metal_mirror", "metal_fuzz", "diel_cant",
                "diel_schlick", "diel_refract_front", "diel_refract_back", "gloss_specular", "gloss_diffuse", "iso_light",
                "iso_no_light", "emit_front", "emit_back", "miss_none", "miss_black", "miss_solid", "miss_textured",
                "miss_short")
    assert sum(ev[k] for k in scatters) == segs


def test_scenes_sit_on_their_side_of_each_limit():
    I = INFO
    # the flat program: a box() of glass is six flat quads, a lambertian one a slab record; an instance removes it
    assert (I["glass"]["flat_quads"], I["glass"]["flat_boxes"]) == (12, 0)
    assert (I["backlight"]["flat_quads"], I["backlight"]["flat_boxes"]) == (6, 1)
    for name in ("glass_rot", "glass067_rot", "gloss_rot", "chain", "smoke_thick", "smoke_ball", "spheres_list"):
        assert family(name) == "linear", name
    # FlatTrav<.,1,0>: 32 materials, 64 quads (rt_plan.h kFlatLds)
    for name, n in (("mats32", 32), ("mats33", 33)):
        desc, _ = S.SCENES[name]()
        mats = [desc.materials[i] for i in range(desc.num_materials)]
        assert len(mats) == n and family(name) == "flat"
        # no two alike, so the compiler shares none: the scene's table has n materials (it counts unused ones too)
        assert len({(m.kind, tuple(desc.textures[m.texture].color), m.fuzz) for m in mats}) == n
    assert I["quads64"]["flat_quads"] == 64 and I["quads65"]["flat_quads"] == 65
    # past the linear program's 96 ops (rt_scene.h kLinearMax): no linear program, the wide tree or the binary BVH
    for name in S.BVH_SCENES:
        assert I[name]["linear_ops"] == 0 and I[name]["bvh_nodes"] > 0, name
        assert (I[name]["wide_nodes"] > 0) == (name not in ("instanced", "mesh_extras", "mesh_tris_extras")), name
    # the wide tree's kinds (1 spheres, 2 triangles, 4 quads, 8 moving spheres) and where it lives
    kinds = {"spheres_nl": 1, "spheres_nl_small": 1, "spheres_light": 1, "spheres_small": 1, "spheres_nl_hbm": 1, "spheres_light_hbm": 1,
             "mesh_tris": 2, "terrain": 2, "mesh": 6, "mesh_small": 6, "mesh_deep": 6, "terrain_ll": 6, "mesh_image": 6,
             "mesh_perlin": 6, "mesh_ll": 6, "mesh_checker_light": 6, "mesh_extras": 0, "mesh_tris_extras": 0, "instanced": 0,
             "mixed_static": 7, "mixed_static_hbm": 7, "mixed": 15, "mixed_hbm": 15}
    assert set(kinds) == S.BVH_SCENES
    for name, k in kinds.items():
        assert I[name]["wide_kinds"] == k, name
        hbm = name.endswith("_hbm") or name.startswith("terrain")
        # rt_plan.h wide_tree_in_lds: at most 4096 primitive words and 40 KiB; the LDS scenes stay far below both
        assert (I[name]["wide_prim_words"] > 4096) if hbm else (I[name]["wide_prim_words"] <= 1024), name
    # the binary BVH: at most 256 nodes (fp32 keeps them in LDS) or more; at most 8, 9 to 16, more than 16 stack entries
    assert I["spheres_small"]["stack_need"] <= 8 and I["spheres_small"]["bvh_nodes"] <= 256
    assert 9 <= I["mesh"]["stack_need"] <= 16 and I["mesh"]["bvh_nodes"] <= 256
    assert 9 <= I["spheres_nl_hbm"]["stack_need"] <= 16 and I["spheres_nl_hbm"]["bvh_nodes"] > 256
    assert 16 < I["mesh_deep"]["stack_need"] < 32 and I["mesh_deep"]["bvh_nodes"] <= 256
    # more than 256 nodes on 8 entries: a single tree cannot (8 entries are at most 7 levels of nodes, 127), the many
    # small trees of `instanced` do
    assert I["instanced"]["bvh_nodes"] > 256 and I["instanced"]["stack_need"] <= 8
    assert all(i["stack_need"] > 8 for n, i in I.items() if i["bvh_nodes"] > 256 and not n.startswith("instanced"))


def test_render_events_sums_like_render():
    # one thread and eight give the same counts: the per-thread arrays are summed as the segment counter is
    desc, cam = S.SCENES["gloss"]()
    a = oracle.render_events(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=1)
    b = oracle.render_events(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
    assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[0], b[0])
    assert a[2]["gloss_specular"] > 0 and a[2]["gloss_diffuse"] > 0
