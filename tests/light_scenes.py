"""Scenes for the light-sampling tests (test_light_scenes.py pins them on the CPU, test_gpu_lights.py renders them):
every kind of sampled light -- an axis-aligned quad in each of its six (axis of u, axis of v) orientations and with
extents of both signs, a parallelogram off the axes, a sphere, a moving sphere, and the base-class light of a
hittable_list -- inside the scenes that select each path kernel. Every generator returns (desc, cam); the sizes are
these tests' own, not a workload's.
"""
import itertools
import random

import numpy as np

from rt_amd.scene import SceneBuilder, perspective

# ------------------------------------------------------------------ signed axis permutations
PERMS = list(itertools.permutations(range(3)))
SIGNS = [(1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1)]


def matrix(perm, signs):
    """M with M[i, perm[i]] = signs[i]: (M v)[i] = signs[i] * v[perm[i]]."""
    m = np.zeros((3, 3))
    for i in range(3):
        m[i, perm[i]] = signs[i]
    return m


MATRICES = [matrix(p, s) for p in PERMS for s in SIGNS]  # 24: index 4 * perm + sign set


def axis_of(v):
    """The axis an axis-parallel vector lies along, and the sign of its extent."""
    nz = [k for k in range(3) if v[k] != 0]
    assert len(nz) == 1, v
    return nz[0], (1 if v[nz[0]] > 0 else -1)


def light_quad(desc):
    """(q, u, v) of the descriptor's light when it is a quad."""
    o = desc.objects[desc.light]
    return np.array(o.a[:]), np.array(o.b[:]), np.array(o.c[:])


# ------------------------------------------------------------------ the room
ROOM_SIZE = (400.0, 300.0, 500.0)
WALL_COLOURS = [(.65, .05, .05), (.12, .45, .15), (.73, .73, .73), (.6, .6, .73), (.73, .6, .4), (.5, .7, .7)]
ROOM_LIGHT = ((130, 299, 180), (140, 0, 0), (0, 0, 110))
OFF_AXIS_LIGHT = ((130, 250, 180), (100, 0, 30), (10, 25, 120))  # u x v = (-750, -11700, 2500): it faces down
ROOM_VARIANTS = ("ll", "metal", "smoke", "mats16", "mats17", "smoke16", "smoke17", "offaxis", "offaxis_smoke",
                 "offaxis_apart", "sphere", "sphere_smoke", "sphere_apart")


def room(M, variant="ll", width=32):
    """The open room of test_gpu_rooms.room_scene("open_px") -- 400 x 300 x 500, faces 0, 2, 3, 4, 5 each with a colour
    of its own, a box (150,0,230)-(240,160,320), a ceiling light of emission 15, seen through the opening -- with
    every point and vector multiplied by the signed permutation matrix M. Where det M < 0 each quad's u and v are
    swapped, so that every normal (u x v) keeps its sense: walls and light face into the room under every M.

    ll: lambertian walls and box (the flat program's LL form). metal: wall 0 is metal (the general form).
    smoke: the box is volume(box, 0.01, white) (the linear program with volumes; the LLI form).
    mats16 / mats17, smoke16 / smoke17: small quads on the floor, each with a lambertian colour of its own, bring
    the descriptor's distinct materials (the light's and the smoke's included) to 16 and to 17: either side of
    the n_mats <= 16 condition of the LL and LLI forms.
    offaxis: the light is a parallelogram off the axes, a member of the world (no flat program); offaxis_smoke: the
    same with the smoke box; offaxis_apart: the ll room with its ceiling quad, and the parallelogram as the sampled
    light without being a member (the flat program's general form).
    sphere / sphere_smoke / sphere_apart: the same three with an emitting sphere((200,220,250), 30) as the light."""
    assert variant in ROOM_VARIANTS, variant
    M = np.asarray(M, float)
    flip = np.linalg.det(M) < 0
    s = SceneBuilder()
    sx, sy, sz = ROOM_SIZE
    faces = {0: ((0, 0, 0), (0, sy, 0), (0, 0, sz)), 2: ((0, 0, 0), (sx, 0, 0), (0, 0, sz)),
             3: ((sx, sy, sz), (-sx, 0, 0), (0, 0, -sz)), 4: ((0, 0, 0), (sx, 0, 0), (0, sy, 0)),
             5: ((0, 0, sz), (sx, 0, 0), (0, sy, 0))}

    def quad(q, u, v, mat):
        q, u, v = (M @ np.asarray(x, float) for x in (q, u, v))
        return s.quad(q, v, u, mat) if flip else s.quad(q, u, v, mat)

    mats = [s.lambertian(s.solid(c)) for c in WALL_COLOURS]
    if variant == "metal":
        mats[0] = s.metal(s.solid((0.8, 0.85, 0.88)), 0.05)
    emit = s.diffuse_light(s.solid((15, 15, 15)))
    w = [quad(*faces[f], mats[f]) for f in (0, 2, 3, 4, 5)]
    corners = [M @ np.array(c, float) for c in ((150, 0, 230), (240, 160, 320))]
    lo, hi = np.minimum(*corners), np.maximum(*corners)
    box_mat = s.lambertian(s.solid((0.4, 0.5, 0.75))) if variant in ("mats16", "mats17") else mats[2]
    box = s.translate(s.box((0, 0, 0), hi - lo, box_mat), lo)  # (a translated box(), as room_scene's: a slab record)
    smoke = variant in ("smoke", "smoke16", "smoke17", "offaxis_smoke", "sphere_smoke")
    if smoke:
        box = s.volume(box, 0.01, s.solid((1, 1, 1)))
    members = w[:2] + [box] + w[2:]  # the walls are not neighbours in the list
    if variant in ("mats16", "mats17", "smoke16", "smoke17"):
        want = 16 if variant.endswith("16") else 17
        rnd = random.Random(16)
        colour = lambda: s.lambertian(s.solid((0.2 + 0.7 * rnd.random(), 0.2 + 0.7 * rnd.random(),
                                               0.2 + 0.7 * rnd.random())))
        # The flat LL form holds 14 quads (fp32 keeps the walls as quads: 5 + the light + 8) and 16 materials, so the
        # room takes 8 small quads -- with the walls' six, the light's and the box's own that is 16 materials, the
        # last one in use -- and the 17th (mats17) is one that no object uses, so only n_mats differs. The linear
        # program has no such limit: the smoke room uses every material it adds (the smoke's own is made already).
        n_quads = 8 if not smoke else want - len(s.materials)
        for k in range(n_quads):
            members.append(quad((250 + 14 * k, 1 + k, 30 + 40 * k), (12, 0, 0), (0, 0, 34), colour()))
        while len(s.materials) < want:
            colour()
        assert len(s.materials) == want
    if variant.startswith("sphere"):
        light = s.sphere(M @ np.array((200.0, 220.0, 250.0)), 30.0, emit)
    elif variant.startswith("offaxis"):
        light = quad(*OFF_AXIS_LIGHT, emit)
    else:
        light = quad(*ROOM_LIGHT, emit)
    if variant.endswith("_apart"):
        members.append(quad(*ROOM_LIGHT, emit))  # the emitter in the world; the sampled light is not a member
    else:
        members.append(light)
    cam = perspective(width, 1.0, (1100, 150, 250), (0, 150, 250), 1, 40.0)
    for name in ("pos", "dir", "right", "up"):
        getattr(cam, name)[:] = list(M @ np.array(getattr(cam, name)[:]))
    return s.desc(s.hlist(members), light=light, background=s.solid((0.02, 0.03, 0.05))), cam


# ------------------------------------------------------------------ the mesh under a quad light
UV_PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]  # (axis of u, axis of v); Light::aligned = 1 + index
MESH_VARIANTS = ("ll", "metal", "mats16", "mats17", "offaxis")
CLUSTER = np.array((0.0, 2.5, 0.0))


def facing_quad(uv, centre, toward, size, flip_both=False):
    """(q, u, v) of a size x size quad about `centre` with u along axis uv[0] and v along uv[1], its normal u x v
    toward the point `toward`; flip_both negates both extents (the same normal from the opposite corner)."""
    u, v = np.zeros(3), np.zeros(3)
    u[uv[0]], v[uv[1]] = size, size
    if np.dot(np.cross(u, v), toward - centre) < 0:
        v = -v
    if flip_both:
        u, v = -u, -v
    return centre - 0.5 * u - 0.5 * v, u, v


def mesh_light(uv):
    """The mesh scene's light for the pair uv: on the plane of the third axis, 9 from the cluster -- the two pairs of a
    plane on opposite sides (both above for the y planes: never under the ground) -- and both extents negated for
    every second pair."""
    k = UV_PAIRS.index(uv)
    plane = 3 - uv[0] - uv[1]
    centre = CLUSTER.copy()
    centre[plane] += (9.0, 9.0, -9.0, 9.0, 9.0, -9.0)[k]
    return facing_quad(uv, centre, CLUSTER, 4.0, flip_both=k in (1, 2, 5))


def mesh(uv, variant="ll", width=64):
    """208 seeded triangles without shared edges about (0, 2.5, 0) under one bvh_node with a large ground quad and a
    quad light of orientation uv (u along axis uv[0], v along uv[1]) that faces the cluster: past the linear
    program's leaves, so the wide tree (in LDS) or, in reference order, the binary BVH.
    ll: all lambertian (the wide LL form). metal: every seventh triangle metal (the general triangle + quad form).
    mats16 / mats17: 16 and 17 distinct materials, all in use (the LL form at its limit, and its fallback).
    offaxis: a parallelogram light off the axes (uv unused)."""
    assert variant in MESH_VARIANTS, variant
    rnd = random.Random(208)
    s = SceneBuilder()
    n_lamb = {"mats16": 15, "mats17": 16}.get(variant, 3)
    mats = [s.lambertian(s.solid((0.25 + 0.7 * rnd.random(), 0.25 + 0.7 * rnd.random(), 0.25 + 0.7 * rnd.random())))
            for _ in range(n_lamb)]
    chrome = s.metal(s.solid((0.85, 0.85, 0.9)), 0.1) if variant == "metal" else None
    objs = []
    for i in range(208):
        p = np.array([rnd.uniform(-4, 4), rnd.uniform(0.3, 4.7), rnd.uniform(-4, 4)])
        a = np.array([rnd.uniform(-1.2, 1.2) for _ in range(3)])
        b = np.array([rnd.uniform(-1.2, 1.2) for _ in range(3)])
        m = chrome if (chrome is not None and i % 7 == 0) else mats[i % n_lamb]
        objs.append(s.triangle(p, p + a, p + b, m))
    objs.append(s.quad((-30, -1.01, -30), (60, 0, 0), (0, 0, 60), mats[0]))
    emit = s.diffuse_light(s.solid((12, 12, 12)))
    if variant == "offaxis":
        light = s.quad((-2.2, 10.0, -3.0), (4.0, 0, 1.2), (0.4, 1.0, 4.8), emit)  # u x v = (-1.2, -18.72, 4): down
    else:
        light = s.quad(*mesh_light(uv), emit)
    objs.append(light)
    assert len(s.materials) == n_lamb + 1 + (variant == "metal")
    cam = perspective(width, 1.0, (10, 7, 15), (0, 2, 0), 1, 38.0)
    return s.desc(s.bvh(objs), light=light, background=s.solid((0.1, 0.12, 0.16))), cam


def terrain_hbm(uv=(1, 2), width=32):
    """The 8,192-triangle height field of test_mesh_tree_in_hbm_lit_fp64_and_fp32 (24,576 primitive words: the wide
    tree stays in HBM), its light turned onto an x plane: u along y and v along z (aligned = 4) or the reverse (6)."""
    assert uv in ((1, 2), (2, 1)), uv
    rng = np.random.default_rng(4)
    n, size, amp = 64, 400.0, 30.0
    x = np.linspace(-size / 2, size / 2, n + 1)
    X, Z = np.meshgrid(x, x, indexing="ij")
    H = amp * (np.sin(X / 37.0) * np.cos(Z / 23.0) + 0.3 * rng.standard_normal(X.shape))
    P = np.stack([X, H, Z], -1)
    a, b, c, d = P[:-1, :-1], P[1:, :-1], P[1:, 1:], P[:-1, 1:]
    tris = np.stack([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)],
                    1).reshape(-1, 3, 3)
    s = SceneBuilder()
    ground = s.lambertian(s.solid((0.7, 0.6, 0.5)))
    chrome = s.metal(s.solid((0.9, 0.9, 0.9)), 0.1)
    objs = [s.triangle(t[0], t[1], t[2], chrome if i % 11 == 0 else ground) for i, t in enumerate(tris)]
    centre = np.array((-150.0, 110.0, 0.0))
    light = s.quad(*facing_quad(uv, centre, np.array((0.0, 0.0, 0.0)), 120.0),
                   s.diffuse_light(s.solid((15, 15, 15))))
    objs.append(light)
    cam = perspective(width, 1.0, (180, 140, 160), (0, 0, 0), 1, 50.0)
    return s.desc(s.bvh(objs), light=light, background=s.solid((0.05, 0.07, 0.1))), cam


# ------------------------------------------------------------------ sphere lights
SPHERE_VARIANTS = ("list", "moving", "bvh")


def sphere_light(variant="list", width=32):
    """An emitting sphere((0, 3.2, 0), 0.6) of emission 10 that is also the sampled light.
    list: with a ground sphere and two diffuse spheres in a hittable_list (the linear program of spheres).
    moving: the emitter is a moving sphere; the light then has centre 0, as the reference's center_ (sphere.h:69).
    bvh: the same light over 150 seeded spheres under one bvh_node (the wide tree of spheres, or the binary BVH)."""
    assert variant in SPHERE_VARIANTS, variant
    s = SceneBuilder()
    emit = s.diffuse_light(s.solid((10, 10, 10)))
    ground = s.sphere((0, -100, 0), 100, s.lambertian(s.solid((0.5, 0.55, 0.5))))
    if variant == "moving":
        light = s.moving_sphere((0, 3.2, 0), (0, 3.4, 0), 0.6, emit)
    else:
        light = s.sphere((0, 3.2, 0), 0.6, emit)
    if variant == "bvh":
        rnd = random.Random(150)
        mats = [s.lambertian(s.solid((0.2 + 0.7 * rnd.random(), 0.2 + 0.7 * rnd.random(), 0.2 + 0.7 * rnd.random())))
                for _ in range(5)]
        mats.append(s.metal(s.solid((0.8, 0.8, 0.85)), 0.1))
        objs = [ground, light]
        for i in range(148):
            objs.append(s.sphere((rnd.uniform(-3.5, 3.5), rnd.uniform(0.15, 2.2), rnd.uniform(-3.5, 3.5)),
                                 rnd.uniform(0.1, 0.3), mats[i % 6]))
        world = s.bvh(objs)
    else:
        a = s.sphere((-1.1, 0.7, 0), 0.7, s.lambertian(s.solid((0.7, 0.3, 0.3))))
        b = s.sphere((1.1, 0.7, 0.3), 0.7, s.lambertian(s.solid((0.3, 0.3, 0.7))))
        world = s.hlist([ground, a, b, light])
    cam = perspective(width, 1.0, (0, 2, 6), (0, 1, 0), 1, 50.0)
    return s.desc(world, light=light, background=s.solid((0.25, 0.3, 0.4))), cam


# ------------------------------------------------------------------ the base-class light
BASE_VARIANTS = ("tilted", "flat", "bvh")


def base_light(variant, width=32):
    """The light is hittable_list([emitting quad]): the base class's pdf_value 0 and random (1, 0, 0) (hittable.h:39-41).
    tilted: a ground whose normal has n.x > 0, so the direction (1, 0, 0) has a cosine pdf > 0 on it.
    flat: (1, 0, 0) lies in the ground's plane, both pdfs are 0 and the reference's 0 / 0 makes the pixel NaN.
    bvh: 208 seeded triangles that roughly face +x, and the emitter, under one bvh_node, seen from +x (the wide tree
    and the binary BVH): a first hit has n.x > 0, a later hit from behind has not, so part of the frame is NaN."""
    assert variant in BASE_VARIANTS, variant
    s = SceneBuilder()
    grey = s.lambertian(s.solid((0.6, 0.6, 0.6)))
    emitter = s.quad((-1, 6, -1), (2, 0, 0), (0, 0, 2), s.diffuse_light(s.solid((8, 8, 8))))
    light = s.hlist([emitter])
    sky = s.solid((0.5, 0.6, 0.8))
    if variant == "bvh":
        rnd = random.Random(39)
        mats = [grey, s.lambertian(s.solid((0.7, 0.4, 0.3))), s.lambertian(s.solid((0.3, 0.5, 0.7)))]
        objs = [emitter]
        for i in range(208):
            p = np.array([rnd.uniform(-1, 1), rnd.uniform(0, 5), rnd.uniform(-4, 4)])
            a = np.array([rnd.uniform(-0.2, 0.2), rnd.uniform(0.3, 1.0), rnd.uniform(-0.3, 0.3)])
            b = np.array([rnd.uniform(-0.2, 0.2), rnd.uniform(-0.3, 0.3), rnd.uniform(0.3, 1.0)])
            objs.append(s.triangle(p, p + a, p + b, mats[i % 3]))
        cam = perspective(width, 1.0, (14, 3, 0), (0, 2.5, 0), 1, 24.0)
        return s.desc(s.bvh(objs), light=light, background=sky), cam
    if variant == "flat":
        ground = s.quad((-10, 0, -10), (20, 0, 0), (0, 0, 20), grey)
    else:
        ground = s.quad((-10, 5, -10), (20, -10, 0), (0, 0, 20), grey)
    cam = perspective(width, 1.0, (0, 4, 12), (0, 1, 0), 1, 50.0)
    return s.desc(s.hlist([ground, emitter]), light=light, background=sky), cam
