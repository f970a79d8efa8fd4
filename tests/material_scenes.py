"""Scenes for the material-scatter tests (test_material_scenes.py pins them on the CPU and counts, with the oracle's
event counters, the branches each one reaches; test_gpu_materials.py renders them): every material's scatter, emission
from both faces and through a texture, the miss paths, instances, volumes and the table limits, inside the scenes that
select each path kernel. SCENES maps a name to its generator; every generator returns (desc, cam). The sizes are these
tests' own: 32 x 32, or 64 x 64 for the scenes under a bvh_node (BVH_SCENES).
"""
import math
import random

import numpy as np

import light_scenes as L
from rt_amd.scene import SceneBuilder, fisheye, lens, orthonormal, perspective

SKY = (0.7, 0.8, 1.0)
DIM = (0.02, 0.03, 0.05)


def camera(kind, width, pos, at, fovy, ortho_height):
    """The scene's camera of each model from one position: perspective, or -- the triggers of the kernels' extended
    ("camx") form -- orthonormal (a viewport ortho_height high), fisheye, or lens (focused on `at`)."""
    pos, at = np.asarray(pos, float), np.asarray(at, float)
    if kind == "perspective":
        return perspective(width, 1.0, pos, at, 1, fovy)
    if kind == "orthonormal":
        return orthonormal(width, 1.0, ortho_height, pos, at)
    if kind == "fisheye":
        return fisheye(width, 1.0, pos, at, 1, fovy)
    assert kind == "lens", kind
    return lens(width, 1.0, pos, at, 0.4, float(np.linalg.norm(at - pos)), fovy)


def background(s, bg, scale=0.25):
    """The background texture: a solid colour, "checker" (cells of `scale` on the unit sphere of `miss`), "black"
    (solid 0), or "none" (no background at all: -1)."""
    if bg in (None, "none"):
        return -1
    if bg == "checker":
        return s.checker((0.9, 0.9, 0.9), (0.3, 0.5, 0.9), scale)
    return s.solid((0, 0, 0) if bg == "black" else bg)


# ------------------------------------------------------------------ the room
def _material(s, name):
    """A material by a short name: lamb, glass (1.5), glass067, metal0 / metal05 / metal1 (fuzz 0, 0.5, 1), gloss_hi
    (smoothness 1.5, clamped to 1; specular probability 0.5), gloss_lo (smoothness 0.4; 0.3)."""
    white = s.solid((0.73, 0.73, 0.73))
    return {"lamb": lambda: s.lambertian(white),
            "glass": lambda: s.dielectric(s.solid((1, 1, 1)), 1.5),
            "glass067": lambda: s.dielectric(s.solid((1, 1, 1)), 0.67),
            "metal0": lambda: s.metal(s.solid((0.8, 0.85, 0.88)), 0.0),
            "metal05": lambda: s.metal(s.solid((0.8, 0.7, 0.6)), 0.5),
            "metal1": lambda: s.metal(s.solid((0.7, 0.8, 0.7)), 1.0),
            "gloss_hi": lambda: s.gloss(s.solid((0.7, 0.3, 0.25)), 1.5, 0.5),
            "gloss_lo": lambda: s.gloss(s.solid((0.3, 0.4, 0.7)), 0.4, 0.3)}[name]()


def room(floor="lamb", wall="lamb", block="lamb", rot=0.0, chain=False, vol=None, light="ceiling", bg=DIM,
         n_mats=0, n_quads=0, wall_tex=None, m=0, cam="perspective", width=32):
    """light_scenes.room's open room (400 x 300 x 500, seen through its open face from +x) under the signed permutation
    L.MATRICES[m], with these parts to choose:
    floor, wall, block: the material (_material) of the floor quad, of the far wall and of the block
      box((150,0,230), (240,160,320)); block None: no block.
    rot: the block is rotate_y(box about the origin, rot) moved into place, an instance, not a translated box().
    chain: the block, and a metal sphere beside it, each sit in translate(rotate_x(rotate_y(rotate_z(.)))).
    vol: (boundary, density) makes the block a volume of white smoke: boundary "box", or "sphere" (radius 70). With
      rot or chain the wrappers go around the volume, translate(rotate(volume(box))): a hit in the smoke is a hit
      through an instance.
    light: "ceiling" (light_scenes.ROOM_LIGHT), "checker" (the same quad with a checker texture), "back" (a quad
      hanging in mid-room whose front faces the far wall, so the camera sees its back) or None.
    bg: the background (background()); n_mats: distinct materials in all, by small quads on the floor;
    n_quads: flat quads in all, by small quads of one material; wall_tex: "image", "perlin", "value" or "worley" on the
    far wall.
    cam: perspective, orthonormal, fisheye or lens."""
    M = np.asarray(L.MATRICES[m], float)
    flip = np.linalg.det(M) < 0
    s = SceneBuilder(rand=random.Random(7).random)
    sx, sy, sz = L.ROOM_SIZE
    faces = {0: ((0, 0, 0), (0, sy, 0), (0, 0, sz)), 2: ((0, 0, 0), (sx, 0, 0), (0, 0, sz)),
             3: ((sx, sy, sz), (-sx, 0, 0), (0, 0, -sz)), 4: ((0, 0, 0), (sx, 0, 0), (0, sy, 0)),
             5: ((0, 0, sz), (sx, 0, 0), (0, sy, 0))}

    def quad(q, u, v, mat):
        q, u, v = (M @ np.asarray(x, float) for x in (q, u, v))
        return s.quad(q, v, u, mat) if flip else s.quad(q, u, v, mat)

    mats = {f: s.lambertian(s.solid(c)) for f, c in enumerate(L.WALL_COLOURS)}
    if floor != "lamb":
        mats[2] = _material(s, floor)
    if wall != "lamb":
        mats[0] = _material(s, wall)
    if wall_tex == "image":
        mats[0] = s.lambertian(s.image(np.random.default_rng(3).random((8, 8, 3))))
    elif wall_tex == "perlin":
        mats[0] = s.lambertian(s.perlin(40.0))
    elif wall_tex == "value":
        mats[0] = s.lambertian(s.value(4))
    elif wall_tex == "worley":
        mats[0] = s.lambertian(s.worley())
    members = [quad(*faces[f], mats[f]) for f in (0, 2)]
    if block is not None or vol is not None:
        bm = mats[3] if block in (None, "lamb") else _material(s, block)
        lo, hi = np.array((150.0, 0.0, 230.0)), np.array((240.0, 160.0, 320.0))
        half = (hi - lo) / 2

        def place(obj, centre):
            if chain:
                return s.translate(s.rotate(0, s.rotate(1, s.rotate(2, obj, 20.0), 30.0), 15.0), centre)
            return s.translate(s.rotate(1, obj, rot), centre)

        if vol is not None and vol[0] == "sphere":
            body = s.sphere(M @ ((lo + hi) / 2), 70.0, bm)
        elif rot or chain:
            assert m == 0
            centre = (lo + hi) / 2 + (np.array((0, 40.0, 0)) if chain else 0)
            if vol is not None:  # the chain wraps the volume itself (the volume, not its boundary, is the instance)
                body, vol = place(s.volume(s.box(-half, half, bm), vol[1], s.solid((1, 1, 1))), centre), None
            else:
                body = place(s.box(-half, half, bm), centre)
        else:
            c = [M @ lo, M @ hi]
            body = s.translate(s.box((0, 0, 0), np.maximum(*c) - np.minimum(*c), bm), np.minimum(*c))
        if vol is not None:
            body = s.volume(body, vol[1], s.solid((1, 1, 1)))
        members.append(body)
        if chain:
            members.append(place(s.sphere((0, 0, 0), 55.0, _material(s, "metal05")), (250.0, 70.0, 110.0)))
    members += [quad(*faces[f], mats[f]) for f in (3, 4, 5)]
    rnd = random.Random(33)
    colour = lambda: s.lambertian(s.solid((0.2 + 0.7 * rnd.random(), 0.2 + 0.7 * rnd.random(), 0.2 + 0.7 * rnd.random())))
    k = 0
    if n_mats:  # small quads on the floor, each with a material of its own, all in use
        want = n_mats - (1 if light else 0)
        while len(s.materials) < want:
            members.append(quad((250 + 4 * k, 1 + 0.25 * k, 20 + 14 * k), (12, 0, 0), (0, 0, 12), colour()))
            k += 1
    if n_quads:
        one = colour()
        have = 5 + (6 if block is not None else 0) + (1 if light else 0) + k
        for j in range(n_quads - have):
            members.append(quad((330 + (j % 2) * 14, 1 + 0.25 * j, 10 + 15 * (j // 2)), (12, 0, 0), (0, 0, 12), one))
    lid = -1
    if light:
        if light == "checker":
            emit = s.diffuse_light(s.checker((15, 15, 15), (4, 8, 15), 30.0))
        else:
            emit = s.diffuse_light(s.solid((30, 30, 30) if light == "back" else (15, 15, 15)))
        if light == "back":  # u x v = (0,0,110) x (0,100,0) = (-11000, 0, 0): the front faces the far wall
            lid = quad((200, 100, 180), (0, 0, 110), (0, 100, 0), emit)
        else:
            lid = quad(*L.ROOM_LIGHT, emit)
        members.append(lid)
    if n_mats:
        assert len(s.materials) == n_mats, len(s.materials)
    assert m == 0 or cam == "perspective"
    c = camera(cam, width, (1100, 150, 250), (200, 150, 250), 40.0, 320.0)
    for name in ("pos", "dir", "right", "up"):
        getattr(c, name)[:] = list(M @ np.array(getattr(c, name)[:]))
    return s.desc(s.hlist(members), light=lid, background=background(s, bg)), c


# ------------------------------------------------------------------ triangles and quads under a bvh_node
def prism(s, centre, half, mat):
    """A closed box of 12 triangles about `centre` (outward normals): flat faces, so a ray that refracted in through
    one face meets the adjacent ones beyond the critical angle of glass."""
    c, h = np.asarray(centre, float), np.asarray(half, float)
    out = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            n, u, v = np.zeros(3), np.zeros(3), np.zeros(3)
            n[axis], u[a], v[b] = sign * h[axis], h[a], h[b]
            if sign < 0:
                u, v = v, u  # (u x v keeps pointing along n)
            p = [c + n - u - v, c + n + u - v, c + n + u + v, c + n - u + v]
            out += [s.triangle(p[0], p[1], p[2], mat), s.triangle(p[0], p[2], p[3], mat)]
    return out


MESH_MATS = ("lamb", "metal0", "metal05", "metal1", "gloss_hi", "gloss_lo", "lamb")


def mesh(variant="quads", n=208, deep=0, ground_tex=None, lamb=False, light_tex=None, extras=False, bg=None,
         cam="perspective", width=64):
    """n seeded triangles about (0, 2.5, 0) whose materials cycle through MESH_MATS, and a glass prism of 12 triangles
    in front of them, under one bvh_node: past the linear program's leaves.
    quads: over a ground quad under a quad light (the wide kernel of triangles | quads, or the binary BVH).
    tris: the ground is two triangles and there is no light, under a bright sky (the triangle-only wide kernel).
    ground_tex: "image" or "perlin" on the ground quad (the binary BVH's extended kernels).
    lamb: every triangle lambertian and no prism (the wide LL form). light_tex "checker": the light emits through a
    checker texture. bg: the background (background()) in place of the variant's own.
    extras: a rotated glass box (an instance) and a box of smoke among the triangles: no wide tree, the binary BVH.
    deep > 0: that many more triangles behind the camera, each 20 times as far away (and as large) as the one before.
    All but the farthest then fall into the first of the SAH split's 16 bins, so every level of the binary tree peels
    one of them before the cluster's own tree begins: a deep tree from few primitives."""
    assert variant in ("quads", "tris"), variant
    rnd = random.Random(208)
    s = SceneBuilder(rand=random.Random(7).random)
    mats = [_material(s, name) if name != "lamb" else
            s.lambertian(s.solid((0.25 + 0.7 * rnd.random(), 0.25 + 0.7 * rnd.random(), 0.25 + 0.7 * rnd.random())))
            for name in (("lamb",) * 3 if lamb else MESH_MATS)]
    objs = []
    for i in range(n):
        p = np.array([rnd.uniform(-4, 4), rnd.uniform(0.3, 4.7), rnd.uniform(-4, 1.5)])
        a = np.array([rnd.uniform(-1.2, 1.2) for _ in range(3)])
        b = np.array([rnd.uniform(-1.2, 1.2) for _ in range(3)])
        objs.append(s.triangle(p, p + a, p + b, mats[i % len(mats)]))
    if not lamb:
        objs += prism(s, (1.5, 1.6, 4.0), (1.1, 1.5, 0.9), _material(s, "glass"))
    if extras:
        glass = s.box((-0.8, -1.0, -0.8), (0.8, 1.0, 0.8), _material(s, "glass067"))
        objs.append(s.translate(s.rotate(1, glass, 30.0), (4.5, 0.2, 3.0)))
        objs.append(s.volume(s.translate(s.box((0, 0, 0), (2.0, 2.0, 2.0), mats[0]), (-3.5, -0.9, 3.5)), 0.8,
                             s.solid((1, 1, 1))))
    for k in range(deep):
        f = 20.0 ** k
        p = np.array((40.0 * f, 30.0 * f, 60.0 * f))
        objs.append(s.triangle(p, p + np.array((0.8 * f, 0, 0)), p + np.array((0, 0.8 * f, 0)), mats[0]))
    lid = -1
    if variant == "quads":
        ground = {None: lambda: mats[0], "image": lambda: s.lambertian(s.image(np.random.default_rng(3).random((8, 8, 3)))),
                  "perlin": lambda: s.lambertian(s.perlin(2.0))}[ground_tex]()
        objs.append(s.quad((-30, -1.01, -30), (60, 0, 0), (0, 0, 60), ground))
        emit = s.checker((12, 12, 12), (3, 6, 12), 1.0) if light_tex == "checker" else s.solid((12, 12, 12))
        lid = s.quad(*L.mesh_light((0, 2)), s.diffuse_light(emit))
        objs.append(lid)
        back = (0.1, 0.12, 0.16)
    else:
        g = [np.array(p, float) for p in ((-30, -1.01, -30), (30, -1.01, -30), (30, -1.01, 30), (-30, -1.01, 30))]
        objs += [s.triangle(g[0], g[2], g[1], mats[0]), s.triangle(g[0], g[3], g[2], mats[0])]  # normals up
        back = SKY
    return (s.desc(s.bvh(objs), light=lid, background=background(s, bg or back)),
            camera(cam, width, (10, 7, 15), (0, 2, 0), 38.0, 12.0))


def terrain(variant="tris", cam="perspective", width=64):
    """light_scenes.terrain_hbm's 8,192 triangles: the wide tree stays in HBM.
    tris: no light and no quad, under a bright sky, every eleventh triangle metal of fuzz 0.5: the triangle-only wide
    kernel. ll: all lambertian under that scene's quad light: the wide LL form over a tree in HBM."""
    assert variant in ("tris", "ll"), variant
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
    chrome = _material(s, "metal05") if variant == "tris" else s.lambertian(s.solid((0.4, 0.6, 0.5)))
    objs = [s.triangle(t[0], t[1], t[2], chrome if i % 11 == 0 else ground) for i, t in enumerate(tris)]
    lid = -1
    if variant == "ll":
        lid = s.quad(*L.facing_quad((1, 2), np.array((-150.0, 110.0, 0.0)), np.zeros(3), 120.0),
                     s.diffuse_light(s.solid((15, 15, 15))))
        objs.append(lid)
    back = s.solid(SKY if variant == "tris" else (0.05, 0.07, 0.1))
    return s.desc(s.bvh(objs), light=lid, background=back), camera(cam, width, (180, 140, 160), (0, 0, 0), 50.0, 300.0)


# ------------------------------------------------------------------ spheres
def spheres(n=150, light=False, world="bvh", bg=None, cam="perspective", width=64):
    """A ground sphere and seeded spheres -- lambertian, metal of fuzz 0, 0.5 and 1, glass 1.5 and glass 0.67 in turn --
    under a bright sky with no light (the NL shade form) or, light=True, under light_scenes.sphere_light's emitting
    sphere (the general form). world "bvh": under one bvh_node (the wide tree of spheres, or the binary BVH); "list":
    in a hittable_list (the linear program of spheres; n <= 90).
    n <= 200: n spheres of radius 0.18 to 0.4 (the wide tree in LDS), over a checker ground where there is no light.
    n > 200 (the tree in HBM): 40 such spheres in view, and n small lambertian ones of radius 0.04 to 0.09 spread thinly
    behind the camera, where about one bounce ray in a hundred meets one. Small spheres do not fill the view: the
    reference's sphere test (sphere.h:40-74) subtracts b * b and 4 a c, which agree to (radius / distance)^2, so in
    fp32 the hit point of a sphere of radius 0.065 at distance 6 is off by some 1e-3 radii, the next bounce meets another
    sphere, and every fp32 kernel alike differs from the oracle by more than 1e-3 in a tenth to a fifth of the pixels
    (measured with the small spheres in view: 873 of 4,096 with specular ones, 396 with lambertian ones, the same
    count in the wide and in the binary kernel)."""
    s = SceneBuilder()
    rnd = random.Random(n)
    mats = [s.lambertian(s.solid((0.7, 0.4, 0.3))), _material(s, "metal0"), _material(s, "metal05"),
            _material(s, "metal1"), _material(s, "glass"), _material(s, "glass067"),
            s.lambertian(s.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9), 0.32)), s.lambertian(s.solid((0.3, 0.5, 0.7)))]
    plain = s.lambertian(s.solid((0.5, 0.55, 0.5)))
    objs = [s.sphere((0, -100, 0), 100, mats[6] if not light and n <= 200 else plain)]
    lid = -1
    if light:
        lid = s.sphere((0, 3.2, 0), 0.6, s.diffuse_light(s.solid((10, 10, 10))))
        objs.append(lid)
    for i in range(min(n, 40) if n > 200 else n):
        r = rnd.uniform(0.18, 0.4)
        objs.append(s.sphere((rnd.uniform(-3.5, 3.5), rnd.uniform(r, 2.2), rnd.uniform(-3.5, 3.5)), r, mats[i % 6]))
    for i in range(n if n > 200 else 0):
        r = rnd.uniform(0.04, 0.09)
        objs.append(s.sphere((rnd.uniform(-20, 20), rnd.uniform(r, 5.0), rnd.uniform(9, 30)), r,
                             (mats[0], mats[7])[i % 2]))
    root = s.bvh(objs) if world == "bvh" else s.hlist(objs)
    # (a coarse checker: mirrors and lenses see the background, and every cell edge is a threshold for fp32)
    return (s.desc(root, light=lid, background=background(s, bg or ((0.25, 0.3, 0.4) if light else SKY), 1.0)),
            camera(cam, width, (0, 2, 6), (0, 1, 0), 50.0, 6.0))


def mixed(scale=1, moving=True, cam="perspective", width=64):
    """Spheres, moving spheres, triangles and quads, small and large, under one bvh_node and a quad light: the generic
    wide kernel, its tree in LDS (scale 1: 130 primitives) or in HBM (scale 24). The moving spheres are metal or glass:
    the reference's normal of a moving sphere is not a unit vector (sphere.h:69), and a material with a scattering pdf
    would multiply every bounce by its length. moving=False: static spheres in their place (for fp32 rows)."""
    s = SceneBuilder()
    rnd = random.Random(5 + scale)
    mats = [s.lambertian(s.solid((0.6, 0.5, 0.4))), _material(s, "metal05"), _material(s, "glass"),
            _material(s, "gloss_lo"), s.lambertian(s.solid((0.3, 0.6, 0.5)))]
    size = 1.0 / math.sqrt(scale)
    objs = [s.quad((-30, -0.01, -30), (60, 0, 0), (0, 0, 60), mats[0]),
            s.sphere((-2.5, 1.0, -2.0), 1.0, mats[2]), s.sphere((2.6, 0.9, -1.5), 0.9, mats[1])]
    pt = lambda: np.array([rnd.uniform(-3.5, 3.5), rnd.uniform(0.3, 3.0), rnd.uniform(-3.5, 3.5)])
    vec = lambda: np.array([rnd.uniform(-0.8, 0.8) for _ in range(3)]) * size
    for i in range(40 * scale):
        objs.append(s.sphere(pt(), rnd.uniform(0.15, 0.3) * size, mats[i % 5]))
    for i in range(12 * scale):
        p = pt()
        r = rnd.uniform(0.15, 0.3) * size
        objs.append(s.moving_sphere(p, p + np.array((0, 0.3 * size, 0)), r, mats[1 + i % 2]) if moving else
                    s.sphere(p, r, mats[1 + i % 2]))
    for i in range(50 * scale):
        p = pt()
        objs.append(s.triangle(p, p + vec(), p + vec(), mats[i % 5]))
    for i in range(25 * scale):
        objs.append(s.quad(pt(), vec(), vec(), mats[i % 5]))
    # a low light that faces down (u x v = (0, -4, 0)): the camera, above it, sees its back
    lid = s.quad((-1, 2.6, 0.5), (2, 0, 0), (0, 0, 2), s.diffuse_light(s.solid((40, 40, 40))))
    objs.append(lid)
    return (s.desc(s.bvh(objs), light=lid, background=s.solid((0.1, 0.12, 0.16))),
            camera(cam, width, (0, 3, 9), (0, 1.2, 0), 50.0, 8.0))


def instanced(bg=None, cam="perspective", width=64):
    """Many small trees instead of one: a hittable_list of 7 x translate(hittable_list of 8 x translate(bvh_node of
    32 evenly spaced spheres in a row)), 1,792 small lambertian spheres spread thinly behind the camera (as in
    spheres(n > 200), and for its reason), and in view light_scenes.sphere_light's emitter over 24 large spheres of
    every material. Each translate has a tree of its own, 7 nodes that add to the scene's node count, while the stack
    need grows by the nesting alone: 401 nodes and 8 stack entries, the one shape that gives fp32 rays the binary
    BVH with its nodes in HBM and the 8-entry stack. Past the linear program's 96 ops and no wide tree (instances)."""
    s = SceneBuilder()
    rnd = random.Random(64)
    mats = [s.lambertian(s.solid((0.7, 0.4, 0.3))), _material(s, "metal0"), _material(s, "metal05"),
            _material(s, "metal1"), _material(s, "glass"), _material(s, "glass067")]
    small = [s.lambertian(s.solid((0.3, 0.5, 0.7))), s.lambertian(s.solid((0.6, 0.6, 0.3)))]
    row = s.bvh([s.sphere((-20.0 + 1.3 * i, 0.1, 9.0), 0.07, small[i % 2]) for i in range(32)])
    layer = s.hlist([s.translate(row, (0, 0, 2.6 * k)) for k in range(8)])
    members = [s.translate(layer, (0, 0.7 * j, 0)) for j in range(7)]
    # what is in view: an eighth member, a small tree too (a world of up to 8 members stays a list; a ninth would put
    # a tree above them and two more entries on the stack)
    lid = s.sphere((0, 3.2, 0), 0.6, s.diffuse_light(s.solid((10, 10, 10))))
    seen = [s.sphere((0, -100, 0), 100, s.lambertian(s.solid((0.5, 0.55, 0.5)))), lid]
    for i in range(24):
        r = rnd.uniform(0.25, 0.45)
        seen.append(s.sphere((rnd.uniform(-3.5, 3.5), rnd.uniform(r, 2.2), rnd.uniform(-3.5, 3.5)), r, mats[i % 6]))
    members.append(s.translate(s.bvh(seen), (0, 0, 0)))
    return (s.desc(s.hlist(members), light=lid, background=background(s, bg or (0.25, 0.3, 0.4), 1.0)),
            camera(cam, width, (0, 2, 6), (0, 1, 0), 50.0, 6.0))


# ------------------------------------------------------------------ the scenes by name
# name -> generator(cam=camera model) -> (desc, cam)
SCENES = {
    # the flat program (a box() of glass, metal or gloss is six flat quads; a lambertian one a slab record); under
    # RT_TRAV_ORDERED, or another camera than the perspective one, the linear program of quads
    "glass": lambda **k: room(block="glass", **k),
    "glass_neg": lambda **k: room(block="glass", m=7, **k),  # a reflected room: -0 components in the faces' normals
    "glass067": lambda **k: room(block="glass067", **k),
    "gloss": lambda **k: room(floor="gloss_hi", block="gloss_lo", **k),
    "metal": lambda **k: room(floor="metal05", wall="metal0", block="metal1", **k),
    "nolight": lambda **k: room(floor="metal05", block="glass", light=None, bg=SKY, **k),
    "nolight_checker": lambda **k: room(floor="gloss_lo", light=None, bg="checker", **k),
    "dark": lambda **k: room(block="glass", bg=(0, 0, 0), **k),     # a black background
    "nobg": lambda **k: room(floor="metal05", bg=None, **k),       # no background
    "backlight": lambda **k: room(light="back", **k),        # all lambertian: the LL form
    "backlight_metal": lambda **k: room(light="back", wall="metal05", **k),
    "checker_light": lambda **k: room(light="checker", **k),
    "mats32": lambda **k: room(floor="metal05", n_mats=32, **k),
    "mats33": lambda **k: room(floor="metal05", n_mats=33, **k),
    "quads64": lambda **k: room(floor="metal05", block=None, n_quads=64, **k),
    "quads65": lambda **k: room(floor="metal05", block=None, n_quads=65, **k),
    "quads69": lambda **k: room(floor="metal05", block=None, n_quads=69, **k),  # (fp64 holds the five walls as a room)
    "quads70": lambda **k: room(floor="metal05", block=None, n_quads=70, **k),
    # instances: the linear program
    "glass_rot": lambda **k: room(block="glass", rot=25.0, **k),
    "glass067_rot": lambda **k: room(block="glass067", rot=25.0, **k),
    "gloss_rot": lambda **k: room(floor="gloss_hi", block="gloss_lo", rot=25.0, **k),
    "chain": lambda **k: room(block="glass", chain=True, **k),  # with a sphere: the linear program of spheres
    "chain_image": lambda **k: room(block="glass", chain=True, wall_tex="image", **k),
    # volumes
    "smoke_thick": lambda **k: room(vol=("box", 0.05), **k),
    "smoke_thin": lambda **k: room(vol=("box", 0.002), **k),
    "smoke_chain": lambda **k: room(vol=("box", 0.02), chain=True, **k),
    "smoke_ball": lambda **k: room(vol=("sphere", 0.02), **k),
    "smoke_nolight": lambda **k: room(vol=("box", 0.02), light=None, bg=SKY, **k),
    # picture and noise textures (a trigger of the extended kernels, like the cameras)
    "glass_image": lambda **k: room(block="glass", wall_tex="image", **k),
    "metal_perlin": lambda **k: room(floor="metal05", block="metal1", wall_tex="perlin", **k),
    "gloss_value": lambda **k: room(floor="gloss_hi", block="gloss_lo", wall_tex="value", **k),
    "smoke_value": lambda **k: room(vol=("box", 0.02), wall_tex="value", **k),
    "glass_worley": lambda **k: room(block="glass", wall_tex="worley", **k),
    # spheres
    "spheres_list": lambda **k: spheres(60, light=True, world="list", width=32, **k),
    "spheres_nl": lambda **k: spheres(150, **k),
    "spheres_light": lambda **k: spheres(150, light=True, **k),
    "spheres_nl_hbm": lambda **k: spheres(3000, **k),
    "spheres_light_hbm": lambda **k: spheres(3000, light=True, **k),
    # meshes
    "mesh": lambda **k: mesh("quads", **k),
    "mesh_tris": lambda **k: mesh("tris", **k),
    "mesh_small": lambda **k: mesh("quads", n=90, **k),
    "mesh_deep": lambda **k: mesh("quads", deep=9, **k),
    "terrain": lambda **k: terrain("tris", **k),
    "terrain_ll": lambda **k: terrain("ll", **k),
    "mesh_ll": lambda **k: mesh("quads", lamb=True, **k),
    "mesh_checker_light": lambda **k: mesh("quads", light_tex="checker", **k),
    "mesh_extras": lambda **k: mesh("quads", extras=True, **k),
    "mesh_tris_extras": lambda **k: mesh("tris", extras=True, **k),
    "mesh_image": lambda **k: mesh("quads", ground_tex="image", **k),
    "mesh_perlin": lambda **k: mesh("quads", ground_tex="perlin", **k),
    "spheres_small": lambda **k: spheres(100, light=True, **k),
    "spheres_nl_small": lambda **k: spheres(100, **k),
    "instanced": instanced,
    "mixed": lambda **k: mixed(1, **k),
    "mixed_hbm": lambda **k: mixed(24, **k),
    "mixed_static": lambda **k: mixed(1, moving=False, **k),
    "mixed_static_hbm": lambda **k: mixed(24, moving=False, **k),
}
BVH_SCENES = {"instanced", "mesh", "mesh_checker_light", "mesh_deep", "mesh_extras", "mesh_image", "mesh_ll", "mesh_perlin",
              "mesh_small", "mesh_tris", "mesh_tris_extras", "mixed", "mixed_hbm", "mixed_static", "mixed_static_hbm", "spheres_light",
              "spheres_light_hbm", "spheres_nl", "spheres_nl_hbm", "spheres_nl_small",
              "spheres_small", "terrain", "terrain_ll"}


def build(name, cam="perspective"):
    """(desc, cam) of a scene by name; "name@bg" builds it with the background bg: "none", "black" or "checker"."""
    base, _, bg = name.partition("@")
    return SCENES[base](cam=cam, bg=bg) if bg else SCENES[base](cam=cam)
