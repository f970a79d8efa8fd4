"""Rooms of the flat program (rt_scene.h FlatRoomT, rt_room.h room_rule, rt_device.h trace_flat): five or six
quads that are the faces of one axis-aligned box are traced as one open-box slab test.

Renders, 64x64, 16 spp, depth 8, against the fp64 oracle: fp64 within 1e-9 relative, fp32 per-channel RMSE below
1e-4, the flat program against the reference-ordered linear program (RT_TRAV_ORDERED) likewise, as
test_gpu_flat.py holds them. Ray queries on the Cornell scene against the numpy brute force of trace_ref.py:
t, object, material and side equal on every ray; rays aimed exactly at a wall edge or corner (a class of their own,
under 2 % of the list) are held to t and "one of the adjacent walls". t "equal" means the project's bounds for a
value computed by two formulas: 1e-9 relative in fp64, and in fp32 8 x the error of the reference's formulas
evaluated in numpy float32 on the same rays (test_gpu_trace.py's bound and its reasoning).
"""
import numpy as np
import pytest

import oracle
import rt_amd
import trace_ref
from rt_amd import abi, scenes
from rt_amd.scene import SceneBuilder, perspective

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
INF = np.inf


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


def rmse(a, b):
    return np.sqrt(((a - b) ** 2).reshape(-1, 3).mean(0))


def walls(s, size, faces, mats):
    """Face f of [0, size]: on plane lo (even f) or hi (odd f) of axis f // 2, with material mats[f]."""
    sx, sy, sz = size
    q = {0: ((0, 0, 0), (0, sy, 0), (0, 0, sz)), 1: ((sx, 0, 0), (0, sy, 0), (0, 0, sz)),
         2: ((0, 0, 0), (sx, 0, 0), (0, 0, sz)), 3: ((sx, sy, sz), (-sx, 0, 0), (0, 0, -sz)),
         4: ((0, 0, 0), (sx, 0, 0), (0, sy, 0)), 5: ((0, 0, sz), (sx, 0, 0), (0, sy, 0))}
    return [s.quad(*q[f], mats[f]) for f in faces]


def room_scene(name, width=64):
    """-> desc, cam of a 400 x 300 x 500 room with a wall of its own colour per face, a box and a light in it."""
    s = SceneBuilder()
    size = (400.0, 300.0, 500.0)
    cols = [(.65, .05, .05), (.12, .45, .15), (.73, .73, .73), (.6, .6, .73), (.73, .6, .4), (.5, .7, .7)]
    mats = [s.lambertian(s.solid(c)) for c in cols]
    light = s.diffuse_light(s.solid((15, 15, 15)))
    lq = s.quad((130, 299, 180), (140, 0, 0), (0, 0, 140), light)
    box = s.translate(s.box((0, 0, 0), (90, 160, 90), mats[2]), (150, 0, 230))
    if name == "open_px":  # open toward +x, seen from outside through the opening
        w = walls(s, size, [0, 2, 3, 4, 5], mats)
        cam = perspective(width, 1.0, (1100, 150, 250), (0, 150, 250), 1, 40.0)
    elif name == "closed":  # six world quads, the camera inside
        w = walls(s, size, [0, 1, 2, 3, 4, 5], mats)
        cam = perspective(width, 1.0, (200, 150, 20), (200, 140, 500), 1, 75.0)
    elif name == "metal_wall":  # one metal wall: the general kernel, a material per face
        mats[0] = s.metal(s.solid((0.8, 0.85, 0.88)), 0.05)
        w = walls(s, size, [0, 1, 2, 3, 5], mats)
        cam = perspective(width, 1.0, (200, 150, -600), (200, 150, 0), 1, 40.0)
    else:  # short_wall: the back wall ends below the ceiling, so the five walls are no room
        w = walls(s, size, [0, 1, 2, 3], mats)
        w.append(s.quad((0, 0, 500), (400, 0, 0), (0, 250, 0), mats[5]))
        cam = perspective(width, 1.0, (200, 150, -600), (200, 150, 0), 1, 40.0)
    members = w[:2] + [box] + w[2:] + [lq]  # the walls are not neighbours in the list
    return s.desc(s.hlist(members), light=lq, background=s.solid((0.02, 0.03, 0.05))), cam


def scene_of(name, width=64):
    if name == "cornell":
        desc, cam, _, _ = scenes.cornell_box(width=width)
        return desc, cam
    return room_scene(name, width)


@pytest.mark.parametrize("name", ["cornell", "open_px", "closed", "metal_wall", "short_wall"])
def test_renders_match_the_oracle(ctx, name):
    desc, cam = scene_of(name)
    st, info, msg = abi.scene_check(desc)
    walls_n = {"cornell": 5, "open_px": 5, "closed": 6, "metal_wall": 5, "short_wall": 5}[name]
    assert st == abi.RT_OK and info.flat_quads == walls_n + 1 and info.flat_boxes == (2 if name == "cornell" else 1), msg
    ctx.upload(desc)
    ref, _ = oracle.render(oracle.from_desc(desc), cam, 16, 8, seed=11)
    f64 = ctx.render(cam, 16, 8, seed=11, precision=F64)
    rel = np.abs(f64 - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{name}: fp64 max rel err {rel.max():.2e}, pixels beyond 1e-9: {int((rel > 1e-9).any(-1).sum())}")
    assert (rel <= 1e-9).all()
    flat = ctx.render(cam, 16, 8, seed=11, precision=F32).astype(np.float64)
    ordered = ctx.render(cam, 16, 8, seed=11, precision=F32, traversal=abi.RT_TRAV_ORDERED).astype(np.float64)
    print(f"{name}: fp32 rmse flat {rmse(flat, ref)}, ordered {rmse(ordered, ref)}, flat - ordered {rmse(flat, ordered)}")
    assert (rmse(flat, ref) < 1e-4).all()
    assert (rmse(ordered, ref) < 1e-4).all()
    assert (rmse(flat, ordered) < 1e-4).all()
    assert ref.max() > 0.05  # the scene is lit


@pytest.mark.parametrize("prec", [F64, F32])
def test_schedules_give_the_same_image(ctx, prec):
    desc, cam = room_scene("open_px")
    ctx.upload(desc)
    persistent = ctx.render(cam, 16, 8, seed=5, precision=prec)
    wavefront = ctx.render(cam, 16, 8, seed=5, precision=prec, segments_per_launch=4)
    assert persistent.max() > 0 and np.array_equal(persistent, wavefront)


# ------------------------------------------------------------------ ray queries on the Cornell scene
S = 555.0


def cornell_rays():
    """-> rays (n, 8), edge (n,) bool: the rays aimed exactly at a wall edge or corner, and the targets of those."""
    rng = np.random.default_rng(77)
    o, d = [], []

    def add(oo, dd):
        o.append(np.asarray(oo, np.float64))
        d.append(np.asarray(dd, np.float64))

    n = 640

    def inside(k):
        # Anywhere in the room but the space the two boxes share (x 100..215, y 0..165, z 200..265): a ray from
        # there that leaves through y = 0 meets both box bottoms at one t, a tie between two box() records that
        # the world's bvh_node order decides (in the reference too), not the list order the brute force walks.
        p = rng.uniform(1, S - 1, (k, 3))
        both = (p[:, 0] > 99) & (p[:, 0] < 216) & (p[:, 1] < 166) & (p[:, 2] > 199) & (p[:, 2] < 266)
        p[both, 1] += 170.0
        return p

    # from inside, any direction (some leave through the opening: misses)
    add(inside(n), rng.uniform(-1, 1, (n, 3)))
    # from outside toward the back of the walls (and of the opening, from z < 0)
    oo = rng.uniform(-400, S + 400, (n, 3))
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    oo[np.arange(n), ax] = np.where(side == 1, S + rng.uniform(1, 600, n), -rng.uniform(1, 600, n))
    add(oo, rng.uniform(0, S, (n, 3)) - oo)
    # from inside toward the plane of the opening, inside it and just beside it
    oo = inside(n)
    tg = rng.uniform(-40, S + 40, (n, 3))
    tg[:, 2] = 0.0
    add(oo, (tg - oo) * rng.uniform(0.5, 3, (n, 1)))
    # origin exactly on a wall plane, within the wall or beside it
    oo = rng.uniform(-30, S + 30, (n, 3))
    ax, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    oo[np.arange(n), ax] = np.where(side == 1, S, 0.0)
    add(oo, rng.uniform(-1, 1, (n, 3)))
    # a direction component of exactly zero, of either sign
    dd = rng.uniform(-1, 1, (n, 3))
    dd[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.integers(0, 2, n) == 1, 0.0, -0.0)
    add(rng.uniform(-200, S + 200, (n, 3)), dd)
    # grazing: |d_A| < 1e-9 on one axis
    dd = rng.uniform(-1, 1, (n, 3))
    dd[np.arange(n), rng.integers(0, 3, n)] = rng.uniform(-1e-9, 1e-9, n)
    add(inside(n), dd)
    plain = sum(len(x) for x in o)
    # exactly at an edge or a corner between existing walls, from integer origins (d = target - o is exact, t = 1);
    # the boxes and the light are kept out of the way: origins above the boxes, targets on the ceiling's and the
    # back wall's edges and their corners
    m = 72
    oo = np.stack([rng.integers(20, 536, m), rng.integers(400, 500, m), rng.integers(20, 300, m)], -1).astype(np.float64)
    tg = np.empty((m, 3))
    kind = np.arange(m) % 4
    u = rng.integers(1, 555, m).astype(np.float64)
    xs = np.where(rng.integers(0, 2, m) == 1, S, 0.0)
    tg[kind == 0] = np.stack([xs, np.full(m, S), 300 + u * 0.25], -1)[kind == 0]  # ceiling | side wall
    tg[kind == 1] = np.stack([u, np.full(m, S), np.full(m, S)], -1)[kind == 1]    # ceiling | back wall
    tg[kind == 2] = np.stack([xs, 380 + u * 0.25, np.full(m, S)], -1)[kind == 2]  # side wall | back wall
    tg[kind == 3] = np.stack([xs, np.full(m, S), np.full(m, S)], -1)[kind == 3]   # a corner
    add(oo, tg - oo)
    o, d = np.concatenate(o), np.concatenate(d)
    rays = np.empty((len(o), 8))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, d, 0.0, INF
    edge = np.arange(len(o)) >= plain
    return rays, edge, tg


@pytest.fixture(scope="module")
def cornell_ref():
    desc, _, _, _ = scenes.cornell_box(width=16)
    s = desc._owner
    rays, edge, targets = cornell_rays()
    leaves = trace_ref.flatten(s, desc.world)
    ref = trace_ref.trace(leaves, rays)
    floor = trace_ref.trace(leaves, rays, dtype=np.float32)
    return desc, rays, edge, targets, ref, floor


def rel_err(a, b):
    m = np.isfinite(b)
    return float((np.abs(a[m] - b[m]) / np.maximum(1.0, np.abs(b[m]))).max()) if m.any() else 0.0


@pytest.mark.parametrize("prec", [F64, F32])
def test_cornell_queries_match_the_brute_force(ctx, cornell_ref, prec):
    desc, rays, edge, targets, ref, floor = cornell_ref
    s = desc._owner
    assert 3800 <= len(rays) <= 4200 and edge.mean() <= 0.02
    ctx.upload(desc)
    assert ctx.trace_family(prec, abi.RT_TRAV_AUTO) == "FLAT"
    geom, ids = ctx.trace_rays(rays, precision=prec)
    t, obj, mat, front = geom[:, 0], ids[:, 0], ids[:, 1], ids[:, 3]
    wall_objs = [i for i, ob in enumerate(s.objects) if ob.kind == abi.RT_OBJ_QUAD][:5]
    hit = np.isfinite(ref["t"])
    seen = set(ref["obj"][hit & ~edge])
    assert set(wall_objs) <= seen and 0.05 < (~hit).mean() < 0.5  # every wall, and rays that leave by the opening
    if prec == F64:
        tol = 1e-9
    else:
        ok = hit & (floor["obj"] == ref["obj"]) & ~edge
        tol = 8 * rel_err(floor["t"][ok], ref["t"][ok])
    p = ~edge
    bad = p & ((np.isfinite(t) != hit) | (obj != ref["obj"]) | (mat != ref["material"]) | (front != ref["front"]))
    print(f"precision {prec}: {int(bad.sum())} of {int(p.sum())} rays differ in hit, object, material or side; "
          f"t rel err {rel_err(t[p], ref['t'][p]):.2e} (bound {tol:.2e})")
    assert not bad.any(), (rays[bad][:4], obj[bad][:4], ref["obj"][bad][:4])
    assert rel_err(t[p], ref["t"][p]) <= tol
    # the edge and corner rays: t, and one of the walls that meet there
    adj = []
    for tg in targets:
        a = set()
        for f, k in ((0, 0), (1, 0), (3, 1), (5, 2)):
            if tg[k] == (S if f & 1 else 0.0):
                a.add(wall_objs[[1, 0, 2, 3, 5].index(f)])  # cornell_box lists x = 555, x = 0, y = 0, y = 555, z = 555
        adj.append(a)
    e_t, e_obj = t[edge], obj[edge]
    print(f"precision {prec}: edge rays t err {np.abs(e_t - 1.0).max():.2e}")
    assert np.isfinite(e_t).all() and np.abs(e_t - 1.0).max() <= max(tol, 1e-9)
    assert all(len(a) >= 2 and o_ in a for a, o_ in zip(adj, e_obj))
    assert (mat[edge] == [s.objects[i].material for i in e_obj]).all()
    normals = [np.cross(s.objects[i].b[:], s.objects[i].c[:]) for i in e_obj]  # side: against the wall's own normal
    assert (front[edge] == [int(np.dot(d, n) < 0) for d, n in zip(rays[edge, 3:6], normals)]).all()
