"""The generators of light_scenes.py, pinned without a GPU, so that test_gpu_lights.py cannot hide a gap: the rooms
cover every orientation and sign of an axis-aligned quad light, every oracle frame is lit (and finite where it
should be), and the scene compiler (abi.scene_check) makes of each scene the program its GPU rows count on.

rt_scene_info does not show whether the flat program's walls became a room record (test_room_compile.py reads that
from the compiler itself); what is held here for the reflected rooms, negative coordinates included, is that all 24
keep the flat program with their six quads and the box as a slab record.
"""
import numpy as np
import pytest

import light_scenes as L
import oracle
from rt_amd import abi

SPP, DEPTH, SEED = 16, 8, 11  # test_gpu_lights.py's


def check(desc):
    st, info, msg = abi.scene_check(desc)
    assert st == abi.RT_OK, msg
    return info


def frame(desc, cam):
    ref, _ = oracle.render(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
    return ref


def test_the_24_matrices_are_the_signed_permutations():
    assert len(L.MATRICES) == 24 and len({m.tobytes() for m in L.MATRICES}) == 24
    for m in L.MATRICES:
        assert np.array_equal(np.abs(m).sum(0), [1, 1, 1]) and np.array_equal(np.abs(m).sum(1), [1, 1, 1])
    assert sorted(round(np.linalg.det(m)) for m in L.MATRICES) == [-1] * 12 + [1] * 12


def test_rooms_cover_every_orientation_and_sign_of_the_light():
    seen = set()
    for M in L.MATRICES:
        desc, _ = L.room(M, "ll")
        q, u, v = L.light_quad(desc)
        (U, su), (V, sv) = L.axis_of(u), L.axis_of(v)
        seen.add((U, V, su, sv))
        # the normal keeps its sense: the light faces into the room (toward the image of the room's centre)
        centre = M @ (np.array(L.ROOM_SIZE) / 2)
        assert np.dot(np.cross(u, v), centre - (q + 0.5 * u + 0.5 * v)) > 0
    assert {s[:2] for s in seen} == set(L.UV_PAIRS)                      # all six (axis of u, axis of v) pairs
    assert {s[2] for s in seen} == {1, -1} and {s[3] for s in seen} == {1, -1}  # both signs of both extents
    for uv in L.UV_PAIRS:  # per pair: two sign pairs, u or v of either sign among them
        signs = {s[2:] for s in seen if s[:2] == uv}
        assert len(signs) == 2 and len({a for a, _ in signs} | {b for _, b in signs}) == 2, (uv, signs)


def test_reflected_rooms_keep_the_flat_program_and_render_alike():
    means = []
    for i, M in enumerate(L.MATRICES):
        desc, cam = L.room(M, "ll")
        info = check(desc)
        # five walls and the light as flat quads, the box as a slab record, under every M (negative coordinates too)
        assert (info.flat_quads, info.flat_boxes, info.quads, info.instances) == (6, 1, 12, 1), i
        ref = frame(desc, cam)
        assert np.isfinite(ref).all(), i
        means.append(ref.mean())
    # one scene up to symmetry: the frames' means differ by the sampling noise of 32 x 32 x 16 samples alone
    print(f"means {min(means):.4f} .. {max(means):.4f}")
    assert min(means) > 0.05 and max(means) - min(means) < 0.05 * np.mean(means), (min(means), max(means))


@pytest.mark.parametrize("variant,flat,volumes,spheres", [
    ("metal", (6, 1), 0, 0), ("smoke", (0, 0), 1, 0), ("mats16", (14, 1), 0, 0), ("mats17", (14, 1), 0, 0),
    ("smoke16", (0, 0), 1, 0), ("smoke17", (0, 0), 1, 0),
    ("offaxis", (0, 0), 0, 0),        # a member light off the axes removes the flat program
    ("offaxis_smoke", (0, 0), 1, 0),
    ("offaxis_apart", (6, 1), 0, 0),  # the same light apart from the world leaves it
    ("sphere", (0, 0), 0, 1), ("sphere_smoke", (0, 0), 1, 1), ("sphere_apart", (6, 1), 0, 0)])
def test_room_variants_compile_as_their_rows_expect(variant, flat, volumes, spheres):
    for i in (5, 14, 18):  # the matrices test_gpu_lights.py writes out for these variants
        desc, cam = L.room(L.MATRICES[i], variant)
        info = check(desc)
        assert (info.flat_quads, info.flat_boxes) == flat and info.volumes == volumes and info.spheres == spheres
        assert info.linear_ops > 0  # a hittable_list within the linear program's leaves
        ref = frame(desc, cam)
        assert np.isfinite(ref).all() and ref.mean() > 0.05
    n_mats = len(desc._owner.materials)
    assert n_mats == {"mats16": 16, "mats17": 17, "smoke16": 16, "smoke17": 17}.get(variant, n_mats)


@pytest.mark.parametrize("variant", L.MESH_VARIANTS)
def test_mesh_scenes_are_wide_trees_of_triangles_and_quads(variant):
    for uv in L.UV_PAIRS if variant in ("ll", "metal") else [(1, 2)]:
        desc, cam = L.mesh(uv, variant)
        info = check(desc)
        # past the linear program's leaves: no linear program, a binary BVH, and the wide tree of triangles | quads
        assert info.linear_ops == 0 and info.bvh_nodes > 0 and info.wide_nodes > 0 and info.wide_kinds == 6
        assert (info.triangles, info.quads) == (208, 2)
        q, u, v = L.light_quad(desc)
        if variant != "offaxis":
            assert (L.axis_of(u)[0], L.axis_of(v)[0]) == uv
        assert np.dot(np.cross(u, v), L.CLUSTER - (q + 0.5 * u + 0.5 * v)) > 0  # it faces the cluster
        ref = frame(desc, cam)
        assert np.isfinite(ref).all() and ref.mean() > 0.05
    if variant in ("mats16", "mats17"):
        used = {desc.objects[i].material for i in range(desc.num_objects) if desc.objects[i].material >= 0}
        assert len(used) == len(desc._owner.materials) == (16 if variant == "mats16" else 17)


@pytest.mark.parametrize("uv", [(1, 2), (2, 1)])
def test_terrain_keeps_its_tree_in_hbm_under_a_light_on_an_x_plane(uv):
    desc, cam = L.terrain_hbm(uv, width=64)
    info = check(desc)
    assert info.triangles == 8192 and info.wide_kinds == 6
    assert info.wide_prim_words > 4096  # past what an LDS-resident tree may hold (rt_plan.h wide_tree_in_lds)
    q, u, v = L.light_quad(desc)
    assert (L.axis_of(u)[0], L.axis_of(v)[0]) == uv and np.cross(u, v)[0] > 0
    ref = frame(desc, cam)
    assert np.isfinite(ref).all() and ref.mean() > 0.05


def test_sphere_light_scenes():
    for variant, kinds in (("list", 0), ("moving", 0), ("bvh", 1)):
        desc, cam = L.sphere_light(variant, width=64 if variant == "bvh" else 32)
        info = check(desc)
        assert desc.objects[desc.light].kind == abi.RT_OBJ_SPHERE
        if variant == "bvh":  # spheres only under one bvh_node: the wide kernel of spheres, with a light (not NL)
            assert info.spheres == 150 and info.wide_kinds == 1 and info.linear_ops == 0 and info.bvh_nodes > 0
        else:
            assert info.spheres == 4 and info.linear_ops == 4 and info.bvh_nodes == 0
        assert desc.objects[desc.light].moving == (1 if variant == "moving" else 0)
        ref = frame(desc, cam)
        assert np.isfinite(ref).all() and ref.mean() > 0.05


def test_base_light_scenes():
    tilted, cam = L.base_light("tilted")
    info = check(tilted)
    assert tilted.objects[tilted.light].kind == abi.RT_OBJ_LIST
    assert info.linear_ops == 2 and info.flat_quads == 0  # the tilted ground is no flat quad
    ref = frame(tilted, cam)
    assert np.isfinite(ref).all() and ref.mean() > 0.05  # n.x > 0 on the ground: no zero pdf
    flat, cam = L.base_light("flat")
    info = check(flat)
    assert info.linear_ops == 2 and info.flat_quads == 2
    ref = frame(flat, cam)
    fin = np.isfinite(ref).all(-1)
    # (1, 0, 0) lies in the ground's plane: light pdf 0 and cosine pdf 0, the reference's 0 / 0
    assert 0.2 < fin.mean() < 0.8 and ref[fin].mean() > 0.05, fin.mean()
    # under a bvh_node: triangles that face the camera (n.x > 0 on a first hit), NaN where a path meets one from behind
    mesh, cam = L.base_light("bvh", width=64)
    info = check(mesh)
    assert info.linear_ops == 0 and info.wide_kinds == 6 and (info.triangles, info.quads) == (208, 1)
    ref = frame(mesh, cam)
    fin = np.isfinite(ref).all(-1)
    assert 0.2 < fin.mean() < 0.8 and ref[fin].mean() > 0.05, fin.mean()
