"""The kernel a ray batch launches (rt_plan.h radiance_kernel, through rt_amd.plan_radiance_kernel), without a GPU: for
every scene and traversal of the two GPU tables (test_gpu_materials.ROWS, test_gpu_lights.TABLE), in both precisions, it
is the kernel a perspective render of the scene takes on the persistent schedule, in its "rays" form -- the extended
form ("camx") exactly where the scene's textures give that render one. And the tables reach every persistent kernel
in its rays form, except the ones LEFT_OUT lists with their reasons."""
import pytest

import material_scenes as S
import rt_amd
import test_gpu_lights as lights
import test_gpu_materials as materials
from kernel_tags import all_tags
from rt_amd import abi

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64

# The persistent tags no scene of the tables reaches in the rays form: a batch has no camera model, so its extended
# form comes from a picture or noise texture alone, and the tables hold such a texture only in some families.
LEFT_OUT = {
    # LLI is lambertian + isotropic + light with solid textures only (rt_plan.h lamb_iso_light_scene): with a texture
    # that needs the extended form the scene is no LLI scene. Only another camera model launches this kernel.
    "LinearTrav<{p},0,0,1,1> camx rays persist": "an LLI scene has solid textures only: extended by the camera alone",
    # the tables' scenes of all kinds (smoke_ball, smoke_chain) have solid textures; their extended rows use a lens or
    # a fisheye camera
    "LinearTrav<{p},1,1,1,0> camx rays persist": "no all-kinds scene with a picture or noise texture in the tables",
    # the picture and noise meshes (mesh_image, mesh_perlin) have under 256 nodes and need 9 to 11 stack entries:
    # StackTrav<f32,16,1> and StackTrav<f64,16,0>. The other stack sizes are extended by a fisheye camera only.
    "StackTrav<{p},8,0> camx rays persist": "no textured BVH scene on 8 stack entries in the tables",
    "StackTrav<{p},32,0> camx rays persist": "no textured BVH scene on 32 stack entries in the tables",
    "StackTrav<f32,16,0> camx rays persist": "no textured fp32 BVH scene past 256 nodes in the tables",
}


def rays_form(tag):
    assert tag.endswith(" persist"), tag
    return tag[:-len(" persist")] + " rays persist"


def scenes():
    """(what, scene key, traversal) -> (desc, perspective cam): every scene and traversal of the two tables, once."""
    out = {}
    for name, trav in sorted({(r[0], r[1]) for r in materials.ROWS}):
        out[("materials", name, trav)] = lambda name=name: S.build(name, "perspective")
    for key, trav in sorted({(r[0], r[2]) for r in lights.TABLE}):
        out[("lights", key, trav)] = lambda key=key: lights.scene(key)
    return out


@pytest.fixture(scope="module")
def planned():
    """(what, key, traversal, precision) -> (the batch's tag, the perspective render's tag)."""
    got = {}
    built = {}
    for (what, key, trav), build in scenes().items():
        if (what, key) not in built:
            built[(what, key)] = build()
        desc, cam = built[(what, key)]
        assert cam.mode == abi.RT_CAM_PERSPECTIVE
        for prec in (F32, F64):
            got[(what, key, trav, prec)] = (rt_amd.plan_radiance_kernel(desc, prec, trav),
                                            rt_amd.plan_kernel(desc, cam, precision=prec, traversal=trav,
                                                               segments_per_launch=0))
    return got


def test_a_batch_takes_the_perspective_renders_kernel_in_its_rays_form(planned):
    assert len(planned) >= 2 * 150
    for row, (batch, render) in planned.items():
        assert batch == rays_form(render), row
        assert (" camx " in batch) == (" camx " in render), row
    # the extended form by the textures alone: some scenes have it, most do not
    assert 0 < sum(" camx " in b for b, _ in planned.values()) < len(planned) // 4


def test_every_persistent_kernel_is_reached_in_its_rays_form(planned):
    want = {rays_form(t) for t in all_tags() if t.endswith(" persist")}
    assert len(want) == 64
    got = {b for b, _ in planned.values()}
    assert got <= want
    left = set()
    for tag in LEFT_OUT:
        left |= {tag.format(p=p) for p in ("f32", "f64")}
    assert left <= want and not (left & got), sorted(left & got)  # each one exists, and none is reached after all
    assert want - got == left, sorted((want - got) ^ left)


def test_unknown_arguments_plan_nothing():
    desc, _ = S.build("glass", "perspective")
    with pytest.raises(ValueError):
        rt_amd.plan_radiance_kernel(desc, 7, 0)
    with pytest.raises(ValueError):
        rt_amd.plan_radiance_kernel(desc, F32, 5)
