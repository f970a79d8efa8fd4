"""planned = written: for every row of the two GPU tables (test_gpu_lights.TABLE, test_gpu_materials.TABLE), the kernel
rt_plan.h path_kernel chooses for the row's scene, precision, traversal, schedule and camera (rt_amd.plan_kernel, which
compiles the descriptor on the host) is the tag the row writes out by hand. On the GPU the same rows assert written =
launched (ctx.last_kernel() == tag), so the three agree; this half needs no GPU."""
import material_scenes as S
import rt_amd
import test_gpu_lights as lights
import test_gpu_materials as materials


def check(rows, build):
    """rows of (scene key, camera kind or None, precision, traversal, segments_per_launch, tag); build(key, camera kind)
    -> (desc, cam), called once per scene and camera."""
    scenes = {}
    for key, cam_kind, prec, trav, sched, tag in rows:
        if (key, cam_kind) not in scenes:
            scenes[(key, cam_kind)] = build(key, cam_kind)
        desc, cam = scenes[(key, cam_kind)]
        got = rt_amd.plan_kernel(desc, cam, precision=prec, traversal=trav, segments_per_launch=sched)
        assert got == tag, (key, cam_kind, prec, trav, sched)


def test_every_light_row_plans_its_tag():
    assert len(lights.TABLE) == 201
    check([(key, None, prec, trav, sched, tag) for key, prec, trav, sched, tag, _ in lights.TABLE],
          lambda key, _: lights.scene(key))


def test_every_material_row_plans_its_tag():
    assert len(materials.TABLE) == 367
    check([(name, cam, prec, trav, sched, tag) for name, prec, trav, sched, cam, tag in materials.TABLE],
          lambda name, cam: S.build(name, cam or "perspective"))
