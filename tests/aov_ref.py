"""Host-side yardsticks of the feature-buffer tests (test_gpu_aov.py): the perspective camera ray restated in numpy
from rt_camera_desc and the counter RNG (camera.h:244-251, 293), per-pixel feature means from the brute-force closest
hits of tests/trace_ref.py, and the scene clone whose oracle render is the albedo channel."""
import ctypes

import numpy as np

from rt_amd import abi
from rt_amd.scene import SceneBuilder


def unit24(u32):
    """The device's to_unit: the top 24 bits of a draw as a fraction in [0, 1)."""
    return (u32 >> 8) / 16777216.0


def packed_pixels(cam, tiles=None):
    """(x, y) of the pixels in the order render packs `tiles` (default: the whole image)."""
    if tiles is None:
        tiles = [(0, 0, cam.image_width, cam.image_height)]
    out = []
    for x0, y0, w, h in tiles:
        out += [(x0 + i, y0 + j) for j in range(h) for i in range(w)]
    return out


def perspective_rays(cam, spp, seed=1, first_sample=0, tiles=None):
    """camera::generate_ray's perspective branch: (npix * spp, 8) rows o, d, time, inf."""
    assert cam.mode == abi.RT_CAM_PERSPECTIVE
    lib = abi.load()
    W, H = cam.image_width, cam.image_height
    pos, d, right, up = (np.array(v[:]) for v in (cam.pos, cam.dir, cam.right, cam.up))
    du = right * cam.viewport_width / W      # camera.h:137-141
    dv = up * -cam.viewport_height / H
    dir00 = cam.focal_length * d - cam.viewport_width / 2.0 * right + cam.viewport_height / 2.0 * up + 0.5 * (du + dv)
    rows = []
    for x, y in packed_pixels(cam, tiles):
        for s in range(first_sample, first_sample + spp):
            u = [unit24(lib.rt_rng_u32(seed, y * W + x, s, k)) for k in range(3)]
            rd = dir00 + x * du + y * dv + (u[0] - 0.5) * du + (u[1] - 0.5) * dv
            rows.append(list(pos) + list(rd) + [u[2], np.inf])
    return np.array(rows)


def solid_color(builder, tex):
    t = builder.textures[tex]
    assert t.kind == abi.RT_TEX_SOLID
    return np.array(t.color[:])


def features(desc, rays, ref, spp, dtype=np.float64):
    """Per-pixel means of the per-ray contributions, from trace_ref.trace's answer `ref` for `rays` (solid textures
    only): dict(albedo, normal, depth, hit, ids) with ids those of each pixel's first ray."""
    s = desc._owner
    n = rays.shape[0]
    hit = np.isfinite(ref["t"])
    alb = np.zeros((n, 3))
    if desc.background >= 0:  # the unit sphere about the origin is always hit (|d| < 1000): the colour of a miss
        alb[:] = solid_color(s, desc.background).astype(dtype)
    for m in set(ref["material"][hit]):
        alb[hit & (ref["material"] == m)] = solid_color(s, s.materials[m].texture).astype(dtype)
    dlen = np.sqrt((rays[:, 3:6] ** 2).sum(1))
    depth = np.where(hit, np.where(hit, ref["t"], 0.0).astype(np.float64) * dlen, 0.0)
    mean = lambda a: a.reshape((n // spp, spp) + a.shape[1:]).mean(1)
    ids = np.stack([ref["obj"], ref["material"], ref["kind"], ref["front"]], 1).astype(np.int32)
    return dict(albedo=mean(alb), normal=mean(np.asarray(ref["n"], np.float64)), depth=mean(depth),
                hit=mean(hit.astype(np.float64)), ids=ids[::spp])


def as_lights(desc):
    """The scene with every material turned into a diffuse_light of the same texture and no importance-sampled
    light: rendered with max_depth 1 a sample is the texture at its first front-face hit, or the background."""
    src = desc._owner
    s = SceneBuilder(rand=lambda: 0.0)
    s.objects, s.children, s.textures, s.tex_data = src.objects, src.children, src.textures, src.tex_data
    if hasattr(src, "image_data"):
        s.image_data = src.image_data
    s.materials = [abi.rt_material(kind=abi.RT_MAT_DIFFUSE_LIGHT, texture=m.texture, fuzz=0.0, refraction=1.0,
                                   smoothness=0.0, specular_prob=0.0) for m in src.materials]
    return s.desc(desc.world, light=-1, background=desc.background)


def copy_camera(cam, **changes):
    c = abi.rt_camera_desc()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(cam), ctypes.sizeof(c))
    for k, v in changes.items():
        setattr(c, k, v)
    return c
