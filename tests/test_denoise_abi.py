"""The denoiser's entry points (rt_denoise, rt_denoise_check, rt_dev_denoise_host) without a GPU: the symbols and the
ABI version they leave alone, the parameter struct's layout against the C compiler's, the parameter rules one violation
at a time, the host loop over the kernels' own arithmetic (csrc/rt_denoise.h) against the numpy reference, and that
loop under the sanitizers on the shapes at which border indexing can go wrong."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as R
import rt_amd
from rt_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "rt_hip.h")
CSRC = os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native", "denoise_host.cpp")
FIELDS = ("width", "height", "iterations", "precision", "on_device", "flags", "sigma_color", "sigma_normal",
          "sigma_depth", "albedo_eps", "color_eps", "depth_eps")
FRAMES = R.frames()
FRAMES32 = {k: R.rounded_to_float(v) for k, v in FRAMES.items()}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = abi.load()
    for name in ("rt_denoise", "rt_denoise_check"):
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert hasattr(lib, "rt_dev_denoise_host") and "rt_dev_denoise_host" not in abi.SIGNATURES
    assert lib.rt_abi_version() == 8 == abi.ABI_VERSION  # new symbols only
    assert callable(getattr(rt_amd.Context, "denoise", None)) and callable(rt_amd.adaptive_variance)
    with open(HDR) as f:
        text = f.read()
    assert "rt_status rt_denoise(rt_context* ctx, const rt_denoise_params* params, const void* rgb_in" in text
    assert "rt_dev_denoise_host" not in text
    assert abi.RT_DENOISE_DEMODULATE == 1 and "#define RT_DENOISE_DEMODULATE 1" in text


def test_denoise_params_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' % HDR +
                    'printf("%zu", sizeof(rt_denoise_params));\n' +
                    "".join('printf(" %%zu %%zu", offsetof(rt_denoise_params, %s), '
                            'sizeof(((rt_denoise_params*)0)->%s));\n' % (f, f) for f in FIELDS) +
                    'printf("\\n");\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = abi.rt_denoise_params
    want = [ctypes.sizeof(P)]
    for f in FIELDS:
        want += [getattr(P, f).offset, getattr(P, f).size]
    assert got == want
    assert [name for name, _ in P._fields_] == list(FIELDS)
    assert ctypes.sizeof(P) == 72 and P.sigma_color.offset == 24  # 6 x 4 + 6 x 8, no padding


def params(**kw):
    base = dict(width=33, height=31, iterations=5, precision=abi.RT_PREC_F32, on_device=0,
                flags=abi.RT_DENOISE_DEMODULATE, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, albedo_eps=1e-2,
                color_eps=1e-8, depth_eps=1e-3)
    base.update(kw)
    return abi.rt_denoise_params(**base)


def check(prm):
    why = ctypes.create_string_buffer(256)
    st = abi.load().rt_denoise_check(ctypes.byref(prm) if prm is not None else None, why, len(why))
    return st, why.value.decode()


def test_check_accepts_the_defaults_and_the_limits():
    assert check(params()) == (abi.RT_OK, "")
    for kw in (dict(width=1, height=1), dict(width=65535, height=32767), dict(width=32767, height=65535),
               dict(iterations=1), dict(iterations=8), dict(precision=abi.RT_PREC_F64), dict(on_device=1),
               dict(flags=0, albedo_eps=0.0), dict(color_eps=0.0, depth_eps=0.0)):
        assert check(params(**kw)) == (abi.RT_OK, ""), kw


BAD = [dict(width=0), dict(height=0), dict(width=-3), dict(width=65536), dict(height=65536),
       dict(width=65535, height=32769),  # 2^31 + 32767 pixels
       dict(width=46341, height=46341),  # just above 2^31
       dict(iterations=0), dict(iterations=9), dict(precision=2), dict(precision=-1), dict(flags=2), dict(flags=3),
       dict(flags=-1)]
for _name in ("sigma_color", "sigma_normal", "sigma_depth"):
    BAD += [{_name: v} for v in (0.0, -1.0, math.inf, math.nan)]
for _name in ("albedo_eps", "color_eps", "depth_eps"):
    BAD += [{_name: v} for v in (-1e-9, math.inf, math.nan)]
BAD += [dict(albedo_eps=0.0)]  # (demodulating)


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_check_refuses_each_rule_with_a_reason(kw):
    st, why = check(params(**kw))
    assert st == abi.RT_ERR_INVALID_ARGUMENT and len(why) > 5, (kw, why)


def test_check_without_parameters_or_a_buffer():
    assert check(None)[0] == abi.RT_ERR_INVALID_ARGUMENT
    lib = abi.load()
    assert lib.rt_denoise_check(ctypes.byref(params()), None, 0) == abi.RT_OK
    assert lib.rt_denoise_check(ctypes.byref(params(iterations=0)), None, 0) == abi.RT_ERR_INVALID_ARGUMENT
    short = ctypes.create_string_buffer(b"x" * 8, 8)  # the reason is cut to the buffer, with its terminator
    assert lib.rt_denoise_check(ctypes.byref(params(iterations=0)), short, 4) == abi.RT_ERR_INVALID_ARGUMENT
    assert short.raw[3:4] == b"\0" and short.raw[4:8] == b"xxxx"


def test_null_pointers_and_bad_parameters_are_refused_before_any_device():
    lib = abi.load()
    rgb, feat = (ctypes.c_float * 3)(), (ctypes.c_double * 8)()
    one = params(width=1, height=1)
    # without a context the checks that need none still run, and rt_last_error(NULL) names the one that refused
    def refused(prm, a, b, c):
        st = lib.rt_denoise(None, ctypes.byref(prm) if prm is not None else None, a, b, None, c, None)
        assert st == abi.RT_ERR_INVALID_ARGUMENT
        return lib.rt_last_error(None).decode()
    assert refused(one, rgb, feat, rgb) == "null context"
    for args in ((None, rgb, feat, rgb), (one, None, feat, rgb), (one, rgb, None, rgb), (one, rgb, feat, None)):
        assert refused(*args) == "null argument"
    assert refused(params(iterations=0), rgb, feat, rgb) == check(params(iterations=0))[1] != ""
    assert refused(params(sigma_depth=math.nan), rgb, feat, rgb) == check(params(sigma_depth=math.nan))[1] != ""
    assert lib.rt_dev_denoise_host(None, rgb, feat, None, rgb) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_dev_denoise_host(ctypes.byref(one), None, feat, None, rgb) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_dev_denoise_host(ctypes.byref(one), rgb, None, None, rgb) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_dev_denoise_host(ctypes.byref(one), rgb, feat, None, None) == abi.RT_ERR_INVALID_ARGUMENT
    assert lib.rt_dev_denoise_host(ctypes.byref(params(width=1, height=1, iterations=0)), rgb, feat, None,
                                   rgb) == abi.RT_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ the host loop against the numpy reference
F64_BOUND, F32_BOUND = 1e-9, 1e-4  # the project's bars: fp64 max |diff|, fp32 RMSE, both relative to max |ref|
_max_dev32 = [0.0]


def compare(out, ref, f64):
    """The two bounds every comparison with the reference uses -> the largest deviation relative to max |ref|."""
    assert out.shape == ref.shape and np.isfinite(ref).all()
    assert np.isfinite(out).all()  # (the reference has no NaN on these frames, so the output has none)
    scale = np.abs(ref).max()
    dev = float(np.abs(out.astype(np.float64) - ref).max() / scale)
    if f64:
        assert dev < F64_BOUND, dev
    else:
        rmse = float(np.sqrt(((out.astype(np.float64) - ref) ** 2).mean()) / scale)
        assert rmse < F32_BOUND, (rmse, dev)
    return dev


@pytest.mark.parametrize("use_var", [True, False], ids=["var", "novar"])
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("name", list(FRAMES))
def test_host_loop_matches_the_reference(name, iterations, use_var):
    """fp64 to 1e-9 x max|ref| (measured: 1.1e-15 at most), fp32 RMSE below 1e-4 x max|ref| on the float-rounded
    inputs (measured: 1.0e-7 at most). The largest fp32 deviation of a single value, measured on the first run:
    5.3e-7 x max|ref| (frame A, 5 passes) -- a few float ulps, as a chain of convex combinations should give."""
    fr = FRAMES[name]
    var = fr["var"] if use_var else None
    ref = R.denoise(fr["rgb"], fr["feat"], var, iterations=iterations)
    compare(rt_amd.denoise_host(fr["rgb"], fr["feat"], var, iterations=iterations), ref, True)
    fr = FRAMES32[name]
    var = fr["var"] if use_var else None
    ref = R.denoise(fr["rgb"], fr["feat"], var, iterations=iterations)
    out = rt_amd.denoise_host(fr["rgb"].astype(np.float32), fr["feat"], var, iterations=iterations)
    assert out.dtype == np.float32
    dev = compare(out, ref, False)
    _max_dev32[0] = max(_max_dev32[0], dev)
    print(f"{name} iterations {iterations} var {use_var}: fp32 max deviation {dev:.3g} x max|ref| "
          f"(largest so far {_max_dev32[0]:.3g})")


def test_host_loop_without_demodulation_and_in_place():
    fr = FRAMES["A"]
    ref = R.denoise(fr["rgb"], fr["feat"], fr["var"], demodulate=False, sigma_color=1.5, sigma_normal=0.3,
                    sigma_depth=2.0, color_eps=1e-6, depth_eps=1e-2)
    out = rt_amd.denoise_host(fr["rgb"], fr["feat"], fr["var"], demodulate=False, sigma_color=1.5, sigma_normal=0.3,
                              sigma_depth=2.0, color_eps=1e-6, depth_eps=1e-2)
    compare(out, ref, True)
    # rgb_out == rgb_in
    buf = fr["rgb"].copy()
    prm = params(precision=abi.RT_PREC_F64, flags=0, sigma_color=1.5, sigma_normal=0.3, sigma_depth=2.0,
                 color_eps=1e-6, depth_eps=1e-2)
    st = abi.load().rt_dev_denoise_host(ctypes.byref(prm), buf.ctypes.data, fr["feat"].ctypes.data,
                                        fr["var"].ctypes.data, buf.ctypes.data)
    assert st == abi.RT_OK and np.array_equal(buf, out)


def test_adaptive_variance_is_the_estimators_se2():
    rng = np.random.default_rng(5)
    rgb = rng.random((4, 5, 3)).astype(np.float32)
    se2 = rng.random((4, 5)) * 1e-3
    floor = 0.02
    level = rgb.astype(np.float64).sum(-1) / 3.0
    err = np.sqrt(se2 / 3.0) / (floor + level)  # include/rt_hip.h, "adaptive sampling"
    var = rt_amd.adaptive_variance(dict(rgb=rgb, err=err, spp=None), floor)
    assert var.dtype == np.float64 and np.allclose(var, se2, rtol=1e-12, atol=0)


# ------------------------------------------------------------------ the host loop under the sanitizers
def test_host_loop_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "denoise_host_san")
    try:
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, NATIVE], check=True)
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/native/denoise_host.cpp failed")
    for W, H in R.EDGE_SHAPES + ((33, 31), (2, 2), (3, 300)):
        for iterations, use_var, f64 in ((1, 1, 1), (8, 1, 0), (5, 0, 1)):
            r = subprocess.run([exe, str(W), str(H), str(iterations), str(use_var), str(f64)], capture_output=True)
            assert r.returncode == 0, (W, H, iterations, r.stderr.decode()[-2000:])
            fin, npix, _ = r.stdout.decode().split()
            assert int(fin) == int(npix) == W * H  # the broken pixel is repaired
