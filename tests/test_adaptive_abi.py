"""The adaptive sampler's entry points (rt_render_adaptive, rt_adaptive_check, rt_dev_adaptive_error) without a GPU:
the symbols and the ABI version they leave alone, the parameter struct's layout against the C compiler's, the argument
rules one violation at a time, and the estimator's arithmetic -- the one copy the kernel runs -- against numpy."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import adaptive_reference as ref
import rt_amd
from rt_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "rt_hip.h")
FIELDS = ("seed", "min_spp", "max_spp", "step_spp", "batch", "max_depth", "precision", "traversal", "on_device",
          "threshold", "floor")


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = abi.load()
    for name in ("rt_render_adaptive", "rt_adaptive_check", "rt_dev_adaptive_error"):
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert lib.rt_abi_version() == 8 == abi.ABI_VERSION  # new symbols only
    assert callable(getattr(rt_amd.Context, "render_adaptive", None))
    with open(HDR) as f:
        assert "rt_status rt_render_adaptive(rt_context* ctx, const rt_camera_desc* cam, const rt_adaptive_params*" in f.read()


def test_adaptive_params_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' % HDR +
                    'printf("%zu", sizeof(rt_adaptive_params));\n' +
                    "".join('printf(" %%zu %%zu", offsetof(rt_adaptive_params, %s), '
                            'sizeof(((rt_adaptive_params*)0)->%s));\n' % (f, f) for f in FIELDS) +
                    'printf("\\n");\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = abi.rt_adaptive_params
    want = [ctypes.sizeof(P)]
    for f in FIELDS:
        want += [getattr(P, f).offset, getattr(P, f).size]
    assert got == want
    assert [name for name, _ in P._fields_] == list(FIELDS)
    assert ctypes.sizeof(P) == 56 and P.threshold.offset == 40  # written out once: 8 + 8 x 4 + 2 x 8, no padding


def params(**kw):
    base = dict(seed=1, min_spp=8, max_spp=64, step_spp=8, batch=4, max_depth=8, precision=abi.RT_PREC_F32,
                traversal=abi.RT_TRAV_AUTO, on_device=0, threshold=0.05, floor=0.01)
    base.update(kw)
    return abi.rt_adaptive_params(**base)


def check(prm):
    err = ctypes.create_string_buffer(256)
    st = abi.load().rt_adaptive_check(ctypes.byref(prm) if prm is not None else None, err, len(err))
    return st, err.value.decode()


def test_null_context_is_rejected_without_a_device():
    lib = abi.load()
    cam = abi.rt_camera_desc(image_width=1, image_height=1)
    tile = (abi.rt_tile * 1)(abi.rt_tile(0, 0, 1, 1))
    rgb, spp, err = (ctypes.c_float * 3)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 1)()
    assert lib.rt_render_adaptive(None, ctypes.byref(cam), ctypes.byref(params()), tile, 1, rgb, spp, err,
                                  None) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"null" in lib.rt_last_error(None)


GOOD = [dict(), dict(threshold=0.0), dict(threshold=math.inf), dict(min_spp=64), dict(batch=1, step_spp=1, min_spp=2),
        dict(batch=3, step_spp=6, min_spp=12, max_spp=60), dict(max_depth=0), dict(precision=abi.RT_PREC_F64),
        dict(traversal=abi.RT_TRAV_ORDERED), dict(floor=1e-300), dict(min_spp=16, step_spp=16, batch=8)]
# one rule broken at a time
BAD = [dict(batch=0), dict(batch=-4),
       dict(step_spp=2), dict(step_spp=0), dict(step_spp=6, min_spp=12, max_spp=60),  # below / no multiple of batch
       dict(min_spp=12, step_spp=8), dict(max_spp=60, step_spp=8),  # no multiples of step_spp
       dict(batch=8, step_spp=8, min_spp=8),  # fewer than two batches
       dict(min_spp=0),
       dict(min_spp=72),  # above max_spp
       dict(max_depth=-1),
       dict(precision=2), dict(precision=-1), dict(traversal=2),
       dict(threshold=-1e-9), dict(threshold=math.nan), dict(threshold=-math.inf),
       dict(floor=0.0), dict(floor=-0.01), dict(floor=math.inf), dict(floor=math.nan)]


@pytest.mark.parametrize("kw", GOOD, ids=repr)
def test_check_accepts(kw):
    assert check(params(**kw)) == (abi.RT_OK, "")


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_check_refuses(kw):
    st, msg = check(params(**kw))
    assert st == abi.RT_ERR_INVALID_ARGUMENT and msg


def test_check_null_and_short_buffers():
    assert check(None)[0] == abi.RT_ERR_INVALID_ARGUMENT
    lib = abi.load()
    assert lib.rt_adaptive_check(ctypes.byref(params(batch=0)), None, 0) == abi.RT_ERR_INVALID_ARGUMENT
    small = ctypes.create_string_buffer(b"\xff" * 8, 8)
    assert lib.rt_adaptive_check(ctypes.byref(params(batch=0)), small, 4) == abi.RT_ERR_INVALID_ARGUMENT
    assert small.raw[3:4] == b"\0" and small.raw[4:] == b"\xff" * 4  # terminated inside errlen, nothing past it


# ------------------------------------------------------------------ the estimator
def device_error(K, batch, S, Q, floor):
    D3 = ctypes.c_double * 3
    mean, err = D3(), ctypes.c_double()
    abi.load().rt_dev_adaptive_error(int(K), int(batch), D3(*S), D3(*Q), floor, mean, ctypes.byref(err))
    return np.array(mean[:]), err.value


def same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def moments(s):
    """The moments of the batch sums s (K, 3), added in batch order as the resolve adds them."""
    S, Q = np.zeros(3), np.zeros(3)
    for row in np.asarray(s, np.float64):
        S += row
        Q += row * row
    return S, Q


def compare(s, batch, floor):
    K = len(s)
    S, Q = moments(s)
    mean, err = device_error(K, batch, S, Q, floor)
    rmean, rse2, rerr = ref.estimate(np.array([K]), batch, S[None], Q[None], floor)
    assert same(mean, rmean[0]) and same(err, rerr[0]), (s, batch, floor, mean, rmean, err, rerr)
    return mean, err


def test_estimator_matches_the_numpy_formula_on_random_moments():
    rng = np.random.default_rng(7)
    for _ in range(300):
        K = int(rng.integers(2, 65))
        batch = int(rng.choice([1, 3, 4, 8, 32]))
        s = rng.gamma(0.7, 2.0, (K, 3)) * batch * 10.0 ** rng.integers(-6, 4)
        mean, err = compare(s, batch, float(10.0 ** rng.integers(-4, 1)))
        assert np.isfinite(mean).all() and err > 0
    # ... and on moments that belong to no samples (Q far below S^2 / K: every channel clamps to 0)
    mean, err = device_error(5, 4, [3.0, 4.0, 5.0], [0.1, 0.1, 0.1], 0.01)
    assert err == 0.0 and same(mean, np.array([3.0, 4.0, 5.0]) / 20.0)


def test_estimator_written_out_by_hand():
    # K = 2 batches of 4: sums (4, 8) in red, 2 and 2 in green, 0 in blue
    S, Q = [12.0, 4.0, 0.0], [80.0, 8.0, 0.0]
    mean, err = device_error(2, 4, S, Q, 0.5)
    assert same(mean, [1.5, 0.5, 0.0])
    # var = (80 - 144 / 2) / 1 = 8, 0, 0; se2 = 8 / (2 * 16) = 0.25; err = sqrt(0.25 / 3) / (0.5 + 2 / 3)
    assert err == math.sqrt(0.25 / 3.0) / (0.5 + (2.0 / 3.0))


def test_estimator_edge_cases():
    # all batch sums equal: the variance clamps to 0 (or is a rounding-sized positive number, never negative or NaN)
    for v in (0.0, 1.0, 0.1, 1e-7, 3.3333333333333335, 1e12):
        for K in (2, 3, 7, 16):
            mean, err = compare(np.full((K, 3), v), 4, 0.01)
            assert err >= 0.0 and err < 1e-7, (v, K, err)
    mean, err = compare(np.zeros((2, 3)), 4, 0.01)  # a black pixel: err is 0, not 0 / 0
    assert err == 0.0 and (mean == 0).all()
    # K = 2, the smallest count with a variance (K - 1 = 1)
    compare([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]], 4, 0.01)
    # a NaN sum poisons err (so the pixel fails err <= threshold and runs to max_spp), and only its channel's mean
    mean, err = compare([[1.0, math.nan, 3.0], [3.0, 2.0, 1.0], [1.0, 1.0, 1.0]], 4, 0.01)
    assert math.isnan(err) and math.isnan(mean[1]) and np.isfinite(mean[[0, 2]]).all()
    assert not (err <= math.inf)
    # an infinite sum: inf - inf in the variance, a NaN err again
    mean, err = compare([[1.0, math.inf, 3.0], [3.0, 2.0, 1.0]], 4, 0.01)
    assert math.isnan(err)
