"""The radiance query's entry point (rt_radiance) without a GPU: the symbol, the ABI version it leaves alone, the
parameter struct's layout against the C compiler's, and the one argument check that needs no context."""
import ctypes
import os
import subprocess

from rt_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "rt_hip.h")
FIELDS = ("seed", "spp", "first_sample", "max_depth", "precision", "traversal", "samples_per_item", "ray_base",
          "on_device")


def test_symbol_is_exported_and_the_abi_version_stays():
    lib = abi.load()
    assert "rt_radiance" in abi.SIGNATURES
    assert lib.rt_radiance is not None and lib.rt_dev_plan_radiance is not None
    assert lib.rt_abi_version() == 8 == abi.ABI_VERSION  # the call is an addition


def test_radiance_params_layout_matches_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){\n' % HDR +
                    'printf("%zu", sizeof(rt_radiance_params));\n' +
                    "".join('printf(" %%zu %%zu", offsetof(rt_radiance_params, %s), '
                            'sizeof(((rt_radiance_params*)0)->%s));\n' % (f, f) for f in FIELDS) +
                    'printf("\\n");\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = abi.rt_radiance_params
    want = [ctypes.sizeof(P)]
    for f in FIELDS:
        want += [getattr(P, f).offset, getattr(P, f).size]
    assert got == want
    assert [name for name, _ in P._fields_] == list(FIELDS)
    assert ctypes.sizeof(P) == 40 and P.ray_base.offset == 32  # written out once: 8 + 8 x 4 bytes, no padding


def test_null_context_is_rejected_without_a_device():
    lib = abi.load()
    prm = abi.rt_radiance_params(seed=1, spp=1, max_depth=1, precision=abi.RT_PREC_F64)
    rays = (ctypes.c_double * 8)()
    out = (ctypes.c_double * 3)()
    assert lib.rt_radiance(None, ctypes.byref(prm), rays, 1, out, None) == abi.RT_ERR_INVALID_ARGUMENT
    assert b"null" in lib.rt_last_error(None)
