"""CPU: the C ABI surface of the radiance queries (rr_shade_rays[_device]) and the code generation of their kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
_P = C.c_void_p
NEW = {
    "rr_shade_rays": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_capi.DispatchParams), _P, _P, _P]),
    "rr_shade_rays_device": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_capi.DispatchParams), _P, _P, _P]),
}


def test_shade_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    assert re.search(r"#define RRDXR_ABI_VERSION 3\b", open(HEADER).read())
    assert callable(rr.Renderer.shade_rays)


def test_shade_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   'int f(rr_context* c, const rr_ray* r, const rr_dispatch_params* p, float* f32, uint8_t* u8, uint32_t* n,\n'
                   '      const void* dr, void* df, void* du, void* dn) {\n'
                   '    int (*a)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays;\n'
                   '    int (*b)(rr_context*, const void*, uint32_t, const rr_dispatch_params*, void*, void*, void*) = rr_shade_rays_device;\n'
                   '    return a(c, r, 1, p, f32, u8, n) | b(c, dr, 1, p, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_shade_entry_points_reject_a_null_context():
    L = rr.lib()
    r = (C.c_byte * 48)()
    f = (C.c_float * 4)()
    assert L.rr_shade_rays(None, r, 1, None, f, None, None) == 1            # RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_device(None, r, 1, None, f, None, None) == 1


@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_shade_kernels_exist_and_spill_no_more_than_the_render_kernels(tmp_path):
    """every k_shade_rays<STACK, PEND, TLAS, E> the host can launch is in the code objects, and holds no more scratch_
    instructions than k_render_fused<STACK, PEND, false, TLAS, false, E, *>, which parks the same rays"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    shade = {n: v for n, v in k.items() if "k_shade_rays<" in n}
    assert len(shade) == len(LAUNCHABLE), sorted(shade)
    for stack, pend, tlas, e in LAUNCHABLE:
        mine = [v for n, v in shade.items() if "k_shade_rays" + template_args(stack, pend, tlas, e) in n]
        ref = [v for n, v in k.items() if "k_render_fused<%d, %d, false, %s, false, %s, " % (stack, pend, "true" if tlas else "false", e) in n]
        assert len(mine) == 1 and len(ref) == 1, (stack, pend, tlas, e, mine, ref)
        print("k_shade_rays%s: %d scratch instructions, k_render_fused: %d" % (template_args(stack, pend, tlas, e), mine[0], ref[0]))
        assert mine[0] <= ref[0], (stack, pend, tlas, e, mine[0], ref[0])
