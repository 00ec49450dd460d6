"""CPU: the C ABI surface of transparent shadows (rr_set_shadow_steps, rr_get_shadow_steps, RR_SHADOW_MAX_STEPS) and what the header
says about them.  A context exists only on a machine with a device, so what is refused here is the null context; the refusal of
k > RR_SHADOW_MAX_STEPS, with its text, is in test_gpu_shadows.py."""
import ctypes as C
import os
import re
import subprocess

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
SURFACES_H = os.path.join(ROOT, "refraction_raytracing_dxr_amd", "csrc", "rr_render_surfaces.h")
RR_ERR_INVALID_ARGUMENT = 1
NEW = {
    "rr_set_shadow_steps": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rr_get_shadow_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
}


def test_shadow_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3                       # additive: the version stays
    assert rr.SHADOW_MAX_STEPS == 16 and _capi.SHADOW_MAX_STEPS == 16
    assert callable(rr.Renderer.set_shadow_steps) and callable(rr.Renderer.shadow_steps)


def test_the_header_states_the_contract_and_its_limits():
    text = open(HEADER).read()
    assert re.search(r"#define RR_SHADOW_MAX_STEPS 16\b", text) and re.search(r"#define RRDXR_ABI_VERSION 3\b", text)
    for phrase in (r"T\.ch = T\.ch \* rr_expf_neg\(-\(sigma_c\.ch \* t\)\)", r"Xs\.ch = fmaf\(t, Ld\.ch, Xs\.ch\) and fs = fs - t",
                   r"!\(fs > tmin_secondary\)", r"the cap is conservative", r"E\.ch = fmaf\(radiance\.ch, f \* T\.ch, E\.ch\)", r"f \* 1\.0f == f",
                   r"changes nothing anywhere", r"shadow_mask & 1", r"Fresnel loss and bending at the interfaces", r"absorption beyond the last hit",
                   r"caustics"):
        assert re.search(phrase, text), phrase
    # the lists of what is not covered no longer name transparent shadows; they name what the walk leaves out
    for path in (HEADER, SURFACES_H):
        src = open(path).read()
        lists = re.findall(r"Not covered:.*?(?:\*/|\n\s*(?:\*|//)\s*\n|\n#pragma)", src, flags=re.S)
        assert lists, path
        assert not any(re.search(r"transparent shadows", item, flags=re.I) for item in lists), path
        assert sum(bool(re.search(r"Fresnel loss", item)) and bool(re.search(r"caustics", item)) and bool(re.search(r"absorption beyond", item))
                   for item in lists) >= (2 if path == HEADER else 1), path


def test_shadow_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(RR_SHADOW_MAX_STEPS == 16, "cap");\n'
                   'int f(rr_context* c, uint32_t* k) {\n'
                   '    int (*a)(rr_context*, uint32_t) = rr_set_shadow_steps;\n'
                   '    int (*b)(rr_context*, uint32_t*) = rr_get_shadow_steps;\n'
                   '    return a(c, RR_SHADOW_MAX_STEPS) | b(c, k);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_shadow_entry_points_reject_a_null_context():
    L = rr.lib()
    k = C.c_uint32(7)
    for steps in (0, 8, 16, 17):
        assert L.rr_set_shadow_steps(None, steps) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_get_shadow_steps(None, C.byref(k)) == RR_ERR_INVALID_ARGUMENT and k.value == 7
