"""CPU: the C ABI surface of the update builds (DXR ALLOW_UPDATE / PERFORM_UPDATE) and vertex updates."""
import ctypes as C
import os
import subprocess

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rr_build_tlas_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "rr_update_mesh_vertices": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "rr_update_mesh_vertices_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
}


def test_update_flags_have_the_dxr_values():
    assert _capi.BUILD_ALLOW_UPDATE == 0x1 and _capi.BUILD_PERFORM_UPDATE == 0x20
    hdr = open(os.path.join(ROOT, "include", "rrdxr.h")).read()
    assert "#define RR_BUILD_ALLOW_UPDATE   0x1u" in hdr and "#define RR_BUILD_PERFORM_UPDATE 0x20u" in hdr


def test_update_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert _capi.SYMBOLS["rr_build_blas_ex"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32])
    assert rr.lib().rr_abi_version() == 3


def test_update_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "u.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(RR_BUILD_ALLOW_UPDATE == 0x1u && RR_BUILD_PERFORM_UPDATE == 0x20u, "dxr flags");\n'
                   'int f(rr_context* c, const rr_instance_desc* d, const rr_vertex* v, const void* dv) {\n'
                   '    int (*a)(rr_context*, const rr_instance_desc*, uint32_t, uint32_t) = rr_build_tlas_ex;\n'
                   '    int (*b)(rr_context*, uint32_t, const rr_vertex*, uint32_t) = rr_update_mesh_vertices;\n'
                   '    int (*e)(rr_context*, uint32_t, const void*, uint32_t) = rr_update_mesh_vertices_device;\n'
                   '    return a(c, d, 1, RR_BUILD_ALLOW_UPDATE) | b(c, 0, v, 3) | e(c, 0, dv, 3)\n'
                   '         | rr_build_blas_ex(c, 0, RR_BUILD_PERFORM_UPDATE);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "u.o")], check=True)


def test_update_entry_points_reject_a_null_context():
    L = rr.lib()
    v = (C.c_byte * 32)()
    assert L.rr_update_mesh_vertices(None, 0, v, 1) == 1                # RR_ERR_INVALID_ARGUMENT
    assert L.rr_update_mesh_vertices_device(None, 0, v, 1) == 1
    assert L.rr_build_tlas_ex(None, v, 1, _capi.BUILD_PERFORM_UPDATE) == 1
