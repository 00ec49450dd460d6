"""CPU: the C ABI surface of rr_download_tlas, the read-only twin of rr_download_blas for the top level."""
import ctypes as C
import os
import subprocess

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)])


def test_download_tlas_resolves_with_its_signature():
    lib = C.CDLL(rr.lib_path())
    assert hasattr(lib, "rr_download_tlas")
    assert _capi.SYMBOLS["rr_download_tlas"] == SIG
    assert "int  rr_download_tlas(rr_context* ctx, void* nodes, void* qnodes, uint32_t* n_nodes, float grid_org_cell[6]);" in \
        open(os.path.join(ROOT, "include", "rrdxr.h")).read()
    assert rr.lib().rr_abi_version() == 3
    assert callable(rr.Renderer.download_tlas)


def test_download_tlas_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rrdxr.h"\n'
                   'int f(rr_context* c, void* nodes, void* q) {\n'
                   '    int (*a)(rr_context*, void*, void*, uint32_t*, float*) = rr_download_tlas;\n'
                   '    uint32_t n = 0;\n'
                   '    float g[6];\n'
                   '    return a(c, nodes, q, &n, g) | rr_download_tlas(c, 0, 0, &n, 0);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)


def test_download_tlas_rejects_a_null_context():
    n = C.c_uint32(7)
    assert rr.lib().rr_download_tlas(None, None, None, C.byref(n), None) == 1        # RR_ERR_INVALID_ARGUMENT
    assert n.value == 7
