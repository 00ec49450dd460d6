"""CPU: the C ABI surface of the multi-hit ray queries (rr_query_rays_multi[_device]) and the code generation of their kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NEW = {
    "rr_query_rays_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rr_query_rays_multi_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
}


def test_multi_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3


def test_header_constants_match_the_binding():
    hdr = open(HEADER).read()
    assert re.search(r"#define RR_QUERY_MAX_HITS 16\b", hdr)
    assert re.search(r"#define RR_HIT_KIND_TRIANGLE_FRONT_FACE 0xFEu", hdr)
    assert re.search(r"#define RR_HIT_KIND_TRIANGLE_BACK_FACE\s+0xFFu", hdr)
    assert re.search(r"#define RRDXR_ABI_VERSION 3\b", hdr)
    assert rr.QUERY_MAX_HITS == 16 and rr.HIT_KIND_FRONT_FACE == 0xFE and rr.HIT_KIND_BACK_FACE == 0xFF


def test_multi_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(RR_QUERY_MAX_HITS == 16, "k");\n'
                   '_Static_assert(RR_HIT_KIND_TRIANGLE_FRONT_FACE == 0xFEu && RR_HIT_KIND_TRIANGLE_BACK_FACE == 0xFFu, "hit kind");\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   'int f(rr_context* c, const rr_ray* r, rr_hit* h, uint32_t* n, const void* dr, void* dh, void* dn) {\n'
                   '    int (*a)(rr_context*, const rr_ray*, uint32_t, uint32_t, rr_hit*, uint32_t*) = rr_query_rays_multi;\n'
                   '    int (*b)(rr_context*, const void*, uint32_t, uint32_t, void*, void*) = rr_query_rays_multi_device;\n'
                   '    return a(c, r, 1, 4, h, n) | b(c, dr, 1, 4, dh, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "m.o")], check=True)


def test_multi_entry_points_reject_a_null_context():
    L = rr.lib()
    r = (C.c_byte * 48)()
    h = (C.c_byte * 24 * 4)()
    n = (C.c_uint32 * 1)()
    assert L.rr_query_rays_multi(None, r, 1, 4, h, n) == 1          # RR_ERR_INVALID_ARGUMENT
    assert L.rr_query_rays_multi_device(None, r, 1, 4, h, n) == 1


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm toolchain not found")
def test_multi_kernels_keep_their_slots_out_of_scratch(tmp_path):
    """every k_query_multi instantiation (STACK x TLAS x KB x COUNT) holds its slots in registers: no scratch_ instruction"""
    import refraction_raytracing_dxr_amd._build as B
    so = tmp_path / "librrdxr.so"
    shutil.copy(B.build(), so)
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    kernels = {}
    for f in sorted(tmp_path.iterdir()):
        if "gfx950" not in f.name:
            continue
        dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "-C", str(f)], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in dis.split("\n"):
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                cur = m.group(1) if "k_query_multi" in m.group(1) else None
                if cur:
                    kernels[cur] = 0
                continue
            if cur and line.strip().startswith("scratch_"):
                kernels[cur] += 1
    assert len(kernels) == 2 * 2 * 5 * 2, sorted(kernels)
    for kb in (1, 2, 4, 8, 16):
        assert any(", %d, true>" % kb in n for n in kernels) and any(", %d, false>" % kb in n for n in kernels), kb
    assert all(v == 0 for v in kernels.values()), {k: v for k, v in kernels.items() if v}
