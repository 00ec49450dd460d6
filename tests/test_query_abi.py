"""CPU: the C ABI surface of the ray queries (DXR TraceRay's InstanceInclusionMask and RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH)
and the Python ray packer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
NEW = {
    "rr_query_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rr_query_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
}


def test_query_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert _capi.SYMBOLS["rr_trace_rays"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
    assert rr.lib().rr_abi_version() == 3


def test_header_has_the_dxr_flag_and_the_mask_field():
    hdr = open(HEADER).read()
    assert re.search(r"#define RR_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH 0x4u\b", hdr)
    assert re.search(r"#define RR_RAY_FLAG_SKIP_CLOSEST_HIT_SHADER\s+0x8u\b", hdr)
    assert _capi.RAY_FLAG_ACCEPT_FIRST_HIT == 0x4 and rr.RAY_FLAG_ACCEPT_FIRST_HIT == 0x4


def test_query_entry_points_and_ray_layout_compile_as_c99(tmp_path):
    src = tmp_path / "q.c"
    src.write_text('#include <stddef.h>\n#include "rrdxr.h"\n'
                   '_Static_assert(RR_RAY_FLAG_ACCEPT_FIRST_HIT_AND_END_SEARCH == 0x4u, "dxr flag");\n'
                   '_Static_assert(sizeof(rr_ray) == 48, "ray size");\n'
                   '_Static_assert(offsetof(rr_ray, flags) == 32, "flags");\n'
                   '_Static_assert(offsetof(rr_ray, instance_mask) == 36, "instance_mask");\n'
                   '_Static_assert(offsetof(rr_ray, pad) == 40 && sizeof(((rr_ray*)0)->pad) == 8, "pad");\n'
                   'int f(rr_context* c, const rr_ray* r, rr_hit* h, const void* dr, void* dh) {\n'
                   '    int (*a)(rr_context*, const rr_ray*, uint32_t, rr_hit*) = rr_query_rays;\n'
                   '    int (*b)(rr_context*, const void*, uint32_t, void*) = rr_query_rays_device;\n'
                   '    return a(c, r, 1, h) | b(c, dr, 1, dh);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "q.o")], check=True)


def test_ray_dtype_has_the_mask_at_offset_36():
    dt = rr.RAY_DTYPE
    assert dt.itemsize == 48
    assert dt.fields["flags"][1] == 32
    assert dt.fields["instance_mask"][1] == 36 and dt.fields["instance_mask"][0] == np.dtype("<u4")
    assert dt.fields["pad"][1] == 40 and dt.fields["pad"][0].shape == (2,)


def test_pack_rays_numpy_bytes():
    o = np.array([[1.0, 2.0, 3.0], [-1.5, 0.0, 0.25]], np.float32)
    d = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], np.float32)
    rays = rr.pack_rays(o, d, 1e-3, np.array([10.0, 20.0]), flags=[0x4, 0x10], instance_mask=[0x81, 0])
    assert rays.dtype == rr.RAY_DTYPE and len(rays) == 2
    want = b""
    for k in range(2):
        want += np.array([*o[k], [1e-3, 1e-3][k], *d[k], [10.0, 20.0][k]], np.float32).tobytes()
        want += np.array([[0x4, 0x10][k], [0x81, 0][k], 0, 0], np.uint32).tobytes()
    assert rays.tobytes() == want


def test_pack_rays_default_mask_passes_every_instance():
    rays = rr.pack_rays(np.zeros((3, 3)), np.tile([0.0, 1.0, 0.0], (3, 1)), 0.0, 1.0)
    assert np.all(rays["instance_mask"] == 0xff) and np.all(rays["flags"] == 0)
    assert np.all(rays["pad"] == 0)


def test_query_entry_points_reject_a_null_context():
    L = rr.lib()
    r = (C.c_byte * 48)()
    h = (C.c_byte * 24)()
    assert L.rr_query_rays(None, r, 1, h) == 1                      # RR_ERR_INVALID_ARGUMENT
    assert L.rr_query_rays_device(None, r, 1, h) == 1
