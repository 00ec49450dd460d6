"""CPU: the C ABI surface of the spectral frames (rr_render_spectral[_device], rr_host_spectral_bands, rr_band)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams)
NEW = {
    "rr_render_spectral": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, _P, C.c_uint32, _P, _P, _P]),
    "rr_render_spectral_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, _P, C.c_uint32, _P, _P, _P]),
    "rr_host_spectral_bands": (C.c_int, [C.c_uint32, C.c_float, C.c_float, _P]),
}


def test_spectral_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    assert re.search(r"#define RRDXR_ABI_VERSION 3\b", open(HEADER).read())
    assert rr.BAND_DTYPE.itemsize == 16 and rr.BAND_DTYPE.names == ("ior", "weight")
    assert rr.BAND_DTYPE.fields["ior"][1] == 0 and rr.BAND_DTYPE.fields["weight"][1] == 4 and rr.BAND_DTYPE["weight"].shape == (3,)
    assert callable(rr.Renderer.render_spectral) and callable(rr.spectral_bands)
    assert "spectral_bands" in rr.__all__


def test_spectral_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(sizeof(rr_band) == 16 && offsetof(rr_band, ior) == 0 && offsetof(rr_band, weight) == 4, "band");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o, rr_band* b,\n'
                   '      float* f32, uint8_t* u8, uint32_t* n, void* df, void* du, void* dn) {\n'
                   '    int (*a)(uint32_t, float, float, rr_band*) = rr_host_spectral_bands;\n'
                   '    int (*d)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, const rr_band*,\n'
                   '             uint32_t, float*, uint8_t*, uint32_t*) = rr_render_spectral;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, const rr_band*,\n'
                   '             uint32_t, void*, void*, void*) = rr_render_spectral_device;\n'
                   '    return a(4, 1.3f, 30.0f, b) | d(c, 8, 8, k, p, o, b, 4, f32, u8, n) | e(c, 8, 8, k, p, o, b, 4, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_spectral_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    bands = np.zeros(1, rr.BAND_DTYPE)
    bands["ior"], bands["weight"] = 1.3, 1.0
    for b in (None, bands.ctypes.data):
        assert L.rr_render_spectral(None, 1, 1, C.byref(sc), None, None, b, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_spectral_device(None, 1, 1, C.byref(sc), None, None, b, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
