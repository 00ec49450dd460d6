"""CPU: the C ABI surface of the supersampled frames (rr_render_samples[_device], rr_host_sample_pattern, rr_host_camera_rays),
the sample rays against the CPU oracle, and the code generation of k_render_samples."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from refraction_raytracing_dxr_amd import _capi
from shading_helpers import H, W, view_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams)
NEW = {
    "rr_host_sample_pattern": (C.c_int, [C.c_uint32, C.POINTER(C.c_float)]),
    "rr_host_camera_rays": (C.c_int, [_SC, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "rr_render_samples": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
    "rr_render_samples_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
}
# D3D's standard multisample patterns in sixteenths of a pixel from the centre
PATTERNS = {
    1: [(0, 0)],
    2: [(4, 4), (-4, -4)],
    4: [(-2, -6), (6, -2), (-6, 2), (2, 6)],
    8: [(1, -3), (-1, 3), (5, 1), (-3, -5), (-5, 5), (-7, -1), (3, 7), (7, -7)],
    16: [(1, 1), (-1, -3), (-3, 2), (4, -1), (-5, -2), (2, 5), (5, 3), (3, -5), (-2, 6), (0, -7), (-4, -6), (-6, 4), (-8, 0), (7, -4),
         (6, 7), (-7, -8)],
}
VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35), (3.7, 0.2)]


# ------------------------------------------------------------------------------------------------- 1. symbols and surface
def test_samples_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    text = open(HEADER).read()
    assert re.search(r"#define RRDXR_ABI_VERSION 3\b", text) and re.search(r"#define RR_MAX_SAMPLES 64\b", text)
    assert rr.MAX_SAMPLES == 64
    assert callable(rr.Renderer.render_samples) and callable(rr.sample_pattern) and callable(rr.camera_rays)


def test_samples_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(RR_MAX_SAMPLES == 64, "samples");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o, float* f32, uint8_t* u8,\n'
                   '      uint32_t* n, void* df, void* du, void* dn, float* pat, rr_ray* rays) {\n'
                   '    int (*a)(uint32_t, float*) = rr_host_sample_pattern;\n'
                   '    int (*b)(const rr_scene_constants*, uint32_t, uint32_t, float, float, float, float, rr_ray*) = rr_host_camera_rays;\n'
                   '    int (*d)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             float*, uint8_t*, uint32_t*) = rr_render_samples;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             void*, void*, void*) = rr_render_samples_device;\n'
                   '    return a(4, pat) | b(k, 8, 8, 0.5f, 0.5f, 1e-4f, 100.0f, rays) | d(c, 8, 8, k, p, o, 4, f32, u8, n) |\n'
                   '           e(c, 8, 8, k, p, o, 4, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_samples_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    assert L.rr_render_samples(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples_device(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 2. patterns
def test_sample_patterns_are_the_d3d_tables():
    L = rr.lib()
    for n, ks in PATTERNS.items():
        assert len(ks) == n
        buf = (C.c_float * (2 * n))()
        assert L.rr_host_sample_pattern(n, buf) == 0
        want = np.array([[np.float32(0.5) + np.float32(kx) / np.float32(16), np.float32(0.5) + np.float32(ky) / np.float32(16)]
                         for kx, ky in ks], np.float32)
        assert np.array(buf, np.float32).tobytes() == want.tobytes(), n
        assert rr.sample_pattern(n).tobytes() == want.tobytes() and rr.sample_pattern(n).shape == (n, 2)
        assert want.min() >= 0.0 and want.max() < 1.0 and len({tuple(r) for r in want}) == n
    buf = (C.c_float * 130)()
    for n in (0, 3, 32, 65):
        assert L.rr_host_sample_pattern(n, buf) == RR_ERR_INVALID_ARGUMENT, n
        with pytest.raises(rr.RRError) as e:
            rr.sample_pattern(n)
        assert e.value.status == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_sample_pattern(4, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 3. sample rays against the oracle


def oracle_rays(M, cam, w, h, xs, ys):
    """rro_generate_camera_ray of pixels (x, y), x in xs, y in ys, of a w x h frame -> origins, directions [len(ys), len(xs), 3]"""
    o = np.zeros((len(ys), len(xs), 3), np.float32)
    d = np.zeros((len(ys), len(xs), 3), np.float32)
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            o[j, i], d[j, i] = O.camera_ray(M, cam, x, y, w, h)
    return o, d


def check_rays(rays, o, d, tmin, tmax):
    assert rays.shape == (W * H,)
    assert rays["origin"].view(np.uint32).tobytes() == o.reshape(-1, 3).view(np.uint32).tobytes()
    mism = int((rays["dir"].view(np.uint32) != d.reshape(-1, 3).view(np.uint32)).any(axis=1).sum())
    assert mism == 0, mism
    assert np.all(rays["tmin"] == np.float32(tmin)) and np.all(rays["tmax"] == np.float32(tmax))
    assert np.all(rays["flags"] == 0) and np.all(rays["instance_mask"] == 0xff) and np.all(rays["pad"] == 0)


@pytest.mark.parametrize("angle,fov", VIEWS)
def test_sample_rays_equal_the_oracles(angle, fov):
    """offset (0.5, 0.5) is rro_generate_camera_ray; an offset that is an odd multiple of 2^-(n+1) per axis is the oracle's ray of
    pixel 2^n x + (2^n o - 0.5) of a frame 2^n times as large (dividend and divisor scaled by the same power of two: the same
    quotient bits), every pixel compared"""
    sc, M, cam = view_constants(angle, fov)
    o, d = oracle_rays(M, cam, W, H, range(W), range(H))
    check_rays(rr.camera_rays(sc, W, H), o, d, 1e-4, 100.0)
    check_rays(rr.camera_rays(sc, W, H, 0.5, 0.5, tmin=0.25, tmax=7.0), o, d, 0.25, 7.0)
    o4, d4 = oracle_rays(M, cam, 4 * W, 4 * H, range(4 * W), range(4 * H))
    eighths = (0.125, 0.375, 0.625, 0.875)
    for oy in eighths:
        for ox in eighths:
            i, j = int(4 * ox - 0.5), int(4 * oy - 0.5)
            check_rays(rr.camera_rays(sc, W, H, ox, oy), o4[j::4, i::4], d4[j::4, i::4], 1e-4, 100.0)
    for oy in (0.0625, 0.9375):
        for ox in (0.0625, 0.9375):
            i, j = int(8 * ox - 0.5), int(8 * oy - 0.5)
            o8, d8 = oracle_rays(M, cam, 8 * W, 8 * H, range(i, 8 * W, 8), range(j, 8 * H, 8))
            check_rays(rr.camera_rays(sc, W, H, ox, oy), o8, d8, 1e-4, 100.0)
    # the offsets move the rays at all
    assert rr.camera_rays(sc, W, H, 0.125, 0.875).tobytes() != rr.camera_rays(sc, W, H).tobytes()


def test_camera_rays_refuse_bad_arguments():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    rays = np.zeros(64, rr.RAY_DTYPE)
    p = rays.ctypes.data
    assert L.rr_host_camera_rays(C.byref(sc), 8, 8, 0.5, 0.5, 1e-4, 100.0, p) == 0
    assert L.rr_host_camera_rays(C.byref(sc), 8, 8, 0.0, 1.0, 1e-4, 100.0, p) == 0
    for ox, oy in ((float("nan"), 0.5), (0.5, float("nan")), (-0.1, 0.5), (0.5, -0.1), (1.5, 0.5), (0.5, 1.5), (float("inf"), 0.5)):
        assert L.rr_host_camera_rays(C.byref(sc), 8, 8, ox, oy, 1e-4, 100.0, p) == RR_ERR_INVALID_ARGUMENT, (ox, oy)
    assert L.rr_host_camera_rays(C.byref(sc), 0, 8, 0.5, 0.5, 1e-4, 100.0, p) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_camera_rays(C.byref(sc), 8, 0, 0.5, 0.5, 1e-4, 100.0, p) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_camera_rays(None, 8, 8, 0.5, 0.5, 1e-4, 100.0, p) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_camera_rays(C.byref(sc), 8, 8, 0.5, 0.5, 1e-4, 100.0, None) == RR_ERR_INVALID_ARGUMENT
    with pytest.raises(rr.RRError):
        rr.camera_rays(sc, 8, 8, ox=1.5)


# ------------------------------------------------------------------------------------------------- 4. codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_sample_kernels_exist(tmp_path):
    """every k_render_samples<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object; its scratch_ instructions
    are printed next to those of k_shade_rays, which runs the same tree without the three accumulators (no assertion on the
    counts: DESIGN 5.6 records them)"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    mine = {n: v for n, v in k.items() if "k_render_samples<" in n}
    assert len(mine) == len(LAUNCHABLE), sorted(mine)
    for variant in LAUNCHABLE:
        args = template_args(*variant)
        got = [v for n, v in mine.items() if "k_render_samples" + args in n]
        ref = [v for n, v in k.items() if "k_shade_rays" + args in n]
        assert len(got) == 1 and len(ref) == 1, (args, got, ref)
        print("k_render_samples%s: %d scratch instructions, k_shade_rays: %d" % (args, got[0], ref[0]))
