"""CPU: nested media -- the C surface of the four calls, the reference restatement (tests/native/nested_ref.c) reduced to the material
reference on closed disjoint scenes, a closed-form ray that neither reference takes part in, the conditions the GPU fixtures are chosen
for, and the kernels in the code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from materials_helpers import H, W, view
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams)
NEW = {
    "rr_shade_rays_nested": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_shade_rays_nested_device": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_render_nested": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
    "rr_render_nested_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
}


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------- (a) the surface
def test_nested_symbols_resolve_with_their_signatures():
    L = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(L, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    assert rr.NESTED_MAX_MEDIA == 4 and rr.NESTED_MAX_MATERIAL == 254
    for name in ("shade_rays_nested", "render_nested"):
        assert callable(getattr(rr.Renderer, name)), name
    text = open(HEADER).read()
    # the header states the contract's four limits and its two consequences
    for phrase in (r"more than RR_NESTED_MAX_MEDIA simultaneous media", r"rays that start inside a medium", r"R0 recomputed",
                   r"lens, spectral and adaptive frames; the dispatch kernels", r"NOT AN INTERFACE", r"byte for byte", r"without priorities",
                   r"still costs one count"):
        assert re.search(phrase, text), phrase


def test_nested_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "n.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(RR_NESTED_MAX_MEDIA == 4 && RR_NESTED_MAX_MATERIAL == 254, "limits");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o,\n'
                   '      const rr_ray* r, float* f32, uint8_t* u8, uint32_t* n, const void* dr, void* df, void* du, void* dn) {\n'
                   '    int (*b)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays_nested;\n'
                   '    int (*b2)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays_materials;\n'
                   '    int (*d)(rr_context*, const void*, uint32_t, const rr_dispatch_params*, void*, void*, void*) = rr_shade_rays_nested_device;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             float*, uint8_t*, uint32_t*) = rr_render_nested;\n'
                   '    int (*e2)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '              float*, uint8_t*, uint32_t*) = rr_render_materials;\n'
                   '    int (*g)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             void*, void*, void*) = rr_render_nested_device;\n'
                   '    (void)b2; (void)e2;\n'
                   '    return b(c, r, 1, p, f32, u8, n) | d(c, dr, 1, p, df, du, dn) | e(c, 8, 8, k, p, o, 4, f32, u8, n) |\n'
                   '           g(c, 8, 8, k, p, o, 4, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "n.o")], check=True)


def test_nested_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    rays = np.zeros(1, rr.RAY_DTYPE)
    assert L.rr_shade_rays_nested(None, rays.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_nested_device(None, None, 1, None, None, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_nested(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_nested_device(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- (b) the reduction of the reference
@pytest.mark.parametrize("scene", ["sphere.obj", "cube.obj", "shell.obj", "disjoint"])
def test_the_reference_reduces_to_the_material_reference(scene):
    """closed, consistently wound, pairwise disjoint instances: culled and unculled TraceRay find the same hits, so the nested reference
    is materials_ref.c bit for bit -- colours, RGBA8 and TraceRay counts, under a uniform and a mixed table"""
    sc = NH.reduction_scene(scene)
    rays = rr.camera_rays(view(*NH.REDUCTION_VIEWS[scene]), W, H)
    for table in (MH.uniform(1.5, 3), MH.MIXED):
        for ml in (2, 3):
            kw = dict(max_refract=8, max_reflect=ml)
            want = MH.ref_shade(sc, rays, table, **kw)
            got = NH.ref_shade(sc, rays, table, **kw)
            assert (want[2] > 1).sum() > 50                         # the scene is in view
            assert NH.reduction_holds(got[3]), got[3]               # the view's condition (nested_helpers.REDUCTION_VIEWS)
            assert bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert [int(v) for v in got[3].absorbed[:len(table)]] == [int(v) for v in want[3]]


@pytest.mark.parametrize("scene", ["sphere.obj", "cube.obj", "shell.obj", "disjoint"])
def test_the_reduction_frames_meet_their_condition(scene):
    """the frames test_gpu_nested.py compares with render_materials: no sample of them has a ray for which culling would matter"""
    sc = NH.reduction_scene(scene)
    v, ml = (NH.DISJOINT_FRAME["view"], NH.DISJOINT_FRAME["max_reflect"]) if scene == "disjoint" else (NH.REDUCTION_VIEWS[scene], 3)
    for table in (MH.uniform(1.5, 3), MH.MIXED):
        tls = NH.frame_tallies(sc, view(*v, NH.FW, NH.FH), NH.FW, NH.FH, rr.sample_pattern(4), table, max_refract=8, max_reflect=ml)
        assert all(NH.reduction_holds(t) for t in tls), [repr(t) for t in tls]
        assert sum(t.interfaces for t in tls) > 1000


# ------------------------------------------------------------------------------------------------- (c) a ray with a closed form
def test_the_closed_form_ray():
    """env * (1 - R)^4 * exp(-sigma_A d_A) * exp(-sigma_B d_B) through two concentric cubes at normal incidence, R = R0 (1 - R0) 32, in
    float64.  Relative tolerance 1e-5: about twenty fp32 roundings at 2^-24, three exp at 1 ulp and a second-order direction error come
    to under 4e-6.  The material tree gives another answer for the same ray: it cannot see the inner cube's front face."""
    sc, ray, want = NH.closed_form()
    # the hit normals are the axis: cube.obj's vertex normals are per face
    o = sc.oracle()
    V, I = sc.meshes[0]
    for origin_x, tmin in ((5.0, 1e-4), (1.0, 1e-3), (0.5, 1e-3), (-0.5, 1e-3)):
        h = o.trace(np.array([origin_x, 0.21, 0.13], np.float32), np.array([-1, 0, 0], np.float32), tmin, 100.0, 0, use_bvh=0)
        assert h.hit
        n = V["norm"][np.asarray(I, np.int64)[3 * h.prim:3 * h.prim + 3]]
        assert np.all(np.abs(n[:, 0]) == 1.0) and np.all(n[:, 1:] == 0.0), n
    kw = dict(max_refract=8, max_reflect=0)
    rgb, _, cnt, tl = NH.ref_shade(sc, ray, NH.CF_TABLE, **kw)
    print("closed form %s, nested reference %s, %s" % (want.tolist(), rgb[0].tolist(), tl))
    assert cnt[0] == 5 and tl.interfaces == 4 and tl.passes == 0 and tl.deepest == 2
    assert np.all(np.abs(rgb[0].astype(np.float64) - want) <= 1e-5 * want)
    mat = MH.ref_shade(sc, ray, NH.CF_TABLE, **kw)[0]
    assert np.all(np.abs(mat[0].astype(np.float64) - want) > 1e-3 * want), mat


# ------------------------------------------------------------------------------------------------- (d) the fixtures are what they are for
@pytest.mark.parametrize("name", ["tumbler", "overlap", "five-deep", "twins", "mirrored", "monkey"])
def test_a_fixture_meets_its_condition(name):
    """conditions on the fixtures, read from the reference's tallies (never masks on a comparison): the tumbler reaches a list of
    three, the overlap removes from the middle of the list, five spheres drop a push, the twins pass, the open monkey removes a row that
    is not there.  The containment, overlap and disjointness behind them are asserted when the scene is made (nested_helpers.py)."""
    for ml in (2, 3):
        sc, rays, ref = NH.fixture_ref(name, ml)
        print("%s, max_reflect %d: %d of %d rays hit; %s" % (name, ml, int((ref[2] > 1).sum()), len(rays), ref[3]))
        assert (ref[2] > 1).sum() > 100
        assert NH.fixture_condition(name, ref[3]), ref[3]
    if name != "monkey":                                        # and the material tree does not explain the frame
        assert not bits_equal(ref[0], MH.ref_shade(sc, rays, NH.TABLE, max_refract=8, max_reflect=3)[0])


# ------------------------------------------------------------------------------------------------- (e) codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_nested_kernels_exist(tmp_path):
    """every k_shade_rays_nested and k_render_nested<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object; their
    scratch_ instructions are printed next to those of the material kernels with the same tree (no assertion on the counts: DESIGN 5.11
    records them)"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    for mine, twin in (("k_render_nested", "k_render_materials"), ("k_shade_rays_nested", "k_shade_rays_mat")):
        found = {n: v for n, v in k.items() if mine + "<" in n}
        assert len(found) == len(LAUNCHABLE), sorted(found)
        for variant in LAUNCHABLE:
            args = template_args(*variant)
            got = [v for n, v in found.items() if mine + args in n]
            ref = [v for n, v in k.items() if twin + args in n]
            assert len(got) == 1 and len(ref) == 1, (args, got, ref)
            print("%s%s: %d scratch instructions, %s: %d" % (mine, args, got[0], twin, ref[0]))
