"""CPU: opaque hit groups -- the C surface of the six calls, the reference restatement (tests/native/surfaces_ref.c) reduced to the
nested reference under an all-glass table, closed forms in float64 that no reference takes part in, the conditions the GPU fixtures are
chosen for, what the setters refuse without a device, and the kernels in the code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
import surfaces_helpers as SH
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from refraction_raytracing_dxr_amd import _capi
from scenes import Scene, load, xf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams)
NEW = {
    "rr_set_surfaces": (C.c_int, [_P, _P, C.c_uint32]),
    "rr_set_lights": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "rr_shade_rays_surfaces": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_shade_rays_surfaces_device": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_render_surfaces": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
    "rr_render_surfaces_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
}
TOL = 1e-5                                                  # the closed forms, relative: test_nested_cpu.py's tolerance for its closed-form ray


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------- (a) the surface
def test_surface_symbols_resolve_with_their_signatures():
    L = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(L, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3                       # additive: the version stays
    assert rr.SURFACE_DTYPE.itemsize == 48 and rr.LIGHT_DTYPE.itemsize == 32 and rr.MAX_LIGHTS == 8
    assert (rr.SURFACE_GLASS, rr.SURFACE_OPAQUE, rr.LIGHT_DIRECTIONAL, rr.LIGHT_POINT) == (0, 1, 0, 1)
    for name in ("set_surfaces", "set_lights", "shade_rays_surfaces", "render_surfaces"):
        assert callable(getattr(rr.Renderer, name)), name
    text = open(HEADER).read()
    for phrase in (r"transparent shadows", r"area lights or environment lighting of opaque surfaces", r"textures", r"NO RAY IS TRACED",
                   r"NOT gated by max_reflect", r"whether or not any instance passes the mask", r"shadow_mask & 1",
                   r"equal the _nested calls byte for byte"):
        assert re.search(phrase, text), phrase


def test_surface_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(sizeof(rr_surface) == 48 && offsetof(rr_surface, albedo) == 4 && offsetof(rr_surface, emission) == 16 &&\n'
                   '               offsetof(rr_surface, specular) == 28 && offsetof(rr_surface, pad) == 40, "surface");\n'
                   '_Static_assert(sizeof(rr_light) == 32 && offsetof(rr_light, kind) == 12 && offsetof(rr_light, radiance) == 16 &&\n'
                   '               offsetof(rr_light, shadow_mask) == 28, "light");\n'
                   '_Static_assert(RR_SURFACE_GLASS == 0 && RR_SURFACE_OPAQUE == 1 && RR_LIGHT_DIRECTIONAL == 0 && RR_LIGHT_POINT == 1 &&\n'
                   '               RR_MAX_LIGHTS == 8, "values");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o, const rr_surface* s,\n'
                   '      const rr_light* l, const rr_ray* r, float* f32, uint8_t* u8, uint32_t* n, const void* dr, void* df, void* du, void* dn) {\n'
                   '    int (*b)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays_surfaces;\n'
                   '    int (*b2)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays_nested;\n'
                   '    int (*d)(rr_context*, const void*, uint32_t, const rr_dispatch_params*, void*, void*, void*) = rr_shade_rays_surfaces_device;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             float*, uint8_t*, uint32_t*) = rr_render_surfaces;\n'
                   '    int (*e2)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '              float*, uint8_t*, uint32_t*) = rr_render_nested;\n'
                   '    int (*g)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             void*, void*, void*) = rr_render_surfaces_device;\n'
                   '    (void)b2; (void)e2;\n'
                   '    return rr_set_surfaces(c, s, 1) | rr_set_lights(c, l, 1, o) | rr_set_lights(c, l, 1, NULL) | b(c, r, 1, p, f32, u8, n) |\n'
                   '           d(c, dr, 1, p, df, du, dn) | e(c, 8, 8, k, p, o, 4, f32, u8, n) | g(c, 8, 8, k, p, o, 4, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "s.o")], check=True)


def test_what_can_be_refused_without_a_device():
    """a null context at every entry point, and what the Python helpers check themselves.  The setters' own refusals are in
    test_gpu_surfaces.py::test_what_the_setters_refuse: as in rr_set_materials, use_device comes before the validation, and a context
    exists only on a machine with a device"""
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    rays = np.zeros(1, rr.RAY_DTYPE)
    row, lt = SH.surfaces(rr.opaque((1, 1, 1))), SH.lights(rr.point_light((0, 1, 0), (1, 1, 1)))
    assert L.rr_set_surfaces(None, row.ctypes.data, 1) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_set_lights(None, lt.ctypes.data, 1, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_surfaces(None, rays.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_surfaces_device(None, None, 1, None, None, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_surfaces(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_surfaces_device(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
    for bad in ((0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 0)):
        with pytest.raises(ValueError):
            rr.directional_light(bad, (1, 1, 1))
    d = rr.directional_light((3, 4, 0), (1, 2, 3), 0x01)
    assert np.allclose(d["v"], (0.6, 0.8, 0.0), atol=1e-7) and d["kind"] == rr.LIGHT_DIRECTIONAL and d["shadow_mask"] == 1
    assert rr.glass()["kind"] == rr.SURFACE_GLASS and rr.opaque((1, 2, 3))["kind"] == rr.SURFACE_OPAQUE
    assert rr.point_light((1, 2, 3), (4, 5, 6))["shadow_mask"] == 0xff


# ------------------------------------------------------------------------------------------------- (b) the reduction of the reference
@pytest.mark.parametrize("name", ["tumbler", "overlap", "five-deep", "twins", "mirrored", "monkey"])
def test_the_reference_reduces_to_the_nested_reference(name):
    """no table, and an all-glass table with lights set: nested_ref.c bit for bit -- colours, RGBA8 and TraceRay counts"""
    for ml in (2, 3):
        sc, rays, want = NH.fixture_ref(name, ml)
        kw = dict(max_refract=8, max_reflect=ml)
        lts = SH.lights(rr.directional_light(SH.SUN, (1, 1, 1)), rr.point_light(SH.LAMP_AT, (2, 2, 2), 0x01))
        for surf, lt, amb in ((None, None, None), (SH.surfaces(*[rr.glass()] * len(NH.TABLE)), lts, (0.5, 0.5, 0.5))):
            got = SH.ref_shade(sc, rays, NH.TABLE, surf, lt, amb, **kw)
            assert bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
            assert got[3].opaque_hits == 0 and got[3].shadow_traced == 0
            assert (got[3].interfaces, got[3].passes, got[3].deepest) == (want[3].interfaces, want[3].passes, want[3].deepest)


# ------------------------------------------------------------------------------------------------- (c) closed forms
ALBEDO = np.array((0.7, 0.6, 0.5))
AMB = np.array((0.05, 0.06, 0.08))
RAD = np.array((1.2, 1.1, 0.9))
KW = dict(max_refract=8, max_reflect=2)


def close(got, want):
    got, want = np.asarray(got, np.float64).reshape(3), np.asarray(want, np.float64).reshape(3)
    print("closed form %s, reference %s" % (want.tolist(), got.tolist()))
    return bool(np.all(np.abs(got - want) <= TOL * np.abs(want)))


def test_closed_form_lit_floor_and_its_shadow():
    """a ray straight down onto the floor y = 0 under a directional light towards (1, 1, 0): albedo * (ambient + radiance * cos 45) at
    x = -1.5; at x = 0 the shadow ray runs into the cube that hovers over x = 1: albedo * ambient"""
    sc, surf = SH.cf_floor()
    lts = SH.lights(rr.directional_light((1, 1, 0), RAD, 0xff))
    rgb, _, cnt, tl = SH.ref_shade(sc, SH.down_ray(-1.5), NH.CF_TABLE, surf, lts, AMB, **KW)
    assert cnt[0] == 2 and tl.shadow_lit == 1
    assert close(rgb[0], ALBEDO * (AMB.astype(np.float32) + RAD.astype(np.float32) * np.cos(np.pi / 4)))
    rgb, _, cnt, tl = SH.ref_shade(sc, SH.down_ray(0.0), NH.CF_TABLE, surf, lts, AMB, **KW)
    assert cnt[0] == 2 and tl.shadow_occluded == 1
    assert close(rgb[0], ALBEDO * AMB.astype(np.float32))
    # a light that does not see the cube (the cube's mask is 1): lit again
    rgb, _, _, tl = SH.ref_shade(sc, SH.down_ray(0.0), NH.CF_TABLE, surf, SH.lights(rr.directional_light((1, 1, 0), RAD, 0x02)), AMB, **KW)
    assert tl.shadow_lit == 1 and close(rgb[0], ALBEDO * (AMB.astype(np.float32) + RAD.astype(np.float32) * np.cos(np.pi / 4)))


def test_closed_form_point_light_above_the_hit():
    """a point light at height h above the hit: albedo * (ambient + radiance / h^2)"""
    sc, surf = SH.cf_floor()
    h = 2.5
    lts = SH.lights(rr.point_light((-1.5, h, 0.13), RAD, 0xff))
    rgb, _, cnt, tl = SH.ref_shade(sc, SH.down_ray(-1.5), NH.CF_TABLE, surf, lts, AMB, **KW)
    assert cnt[0] == 2 and tl.shadow_lit == 1
    assert close(rgb[0], ALBEDO * (AMB.astype(np.float32) + RAD.astype(np.float32) / h ** 2))
    # below the floor's top the light faces the back of the surface: skipped without a ray
    rgb, _, cnt, tl = SH.ref_shade(sc, SH.down_ray(-1.5), NH.CF_TABLE, surf, SH.lights(rr.point_light((-1.5, -h, 0.13), RAD, 0xff)), AMB, **KW)
    assert cnt[0] == 1 and tl.lights_skipped == 1 and close(rgb[0], ALBEDO * AMB.astype(np.float32))


def test_closed_form_perfect_mirror_floor():
    """albedo 0, specular s: env * s, whatever max_reflect says"""
    s = np.array((0.9, 0.5, 0.25), np.float32)
    sc, surf = SH.cf_floor(specular=s, albedo=(0, 0, 0))
    for ml in (0, 2):
        rgb, _, cnt, tl = SH.ref_shade(sc, SH.down_ray(-1.5), NH.CF_TABLE, surf, SH.lights(rr.directional_light((0, 1, 0), RAD)), AMB, max_refract=8,
                                       max_reflect=ml)
        assert cnt[0] == 3 and tl.specular_children == 1            # primary, shadow ray, mirror child
        assert close(rgb[0], np.array(SH.CF_ENV, np.float32).astype(np.float64) * s)


def test_closed_form_emissive_cube_through_two_glass_cubes():
    """NH.closed_form()'s two concentric cubes (rows A and B) round a third of half-side 0.25, emissive with zero albedo: the ray crosses
    two interfaces at normal incidence, 0.5 of A and 0.25 of B: emission * (1 - R)^2 * exp(-sigma_A 0.5) * exp(-sigma_B 0.25)"""
    _, ray, _ = NH.closed_form()
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, 0, (0.5, 0.5, 0.5)), xf(0, 0, 0, (0.25, 0.25, 0.25))], meshes=[0, 0, 0],
                             materials=[0, 1, 2])
    env = np.zeros((8, 16, 3), np.float32)
    env[:] = NH.CF_ENV
    sc = Scene("cf-emissive", [load("cube.obj")], env, inst)
    NH.assert_inside(sc, 2, 1)
    table = np.concatenate([NH.CF_TABLE, np.array([(1.0, (9.0, 9.0, 9.0))], rr.MATERIAL_DTYPE)])        # row 2's glass is never read
    em = np.array((1.5, 1.2, 0.6), np.float32)
    surf = SH.surfaces(rr.glass(), rr.glass(), rr.opaque((0, 0, 0), emission=em))
    rgb, _, cnt, tl = SH.ref_shade(sc, ray, table, surf, SH.lights(rr.directional_light((1, 0, 0), RAD)), AMB, max_refract=8, max_reflect=0)
    assert cnt[0] == 4 and tl.opaque_in_media[2] == 1 and tl.shadow_occluded == 1      # three radiance rays, one shadow ray into the glass
    R0 = (0.2 / 2.2) ** 2
    R = R0 * (1.0 - R0) * 32.0
    sa, sb = NH.CF_TABLE["sigma_a"][0].astype(np.float64), NH.CF_TABLE["sigma_a"][1].astype(np.float64)
    assert close(rgb[0], em.astype(np.float64) * (1.0 - R) ** 2 * np.exp(-sa * 0.5) * np.exp(-sb * 0.25))


# ------------------------------------------------------------------------------------------------- (d) the fixtures' conditions
@pytest.mark.parametrize("name", sorted(SH.FIXTURES))
def test_a_fixture_meets_its_condition(name):
    for ml in (2, 3):
        fx, rays, ref = SH.fixture_ref(name, ml)
        print(name, ml, ref[3])
        assert SH.fixture_condition(name, ref[3]), ref[3]
        assert (ref[2] > 1).mean() > 0.05


def test_the_glass_sphere_shadows_only_lights_that_see_it():
    """table: the sun's shadow rays that cross the glass sphere (mask 0x02) are unoccluded under shadow_mask 0x01 and occluded under
    0xff -- more of its rays are occluded, every other tally of the hits is the same, and only the floor's lit pixels change"""
    fx, rays, ref = SH.fixture_ref("table", 2)
    wide = SH.table(sun_mask=0xff)
    other = wide.ref(rays, max_refract=8, max_reflect=2)
    a, b = ref[3], other[3]
    print(a, b, sep="\n")
    assert b.light_occluded[0] > a.light_occluded[0] and b.light_used[0] == a.light_used[0] and b.light_occluded[1] == a.light_occluded[1]
    assert a.opaque_hits == b.opaque_hits and np.array_equal(ref[2], other[2])
    changed = (ref[0] != other[0]).any(axis=1)
    assert changed.any() and np.all(other[0] <= ref[0])         # positive radiance and albedo: more shadow is never brighter


def test_a_light_no_instance_meets_is_counted_and_unoccluded():
    fx, rays, ref = SH.fixture_ref("table", 2)
    lts = fx.lights.copy()
    lts["shadow_mask"] = 0x80
    got = fx.ref(rays, lts, max_refract=8, max_reflect=2)
    assert got[3].shadow_occluded == 0 and got[3].shadow_traced == ref[3].shadow_traced and np.array_equal(got[2], ref[2])


# ------------------------------------------------------------------------------------------------- (e) the code object
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain is needed")
def test_every_launchable_surface_kernel_is_in_the_code_object(tmp_path):
    ks = kernels(tmp_path)
    for base in ("k_shade_rays_surfaces", "k_render_surfaces"):
        for v in LAUNCHABLE:
            hits = [k for k in ks if ("rr::%s%s" % (base, template_args(*v))) in k]
            assert hits, (base, v)
    # the nested kernels stay beside them
    assert any("rr::k_render_nested<" in k for k in ks) and any("rr::k_shade_rays_nested<" in k for k in ks)
