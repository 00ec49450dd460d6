"""CPU: per-instance glass -- the reference restatement (tests/native/materials_ref.c) proved against the oracle, the exp of the
Beer-Lambert factor, the C ABI surface of the material calls and the code generation of their kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from materials_helpers import H, MIXED, VIEW3, W, lib, monkey_scene, ref_shade, three_scene, uniform, view
from refraction_raytracing_dxr_amd import _capi
from shading_helpers import view_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams)
NEW = {
    "rr_set_materials": (C.c_int, [_P, _P, C.c_uint32]),
    "rr_shade_rays_materials": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_shade_rays_materials_device": (C.c_int, [_P, _P, C.c_uint32, _DP, _P, _P, _P]),
    "rr_render_materials": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
    "rr_render_materials_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _P, _P, _P]),
    "rr_host_expf_neg": (C.c_float, [C.c_float]),
}
# The largest error of rr_host_expf_neg against double exp rounded to float, measured over the grid of the test below, is 1 ulp (0.986
# ulps of the exact value, at x = -5.8439355; 6.9 % of the grid's values are off by one, none by more): DESIGN 3 records it.  The
# bound is that measurement rounded up to an integer.
EXPF_BOUND_ULPS = 1


# ------------------------------------------------------------------------------------------------- (a) the restatement is the oracle's
@pytest.mark.parametrize("scene", ["monkey", "three"])
@pytest.mark.parametrize("ior", [1.3, 1.5])
def test_a_uniform_table_is_the_oracles_frame(scene, ior):
    """rows { ior, 0, 0, 0 }: colour bits, UNORM8 bytes and TraceRay counts of rro_render(accum_mode = 1) under that ior"""
    sc = monkey_scene() if scene == "monkey" else three_scene()
    cam, M, c = view_constants(*VIEW3, W, H)
    for mr, ml in ((8, 2), (8, 3)):
        rgb, u8, cnt, absorbed = ref_shade(sc, rr.camera_rays(cam, W, H), uniform(ior, 3), max_refract=mr, max_reflect=ml)
        ref = sc.oracle().render(M, c, W, H, O.default_params(use_bvh=0, accum_mode=1, use_libm=0, ior=ior, max_refract=mr, max_reflect=ml), want_rays=True)
        assert ref["stats"].hits > 100 and ref["stats"].tir > 0
        assert np.array_equal(rgb.view(np.uint32).reshape(H, W, 3), ref["rgb"].view(np.uint32))
        assert np.array_equal(u8.reshape(H, W, 4), ref["rgba8"])
        assert np.array_equal(cnt.reshape(H, W), ref["rays"].astype(np.uint32))
        assert int(cnt.sum()) == ref["stats"].rays
        assert absorbed[0] > 100                                    # rays do arrive from inside: the factor 1 was multiplied in


def test_the_mixed_view_meets_its_condition():
    """the view test_gpu_materials.py renders: every material of the mixed table absorbs at inside hits, and the mixed frame's ray counts
    differ from those of every uniform table -- under both reflection limits it runs with"""
    sc = three_scene()
    rays = rr.camera_rays(view(*VIEW3), W, H)
    for ml in (2, 3):
        rgb, _, cnt, absorbed = ref_shade(sc, rays, MIXED, max_refract=8, max_reflect=ml)
        diffs = []
        for ior in MIXED["ior"]:
            urgb, _, ucnt, _ = ref_shade(sc, rays, uniform(ior, 3), max_refract=8, max_reflect=ml)
            diffs.append(int((ucnt != cnt).sum()))
            assert (urgb.view(np.uint32) != rgb.view(np.uint32)).any()
        print("max_reflect %d: inside hits absorbed at per material %s; pixels whose ray count differs from the uniform frames %s" %
              (ml, absorbed.tolist(), diffs))
        assert np.all(absorbed >= 1) and min(diffs) >= 1
    # the tint is per channel: the red glass of instance 1 passes more red than green where only it is seen
    clear = MIXED.copy()
    clear["sigma_a"] = 0
    plain = ref_shade(sc, rays, clear, max_refract=8, max_reflect=2)[0]
    tinted = ref_shade(sc, rays, MIXED, max_refract=8, max_reflect=2)[0]
    assert np.all(tinted <= plain) and (tinted < plain).any()       # absorption only removes light (the counts and paths are the same)


# ------------------------------------------------------------------------------------------------- (b) exp for x <= 0
def expf_grid():
    rng = np.random.default_rng(11)
    x = np.concatenate([-np.logspace(-8, np.log10(87.0), 4000), -rng.uniform(0, 87, 60000), -np.exp(rng.uniform(np.log(1e-8), np.log(87.0), 40000))])
    return x.astype(np.float32)


def test_expf_neg_is_exact_at_its_ends_and_within_its_bound():
    f, g = rr.lib().rr_host_expf_neg, lib().mref_expf_neg
    for z in (0.0, -0.0):
        assert np.float32(f(z)).view(np.uint32) == np.float32(1.0).view(np.uint32)
    for cut in (-87.0, float(np.nextafter(np.float32(-87), np.float32(-100))), -88.0, -1e30, float("-inf")):
        assert np.float32(f(cut)).view(np.uint32) == 0, cut
    x = expf_grid()
    assert len(x) == 104000 and x.max() < 0 and x.min() >= -87
    x = np.concatenate([x, np.float32([0.0, -0.0, -87.0, -88.0, -np.inf, np.nextafter(np.float32(-87), np.float32(0))])])
    got = np.array([f(float(v)) for v in x], np.float32)
    again = np.array([g(float(v)) for v in x], np.float32)
    assert got.view(np.uint32).tobytes() == again.view(np.uint32).tobytes()         # the library's copy and the reference's restatement
    assert got.min() >= 0.0 and got.max() <= 1.0
    live = x > np.float32(-87)
    assert np.all(got[~live] == 0) and np.all(got[live] >= np.finfo(np.float32).tiny)   # above the cut: always a normal number
    want = np.exp(x[live].astype(np.float64)).astype(np.float32)
    ulps = np.abs(got[live].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    exact = np.abs(got[live].astype(np.float64) - np.exp(x[live].astype(np.float64))) / np.spacing(want).astype(np.float64)
    print("rr_host_expf_neg against double exp rounded to float: at most %d ulp, %.2f %% of %d values off; %.4f ulps from the exact value at x = %r" %
          (ulps.max(), 100.0 * (ulps > 0).mean(), live.sum(), exact.max(), float(x[live][exact.argmax()])))
    assert ulps.max() <= EXPF_BOUND_ULPS
    # decreasing in -x wherever the rounding lets it show: never more than the bound out of order
    order = np.argsort(x[live])
    steps = np.diff(got[live][order].view(np.int32).astype(np.int64))
    assert steps.min() >= -2 * EXPF_BOUND_ULPS


# ------------------------------------------------------------------------------------------------- (c) the surface
def test_material_symbols_resolve_with_their_signatures():
    L = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(L, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    assert rr.MATERIAL_DTYPE.itemsize == 16 and rr.MATERIAL_DTYPE.names == ("ior", "sigma_a")
    assert rr.MATERIAL_DTYPE.fields["ior"][1] == 0 and rr.MATERIAL_DTYPE.fields["sigma_a"][1] == 4 and rr.MATERIAL_DTYPE["sigma_a"].shape == (3,)
    for name in ("set_materials", "shade_rays_materials", "render_materials"):
        assert callable(getattr(rr.Renderer, name)), name
    text = open(HEADER).read()
    assert re.search(r"params->ior is ignored", text)               # the header says so


def test_material_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(sizeof(rr_material) == 16 && offsetof(rr_material, ior) == 0 && offsetof(rr_material, sigma_a) == 4, "material");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o, const rr_material* m,\n'
                   '      const rr_ray* r, float* f32, uint8_t* u8, uint32_t* n, const void* dr, void* df, void* du, void* dn) {\n'
                   '    int (*a)(rr_context*, const rr_material*, uint32_t) = rr_set_materials;\n'
                   '    int (*b)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays_materials;\n'
                   '    int (*b2)(rr_context*, const rr_ray*, uint32_t, const rr_dispatch_params*, float*, uint8_t*, uint32_t*) = rr_shade_rays;\n'
                   '    int (*d)(rr_context*, const void*, uint32_t, const rr_dispatch_params*, void*, void*, void*) = rr_shade_rays_materials_device;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             float*, uint8_t*, uint32_t*) = rr_render_materials;\n'
                   '    int (*e2)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '              float*, uint8_t*, uint32_t*) = rr_render_samples;\n'
                   '    int (*g)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, uint32_t,\n'
                   '             void*, void*, void*) = rr_render_materials_device;\n'
                   '    float (*h)(float) = rr_host_expf_neg;\n'
                   '    (void)b2; (void)e2;\n'
                   '    return a(c, m, 3) | b(c, r, 1, p, f32, u8, n) | d(c, dr, 1, p, df, du, dn) | e(c, 8, 8, k, p, o, 4, f32, u8, n) |\n'
                   '           g(c, 8, 8, k, p, o, 4, df, du, dn) | (int)h(-1.0f);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "m.o")], check=True)


def test_make_instances_puts_the_material_in_the_low_24_bits_only():
    T = [np.eye(4, dtype=np.float32)[:3]] * 3
    kw = dict(transforms=T, meshes=[0, 1, 0], masks=[1, 0xff, 2], flags=[0, _capi.INSTANCE_FLAG_CULL_DISABLE, _capi.INSTANCE_FLAG_FRONT_CCW])
    plain = rr.make_instances(**kw)
    assert rr.make_instances(materials=None, **kw).tobytes() == plain.tobytes()
    assert rr.make_instances(materials=[0, 0, 0], **kw).tobytes() == plain.tobytes()
    assert np.all(plain["hitgroup_flags"] & 0xffffff == 0)
    made = rr.make_instances(materials=[5, 0xffffff, 0x1000002], **kw)
    assert (made["hitgroup_flags"] & 0xffffff).tolist() == [5, 0xffffff, 2]
    assert np.array_equal(made["hitgroup_flags"] >> 24, plain["hitgroup_flags"] >> 24)
    for name in ("transform", "instance_id_mask", "blas"):
        assert made[name].tobytes() == plain[name].tobytes(), name


def test_material_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    rays = np.zeros(1, rr.RAY_DTYPE)
    assert L.rr_set_materials(None, MIXED.ctypes.data, 3) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_set_materials(None, None, 0) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_materials(None, rays.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_materials_device(None, None, 1, None, None, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_materials(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_materials_device(None, 1, 1, C.byref(sc), None, None, 1, f, None, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- (d) codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_material_kernels_exist(tmp_path):
    """every k_shade_rays_mat and k_render_materials<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object; their
    scratch_ instructions are printed next to those of the scalar kernels with the same tree (no assertion on the counts: DESIGN 5.10
    records them)"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    for mine, twin in (("k_render_materials", "k_render_samples"), ("k_shade_rays_mat", "k_shade_rays")):
        found = {n: v for n, v in k.items() if mine + "<" in n}
        assert len(found) == len(LAUNCHABLE), sorted(found)
        for variant in LAUNCHABLE:
            args = template_args(*variant)
            got = [v for n, v in found.items() if mine + args in n]
            ref = [v for n, v in k.items() if twin + args in n]
            assert len(got) == 1 and len(ref) == 1, (args, got, ref)
            print("%s%s: %d scratch instructions, %s: %d" % (mine, args, got[0], twin, ref[0]))
