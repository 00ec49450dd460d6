"""CPU: lit shutter frames -- the C surface of rr_set_light_shapes, rr_host_moved_lights and rr_render_lit[_device], the arithmetic of
the moved lights, the Python helpers, the kernels in the code object, and the conditions the fixtures of test_gpu_lit.py are chosen
for (read from the surfaces reference alone, never masks on a comparison)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lit_helpers as LH
import materials_helpers as MH
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as KH
from builder_models import _fma32
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from composed_helpers import LENS
from nested_helpers import FH, FW
from refraction_raytracing_dxr_amd import _capi
from test_shutter_cpu import _register_counts, bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP, _LENS = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams), C.POINTER(_capi.Lens)
NEW = {
    "rr_set_light_shapes": (C.c_int, [_P, _P, C.c_uint32]),
    "rr_host_moved_lights": (C.c_int, [_P, _P, C.c_uint32, C.c_float, C.c_float, _P]),
    "rr_render_lit": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _LENS, _P, _P, _P]),
    "rr_render_lit_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _LENS, _P, _P, _P]),
}


# ------------------------------------------------------------------------------------------------- 1. the C surface
def test_lit_symbols_resolve_with_their_signatures():
    L = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(L, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3


def test_lit_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(sizeof(rr_light_shape) == 32 && sizeof(rr_lit_sample) == 32 && sizeof(rr_lit_sample) == sizeof(rr_shutter_sample), "size");\n'
                   '_Static_assert(offsetof(rr_light_shape, ex) == 0 && offsetof(rr_light_shape, ey) == 12 && offsetof(rr_light_shape, pad) == 24, "offsets");\n'
                   '_Static_assert(offsetof(rr_lit_sample, offset) == 0 && offsetof(rr_lit_sample, lens_offset) == 8, "offsets");\n'
                   '_Static_assert(offsetof(rr_lit_sample, band) == 16 && offsetof(rr_lit_sample, key) == 20, "offsets");\n'
                   '_Static_assert(offsetof(rr_lit_sample, light_offset) == 24 && offsetof(rr_shutter_sample, pad) == 24, "offsets");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const rr_lit_sample* s, const rr_lens* l,\n'
                   '      const rr_light_shape* sh, const rr_light* in, rr_light* o, float* f32, uint8_t* u8, uint32_t* n, void* df, void* du, void* dn) {\n'
                   '    int (*a)(rr_context*, const rr_light_shape*, uint32_t) = rr_set_light_shapes;\n'
                   '    int (*m)(const rr_light*, const rr_light_shape*, uint32_t, float, float, rr_light*) = rr_host_moved_lights;\n'
                   '    int (*b)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const rr_lit_sample*,\n'
                   '             uint32_t, const rr_lens*, float*, uint8_t*, uint32_t*) = rr_render_lit;\n'
                   '    int (*d)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const rr_lit_sample*,\n'
                   '             uint32_t, const rr_lens*, void*, void*, void*) = rr_render_lit_device;\n'
                   '    return a(c, sh, 1) | m(in, sh, 1, 0.5f, -0.5f, o) | b(c, 8, 8, k, p, s, 4, l, f32, u8, n) | d(c, 8, 8, k, p, s, 4, l, df, du, dn);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_lit_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    rec = np.zeros(1, rr.LIT_SAMPLE_DTYPE)
    shape = np.zeros(1, rr.LIGHT_SHAPE_DTYPE)
    assert L.rr_set_light_shapes(None, shape.ctypes.data, 1) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_set_light_shapes(None, None, 0) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lit(None, 1, 1, C.byref(sc), None, rec.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lit_device(None, 1, 1, C.byref(sc), None, rec.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    # rr_host_moved_lights takes no context; null tables with rows to move are refused, none to move are fine
    one = np.zeros(1, rr.LIGHT_DTYPE)
    assert L.rr_host_moved_lights(None, None, 1, 0.0, 0.0, one.ctypes.data) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_moved_lights(one.ctypes.data, None, 1, 0.0, 0.0, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_moved_lights(None, None, 0, 0.0, 0.0, None) == 0


def test_the_python_surface_and_the_layouts():
    for name in ("set_light_shapes", "render_lit"):
        assert callable(getattr(rr.Renderer, name)), name
    for name in ("light_shape", "moved_lights", "light_pattern", "lit_samples"):
        assert name in rr.__all__ and callable(getattr(rr, name)), name
    d = rr.LIT_SAMPLE_DTYPE
    assert d is _capi.LIT_SAMPLE_DTYPE and d.itemsize == 32
    assert [d.fields[k][1] for k in ("offset", "lens_offset", "band", "key", "light_offset")] == [0, 8, 16, 20, 24]
    assert d.fields["light_offset"][0].shape == (2,) and d.fields["light_offset"][0].base == np.dtype("<f4")
    s = rr.LIGHT_SHAPE_DTYPE
    assert s is _capi.LIGHT_SHAPE_DTYPE and s.itemsize == 32 and [s.fields[k][1] for k in ("ex", "ey", "pad")] == [0, 12, 24]
    row = rr.light_shape((1, 2, 3), (4, 5, 6))
    assert row.dtype == s and list(row["ex"]) == [1, 2, 3] and list(row["ey"]) == [4, 5, 6] and not row["pad"].any()


# ------------------------------------------------------------------------------------------------- 2. rr_host_moved_lights
def test_moved_lights_is_two_fused_multiply_adds_per_component():
    """against the statement of the header with an exact fmaf (builder_models._fma32: the product and sum in exact rational arithmetic,
    rounded once), over values where fusing, not fusing and the order of the two terms all give different bits"""
    rng = np.random.default_rng(5)
    n = 8
    lts = np.zeros(n, rr.LIGHT_DTYPE)
    lts["v"] = (rng.standard_normal((n, 3)) * [1.0, 1e-3, 1e3]).astype(np.float32)
    lts["kind"] = np.arange(n) % 2
    lts["radiance"] = rng.random((n, 3)).astype(np.float32)
    lts["shadow_mask"] = rng.integers(0, 256, n)
    shapes = np.zeros(n, rr.LIGHT_SHAPE_DTYPE)
    shapes["ex"] = rng.standard_normal((n, 3)).astype(np.float32)
    shapes["ey"] = (rng.standard_normal((n, 3)) * 1e-2).astype(np.float32)
    differs_unfused = False
    for lu, lv in ((1.0, -1.0), (0.3, 0.7), (-0.123456, 0.987654), (0.0, 0.0)):
        lu, lv = np.float32(lu), np.float32(lv)
        got = rr.moved_lights(lts, shapes, lu, lv)
        for f in ("kind", "radiance", "shadow_mask"):
            assert got[f].tobytes() == lts[f].tobytes()
        want = np.array([[_fma32(lv, shapes["ey"][i, c], _fma32(lu, shapes["ex"][i, c], lts["v"][i, c])) for c in range(3)] for i in range(n)], np.float32)
        assert bits_equal(got["v"], want), (lu, lv)
        unfused = (lv * shapes["ey"] + (lu * shapes["ex"] + lts["v"])).astype(np.float32)
        differs_unfused |= not bits_equal(unfused, want)
    assert differs_unfused                                      # (the values can tell an fmaf from a product and a sum)


def test_moved_lights_without_shapes_is_the_identity():
    lts = np.zeros(3, rr.LIGHT_DTYPE)
    lts["v"] = [(-0.0, 1.0, -0.0), (0.0, -0.0, 2.5), (1e-40, -1e-40, 3e38)]
    lts["kind"] = [0, 1, 1]
    lts["radiance"] = [(1, 2, 3), (-1, 0, -0.0), (4, 5, 6)]
    lts["shadow_mask"] = [1, 0xff, 0]
    assert rr.moved_lights(lts, None, 0.75, -1.0).tobytes() == lts.tobytes()
    assert len(rr.moved_lights(np.zeros(0, rr.LIGHT_DTYPE), None, 0.0, 0.0)) == 0
    # a table of zeros is NOT the identity on a -0: fmaf(lu, +0, -0) is +0.  The values are equal, the bits are stated by the fmaf
    zero = np.zeros(3, rr.LIGHT_SHAPE_DTYPE)
    moved = rr.moved_lights(lts, zero, 0.5, 0.5)
    assert np.array_equal(moved["v"], lts["v"]) and not np.signbit(moved["v"][0, 0])
    with pytest.raises(ValueError):
        rr.moved_lights(lts, zero[:2], 0.0, 0.0)


# ------------------------------------------------------------------------------------------------- 3. rr.lit_samples, rr.light_pattern
def test_lit_samples_ordering():
    """sample (a * K + j) * B + b is position a, key j, band b, with the light offset of position a: against a table written by hand"""
    pos = np.array([[0.25, 0.5], [0.75, 0.125]], np.float32)
    lo = np.array([[-1.0, 0.5], [0.25, 1.0]], np.float32)
    rec = rr.lit_samples(pos, 3, 2, None, lo)
    assert rec.dtype == rr.LIT_SAMPLE_DTYPE and len(rec) == 12
    want = [  # position, key, band
        (0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1),
        (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)]
    for k, (a, j, b) in enumerate(want):
        assert tuple(rec["offset"][k]) == tuple(pos[a]) and rec["key"][k] == j and rec["band"][k] == b and tuple(rec["light_offset"][k]) == tuple(lo[a]), k
    assert bits_equal(rec["lens_offset"], rr.lens_pattern(12))
    src = rr.shutter_samples(pos, 3, 2)
    assert all(rec[f].tobytes() == src[f].tobytes() for f in ("offset", "lens_offset", "band", "key"))
    # the default light offsets are light_pattern of the positions; sequences of keys and explicit lens offsets pass through
    rec = rr.lit_samples(4, [5, 2])
    assert bits_equal(rec["light_offset"], np.repeat(rr.light_pattern(4), 2, axis=0)) and list(rec["key"]) == [5, 2] * 4
    loff = np.linspace(-1, 1, 8, dtype=np.float32).reshape(4, 2)
    assert bits_equal(rr.lit_samples(pos, 2, None, loff, lo)["lens_offset"], loff)
    for bad in (lambda: rr.lit_samples(pos, 2, None, None, lo[:1]), lambda: rr.lit_samples(pos, 2, None, None, np.zeros((2, 3), np.float32)),
                lambda: rr.lit_samples(4, 4, 5), lambda: rr.lit_samples(pos, 0), lambda: rr.lit_samples(pos, 2, None, loff[:3])):
        with pytest.raises(ValueError):
            bad()


def test_light_pattern_is_deterministic_and_inside_the_square():
    assert bits_equal(rr.light_pattern(1), np.zeros((1, 2), np.float32))
    assert bits_equal(rr.light_pattern(4), np.array([[-0.75, -0.75], [-0.25, 0.25], [0.25, -0.25], [0.75, 0.75]], np.float32))
    for n in (1, 2, 3, 4, 7, 8, 16, 64):
        p = rr.light_pattern(n)
        assert p.dtype == np.float32 and p.shape == (n, 2) and (np.abs(p) < 1.0).all() and bits_equal(p, rr.light_pattern(n))
        assert len({tuple(r) for r in p}) == n                  # n distinct points
        assert abs(float(p.astype(np.float64).mean(axis=0)[0])) < 1e-6      # the first coordinate is centred
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            rr.light_pattern(bad)


def test_what_render_lit_refuses_before_the_library():
    """the argument checks of the Python layer, which need no device: the renderer is never touched"""
    class Untouched(rr.Renderer):
        def __init__(self):                                     # no context: any call into the library would fail on _h
            self.device = 0
    r = Untouched()
    cam = rr.camera_orbit(0.01)
    rec = rr.lit_samples(2, 1)
    for bad in (lambda: r.render_lit(8, 8, cam, 2), lambda: r.render_lit(-1, 8, cam, 2, keys=1), lambda: r.render_lit(8, 8, cam, rec, keys=1),
                lambda: r.render_lit(8, 8, cam, rec, light_samples=np.zeros((2, 2))), lambda: r.render_lit(8, 8, cam, 16, keys=3, bands=2),
                lambda: r.render_lit(8, 8, cam, 2, keys=1, light_samples=np.zeros((3, 2))), lambda: r.render_lit(8, 8, cam, 2, keys=[0], paired=True),
                lambda: r.render_lit(8, 8, cam, 2, keys=[0, 0], light_samples=np.zeros((1, 2)), paired=True), lambda: r.render_lit(8, 8, cam, 2, keys=0)):
        with pytest.raises(ValueError):
            bad()
    r._h = None                                                 # (so that __del__ has nothing to close)


# ------------------------------------------------------------------------------------------------- 4. codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_lit_kernels_exist(tmp_path):
    """every k_render_lit<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object exactly once; its lane moves, scratch
    instructions and register counts are printed next to those of k_render_shutter and k_render_surfaces with the same tree (no
    assertion on the counts: DESIGN 5.15 records them)"""
    k = kernels(tmp_path)
    regs = _register_counts(tmp_path / "co")
    found = {n: v for n, v in k.items() if "k_render_lit<" in n}
    assert len(found) == len(LAUNCHABLE), sorted(found)
    for variant in LAUNCHABLE:
        args = template_args(*variant)
        rows = []
        for name in ("k_render_lit", "k_render_shutter", "k_render_surfaces"):
            got = [(n, v) for n, v in k.items() if name + args in n]
            assert len(got) == 1, (name, args, got)
            r = [c for m, c in regs.items() if name + args in m]
            rows.append("%s%s: %d lane moves, %d scratch instructions%s" % (name, args, got[0][1]["lane"], got[0][1]["scratch"],
                        ", %d SGPRs, %d VGPRs, %d bytes of scratch per lane" % r[0] if r else ""))
        print("\n".join(rows))


# ------------------------------------------------------------------------------------------------- 5. the fixtures are what they are for
def test_the_soft_shadow_fixture_has_a_penumbra():
    """a condition on the fixture, read from the reference alone: under the four corners of the lamp the floor has pixels that are
    occluded -- colour exactly 0 after exactly two rays, the floor hit and a blocked shadow ray -- under every offset (the umbra) and
    pixels occluded under some offsets but not all (the penumbra).  A kernel that ignores the offsets cannot match the GPU frame test"""
    fx, cam, recs, (rgb, cnt, cols, extras) = LH.soft_ref(2)
    assert len(fx.lights) == 1 and fx.lights["kind"][0] == rr.LIGHT_POINT and fx.lights["shadow_mask"][0] == 0xff and fx.ambient is None
    assert bits_equal(recs["light_offset"], LH.SOFT_OFFSETS) and bits_equal(recs["offset"], np.full((4, 2), 0.5, np.float32))
    occ = np.stack([LH.occluded(e) for e in extras])
    counts = [int(o.sum()) for o in occ]
    umbra, penumbra = int(occ.all(axis=0).sum()), int((occ.any(axis=0) & ~occ.all(axis=0)).sum())
    print("occluded pixels per offset %s, under all four %d, under some but not all %d" % (counts, umbra, penumbra))
    assert penumbra >= 15 and umbra >= 5
    assert all(cols[a].tobytes() != cols[b].tobytes() for a in range(4) for b in range(a + 1, 4))         # the four samples differ


def test_the_moving_olive_meets_its_conditions():
    """the three keys of the moving tumbler with the innermost cube opaque: in every key opaque hits under a list of two media, and
    shadow rays both lit and occluded; the two light offsets change the frame"""
    fx, scs = LH.moving_olive()
    cam = MH.view(*KH.VIEW, FW, FH)
    recs = LH.olive_records()
    _, cnt, cols, extras = fx.lit(cam, FW, FH, recs, LENS, scenes=scs, max_reflect=2, **LH.KW)
    assert sorted(int(r["key"]) for r in recs) == [0, 0, 1, 1, 2, 2]
    for rec, (_, _, tl) in zip(recs, extras):
        assert tl.opaque_in_media[2] > 0 and tl.shadow_lit > 0 and tl.shadow_occluded > 0, (int(rec["key"]), tl)
    assert (cnt > len(recs)).mean() > 0.05
    by_key = {}
    for k, rec in enumerate(recs):
        by_key.setdefault(int(rec["key"]), []).append(k)
    assert all(len(v) == 2 and not bits_equal(recs["light_offset"][v[0]], recs["light_offset"][v[1]]) for v in by_key.values())
