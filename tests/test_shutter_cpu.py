"""CPU: shutter frames -- the C surface of the scene keys and rr_render_shutter[_device], the Python surface, rr.shutter_samples'
ordering, the kernels in the code object, and the conditions the moving-tumbler fixture of test_gpu_shutter.py is chosen for (read
from the nested reference, never masks on a comparison)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import composed_helpers as CH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as SH
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from nested_helpers import FH, FW, TABLE
from refraction_raytracing_dxr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ERR_INVALID_ARGUMENT = 1
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
_P = C.c_void_p
_SC, _DP, _LENS = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams), C.POINTER(_capi.Lens)
NEW = {
    "rr_capture_scene_key": (C.c_int, [_P, C.c_uint32]),
    "rr_release_scene_key": (C.c_int, [_P, C.c_uint32]),
    "rr_scene_key_info": (C.c_int, [_P, C.c_uint32, C.POINTER(_capi.SceneKeyInfo)]),
    "rr_render_shutter": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _LENS, _P, _P, _P]),
    "rr_render_shutter_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, C.c_uint32, _LENS, _P, _P, _P]),
}


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------- 1. the C surface
def test_shutter_symbols_resolve_with_their_signatures():
    L = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(L, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3


def test_shutter_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(RR_MAX_SCENE_KEYS == 16 && RR_ALL_SCENE_KEYS == 0xffffffffu && RR_MAX_SAMPLES == 64, "limits");\n'
                   '_Static_assert(sizeof(rr_shutter_sample) == 32, "size");\n'
                   '_Static_assert(offsetof(rr_shutter_sample, offset) == 0 && offsetof(rr_shutter_sample, lens_offset) == 8, "offsets");\n'
                   '_Static_assert(offsetof(rr_shutter_sample, band) == 16 && offsetof(rr_shutter_sample, key) == 20, "offsets");\n'
                   '_Static_assert(offsetof(rr_shutter_sample, pad) == 24, "offsets");\n'
                   '_Static_assert(sizeof(struct rr_scene_key_info) == 56 && offsetof(struct rr_scene_key_info, bounds) == 16, "info");\n'
                   '_Static_assert(offsetof(struct rr_scene_key_info, stack_need) == 40 && offsetof(struct rr_scene_key_info, bytes) == 48, "info");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const rr_shutter_sample* s, const rr_lens* l,\n'
                   '      struct rr_scene_key_info* i, float* f32, uint8_t* u8, uint32_t* n, void* df, void* du, void* dn) {\n'
                   '    int (*a)(rr_context*, uint32_t) = rr_capture_scene_key;\n'
                   '    int (*r)(rr_context*, uint32_t) = rr_release_scene_key;\n'
                   '    int (*q)(rr_context*, uint32_t, struct rr_scene_key_info*) = rr_scene_key_info;\n'
                   '    int (*b)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const rr_shutter_sample*,\n'
                   '             uint32_t, const rr_lens*, float*, uint8_t*, uint32_t*) = rr_render_shutter;\n'
                   '    int (*d)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const rr_shutter_sample*,\n'
                   '             uint32_t, const rr_lens*, void*, void*, void*) = rr_render_shutter_device;\n'
                   '    return a(c, 0) | q(c, 0, i) | b(c, 8, 8, k, p, s, 4, l, f32, u8, n) | d(c, 8, 8, k, p, s, 4, l, df, du, dn) |\n'
                   '           r(c, RR_ALL_SCENE_KEYS);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


# ------------------------------------------------------------------------------------------------- 2. null contexts, the Python surface
def test_shutter_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    rec = np.zeros(1, rr.SHUTTER_SAMPLE_DTYPE)
    info = rr.SceneKeyInfo()
    assert L.rr_capture_scene_key(None, 0) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_release_scene_key(None, 0) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_scene_key_info(None, 0, C.byref(info)) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_shutter(None, 1, 1, C.byref(sc), None, rec.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_shutter_device(None, 1, 1, C.byref(sc), None, rec.ctypes.data, 1, None, f, None, None) == RR_ERR_INVALID_ARGUMENT


def test_the_python_surface_and_the_layouts():
    for name in ("capture_scene_key", "release_scene_key", "scene_key_info", "render_shutter"):
        assert callable(getattr(rr.Renderer, name)), name
    assert "shutter_samples" in rr.__all__ and callable(rr.shutter_samples)
    assert rr.MAX_SCENE_KEYS == 16 and _capi.MAX_SCENE_KEYS == 16
    d = rr.SHUTTER_SAMPLE_DTYPE
    assert d is _capi.SHUTTER_SAMPLE_DTYPE and d.itemsize == 32
    assert [d.fields[k][1] for k in ("offset", "lens_offset", "band", "key", "pad")] == [0, 8, 16, 20, 24]
    assert d.fields["pad"][0].shape == (2,)
    i = rr.SceneKeyInfo
    assert C.sizeof(i) == 56
    assert [getattr(i, k).offset for k in ("captured", "top_level", "n_instances", "n_triangles", "bounds", "stack_need", "max_material", "bytes")] == \
        [0, 4, 8, 12, 16, 40, 44, 48]


# ------------------------------------------------------------------------------------------------- 3. rr.shutter_samples
def test_shutter_samples_ordering():
    """sample (a * K + j) * B + b is position a, key j, band b: against a table written out by hand"""
    pos = np.array([[0.25, 0.5], [0.75, 0.125]], np.float32)
    rec = rr.shutter_samples(pos, 3, 2)
    assert rec.dtype == rr.SHUTTER_SAMPLE_DTYPE and len(rec) == 12
    want = [  # position, key, band
        (0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 1),
        (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1)]
    for k, (a, j, b) in enumerate(want):
        assert tuple(rec["offset"][k]) == tuple(pos[a]) and rec["key"][k] == j and rec["band"][k] == b, k
    assert not rec["pad"].any()
    assert bits_equal(rec["lens_offset"], rr.lens_pattern(12))
    # sequences name the keys and bands themselves; no bands: band 0; explicit lens offsets
    loff = np.linspace(-1, 1, 8, dtype=np.float32).reshape(4, 2)
    rec = rr.shutter_samples(pos, [5, 2], None, loff)
    assert list(rec["key"]) == [5, 2, 5, 2] and not rec["band"].any() and bits_equal(rec["lens_offset"], loff)
    assert [tuple(o) for o in rec["offset"]] == [tuple(pos[0])] * 2 + [tuple(pos[1])] * 2
    rec = rr.shutter_samples(pos[:1], [1], [3, 0, 3])
    assert list(rec["band"]) == [3, 0, 3] and list(rec["key"]) == [1, 1, 1]
    assert bits_equal(rr.shutter_samples(4, 2)["offset"], np.repeat(rr.sample_pattern(4), 2, axis=0))
    assert len(rr.shutter_samples(4, 4, 4)) == 64
    for bad in (lambda: rr.shutter_samples(4, 4, 5), lambda: rr.shutter_samples(pos, 0), lambda: rr.shutter_samples(pos, [-1]),
                lambda: rr.shutter_samples(pos, 2, None, loff[:3]), lambda: rr.shutter_samples(np.zeros((2, 3), np.float32), 1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------- 4. codegen
def _register_counts(work):
    """{demangled kernel name: (sgprs, vgprs, private segment bytes)} from the notes of the unbundled gfx950 objects, where the
    toolchain's readelf is there; {} otherwise"""
    out = {}
    if not os.path.exists(READELF):
        return out
    for f in sorted(work.iterdir()):
        if "gfx950" not in f.name:
            continue
        text = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True).stdout
        cur = {}
        for line in text.split("\n"):
            line = line.strip()
            for key in (".name:", ".sgpr_count:", ".vgpr_count:", ".private_segment_fixed_size:"):
                if line.startswith(key) or line.startswith("- " + key):
                    cur[key] = line.split(key, 1)[1].strip().strip("'")
            if len(cur) == 4 and (line.startswith(".wavefront_size") or line.startswith(".vgpr_spill_count")):
                out[cur[".name:"]] = (int(cur[".sgpr_count:"]), int(cur[".vgpr_count:"]), int(cur[".private_segment_fixed_size:"]))
                cur = {}
    demangled = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n") if out else []
    return dict(zip(demangled, out.values()))


@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_shutter_kernels_exist(tmp_path):
    """every k_render_shutter<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object exactly once; its lane moves,
    scratch instructions and register counts are printed next to those of k_render_composed with the same tree (no assertion on the
    counts: DESIGN 5.13 records them)"""
    k = kernels(tmp_path)
    regs = _register_counts(tmp_path / "co")
    found = {n: v for n, v in k.items() if "k_render_shutter<" in n}
    assert len(found) == len(LAUNCHABLE), sorted(found)
    for variant in LAUNCHABLE:
        args = template_args(*variant)
        got = [(n, v) for n, v in found.items() if "k_render_shutter" + args in n]
        ref = [(n, v) for n, v in k.items() if "k_render_composed" + args in n]
        assert len(got) == 1 and len(ref) == 1, (args, got, ref)
        for name, (n, v) in (("k_render_shutter", got[0]), ("k_render_composed", ref[0])):
            r = [c for m, c in regs.items() if name + args in m]
            print("%s%s: %d lane moves, %d scratch instructions%s" % (name, args, v["lane"], v["scratch"],
                  ", %d SGPRs, %d VGPRs, %d bytes of scratch per lane" % r[0] if r else ""))


# ------------------------------------------------------------------------------------------------- 5. the fixture is what it is for
def test_the_moving_tumbler_meets_its_conditions():
    """the frame test_gpu_shutter.py compares bit for bit: keys that differ, deep trees, three media at once in every key, nesting and
    a camera outside in every key, blocks outside the union rectangle, and a block only the union rectangle covers in which key 2 is hit"""
    S = len(SH.KEY_ORDER)
    for ml in (2, 3):
        scs, cam, recs, iors, weights, (rgb, cnt, cols, tallies) = SH.moving_ref(ml)
        assert [int(r["key"]) for r in recs] == SH.KEY_ORDER and [int(r["band"]) for r in recs] == SH.BAND_ORDER
        deep = float((cnt > S).mean())
        print("max_reflect %d: %.1f %% of the pixels have a tree deeper than S rays" % (ml, 100 * deep))
        assert deep > 0.05
        p = rr.default_params(max_reflect=ml, **SH.KW)
        rays = CH.sample_rays(cam, FW, FH, recs[0], CH.LENS, p)
        t0 = CH.band_table(TABLE, iors, 0)
        per_key = [NH.ref_shade(sc, rays, t0, max_reflect=ml, **SH.KW) for sc in scs]
        for a in range(SH.N_KEYS):
            assert per_key[a][3].deepest == 3, (a, per_key[a][3])
            for b in range(a + 1, SH.N_KEYS):
                assert not bits_equal(per_key[a][0], per_key[b][0]), (a, b)
        assert all(t.deepest == 3 for t in tallies)
    scs, cam, recs, iors, weights, _ = SH.moving_ref(2)
    eye = np.array(cam.camera_loc[:3], np.float64)
    for sc in scs:                                              # (moving_tumbler asserted the nesting when it made them)
        NH.assert_inside(sc, 1, 0)
        NH.assert_inside(sc, 2, 1)
        b = np.array(list(sc.bounds), np.float64)
        gap = float(np.linalg.norm(np.maximum(np.maximum(b[:3] - eye, eye - b[3:]), 0.0)))
        assert gap > CH.LENS.radius + NH.MARGIN, (sc.key, gap)  # the whole lens disk is outside the outermost instance's box
    union = rr.lens_screen_rect(SH.union_bounds(scs), cam, CH.LENS, FW, FH)
    own = [rr.lens_screen_rect(sc.bounds, cam, CH.LENS, FW, FH) for sc in scs]
    in_union, in_key0 = SH.blocks_inside(union), SH.blocks_inside(own[0])
    print("rectangles of the keys %s, of the union %s" % (own, union))
    assert (~in_union).sum() >= 64                              # a block outside the union rectangle
    hit2 = np.zeros((FH, FW), bool)
    p = rr.default_params(max_reflect=2, **SH.KW)
    for rec in recs:
        if int(rec["key"]) == 2:
            n = NH.ref_shade(scs[2], CH.sample_rays(cam, FW, FH, rec, CH.LENS, p), CH.band_table(TABLE, iors, int(rec["band"])), max_reflect=2, **SH.KW)[2]
            hit2 |= n.reshape(FH, FW) > 1                       # (a primary ray that hits has children)
    only_union = in_union & ~in_key0
    print("%d pixels in blocks that only the union rectangle covers, %d of them hit key 2" % (int(only_union.sum()), int((only_union & hit2).sum())))
    assert (only_union & hit2).any()
