"""CPU: the host side of the thin-lens frames (rr_render_lens[_device], rr_host_lens_rays, rr_host_lens_pattern,
rr_host_lens_screen_rect) -- the C ABI surface, the lens rays against the model evaluated in float64, the built-in lens offsets,
the lens rectangle against a float64 slab test of the rays it lets the kernel skip, and the code generation of k_render_lens."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from refraction_raytracing_dxr_amd import _capi
from scenes import load
from shading_helpers import view_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rrdxr.h")
RR_ERR_INVALID_ARGUMENT = 1
_P = C.c_void_p
_SC, _DP, _LENS = C.POINTER(_capi.SceneConstants), C.POINTER(_capi.DispatchParams), C.POINTER(_capi.Lens)
NEW = {
    "rr_render_lens": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, _P, C.c_uint32, _LENS, _P, _P, _P]),
    "rr_render_lens_device": (C.c_int, [_P, C.c_uint32, C.c_uint32, _SC, _DP, _P, _P, C.c_uint32, _LENS, _P, _P, _P]),
    "rr_host_lens_rays": (C.c_int, [_SC, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, _LENS, C.c_float, C.c_float, _P]),
    "rr_host_lens_pattern": (C.c_int, [C.c_uint32, C.POINTER(C.c_float)]),
    "rr_host_lens_screen_rect": (C.c_int, [C.POINTER(C.c_float), _SC, _LENS, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
}
VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35), (3.7, 0.2)]
W, H = 50, 38


# ------------------------------------------------------------------------------------------------- 1. symbols and struct
def test_lens_symbols_resolve_with_their_signatures():
    lib = C.CDLL(rr.lib_path())
    for name, sig in NEW.items():
        assert hasattr(lib, name), name
        assert _capi.SYMBOLS[name] == sig, name
    assert rr.lib().rr_abi_version() == 3
    assert re.search(r"#define RRDXR_ABI_VERSION 3\b", open(HEADER).read())
    assert C.sizeof(_capi.Lens) == 8 and _capi.Lens.radius.offset == 0 and _capi.Lens.focus_distance.offset == 4
    lens = rr.Lens(0.25, 4.0)
    assert (lens.radius, lens.focus_distance) == (0.25, 4.0)
    assert callable(rr.Renderer.render_lens) and callable(rr.lens_pattern) and callable(rr.lens_rays) and callable(rr.lens_screen_rect)


def test_lens_entry_points_compile_as_c99(tmp_path):
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n'
                   '#include "rrdxr.h"\n'
                   '_Static_assert(RRDXR_ABI_VERSION == 3, "abi");\n'
                   '_Static_assert(sizeof(rr_lens) == 8 && offsetof(rr_lens, radius) == 0 && offsetof(rr_lens, focus_distance) == 4, "lens");\n'
                   'int f(rr_context* c, const rr_scene_constants* k, const rr_dispatch_params* p, const float* o, const float* lo, const rr_lens* l,\n'
                   '      float* f32, uint8_t* u8, uint32_t* n, void* df, void* du, void* dn, float* pat, rr_ray* rays, const float* box, uint32_t* rect) {\n'
                   '    int (*a)(uint32_t, float*) = rr_host_lens_pattern;\n'
                   '    int (*b)(const rr_scene_constants*, uint32_t, uint32_t, float, float, float, float, const rr_lens*, float, float, rr_ray*) =\n'
                   '        rr_host_lens_rays;\n'
                   '    int (*d)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, const float*,\n'
                   '             uint32_t, const rr_lens*, float*, uint8_t*, uint32_t*) = rr_render_lens;\n'
                   '    int (*e)(rr_context*, uint32_t, uint32_t, const rr_scene_constants*, const rr_dispatch_params*, const float*, const float*,\n'
                   '             uint32_t, const rr_lens*, void*, void*, void*) = rr_render_lens_device;\n'
                   '    int (*g)(const float*, const rr_scene_constants*, const rr_lens*, uint32_t, uint32_t, uint32_t*) = rr_host_lens_screen_rect;\n'
                   '    return a(4, pat) | b(k, 8, 8, 0.5f, 0.5f, 0.0f, 0.0f, l, 1e-4f, 100.0f, rays) | d(c, 8, 8, k, p, o, lo, 4, l, f32, u8, n) |\n'
                   '           e(c, 8, 8, k, p, o, lo, 4, l, df, du, dn) | g(box, k, l, 8, 8, rect);\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "l.o")], check=True)


def test_lens_entry_points_reject_a_null_context():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    f = (C.c_float * 4)()
    lens = rr.Lens(0.1, 5.0)
    assert L.rr_render_lens(None, 1, 1, C.byref(sc), None, None, None, 1, C.byref(lens), f, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lens_device(None, 1, 1, C.byref(sc), None, None, None, 1, C.byref(lens), f, None, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 2. radius 0
@pytest.mark.parametrize("angle,fov", VIEWS)
def test_radius_zero_is_the_pinhole(angle, fov):
    sc, _, _ = view_constants(angle, fov, W, H)
    for focus in (0.5, 5.0, 40.0):
        lens = rr.Lens(0.0, focus)
        for ox, oy, lx, ly in ((0.5, 0.5, 0.0, 0.0), (0.125, 0.875, 1.0, -1.0), (0.0, 1.0, -0.3, 0.7), (0.9375, 0.0625, 0.5, 0.5)):
            assert rr.lens_rays(sc, W, H, ox, oy, lx, ly, lens).tobytes() == rr.camera_rays(sc, W, H, ox, oy).tobytes()
        assert rr.lens_rays(sc, W, H, 0.25, 0.75, 0.1, 0.2, lens, tmin=0.25, tmax=7.0).tobytes() == \
            rr.camera_rays(sc, W, H, 0.25, 0.75, tmin=0.25, tmax=7.0).tobytes()


# ------------------------------------------------------------------------------------------------- 3. focus
def model64(sc, lens, w, h, ox, oy):
    """the lens model in float64 from the float32 constants: O, A, B, s and the focal-plane point O + s * R of every pixel [h, w, 3]"""
    M = np.array(sc.proj_inv, np.float64)
    cam = np.array(sc.camera_loc, np.float64)[:3]
    u, v, c = M[[0, 4, 8]], M[[1, 5, 9]], M[[3, 7, 11]]
    A, B = lens.radius * u / np.linalg.norm(u), lens.radius * v / np.linalg.norm(v)
    s = lens.focus_distance / np.linalg.norm(c)
    sx = (np.arange(w) + float(ox)) / w * 2.0 - 1.0
    sy = -((np.arange(h) + float(oy)) / h * 2.0 - 1.0)
    R = sx[None, :, None] * u + sy[:, None, None] * v + c
    return cam, A, B, s, cam + s * R


@pytest.mark.parametrize("angle,fov", VIEWS)
@pytest.mark.parametrize("radius,focus", [(0.05, 3.5), (0.4, 5.0), (1.5, 9.0)])
def test_lens_rays_start_on_the_disk_and_meet_in_the_focal_plane(angle, fov, radius, focus):
    """Every origin lies on the lens disk -- within radius * (1 + 1e-6) of camera_loc and in the plane of A and B, to 1e-6 *
    (|camera_loc| + radius): a coordinate of O + off carries half an ulp of the sum and off's own four roundings, under 2^-22 of
    either -- and every ray passes within 1e-5 * focus_distance of its pixel's focal-plane point: the chain off, s * R, T, normalize
    is about eight roundings of 2^-24, 5e-7 relative, and the bound is 20 times that."""
    sc, _, _ = view_constants(angle, fov, W, H)
    lens = rr.Lens(radius, focus)
    S = 16
    worst_disk = worst_plane = worst_focus = 0.0
    origins = set()
    for (ox, oy), (lx, ly) in zip(rr.sample_pattern(S), rr.lens_pattern(S)):
        rays = rr.lens_rays(sc, W, H, float(ox), float(oy), float(lx), float(ly), lens)
        cam, A, B, s, F = model64(sc, lens, W, H, ox, oy)
        o = rays["origin"].astype(np.float64)
        d = rays["dir"].astype(np.float64)
        assert np.all(o == o[0])                                    # one lens point per sample
        origins.add(o[0].tobytes())
        n = np.cross(A, B)
        n /= np.linalg.norm(n)
        worst_disk = max(worst_disk, float(np.linalg.norm(o[0] - cam)) / radius)
        worst_plane = max(worst_plane, abs(float(np.dot(o[0] - cam, n))) / (np.linalg.norm(cam) + radius))
        want = cam + float(lx) * A + float(ly) * B
        assert np.linalg.norm(o[0] - want) <= 1e-6 * (np.linalg.norm(cam) + radius)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        to_f = F.reshape(-1, 3) - o
        miss = np.linalg.norm(to_f - np.sum(to_f * d, axis=1, keepdims=True) * d, axis=1)
        assert np.all(np.sum(to_f * d, axis=1) > 0)                 # the focal point lies ahead of the lens
        worst_focus = max(worst_focus, float(miss.max()) / focus)
        assert np.all(np.abs(np.linalg.norm(rays["dir"].astype(np.float64), axis=1) - 1.0) < 1e-6)
        assert np.all(rays["tmin"] == np.float32(1e-4)) and np.all(rays["tmax"] == np.float32(100.0))
        assert np.all(rays["flags"] == 0) and np.all(rays["instance_mask"] == 0xff) and np.all(rays["pad"] == 0)
    print("origin at %.9f radii, %.3g off the lens plane, rays pass %.3g focus distances from their focal point" % (worst_disk, worst_plane, worst_focus))
    assert len(origins) == S
    assert worst_disk <= 1.0 + 1e-6
    assert worst_plane <= 1e-6
    assert worst_focus <= 1e-5


def test_lens_rays_refuse_bad_arguments():
    L = rr.lib()
    sc = rr.camera_orbit(0.01)
    rays = np.zeros(64, rr.RAY_DTYPE)
    p = rays.ctypes.data
    ok = rr.Lens(0.2, 5.0)

    def call(lens=ok, ox=0.5, oy=0.5, lx=0.0, ly=0.0, c=sc, w=8, h=8, out=p):
        return L.rr_host_lens_rays(C.byref(c) if c is not None else None, w, h, ox, oy, lx, ly, C.byref(lens) if lens is not None else None,
                                   1e-4, 100.0, out)
    assert call() == 0 and call(lx=1.0, ly=-1.0) == 0 and call(ox=0.0, oy=1.0) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lx=1.5), dict(ly=-1.5), dict(lx=nan), dict(ly=nan), dict(lx=inf), dict(ox=-0.1), dict(oy=1.5), dict(ox=nan), dict(lens=None),
               dict(c=None), dict(out=None), dict(w=0), dict(h=0), dict(w=32769)):
        assert call(**kw) == RR_ERR_INVALID_ARGUMENT, kw
    for radius, focus in ((-0.1, 5.0), (nan, 5.0), (inf, 5.0), (0.2, 0.0), (0.2, -1.0), (0.2, nan), (0.2, inf), (0.0, 0.0), (0.0, nan)):
        assert call(lens=rr.Lens(radius, focus)) == RR_ERR_INVALID_ARGUMENT, (radius, focus)
    # a column of proj_inv without a direction: the centre column always, an axis column only when the aperture is open
    for col, with_pinhole in ((3, True), (0, False), (1, False)):
        bad = rr.scene_constants(np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32))
        for row in range(3):
            bad.proj_inv[4 * row + col] = 0.0
        assert call(c=bad) == RR_ERR_INVALID_ARGUMENT, col
        assert call(c=bad, lens=rr.Lens(0.0, 5.0)) == (RR_ERR_INVALID_ARGUMENT if with_pinhole else 0), col
    with pytest.raises(rr.RRError):
        rr.lens_rays(sc, 8, 8, 0.5, 0.5, 2.0, 0.0, ok)


# ------------------------------------------------------------------------------------------------- 4. the built-in lens offsets
def test_lens_pattern():
    L = rr.lib()
    for n in range(1, 65):
        a = rr.lens_pattern(n)
        assert a.shape == (n, 2) and a.dtype == np.float32
        assert len({tuple(r) for r in a}) == n
        assert np.all(np.hypot(a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)) <= 1.0)
        assert rr.lens_pattern(n).tobytes() == a.tobytes()
        buf = (C.c_float * (2 * n))()
        assert L.rr_host_lens_pattern(n, buf) == 0 and np.array(buf, np.float32).tobytes() == a.tobytes()
    buf = (C.c_float * 132)()
    for n in (0, 65):
        assert L.rr_host_lens_pattern(n, buf) == RR_ERR_INVALID_ARGUMENT, n
        with pytest.raises(rr.RRError) as e:
            rr.lens_pattern(n)
        assert e.value.status == RR_ERR_INVALID_ARGUMENT
    assert L.rr_host_lens_pattern(4, None) == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 5. the rectangle
RW, RH = 203, 117                                               # not multiples of 8


def hits_box(rays, lo, hi):
    """float64 slab test of the rays' [tmin, tmax] against the closed box"""
    o, d = rays["origin"].astype(np.float64), rays["dir"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.fmin(t0, t1), np.fmax(t0, t1)
    flat = d == 0.0                                             # parallel to a slab: inside it for every t, or never
    inside = (o >= lo) & (o <= hi)
    near = np.where(flat, np.where(inside, -np.inf, np.inf), near)
    far = np.where(flat, np.where(inside, np.inf, -np.inf), far)
    enter = np.maximum(near.max(axis=1), rays["tmin"].astype(np.float64))
    leave = np.minimum(far.min(axis=1), rays["tmax"].astype(np.float64))
    return enter <= leave


def outside_blocks(rect, w, h):
    """[h, w] bool: the pixels of the 8x8 blocks that do not touch rect -- k_render_lens' may_hit, negated"""
    x0 = (np.arange(w) // 8) * 8
    y0 = (np.arange(h) // 8) * 8
    in_x = (x0 + 8 > rect[0]) & (x0 < rect[2])
    in_y = (y0 + 8 > rect[1]) & (y0 < rect[3])
    return ~(in_y[:, None] & in_x[None, :])


def test_no_ray_outside_the_lens_rectangle_meets_the_box():
    """monkey.obj from the three orbit views and the wide one from behind, lens radii of 0.05, 0.3 and 1.0 box diagonals, focused before, at and behind the mesh: of the
    blocks render_lens does not trace, no host lens ray meets the mesh's box -- for the four corners of the pixel, each with the four
    corners of the square round the lens and with 32 seeded points of the disk"""
    v, i = load("monkey.obj")
    P = v["position"][i]
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    bounds = np.concatenate([lo, hi]).astype(np.float32)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(11)
    ang, rad = rng.uniform(0, 2 * np.pi, 32), np.sqrt(rng.uniform(0, 1, 32))
    lens_points = [(-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0)] + [(float(r * np.cos(a)), float(r * np.sin(a))) for a, r in zip(ang, rad)]
    whole = (0, 0, (RW + 7) // 8 * 8, (RH + 7) // 8 * 8)
    larger = wholes = checked = 0
    for angle, fov in VIEWS + [(2.2, rr.FOV_Y)]:                # (the two narrow views see the box all over the frame: nothing is culled there)
        sc, _, _ = view_constants(angle, fov, RW, RH)
        pin = rr.lens_screen_rect(bounds, sc, rr.Lens(0.0, 5.0), RW, RH)
        r = (C.c_uint32 * 4)()
        assert rr.lib().rr_host_screen_rect(bounds.ctypes.data_as(C.POINTER(C.c_float)), C.byref(sc), 1, RW, RH, r) == 0
        assert pin == tuple(r)                                  # radius 0: the pinhole's rectangle
        for frac in (0.05, 0.3, 1.0):
            for focus in (2.5, 5.0, 8.0):
                lens = rr.Lens(frac * diag, focus)
                rect = rr.lens_screen_rect(bounds, sc, lens, RW, RH)
                assert rect[0] <= pin[0] and rect[1] <= pin[1] and rect[2] >= pin[2] and rect[3] >= pin[3], (rect, pin)
                larger += rect != whole and (rect[2] - rect[0]) * (rect[3] - rect[1]) > (pin[2] - pin[0]) * (pin[3] - pin[1])
                wholes += rect == whole
                out = outside_blocks(rect, RW, RH).reshape(-1)
                if not out.any():
                    continue
                for lx, ly in lens_points:
                    for ox, oy in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
                        rays = rr.lens_rays(sc, RW, RH, ox, oy, lx, ly, lens)[out]
                        bad = hits_box(rays, lo, hi)
                        assert not bad.any(), (angle, fov, frac, focus, lx, ly, ox, oy, rect, int(bad.sum()))
                        checked += len(rays)
    print("%d rays of untraced blocks checked; %d lens rectangles larger than the pinhole's and not the frame, %d the whole frame" % (checked, larger, wholes))
    assert larger >= 1 and wholes >= 1 and checked > 100000
    assert rr.lens_screen_rect(bounds, None, rr.Lens(0.1, 5.0), RW, RH) == whole
    with pytest.raises(rr.RRError) as e:
        rr.lens_screen_rect(bounds, rr.camera_orbit(0.01), rr.Lens(-1.0, 5.0), RW, RH)
    assert e.value.status == RR_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 6. codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_lens_kernels_exist(tmp_path):
    """every k_render_lens<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object, and k_render_samples still has all of
    its own; the scratch_ instructions of both are printed side by side (no assertion on the counts: DESIGN 5.8 records them)"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    mine = {n: v for n, v in k.items() if "k_render_lens<" in n}
    assert len(mine) == len(LAUNCHABLE), sorted(mine)
    for variant in LAUNCHABLE:
        args = template_args(*variant)
        got = [v for n, v in mine.items() if "k_render_lens" + args in n]
        ref = [v for n, v in k.items() if "k_render_samples" + args in n]
        assert len(got) == 1 and len(ref) == 1, (args, got, ref)
        print("k_render_lens%s: %d scratch instructions, k_render_samples: %d" % (args, got[0], ref[0]))
