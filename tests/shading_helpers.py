"""The ray-tree and supersampling references (radiance queries, supersampled and adaptive frames: test_gpu_shade.py,
test_gpu_samples.py, test_gpu_adaptive.py, test_adaptive_cpu.py, test_samples_abi.py, and the use test_gpu_indexed.py,
test_gpu_stack_rungs.py and test_gpu_capacity_edges.py make of them): views, camera rays, shade_rays against the oracle, two scenes
of test_gpu_parity.py, the resolve and refinement rules and the small frame the sample tests render.  Meshes and scenes on both
sides come from scenes.py; module-scoped fixtures stay in the test modules."""
import ctypes as C

import numpy as np

import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from refraction_raytracing_dxr_amd import _capi
from scenes import load, oracle_scene, xf

F = np.float32
# the frame of the sample tests: small, since the oracle renders it 4 times as large per axis
W, H = 52, 37
LIMITS = [(5, 2, 1.2), (0, 0, 1.2), (8, 3, 1.2), (11, 3, 1.5)]          # max_reflect = 3: the PEND = 8 builds
SUB4 = [(1, 0), (3, 1), (0, 2), (2, 3)]                                  # the built-in 4x pattern as sub-pixels of a 4x4 cell
CELL16 = [(i, j) for j in range(4) for i in range(4)]                    # the whole cell, row-major
ENV = dict(w=128, h=64, seed=3)
# the 16 sub-pixels of a 4x4 cell, the built-in 4x pattern first: a pattern whose prefix of 4 is a pattern of its own
PERM16 = list(SUB4) + [c for c in CELL16 if c not in SUB4]
OFFP16 = np.array([[(2 * i + 1) / 8.0, (2 * j + 1) / 8.0] for i, j in PERM16], np.float32)
# The views and the threshold of the adaptive GPU test (test_gpu_adaptive.py).  The threshold is a tenth of a channel's displayed range: the oracle's frames
# (test_adaptive_cpu.py) then have both classes and both causes well above the floors the tests assert (the figures are printed).
ADAPTIVE_VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35)]
THRESHOLD = 0.1
STAT_FIELDS = ("rays", "primary", "secondary", "hits", "misses", "terminal_hits", "tir", "node_visits", "tri_tests", "pixels",
               "stats_valid", "traversal_overflow", "bvh_depth", "render_kernel", "node_trips", "leaf_trips", "shade_passes", "waves",
               "background_waves", "render_kernel_name")


def env_map():
    return procedural_env(ENV["w"], ENV["h"], seed=ENV["seed"])


def view_constants(angle, fov, w=W, h=H):
    sc = rr.camera_orbit(angle, fov_y=float(np.float32(fov)), aspect=float(np.float32(w / h)))
    return sc, np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)


def camera_rays(M, cam, w, h, tmin=1e-4, tmax=100.0):
    """rro_generate_camera_ray of every pixel, row-major, as ray records with the primary interval"""
    o = np.zeros((h * w, 3), np.float32)
    d = np.zeros((h * w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            o[y * w + x], d[y * w + x] = O.camera_ray(M, cam, x, y, w, h)
    return rr.pack_rays(o, d, np.float32(tmin), np.float32(tmax))


def check_against_oracle(gpu, s, M, cam, w, h, rays, **kw):
    """shade_rays(rays) == rro_render of the camera the rays came from: float bits, RGBA8 with and without Reinhard, counts"""
    ref = s.render(M, cam, w, h, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, **kw), want_rays=True)
    ref_tm = s.render(M, cam, w, h, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, tonemap=1, **kw))
    f32, u8, cnt = gpu.shade_rays(rays, rr.default_params(**kw), rgba8=True, ray_counts=True)
    assert np.all(f32[:, 3] == 1.0) and np.all(u8[:, 3] == 255)
    assert np.array_equal(f32[:, :3].view(np.uint32).reshape(h, w, 3), ref["rgb"].view(np.uint32))
    assert np.array_equal(u8.reshape(h, w, 4), ref["rgba8"])
    assert np.array_equal(cnt.reshape(h, w), ref["rays"].astype(np.uint32))
    f32_tm, u8_tm = gpu.shade_rays(rays, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), rgba8=True)
    assert f32_tm.tobytes() == f32.tobytes()                    # the float colour is not tone-mapped
    assert np.array_equal(u8_tm.reshape(h, w, 4), ref_tm["rgba8"])
    return ref


def instanced_scene():
    """the scene of test_gpu_parity.py::test_instanced_scene_parity (rotated, non-uniformly scaled instances, TRIANGLE_CULL_DISABLE, a
    zero-mask instance) plus a mirrored instance with TRIANGLE_FRONT_COUNTERCLOCKWISE -> (meshes, env map, instances)"""
    inst = rr.make_instances(
        transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4), xf(0.3, 0.2, 2.4, (0.7, 0.7, 0.7), -1.0),
                    xf(0, 1.9, 0, (0.4, 0.4, 0.4), 0.2), xf(0, -1.8, 0.5, (0.5, 0.5, 0.5)), xf(-2.2, 0.1, 0.3, (-0.6, 0.6, 0.6), 0.3)],
        meshes=[1, 0, 1, 0, 0, 1], masks=[1, 1, 0xff, 1, 0, 1],
        flags=[0, 0, 0, _capi.INSTANCE_FLAG_CULL_DISABLE, 0, _capi.INSTANCE_FLAG_FRONT_CCW])
    return [load("cube.obj"), load("monkey.obj")], procedural_env(128, 64, seed=7), inst


def config4_scene():
    """the scene of test_gpu_parity.py::test_config4_multi_blas_scene: shell + cube + ott, three BLASes under one TLAS (trees deeper than 30
    levels) -> (meshes, env map, instances)"""
    def t(tx, ty, tz):
        m = np.eye(4, dtype=np.float32)[:3].copy()
        m[:, 3] = (tx, ty, tz)
        return m
    inst = rr.make_instances(transforms=[t(0, 0, 0), t(0, 0, -4.0), t(0, 0, 4.0)], meshes=[0, 1, 2])
    return [load("shell.obj"), load("cube.obj"), load("ott.obj")], procedural_env(256, 128, seed=4), inst


def unorm8(rgb, tonemap):
    """the oracle library's rro_unorm8 of an [..., 3] float32 colour, after c / (1 + c) in float32 if tonemap; alpha 255"""
    f = O.lib().rro_unorm8
    f.restype, f.argtypes = C.c_uint8, [C.c_float]
    c = np.ascontiguousarray(rgb, np.float32)
    if tonemap:
        c = c / (np.float32(1) + c)
        assert c.dtype == np.float32
    vals, inv = np.unique(c.view(np.uint32), return_inverse=True)
    table = np.array([f(float(v)) for v in vals.view(np.float32)], np.uint8)
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = table[inv.reshape(c.shape)]
    return out


def fold(colours):
    """the resolve rule over a list of [..., 3] float32 colours, in np.float32"""
    s = colours[0].astype(np.float32, copy=True)
    for c in colours[1:]:
        s = s + c
    assert s.dtype == np.float32
    return s / np.float32(len(colours))


def display(c, tonemap):
    """step 2: what store_pixel shows of a channel value, in [0, 1] (np.fmax / np.fmin return the operand that is a number)"""
    m = np.fmax(np.asarray(c, F), F(0))
    if tonemap:
        with np.errstate(invalid="ignore"):
            m = m / (F(1) + m)                                  # inf / inf = NaN, which fmin turns into 1
    v = np.fmin(m, F(1))
    assert v.dtype == F
    return v


def adaptive_reference(colours, n_base, threshold, tonemap):
    """colours [S, h, w, 3] float32, sample s of every pixel -> (mask [h, w] bool, resolved [h, w, 3], r_own [h, w], r_nb [h, w])"""
    colours = np.asarray(colours)
    assert colours.dtype == F and colours.ndim == 4 and colours.shape[3] == 3
    S, h, w, _ = colours.shape
    assert 1 <= n_base <= S
    t = F(threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        sum_b = colours[0].copy()                               # 1. the fold starts AT c_0
        for s in range(1, n_base):
            sum_b = sum_b + colours[s]
        v = display(colours[:n_base], tonemap)                  # 3. own contrast
        r_own = (np.fmax.reduce(v, axis=0) - np.fmin.reduce(v, axis=0)).max(axis=-1)
        base = sum_b / F(n_base)
        b = display(base, tonemap)                              # 4. neighbour contrast
        r_nb = np.zeros((h, w), F)
        dx = np.abs(b[:, 1:] - b[:, :-1]).max(axis=-1)
        dy = np.abs(b[1:] - b[:-1]).max(axis=-1)
        r_nb[:, 1:] = np.maximum(r_nb[:, 1:], dx)
        r_nb[:, :-1] = np.maximum(r_nb[:, :-1], dx)
        r_nb[1:] = np.maximum(r_nb[1:], dy)
        r_nb[:-1] = np.maximum(r_nb[:-1], dy)
        mask = (r_own > t) | (r_nb > t)                         # 5.
        full = sum_b
        for s in range(n_base, S):                              # 6. a refined pixel continues the same fold
            full = full + colours[s]
        out = np.where(mask[..., None], full / F(S), base)
    assert out.dtype == F and r_own.dtype == F and r_nb.dtype == F
    return mask, out, r_own, r_nb


_cache = {}


def oracle_colours(angle, fov, **kw):
    """(colours [16, H, W, 3] in PERM16's order, counts [16, H, W]) of monkey.obj from the CPU oracle's 4W x 4H frame"""
    key = (angle, fov, tuple(sorted(kw.items())))
    if key not in _cache:
        if "scene" not in _cache:
            _cache["scene"] = oracle_scene([load("monkey.obj")], env_map())
        _, M, cam = view_constants(angle, fov)
        ref = _cache["scene"].render(M, cam, 4 * W, 4 * H, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, **kw), want_rays=True)
        rgb = ref["rgb"].reshape(H, 4, W, 4, 3).transpose(1, 3, 0, 2, 4)
        cnt = ref["rays"].astype(np.uint32).reshape(H, 4, W, 4).transpose(1, 3, 0, 2)
        _cache[key] = (np.stack([rgb[j, i] for i, j in PERM16]), np.stack([cnt[j, i] for i, j in PERM16]))
    return _cache[key]
