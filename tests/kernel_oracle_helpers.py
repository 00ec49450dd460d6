"""What the tests that force each render kernel in turn share (test_gpu_kernels_oracle.py, test_gpu_indexed.py,
test_gpu_stack_rungs.py, test_gpu_capacity_edges.py): the renderer fixture with its debug switches, the cached oracle frame of a
scenes.Scene, orbit cameras, and a launch checked against the oracle with the kernel that rendered it asserted."""
import collections
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr

FUSED, LDS, PATHS, STREAM = 0, 1, 2, 7
KERNEL_ID = {"fused": FUSED, "lds": LDS, "paths": PATHS, "stream": STREAM}
COUNTERS = ("rays", "hits", "misses", "terminal_hits", "tir")
DEBUG_VARS = ("RR_DEBUG_KERNEL", "RR_DEBUG_SHAPE", "RR_DEBUG_TICKET", "RR_DEBUG_GROUP_TRACE", "RR_DEBUG_STACK", "RR_DEBUG_TLAS32",
              "RR_DEBUG_TILE_ORDER", "RR_DEBUG_ASYNC", "RR_DEBUG_DIAG")
TALLY = collections.Counter()           # oracle comparisons per asserted render_kernel, over the module (printed by each test)


@pytest.fixture
def make_renderer(monkeypatch):
    """make(kernel, **env) -> a Renderer created with RR_DEBUG_KERNEL=kernel (and the given RR_DEBUG_* switches), closed at
    teardown"""
    made = []

    def make(kernel, **env):
        for k in DEBUG_VARS:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("RR_DEBUG_KERNEL", kernel)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        r = rr.Renderer(0)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


_ORACLE_CACHE = {}


def oracle_frame(scene, sc, W, H, kw, tonemap=0, region=None):
    """the oracle's path-weight render of one slice, cached across kernels (same scene, constants, size and parameters)"""
    M, cam = np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)
    key = (scene.key, M.tobytes(), cam.tobytes(), W, H, tuple(sorted(kw.items())), tonemap, region)
    if key not in _ORACLE_CACHE:
        if len(_ORACLE_CACHE) > 400:
            _ORACLE_CACHE.clear()
        _ORACLE_CACHE[key] = scene.oracle().render(M, cam, W, H, O.default_params(use_bvh=1, accum_mode=1, tonemap=tonemap, **kw),
                                                   region=region)
    return _ORACLE_CACHE[key]


def orbit(angle, n, step=0.13, radius=1.0, height=None):
    """n distinct orbit constants starting at `angle` (a batch's slices each get their own camera)"""
    out = []
    for f in range(n):
        sc = rr.camera_orbit(angle + step * f)
        sc.camera_loc[0] *= radius
        sc.camera_loc[2] *= radius
        if height is not None:
            sc.camera_loc[1] = height
        out.append(sc)
    return out


def _lds_shape_fits(node_bytes, stack_entries, min_shape):
    """rr_render_lds.hip lds_kernel_shape: 12x2, 16x2, 16x1 waves x workgroups per CU within 160 KiB of LDS per CU"""
    for nw, wgs in ((12, 2), (16, 2), (16, 1))[min_shape:]:
        if node_bytes + nw * stack_entries * 64 * 2 <= 160 * 1024 // wgs - 512:
            return True
        if min_shape <= 0:
            return False
    return False


def screen_rect(scene, cams, W, H):
    arr = (rr._capi.SceneConstants * len(cams))(*cams)
    rect = (C.c_uint32 * 4)()
    assert rr.lib().rr_host_screen_rect(scene.bounds, arr, len(cams), W, H, rect) == 0
    return list(rect)


def expected_kernel(kernel, scene, W, H, cams, kw, need, flags=0, shape=0, sharded=False):
    """the kernel the forced switch must have rendered the launch with (rr_choice.cpp pick_kernel)"""
    depth = len(cams)
    refl = kw.get("max_reflect", 2)
    if kernel == "lds":
        n = scene.n_tris()
        n_tiles = ((W + 31) // 32) * ((H + 31) // 32)
        ok = (scene.single and n < 32768 and _lds_shape_fits(max(n - 1, 1) * 32, need + 1, shape) and n_tiles * depth * depth < 1 << 30
              and not sharded)
        return LDS if ok else FUSED
    if kernel == "paths":
        r = [0, 0, W, H] if flags & rr.DISPATCH_DEBUG_NO_CULL else screen_rect(scene, cams, W, H)
        ok = not sharded and refl <= 2 and need <= 39 and r[2] > r[0] and r[3] > r[1] and depth <= 2
        return PATHS if ok else FUSED
    if kernel == "stream":
        ok = not scene.single and refl <= 2 and kw.get("max_refract", 5) <= 62 and need <= 39
        return STREAM if ok else FUSED
    return FUSED


def dispatch(r, W, H, cams, kw, flags):
    p = rr.default_params(flags=flags | rr.DISPATCH_COLLECT_STATS, **kw)
    if len(cams) == 1:
        r.set_camera(cams[0])
        r.dispatch_rays(W, H, p)
    else:
        r.dispatch_rays_batch(W, H, cams, p)
    want_f = bool(flags & rr.DISPATCH_FLOAT_OUTPUT)
    frames = []
    for f in range(len(cams)):
        got = r.read_frame(want_float=want_f, slice=f)
        frames.append(got if want_f else (got, None))
    st = r.stats()
    assert st.traversal_overflow == 0 and st.stats_valid
    return frames, st


def counters(st):
    return tuple(int(getattr(st, k)) for k in COUNTERS)


def check_slice(rgba, f32, ref, tag):
    assert np.all(rgba[..., 3] == 255), tag
    if f32 is not None:
        assert np.all(f32[..., 3] == 1.0), tag
        d = np.argwhere(f32[..., :3].view(np.uint32) != ref["rgb"].view(np.uint32))
        assert len(d) == 0, "%s: %d float channels differ, first at %s: %r / %r" % (tag, len(d), d[0], f32[tuple(d[0])], ref["rgb"][tuple(d[0])])
    d = np.argwhere(rgba != ref["rgba8"])
    assert len(d) == 0, "%s: %d RGBA8 bytes differ, first at %s: %r / %r" % (tag, len(d), d[0], rgba[tuple(d[0])], ref["rgba8"][tuple(d[0])])


def check_launch(r, kernel, scene, W, H, cams, kw, flags, tally, shape=0, oracle_slices=None, tag=""):
    """One launch of len(cams) slices on the forced kernel, asserted to have rendered it, against the oracle:
    depth 1 -- the frame and the counters; depth > 1 -- every slice and the counter sum against single dispatches of the same
    kernel, the oracle on oracle_slices (default: first, middle, last) with those singles' counters."""
    depth = len(cams)
    tm = 1 if flags & rr.DISPATCH_TONEMAP_REINHARD else 0
    frames, st = dispatch(r, W, H, cams, kw, flags)
    want = expected_kernel(kernel, scene, W, H, cams, kw, st.bvh_depth, flags, shape)
    assert st.render_kernel == want, "%s: rendered by kernel %d, expected %d" % (tag, st.render_kernel, want)
    if depth == 1:
        ref = oracle_frame(scene, cams[0], W, H, kw, tm)
        check_slice(frames[0][0], frames[0][1], ref, tag)
        assert counters(st) == counters(ref["stats"]), (tag, counters(st), counters(ref["stats"]))
        tally[st.render_kernel] += 1
        return st.render_kernel
    if oracle_slices is None:
        oracle_slices = sorted({0, depth // 2, depth - 1})
    total = np.zeros(len(COUNTERS), np.int64)
    for f in range(depth):
        one, s1 = dispatch(r, W, H, [cams[f]], kw, flags)
        assert s1.render_kernel == expected_kernel(kernel, scene, W, H, [cams[f]], kw, s1.bvh_depth, flags, shape), (tag, f, s1.render_kernel)
        assert np.array_equal(frames[f][0], one[0][0]), "%s: slice %d of the batch != its single dispatch" % (tag, f)
        if frames[f][1] is not None:
            assert np.array_equal(frames[f][1].view(np.uint32), one[0][1].view(np.uint32)), "%s: slice %d (float)" % (tag, f)
        total += counters(s1)
        if f in oracle_slices:
            ref = oracle_frame(scene, cams[f], W, H, kw, tm)
            check_slice(frames[f][0], frames[f][1], ref, "%s slice %d" % (tag, f))
            assert counters(s1) == counters(ref["stats"]), (tag, f, counters(s1), counters(ref["stats"]))
            tally[st.render_kernel] += 1
    assert tuple(total) == counters(st), (tag, tuple(total), counters(st))
    return st.render_kernel


def report(name, tally):
    TALLY.update(tally)
    print("%s: oracle comparisons by render_kernel %s; module so far %s" % (name, dict(tally), dict(TALLY)))
