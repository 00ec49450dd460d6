"""GPU: adaptive supersampling (Renderer.render_adaptive, rr_render_adaptive[_device]) -- n_base samples for every pixel, n_max
where the base samples show contrast.

The reference is test_adaptive_cpu.adaptive_reference, the rule of include/rrdxr.h in numpy (tested on the CPU in that file),
applied to per-sample colours that come from entry points which exist without this feature: 16 shade_rays calls on
rr.camera_rays, and the CPU oracle's frame 4 times as large per axis.  Every pixel of every output is compared, none sampled,
and every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from shading_helpers import ADAPTIVE_VIEWS as VIEWS
from scenes import gpu, gpu_scene, load  # noqa: F401  (gpu: a fixture)
from shading_helpers import (LIMITS, OFFP16, STAT_FIELDS, THRESHOLD, H, W, adaptive_reference, config4_scene, env_map, oracle_colours, unorm8,
                             view_constants)

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE, RR_ERR_UNSUPPORTED = 1, 5, 7
F = np.float32


_scene = {}


def monkey_scene(gpu):
    """monkey.obj under test_gpu_samples' environment map (built once per renderer)"""
    if _scene.get("monkey") is not gpu:
        m = load("monkey.obj")
        gpu.load_scene(*m, env_map())
        _scene.clear()
        _scene["monkey"] = gpu


def sample_colours(gpu, sc, w, h, offsets, p):
    """one shade_rays call per offset on rr.camera_rays -> (colours [S, h, w, 3], counts [S, h, w])"""
    cols, cnts = [], []
    for ox, oy in offsets:
        f, n = gpu.shade_rays(rr.camera_rays(sc, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), p, ray_counts=True)
        cols.append(f[:, :3].reshape(h, w, 3))
        cnts.append(n.reshape(h, w))
    return np.stack(cols), np.stack(cnts)


def follows_the_rule(got, cols, cnts, n_base, threshold, tonemap):
    """got = (f32, u8, n_rays, n_taken, n_refined) of render_adaptive against adaptive_reference of the per-sample colours;
    returns the reference's mask"""
    f32, u8, cnt, taken, n_ref = got
    S = len(cols)
    mask, want, _, _ = adaptive_reference(cols, n_base, threshold, tonemap)
    assert f32.dtype == F and u8.dtype == np.uint8 and cnt.dtype == np.uint32 and taken.dtype == np.uint32
    assert np.array_equal(taken, np.where(mask, S, n_base).astype(np.uint32)), "%d pixels differ in n_taken" % int((taken != np.where(mask, S, n_base)).sum())
    assert np.all(f32[..., 3] == 1.0)
    mism = int((f32[..., :3].view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    assert mism == 0, "%d pixels differ in their float bits" % mism
    assert np.array_equal(u8, unorm8(want, tonemap))
    want_n = np.where(mask, cnts.sum(axis=0), cnts[:n_base].sum(axis=0)).astype(np.uint32)
    assert np.array_equal(cnt, want_n)
    assert n_ref == int(mask.sum())
    return mask


# ------------------------------------------------------------------------------------------------- 1. every pixel, two references
@pytest.mark.parametrize("tonemap", [False, True])
@pytest.mark.parametrize("limits", [LIMITS[0], LIMITS[2]])
def test_every_pixel_follows_the_rule(gpu, limits, tonemap):
    assert limits[1] == (3 if limits is LIMITS[2] else 2)       # LIMITS[2]: max_reflect = 3, the PEND = 8 builds
    monkey_scene(gpu)
    kw = dict(max_refract=limits[0], max_reflect=limits[1], ior=limits[2])
    p = rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD if tonemap else 0, **kw)
    for angle, fov in VIEWS:
        sc, _, _ = view_constants(angle, fov)
        got = gpu.render_adaptive(W, H, sc, (4, OFFP16), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
        cols, cnts = sample_colours(gpu, sc, W, H, OFFP16, p)
        mask = follows_the_rule(got, cols, cnts, 4, THRESHOLD, tonemap)
        # (from the reference's mask, not from the output: the frame is neither all base nor all refined)
        print("view %s: %d of %d pixels refined" % ((angle, fov), int(mask.sum()), mask.size))
        assert int(mask.sum()) >= 64 and int((~mask).sum()) >= 64
        if not tonemap:
            ocols, ocnts = oracle_colours(angle, fov, **kw)
            omask = follows_the_rule(got, ocols, ocnts, 4, THRESHOLD, False)
            assert np.array_equal(omask, mask)


# ------------------------------------------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("tonemap", [False, True])
def test_each_pixel_is_a_pixel_of_a_supersampled_frame(gpu, tonemap):
    monkey_scene(gpu)
    p = rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD if tonemap else 0, max_refract=8, max_reflect=3)
    sc, _, _ = view_constants(*VIEWS[1])
    f32, u8, cnt, taken, n_ref = gpu.render_adaptive(W, H, sc, (4, OFFP16), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    lo = gpu.render_samples(W, H, sc, OFFP16[:4], p, rgba8=True, ray_counts=True)
    hi = gpu.render_samples(W, H, sc, OFFP16, p, rgba8=True, ray_counts=True)
    assert set(np.unique(taken).tolist()) == {4, 16}
    m = taken == 16
    assert n_ref == int(m.sum()) and 64 <= n_ref <= W * H - 64
    for got, a, b in zip((f32, u8, cnt), lo, hi):
        want = np.where(m.reshape(m.shape + (1,) * (a.ndim - 2)), b, a)
        assert got.tobytes() == want.tobytes()
    assert f32.tobytes() != lo[0].tobytes() and f32.tobytes() != hi[0].tobytes()


# ------------------------------------------------------------------------------------------------- 3. degenerate settings
def test_degenerate_settings(gpu):
    monkey_scene(gpu)
    p = rr.default_params(max_refract=8)
    sc, _, _ = view_constants(*VIEWS[1])
    hi = gpu.render_samples(W, H, sc, OFFP16, p, rgba8=True, ray_counts=True)
    got = gpu.render_adaptive(W, H, sc, (16, OFFP16), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    for a, b in zip(got[:3], hi):
        assert a.tobytes() == b.tobytes()
    assert np.all(got[3] == 16)
    lo = gpu.render_samples(W, H, sc, OFFP16[:4], p, rgba8=True, ray_counts=True)
    got = gpu.render_adaptive(W, H, sc, (4, OFFP16), 1.0, p, rgba8=True, ray_counts=True, sample_counts=True)
    for a, b in zip(got[:3], lo):
        assert a.tobytes() == b.tobytes()
    assert np.all(got[3] == 4) and got[4] == 0


def test_one_base_sample_and_64_random_ones(gpu):
    monkey_scene(gpu)
    w, h = 16, 9
    p = rr.default_params(max_refract=8, max_reflect=3)
    sc, _, _ = view_constants(1.3, 0.35, w, h)
    offs = np.random.default_rng(11).random((64, 2), dtype=np.float32)
    got = gpu.render_adaptive(w, h, sc, (1, offs), 0.05, p, rgba8=True, ray_counts=True, sample_counts=True)
    cols, cnts = sample_colours(gpu, sc, w, h, offs, p)
    mask = follows_the_rule(got, cols, cnts, 1, 0.05, False)        # (one sample: only the neighbours can refine a pixel)
    assert mask.any() and not mask.all()


# ------------------------------------------------------------------------------------------------- 4. built-in pattern
@pytest.mark.parametrize("n_base,n_max", [(4, 16), (2, 8)])
def test_builtin_pattern(gpu, n_base, n_max):
    monkey_scene(gpu)
    p = rr.default_params(max_refract=8)
    sc, _, _ = view_constants(*VIEWS[1])
    a = gpu.render_adaptive(W, H, sc, (n_base, n_max), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    b = gpu.render_adaptive(W, H, sc, (n_base, rr.sample_pattern(n_max)), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4] and 0 < a[4] < W * H


# ------------------------------------------------------------------------------------------------- 5. two-level scene and culling
def test_two_level_scene_and_culling(gpu):
    meshes, env, inst = config4_scene()
    _scene.clear()
    gpu_scene(gpu, meshes, env, inst)
    w, h = 203, 117                                             # not multiples of 8
    sc, _, _ = view_constants(0.01, rr.FOV_Y, w, h)             # the reference's wide view: most blocks are background
    p = rr.default_params(max_refract=8)
    nocull = rr.default_params(max_refract=8, flags=rr.DISPATCH_DEBUG_NO_CULL)
    offs = rr.sample_pattern(8)
    culled = gpu.render_adaptive(w, h, sc, (2, 8), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    traced = gpu.render_adaptive(w, h, sc, (2, 8), THRESHOLD, nocull, rgba8=True, ray_counts=True, sample_counts=True)
    for a, b in zip(culled[:4], traced[:4]):
        assert a.tobytes() == b.tobytes()
    assert culled[4] == traced[4]
    cols, cnts = sample_colours(gpu, sc, w, h, offs, p)
    mask = follows_the_rule(culled, cols, cnts, 2, THRESHOLD, False)
    follows_the_rule(traced, cols, cnts, 2, THRESHOLD, False)
    assert int(mask.sum()) >= 64 and (cnts.sum(axis=0) == 8).mean() > 0.5 and (cnts.sum(axis=0) > 8).mean() > 0.02


# ------------------------------------------------------------------------------------------------- 6. device variant
def device_call(gpu, sc, w, h, p, offs, n_base, threshold, ws, ws_bytes, outs):
    P = C.c_void_p
    o = np.ascontiguousarray(offs, np.float32)
    return rr.lib().rr_render_adaptive_device(gpu._h, w, h, C.byref(sc), C.byref(p), o.ctypes.data, n_base, len(o), threshold,
                                              *[P(t.data_ptr()) if t is not None else None for t in outs], P(ws), ws_bytes)


def test_device_variant_on_a_torch_stream(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    p = rr.default_params(max_refract=8, flags=rr.DISPATCH_TONEMAP_REINHARD)
    host = gpu.render_adaptive(w, h, sc, (4, OFFP16), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
    assert 0 < host[4] < w * h
    stream = torch.cuda.Stream(device=dev)
    gpu.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            outs = gpu.render_adaptive(w, h, sc, (4, OFFP16), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True, device=True)
            f32, u8, cnt, taken = outs
            after = f32.sum()                                   # work queued behind it on the same stream
            # two calls back to back on one workspace, the first with a threshold that refines far more
            need = rr.lib().rr_host_adaptive_workspace_bytes(w, h)
            ws = torch.empty(need + 32, dtype=torch.uint8, device=dev)
            o1 = [torch.empty((h, w, 4), dtype=torch.float32, device=dev), torch.empty((h, w, 4), dtype=torch.uint8, device=dev),
                  torch.empty((h, w), dtype=torch.int32, device=dev), torch.empty((h, w), dtype=torch.int32, device=dev)]
            o2 = [torch.empty_like(t) for t in o1]
            assert ws.data_ptr() % 16 == 0
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, 0.0, ws.data_ptr(), need, o1) == 0
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, ws.data_ptr(), need, o2) == 0
            # refused before anything is launched: o1 keeps the first call's result
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, ws.data_ptr(), need - 1, o1) == RR_ERR_INVALID_ARGUMENT
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, ws.data_ptr() + 8, need, o1) == RR_ERR_INVALID_ARGUMENT
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, None, need, o1) == RR_ERR_INVALID_ARGUMENT
            bad = [o1[0].view(-1)[1:], None, None, None]        # a float pointer 4 bytes off
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, ws.data_ptr(), need, bad) == RR_ERR_INVALID_ARGUMENT
            bad = [o1[0], None, None, o1[3].view(torch.uint8).view(-1)[2:]]
            assert device_call(gpu, sc, w, h, p, OFFP16, 4, THRESHOLD, ws.data_ptr(), need, bad) == RR_ERR_INVALID_ARGUMENT
        stream.synchronize()
        assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and cnt.dtype == torch.int32 and taken.dtype == torch.int32
        assert tuple(f32.shape) == (h, w, 4) and tuple(u8.shape) == (h, w, 4) and tuple(cnt.shape) == (h, w) and f32.device.index == gpu.device
        for d, want in list(zip(outs, host[:4])) + list(zip(o2, host[:4])):
            assert d.cpu().numpy().tobytes() == want.tobytes()
        assert np.isfinite(float(after))
    finally:
        gpu.reset_stream()
    zero = gpu.render_adaptive(w, h, sc, (4, OFFP16), 0.0, p, rgba8=True, ray_counts=True, sample_counts=True)
    assert zero[4] > host[4]
    for d, want in zip(o1, zero[:4]):
        assert d.cpu().numpy().tobytes() == want.tobytes()


def test_device_calls_on_two_streams_keep_two_workspaces(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    sc, _, _ = view_constants(0.4, 0.3, 40, 24)
    host = gpu.render_adaptive(40, 24, sc, (2, 8), THRESHOLD)
    a, b = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    try:
        outs = []
        for st in (a, b, a):
            gpu.set_stream(st.cuda_stream)
            with torch.cuda.stream(st):
                outs.append(gpu.render_adaptive(40, 24, sc, (2, 8), THRESHOLD, device=True))
        a.synchronize()
        b.synchronize()
        assert len(gpu._adaptive_ws) >= 2 and gpu._adaptive_ws[a.cuda_stream] is not gpu._adaptive_ws[b.cuda_stream]
        for o in outs:
            assert o.cpu().numpy().tobytes() == host[0].tobytes()
    finally:
        gpu.reset_stream()


def test_refine_pass_as_a_loop_over_the_list(gpu, monkeypatch):
    """RR_DEBUG_REFINE_GROUPS (read when a context is created) gives k_adaptive_refine a grid smaller than the list, so that its
    waves make several trips: the same bytes as the worst-case grid's single trip"""
    monkey_scene(gpu)
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    p = rr.default_params(max_refract=8, max_reflect=3)
    want = gpu.render_adaptive(w, h, sc, (4, OFFP16), 0.0, p, rgba8=True, ray_counts=True, sample_counts=True)
    assert want[4] > 3 * 256                                    # more than one trip of three workgroups, more than three of one
    for groups in ("1", "3"):
        monkeypatch.setenv("RR_DEBUG_REFINE_GROUPS", groups)
        looped = rr.Renderer(gpu.device)
        monkeypatch.delenv("RR_DEBUG_REFINE_GROUPS")
        try:
            m = load("monkey.obj")
            looped.load_scene(*m, env_map())
            got = looped.render_adaptive(w, h, sc, (4, OFFP16), 0.0, p, rgba8=True, ray_counts=True, sample_counts=True)
        finally:
            looped.close()
        for x, y in zip(got[:4], want[:4]):
            assert x.tobytes() == y.tobytes()
        assert got[4] == want[4]


# ------------------------------------------------------------------------------------------------- 7. not a dispatch
def test_an_adaptive_frame_leaves_the_context_alone(gpu):
    import torch
    monkey_scene(gpu)
    w, h = 160, 120
    sc, _, _ = view_constants(0.3, 0.4, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    before = {k: getattr(st, k) for k in STAT_FIELDS}
    assert "render_kernel_name" in before and before["rays"] > w * h
    sc2, _, _ = view_constants(2.0, 0.2, 90, 50)
    gpu.set_tile_partition(1, 2)                                # ignored: the whole frame is rendered
    try:
        a = gpu.render_adaptive(90, 50, sc2, (4, 16), THRESHOLD, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    finally:
        gpu.set_tile_partition(0, 1)
    b = gpu.render_adaptive(90, 50, sc2, (4, 16), THRESHOLD, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] > 0
    gpu.render_adaptive(90, 50, sc2, (2, 8), THRESHOLD, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, device=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


# ------------------------------------------------------------------------------------------------- 8. arguments
def test_bad_arguments_are_refused(gpu):
    monkey_scene(gpu)
    sc, _, _ = view_constants(1.3, 0.35, 8, 8)
    half = np.full((65, 2), 0.5, np.float32)

    def refused(status, samples, threshold=0.1, params=None, **kw):
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                gpu.render_adaptive(8, 8, sc, samples, threshold, params, device=device, **kw)
            assert e.value.status == status, (samples, threshold)
    refused(RR_ERR_INVALID_ARGUMENT, (0, 4))
    refused(RR_ERR_INVALID_ARGUMENT, (0, half[:4]))
    refused(RR_ERR_INVALID_ARGUMENT, (8, 4))
    refused(RR_ERR_INVALID_ARGUMENT, (5, half[:4]))
    refused(RR_ERR_INVALID_ARGUMENT, (4, half))                 # n_max = 65
    refused(RR_ERR_INVALID_ARGUMENT, (2, 3))                    # no built-in pattern of 3
    for bad in (-0.1, 1.5, np.nan):
        o = half[:4].copy()
        o[3, 1] = bad
        refused(RR_ERR_INVALID_ARGUMENT, (2, o))
    for t in (float("nan"), float("inf"), -1.0):
        refused(RR_ERR_INVALID_ARGUMENT, (4, 16), t)
    refused(RR_ERR_UNSUPPORTED, (4, 16), params=rr.default_params(max_reflect=9))
    # no colour output requested
    L = rr.lib()
    n = np.zeros((8, 8), np.uint32)
    assert L.rr_render_adaptive(gpu._h, 8, 8, C.byref(sc), None, None, 4, 16, 0.1, None, None, n.ctypes.data, n.ctypes.data, None) == RR_ERR_INVALID_ARGUMENT
    # the limits themselves are fine: 64 samples, threshold 0, NULL params and NULL n_refined
    f = np.zeros((8, 8, 4), np.float32)
    assert L.rr_render_adaptive(gpu._h, 8, 8, C.byref(sc), None, half[:64].ctypes.data, 64, 64, 0.0, f.ctypes.data, None, None, None, None) == 0
    assert f.tobytes() == gpu.render_samples(8, 8, sc, half[:64]).tobytes()


def test_adaptive_frames_need_a_built_scene(gpu):
    fresh = rr.Renderer(gpu.device)
    try:
        sc, _, _ = view_constants(0.4, 0.3, 8, 8)
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                fresh.render_adaptive(8, 8, sc, (4, 16), device=device)
            assert e.value.status == RR_ERR_STATE
    finally:
        fresh.close()
