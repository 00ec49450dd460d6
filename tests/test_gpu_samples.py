"""GPU: supersampled frames (Renderer.render_samples, rr_render_samples[_device]) -- S primary rays per pixel through S sub-pixel
positions, each with the shader's whole ray tree, resolved in the kernel.

Two references.  The CPU oracle (accum_mode=1, use_libm=0: the kernels' summation order) renders a frame 4 times as large per
axis, whose pixels ARE the sub-pixel samples of the base frame for offsets that are odd multiples of 1/8 (test_samples_abi.py
shows the rays equal bit for bit); its colours are folded in np.float32 by the resolve rule, ((c_0 + c_1) + ...) / S.  And the
radiance queries: the same fold over S shade_rays calls on rr.camera_rays.  Every pixel is compared, none sampled."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from scenes import gpu, gpu_scene, load, oracle_scene  # noqa: F401  (gpu: a fixture)
from shading_helpers import CELL16, LIMITS, STAT_FIELDS, SUB4, H, W, config4_scene, env_map, fold, instanced_scene, unorm8, view_constants

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE, RR_ERR_UNSUPPORTED = 1, 5, 7
VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35), (3.7, 0.2)]
OFF16 = np.array([[(2 * i + 1) / 8.0, (2 * j + 1) / 8.0] for i, j in CELL16], np.float32)


def check(got, want_rgb, want_cnt, tonemap):
    f32, u8, cnt = got
    assert f32.dtype == np.float32 and u8.dtype == np.uint8 and cnt.dtype == np.uint32
    assert np.all(f32[..., 3] == 1.0)
    mism = int((f32[..., :3].view(np.uint32) != want_rgb.view(np.uint32)).any(axis=-1).sum())
    assert mism == 0, "%d pixels differ in their float bits" % mism
    assert np.array_equal(u8, unorm8(want_rgb, tonemap))
    assert np.array_equal(cnt, want_cnt.astype(np.uint32))


def shade_fold(gpu, sc, w, h, offsets, p):
    """fold of len(offsets) shade_rays calls on rr.camera_rays -> (rgb [h, w, 3], counts [h, w])"""
    cols, total = [], np.zeros(w * h, np.uint32)
    for ox, oy in offsets:
        f, n = gpu.shade_rays(rr.camera_rays(sc, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), p, ray_counts=True)
        cols.append(f[:, :3])
        total += n
    return fold(cols).reshape(h, w, 3), total.reshape(h, w)


def monkey_scene(gpu):
    m = load("monkey.obj")
    gpu.load_scene(*m, env_map())


# ------------------------------------------------------------------------------------------------- 1. one centre sample is a dispatch
@pytest.mark.parametrize("flags", [0, rr.DISPATCH_TONEMAP_REINHARD])
def test_one_centre_sample_is_a_dispatch(gpu, flags):
    monkey_scene(gpu)
    w, h = 203, 117                                             # not multiples of 8
    sc, _, _ = view_constants(0.8, 0.3, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | flags, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    p = rr.default_params(flags=flags, max_refract=8)
    g32, g8, gn = gpu.render_samples(w, h, sc, 1, p, rgba8=True, ray_counts=True)
    assert g32.shape == (h, w, 4) and g8.shape == (h, w, 4) and gn.shape == (h, w)
    assert g32.tobytes() == f32.tobytes() and g8.tobytes() == rgba.tobytes()
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) > 100
    _, cnt = gpu.shade_rays(rr.camera_rays(sc, w, h), p, ray_counts=True)
    assert np.array_equal(gn.reshape(-1), cnt) and (cnt > 1).mean() > 0.1
    # four copies of the centre: the sum of four equal finite values divided by 4 is exact
    q32, q8, qn = gpu.render_samples(w, h, sc, np.full((4, 2), 0.5, np.float32), p, rgba8=True, ray_counts=True)
    assert q32.tobytes() == f32.tobytes() and q8.tobytes() == rgba.tobytes()
    assert np.array_equal(qn, 4 * gn)


# ------------------------------------------------------------------------------------------------- 2. oracle parity
_single = {}


def single_scene(gpu, name):
    if _single.get("name") != name:
        m = load(name)
        env = env_map()
        gpu.load_scene(*m, env)
        s = oracle_scene([m], env)
        _single.clear()
        _single.update(name=name, s=s)
    return _single["s"]


def oracle_samples(s, M, cam, w, h, **kw):
    """the oracle's 4w x 4h frame as sub-pixel samples: rgb [4, 4, h, w, 3] and counts [4, 4, h, w], indexed [sub y][sub x]"""
    ref = s.render(M, cam, 4 * w, 4 * h, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, **kw), want_rays=True)
    rgb = ref["rgb"].reshape(h, 4, w, 4, 3).transpose(1, 3, 0, 2, 4)
    cnt = ref["rays"].astype(np.uint32).reshape(h, 4, w, 4).transpose(1, 3, 0, 2)
    return rgb, cnt


def check_against_oracle(gpu, s, sc, M, cam, w, h, patterns, **kw):
    """render_samples == the fold of the oracle's sub-pixels, with and without Reinhard; patterns: [(samples argument, [(sub x, sub y)])].
    Returns the oracle's counts."""
    rgb, cnt = oracle_samples(s, M, cam, w, h, **kw)
    for samples, subs in patterns:
        want = fold([rgb[j, i] for i, j in subs])
        want_n = sum(cnt[j, i] for i, j in subs)
        for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
            got = gpu.render_samples(w, h, sc, samples, rr.default_params(flags=flags, **kw), rgba8=True, ray_counts=True)
            check(got, want, want_n, flags != 0)
    return cnt


@pytest.mark.parametrize("max_refract,max_reflect,ior", LIMITS)
@pytest.mark.parametrize("name", ["cube.obj", "monkey.obj", "shell.obj"])          # (the mesh varies slowest: one scene build per mesh)
def test_oracle_parity(gpu, name, max_refract, max_reflect, ior):
    s = single_scene(gpu, name)
    differ = total = 0
    for angle, fov in VIEWS:
        sc, M, cam = view_constants(angle, fov)
        cnt = check_against_oracle(gpu, s, sc, M, cam, W, H, [(4, SUB4), (OFF16, CELL16)],
                                   max_refract=max_refract, max_reflect=max_reflect, ior=ior)
        if (max_refract, max_reflect) == LIMITS[0][:2]:
            four = np.stack([cnt[j, i] for i, j in SUB4])
            differ += int((four != four[0]).any(axis=0).sum())
            total += W * H
    if total:
        # against a vacuous pass: the samples of a pixel are different rays with different trees (with the oracle and a random
        # environment map: monkey 7.0 %, 28.5 % and 41.7 % of the pixels per view, 26 % overall)
        print("%s: %.3f of the pixels have 4x samples whose TraceRay counts differ" % (name, differ / total))
        if name == "monkey.obj":
            assert differ * 10 >= total, (differ, total)


# ------------------------------------------------------------------------------------------------- 3. two-level


@pytest.mark.parametrize("angle", [0.6, 0.01])
@pytest.mark.parametrize("scene", [instanced_scene, config4_scene])
def test_oracle_parity_two_level(gpu, scene, angle):
    meshes, env, inst = scene()
    gpu_scene(gpu, meshes, env, inst)
    s = oracle_scene(meshes, env, inst)
    w, h = 50, 38
    sc = rr.camera_orbit(angle)
    M, cam = np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)
    for mr, ml, ior in ((8, 2, 1.2), (5, 3, 1.2)):
        cnt = check_against_oracle(gpu, s, sc, M, cam, w, h, [(4, SUB4)], max_refract=mr, max_reflect=ml, ior=ior)
        assert (cnt > 1).mean() > 0.02


# ------------------------------------------------------------------------------------------------- 4. culling
def test_background_blocks_are_culled_without_a_trace_of_it(gpu):
    monkey_scene(gpu)
    w, h = 203, 117
    sc, _, _ = view_constants(0.01, rr.FOV_Y, w, h)             # the reference's wide view: most blocks are background
    p = rr.default_params(max_refract=8)
    culled = gpu.render_samples(w, h, sc, 8, p, rgba8=True, ray_counts=True)
    traced = gpu.render_samples(w, h, sc, 8, rr.default_params(max_refract=8, flags=rr.DISPATCH_DEBUG_NO_CULL), rgba8=True, ray_counts=True)
    for a, b in zip(culled, traced):
        assert a.tobytes() == b.tobytes()
    rgb, cnt = shade_fold(gpu, sc, w, h, rr.sample_pattern(8), p)
    check(culled, rgb, cnt, False)
    assert (cnt == 8).mean() > 0.5 and (cnt > 8).mean() > 0.02


# ------------------------------------------------------------------------------------------------- 5. edges of the launch
GRID64 = np.array([[((i % 8) + 0.5) / 8, ((i // 8) + 0.5) / 8] for i in range(64)], np.float32)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (8, 8), (9, 65), (64, 1)])
def test_edges_of_the_launch(gpu, w, h):
    monkey_scene(gpu)
    sc, _, _ = view_constants(1.3, 0.35, w, h)
    p = rr.default_params(max_refract=8, max_reflect=3)
    L = rr.lib()
    for samples, offs in ((1, rr.sample_pattern(1)), (2, rr.sample_pattern(2)), (GRID64, GRID64)):
        rgb, cnt = shade_fold(gpu, sc, w, h, offs, p)
        got = gpu.render_samples(w, h, sc, samples, p, rgba8=True, ray_counts=True)
        check(got, rgb, cnt, False)
        if h > 1:
            assert (cnt > len(offs)).any()
        # each output on its own
        assert gpu.render_samples(w, h, sc, samples, p).tobytes() == got[0].tobytes()
        assert np.array_equal(gpu.render_samples(w, h, sc, samples, p, ray_counts=True)[1], got[2])
        only8 = np.zeros((h, w, 4), np.uint8)
        n = len(offs)
        o = np.ascontiguousarray(offs, np.float32)
        assert L.rr_render_samples(gpu._h, w, h, C.byref(sc), C.byref(p), o.ctypes.data, n, None, only8.ctypes.data, None) == 0
        assert only8.tobytes() == got[1].tobytes()
        assert L.rr_render_samples(gpu._h, w, h, C.byref(sc), C.byref(p), o.ctypes.data, n, None, None, got[2].ctypes.data) == RR_ERR_INVALID_ARGUMENT


def test_bad_arguments_are_refused(gpu):
    monkey_scene(gpu)
    sc, _, _ = view_constants(1.3, 0.35, 8, 8)
    L = rr.lib()
    f = np.zeros((8, 8, 4), np.float32)
    for samples in (np.zeros((0, 2), np.float32), np.full((65, 2), 0.5, np.float32), 0, 3, 32, 65):
        with pytest.raises(rr.RRError) as e:
            gpu.render_samples(8, 8, sc, samples)
        assert e.value.status == RR_ERR_INVALID_ARGUMENT, samples
    for bad in (np.nan, -0.1, 1.5, np.inf):
        for axis in (0, 1):
            o = np.full((3, 2), 0.5, np.float32)
            o[2, axis] = bad
            with pytest.raises(rr.RRError) as e:
                gpu.render_samples(8, 8, sc, o)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, bad
    gpu.render_samples(8, 8, sc, np.array([[0.0, 1.0], [1.0, 0.0]], np.float32))          # the closed interval
    for w, h in ((0, 8), (8, 0), (32769, 8), (8, 32769)):
        assert L.rr_render_samples(gpu._h, w, h, C.byref(sc), None, None, 1, f.ctypes.data, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples(gpu._h, 8, 8, None, None, None, 1, f.ctypes.data, None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples(gpu._h, 8, 8, C.byref(sc), None, None, 1, f.ctypes.data, None, None) == 0      # NULL params: the defaults
    assert f.tobytes() == gpu.render_samples(8, 8, sc, 1).tobytes()
    for bad, status in ((dict(max_reflect=9), RR_ERR_UNSUPPORTED), (dict(max_refract=-1), RR_ERR_INVALID_ARGUMENT),
                        (dict(max_reflect=-1), RR_ERR_INVALID_ARGUMENT), (dict(ior=0.0), RR_ERR_INVALID_ARGUMENT)):
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                gpu.render_samples(8, 8, sc, 4, rr.default_params(**bad), device=device)
            assert e.value.status == status, bad


# ------------------------------------------------------------------------------------------------- 6. device path
def test_device_path_equals_host_path(gpu):
    import torch
    monkey_scene(gpu)
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    p = rr.default_params(max_refract=8, flags=rr.DISPATCH_TONEMAP_REINHARD)
    f32, u8, cnt = gpu.render_samples(w, h, sc, 4, p, rgba8=True, ray_counts=True)
    assert (cnt > 4).mean() > 0.1
    df, du, dc = gpu.render_samples(w, h, sc, 4, p, rgba8=True, ray_counts=True, device=True)
    gpu.wait()
    torch.cuda.synchronize()
    assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32
    assert tuple(df.shape) == (h, w, 4) and tuple(du.shape) == (h, w, 4) and tuple(dc.shape) == (h, w)
    assert df.device.index == gpu.device
    assert df.cpu().numpy().tobytes() == f32.tobytes() and du.cpu().numpy().tobytes() == u8.tobytes()
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), cnt)
    only = gpu.render_samples(w, h, sc, 4, p, device=True)
    gpu.wait()
    assert only.cpu().numpy().tobytes() == f32.tobytes()


def test_device_path_is_ordered_on_torch_stream(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    p = rr.default_params(max_refract=8)
    host = gpu.render_samples(w, h, sc, OFF16, p, rgba8=True, ray_counts=True)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        torch.cuda.synchronize()
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        big = torch.randn((4096, 4096), device=dev, generator=g)
        big = big @ big                                     # queued ahead of the frame on the same stream
        f32, u8, cnt = gpu.render_samples(w, h, sc, OFF16, p, rgba8=True, ray_counts=True, device=True)     # no synchronisation in between
        after = f32.sum() + big[0, 0] * 0.0                 # and work queued behind it
        torch.cuda.current_stream().synchronize()
        assert f32.cpu().numpy().tobytes() == host[0].tobytes() and u8.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), host[2])
        assert np.isfinite(float(after))
    finally:
        gpu.reset_stream()


def test_device_path_refuses_misaligned_pointers(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    sc, _, _ = view_constants(0.4, 0.3, 8, 8)
    L = rr.lib()
    out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
    aux = torch.zeros(64 + 4, dtype=torch.int32, device=dev)
    P = C.c_void_p
    a = (gpu._h, 8, 8, C.byref(sc), None, None, 4)
    assert out.data_ptr() % 16 == 0 and aux.data_ptr() % 4 == 0
    assert L.rr_render_samples_device(*a, P(out.data_ptr()), P(aux.data_ptr()), P(aux.data_ptr())) == 0
    assert L.rr_render_samples_device(*a, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples_device(*a, P(out.data_ptr()), P(aux.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples_device(*a, P(out.data_ptr()), None, P(aux.data_ptr() + 1)) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_samples_device(*a, None, None, P(aux.data_ptr())) == RR_ERR_INVALID_ARGUMENT
    gpu.wait()


# ------------------------------------------------------------------------------------------------- 7. leaves the context alone
def test_a_supersampled_frame_leaves_the_context_alone(gpu):
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
    assert before["rays"] > w * h
    sc2, _, _ = view_constants(2.0, 0.2, 90, 50)
    gpu.render_samples(90, 50, sc2, 4, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.render_samples(90, 50, sc2, 2, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True, device=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


def test_supersampled_frames_need_a_built_scene(gpu):
    fresh = rr.Renderer(gpu.device)
    try:
        sc, _, _ = view_constants(0.4, 0.3, 8, 8)

        def refused():
            for device in (False, True):
                with pytest.raises(rr.RRError) as e:
                    fresh.render_samples(8, 8, sc, 4, device=device)
                assert e.value.status == RR_ERR_STATE
        refused()                                                               # nothing built
        m = load("cube.obj")
        mid = fresh.upload_mesh(*m)
        fresh.build_blas(mid, allow_update=True)
        refused()                                                               # BLAS built, no TLAS yet
        fresh.build_tlas(rr.make_instances(meshes=[mid]), allow_update=True)
        fresh.upload_envmap(procedural_env(64, 32, seed=1))
        a = fresh.render_samples(8, 8, sc, 4)
        fresh.update_mesh_vertices(mid, m[0])
        fresh.build_blas(mid, update=True)
        refused()                                                               # BLAS updated, TLAS not
        fresh.build_tlas(rr.make_instances(meshes=[mid]), update=True)
        assert fresh.render_samples(8, 8, sc, 4).tobytes() == a.tobytes()
    finally:
        fresh.close()
