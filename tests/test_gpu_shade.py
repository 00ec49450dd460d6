"""GPU: radiance queries (Renderer.shade_rays, rr_shade_rays[_device]) -- the shader's whole ray tree on caller rays.

The reference is the CPU oracle in path-weight mode (accum_mode=1, use_libm=0: the kernels' summation order): shading the rays
rro_generate_camera_ray gives for every pixel of a frame must reproduce rro_render's float colours bit for bit, its RGBA8 (with
and without Reinhard) and its per-pixel TraceRay counts.  Every ray is compared, none sampled."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from scenes import gpu, gpu_scene, load, oracle_scene, to_dev, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import STAT_FIELDS, camera_rays, check_against_oracle, config4_scene, instanced_scene, view_constants

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE, RR_ERR_UNSUPPORTED = 1, 5, 7
W, H = 160, 120
# (orbit angle, fov_y): the reference's camera, then two narrow fields of view in which the mesh fills the frame.  Chosen on the
# CPU with the oracle (default bounce limits): the share of rays with more than one TraceRay call over the three views is
# cube 0.72, sphere 0.78, monkey 0.42, shell 0.78
VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35), (3.7, 0.2)]
LIMITS = [(mr, ml, 1.2) for mr in (0, 1, 5, 11) for ml in (0, 2, 3)] + [(5, 2, 1.5), (11, 3, 1.05)]     # ml = 3: the PEND = 8 builds


# ------------------------------------------------------------------------------------------------- 1. oracle parity, one BLAS
_single = {}


def single_scene(gpu, name):
    """(oracle scene, [(M, cam, rays)] per view); the GPU scene is rebuilt when the mesh changes"""
    if _single.get("name") != name:
        m = load(name)
        env = procedural_env(128, 64, seed=3)
        gpu.load_scene(*m, env)
        s = oracle_scene([m], env)
        views = []
        for angle, fov in VIEWS:
            _, M, cam = view_constants(angle, fov, W, H)
            views.append((M, cam, camera_rays(M, cam, W, H)))
        _single.clear()
        _single.update(name=name, s=s, views=views)
    return _single["s"], _single["views"]


@pytest.mark.parametrize("max_refract,max_reflect,ior", LIMITS)
@pytest.mark.parametrize("name", ["cube.obj", "sphere.obj", "monkey.obj", "shell.obj"])        # (the mesh varies slowest: one scene build per mesh)
def test_oracle_parity_single_blas(gpu, name, max_refract, max_reflect, ior):
    s, views = single_scene(gpu, name)
    deep = total = 0
    for M, cam, rays in views:
        check_against_oracle(gpu, s, M, cam, W, H, rays, max_refract=max_refract, max_reflect=max_reflect, ior=ior)
        # against a vacuous pass: the mesh is in view (counted with the reference's bounce limits, whatever this case's are)
        cov = s.render(M, cam, W, H, O.default_params(use_bvh=1, accum_mode=1), want_rays=True)["rays"]
        deep += int((cov > 1).sum())
        total += cov.size
    print("%s: %.3f of the rays have more than one TraceRay call" % (name, deep / total))
    assert deep * 4 >= total, (name, deep, total)


# ------------------------------------------------------------------------------------------------- 2. oracle parity, two-level


def two_level_check(gpu, meshes, env, inst, angle, w, h, limits):
    gpu_scene(gpu, meshes, env, inst)
    s = oracle_scene(meshes, env, inst)
    sc = rr.camera_orbit(angle)
    M, cam = np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)
    rays = camera_rays(M, cam, w, h)
    for mr, ml, ior in limits:
        ref = check_against_oracle(gpu, s, M, cam, w, h, rays, max_refract=mr, max_reflect=ml, ior=ior)
    return ref


def test_oracle_parity_instanced_scene(gpu):
    """the scene of test_instanced_scene_parity (rotated, non-uniformly scaled instances, TRIANGLE_CULL_DISABLE, a zero-mask
    instance) plus a mirrored instance with TRIANGLE_FRONT_COUNTERCLOCKWISE"""
    meshes, env, inst = instanced_scene()
    ref = two_level_check(gpu, meshes, env, inst, 0.6, 200, 150, [(8, 2, 1.2), (0, 0, 1.2), (5, 3, 1.2), (11, 2, 1.5)])
    assert (ref["rays"] > 1).mean() > 0.05


def test_oracle_parity_config4_scene(gpu):
    """the scene of test_config4_multi_blas_scene: shell + cube + ott, three BLASes under one TLAS (trees deeper than 30 levels)"""
    meshes, env, inst = config4_scene()
    ref = two_level_check(gpu, meshes, env, inst, 0.01, 240, 135, [(8, 2, 1.2), (5, 3, 1.2)])
    assert (ref["rays"] > 1).mean() > 0.02


# ------------------------------------------------------------------------------------------------- 3. equals a dispatch
def monkey_scene(gpu):
    m = load("monkey.obj")
    gpu.load_scene(*m, procedural_env(128, 64, seed=5))


@pytest.mark.parametrize("flags", [0, rr.DISPATCH_TONEMAP_REINHARD])
def test_shade_rays_equals_a_dispatch(gpu, flags):
    monkey_scene(gpu)
    w, h = 203, 117                                             # not multiples of 8
    sc, M, cam = view_constants(0.8, 0.3, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | flags, max_refract=8))
    rgba, f32 = gpu.read_frame(want_float=True)
    got_f32, got_u8 = gpu.shade_rays(camera_rays(M, cam, w, h), rr.default_params(flags=flags, max_refract=8), rgba8=True)
    assert got_f32.reshape(h, w, 4).tobytes() == f32.tobytes()
    assert got_u8.reshape(h, w, 4).tobytes() == rgba.tobytes()
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) > 100


# ------------------------------------------------------------------------------------------------- 4. order and neighbours
def test_order_and_neighbours_do_not_matter(gpu):
    monkey_scene(gpu)
    _, M, cam = view_constants(2.1, 0.3, W, H)
    rays = camera_rays(M, cam, W, H)
    p = rr.default_params(max_refract=8, max_reflect=3)
    f32, u8, cnt = gpu.shade_rays(rays, p, rgba8=True, ray_counts=True)
    assert (cnt > 1).mean() > 0.25
    perm = np.random.default_rng(5).permutation(len(rays))
    pf, pu, pc = gpu.shade_rays(rays[perm], p, rgba8=True, ray_counts=True)
    assert pf.tobytes() == f32[perm].tobytes() and pu.tobytes() == u8[perm].tobytes() and np.array_equal(pc, cnt[perm])
    off = W * (H // 2) + 11                                     # a run of rays that crosses the mesh
    for n in (1, 63, 64, 65, 257):
        qf, qu, qc = gpu.shade_rays(rays[off:off + n], p, rgba8=True, ray_counts=True)
        assert qf.tobytes() == f32[off:off + n].tobytes() and qu.tobytes() == u8[off:off + n].tobytes()
        assert np.array_equal(qc, cnt[off:off + n])
    ef, eu, ec = gpu.shade_rays(rays[:0], p, rgba8=True, ray_counts=True)
    assert ef.shape == (0, 4) and eu.shape == (0, 4) and ec.shape == (0,)
    # each output on its own
    assert gpu.shade_rays(rays, p).tobytes() == f32.tobytes()
    assert np.array_equal(gpu.shade_rays(rays, p, ray_counts=True)[1], cnt)
    L = rr.lib()
    only8 = np.zeros((len(rays), 4), np.uint8)
    assert L.rr_shade_rays(gpu._h, rays.ctypes.data, len(rays), C.byref(p), None, only8.ctypes.data, None) == 0
    assert only8.tobytes() == u8.tobytes()
    assert L.rr_shade_rays(gpu._h, rays.ctypes.data, len(rays), C.byref(p), None, None, cnt.ctypes.data) == RR_ERR_INVALID_ARGUMENT
    for bad, status in ((dict(max_reflect=9), RR_ERR_UNSUPPORTED), (dict(max_refract=-1), RR_ERR_INVALID_ARGUMENT),
                        (dict(max_reflect=-1), RR_ERR_INVALID_ARGUMENT), (dict(ior=0.0), RR_ERR_INVALID_ARGUMENT)):
        with pytest.raises(rr.RRError) as e:
            gpu.shade_rays(rays[:64], rr.default_params(**bad))
        assert e.value.status == status, bad


# ------------------------------------------------------------------------------------------------- 5. device path
def test_device_path_equals_host_path(gpu):
    import torch
    monkey_scene(gpu)
    _, M, cam = view_constants(0.4, 0.3, W, H)
    rays = camera_rays(M, cam, W, H)
    p = rr.default_params(max_refract=8)
    f32, u8, cnt = gpu.shade_rays(rays, p, rgba8=True, ray_counts=True)
    for dtype in ("int32", "float32"):
        df, du, dc = gpu.shade_rays(to_dev(rays, gpu, dtype), p, rgba8=True, ray_counts=True)
        gpu.wait()
        torch.cuda.synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32
        assert tuple(df.shape) == (len(rays), 4) and tuple(du.shape) == (len(rays), 4) and tuple(dc.shape) == (len(rays),)
        assert df.cpu().numpy().tobytes() == f32.tobytes() and du.cpu().numpy().tobytes() == u8.tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), cnt)
    only = gpu.shade_rays(to_dev(rays, gpu), p)
    gpu.wait()
    assert only.cpu().numpy().tobytes() == f32.tobytes()
    e = gpu.shade_rays(torch.empty((0, 12), dtype=torch.int32, device="cuda:%d" % gpu.device), p, rgba8=True, ray_counts=True)
    assert tuple(e[0].shape) == (0, 4) and tuple(e[1].shape) == (0, 4) and tuple(e[2].shape) == (0,)


def test_device_path_is_ordered_on_torch_stream(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        torch.cuda.synchronize()
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        n = 1 << 18
        big = torch.randn((4096, 4096), device=dev, generator=g)
        big = big @ big                                     # queue work ahead of the rays on the same stream
        o = torch.randn((n, 3), device=dev, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 4.0], device=dev) + big[0, 0] * 0.0
        d = torch.rand((n, 3), device=dev, generator=g) * 2.0 - 1.0 - o
        d = d / d.norm(dim=1, keepdim=True)
        t = rr.pack_rays(o, d, 1e-4, 100.0)
        p = rr.default_params(max_refract=8)
        f32, u8, cnt = gpu.shade_rays(t, p, rgba8=True, ray_counts=True)       # no synchronisation between the rays and the query
        torch.cuda.current_stream().synchronize()
        rays = np.ascontiguousarray(t.cpu().numpy()).view(rr.RAY_DTYPE).reshape(-1)
        assert np.all(rays["tmin"] == np.float32(1e-4))
        hf, hu, hc = gpu.shade_rays(rays, p, rgba8=True, ray_counts=True)
        assert (hc > 1).sum() > n // 4
        assert f32.cpu().numpy().tobytes() == hf.tobytes() and u8.cpu().numpy().tobytes() == hu.tobytes()
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), hc)
    finally:
        gpu.reset_stream()


def test_device_path_refuses_bad_pointers_and_shapes(gpu):
    import torch
    monkey_scene(gpu)
    dev = "cuda:%d" % gpu.device
    _, M, cam = view_constants(0.4, 0.3, 8, 8)
    t = to_dev(camera_rays(M, cam, 8, 8), gpu)
    flat = torch.zeros(64 * 12 + 4, dtype=torch.int32, device=dev)
    flat[1:1 + 64 * 12] = t.reshape(-1)
    mis = flat[1:1 + 64 * 12].view(64, 12)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 4
    with pytest.raises(rr.RRError) as e:
        gpu.shade_rays(mis)
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    L = rr.lib()
    out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
    P = C.c_void_p
    ok = (P(t.data_ptr()), 64, None, P(out.data_ptr()), None, None)
    assert L.rr_shade_rays_device(gpu._h, *ok) == 0
    assert L.rr_shade_rays_device(gpu._h, P(t.data_ptr()), 64, None, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_device(gpu._h, P(t.data_ptr()), 64, None, P(out.data_ptr()), P(out.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_device(gpu._h, P(t.data_ptr()), 64, None, P(out.data_ptr()), None, P(out.data_ptr() + 1)) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_device(gpu._h, P(t.data_ptr()), 64, None, None, None, P(out.data_ptr())) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_shade_rays_device(gpu._h, P(t.data_ptr()), 0, None, P(out.data_ptr() + 4), None, None) == 0
    gpu.wait()
    for bad in (t.cpu(), t[:, :8].contiguous(), t.reshape(-1), t.to(torch.float64),
                torch.zeros((64, 16), dtype=torch.int32, device=dev)[:, :12]):
        with pytest.raises(ValueError):
            gpu.shade_rays(bad)



def test_host_calls_share_one_staged_output_set(gpu):
    """The host variants of shade_rays, render_samples and render_adaptive stage their outputs through one set of context buffers,
    each sized by whichever call grew it last.  Calls of 100, 63, 144, 5, 9 and 300 elements -- growth, reuse at a smaller size,
    growth again, for each of the three buffers -- must each equal, byte for byte, the same call's device variant into fresh torch
    tensors, which does not touch the set."""
    import torch
    m = load("cube.obj")
    gpu.load_scene(*m, procedural_env(128, 64, seed=5))
    p = rr.default_params(max_refract=8)
    _, M, cam = view_constants(1.3, 0.35, 20, 15)
    rays = camera_rays(M, cam, 20, 15)
    rays = rays[np.random.default_rng(3).permutation(len(rays))]       # (every prefix holds rays that hit the cube)

    def same(host, dev):
        gpu.wait()
        torch.cuda.synchronize()
        assert len(host) == len(dev)
        for a, t in zip(host, dev):
            b = t.cpu().numpy()
            assert a.shape == b.shape and a.tobytes() == b.tobytes()

    def shade(n):
        host = gpu.shade_rays(rays[:n], p, rgba8=True, ray_counts=True)
        same(host, gpu.shade_rays(to_dev(rays[:n], gpu), p, rgba8=True, ray_counts=True))
        return host

    def samples(w, h, n):
        sc, _, _ = view_constants(1.3, 0.35, w, h)
        same(gpu.render_samples(w, h, sc, n, p, rgba8=True, ray_counts=True),
             gpu.render_samples(w, h, sc, n, p, rgba8=True, ray_counts=True, device=True))

    shade(100)
    samples(9, 7, 4)
    sc, _, _ = view_constants(1.3, 0.35, 16, 9)
    kw = dict(samples=(1, 4), params=p, rgba8=True, ray_counts=True, sample_counts=True)
    host = gpu.render_adaptive(16, 9, sc, **kw)
    same(host[:4], gpu.render_adaptive(16, 9, sc, device=True, **kw))
    assert set(np.unique(host[3])) <= {1, 4} and host[4] == int((host[3] == 4).sum())
    shade(5)
    samples(3, 3, 2)
    _, _, cnt = shade(300)
    assert (cnt > 1).any() and (cnt == 1).any()                 # hits and misses: the outputs are not constant


# ------------------------------------------------------------------------------------------------- 6. leaves the context alone


def test_a_radiance_query_leaves_the_context_alone(gpu):
    import torch
    monkey_scene(gpu)
    sc, M, cam = view_constants(0.3, 0.4, W, H)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(W, H, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    before = {k: getattr(st, k) for k in STAT_FIELDS}
    assert before["rays"] > W * H
    _, M2, cam2 = view_constants(2.0, 0.2, W, H)
    rays = camera_rays(M2, cam2, W, H)
    gpu.shade_rays(rays, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.shade_rays(to_dev(rays, gpu), rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


def test_radiance_queries_need_a_built_scene(gpu):
    fresh = rr.Renderer(gpu.device)
    try:
        _, M, cam = view_constants(0.4, 0.3, 8, 8)
        rays = camera_rays(M, cam, 8, 8)
        t = to_dev(rays, fresh)
        for r in (rays, t):
            with pytest.raises(rr.RRError) as e:
                fresh.shade_rays(r)                                             # nothing built
            assert e.value.status == RR_ERR_STATE
        m = load("cube.obj")
        mid = fresh.upload_mesh(*m)
        fresh.build_blas(mid, allow_update=True)
        for r in (rays, t):
            with pytest.raises(rr.RRError) as e:
                fresh.shade_rays(r)                                             # BLAS built, no TLAS yet
            assert e.value.status == RR_ERR_STATE
        fresh.build_tlas(rr.make_instances(meshes=[mid]), allow_update=True)
        fresh.upload_envmap(procedural_env(64, 32, seed=1))
        a = fresh.shade_rays(rays)
        fresh.update_mesh_vertices(mid, m[0])
        fresh.build_blas(mid, update=True)
        for r in (rays, t):
            with pytest.raises(rr.RRError) as e:
                fresh.shade_rays(r)                                             # BLAS updated, TLAS not
            assert e.value.status == RR_ERR_STATE
        fresh.build_tlas(rr.make_instances(meshes=[mid]), update=True)
        assert fresh.shade_rays(rays).tobytes() == a.tobytes()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 7. bad rays terminate
@pytest.mark.parametrize("scene", ["single", "instanced"])
def test_bad_rays_terminate_and_do_not_disturb_good_ones(gpu, scene):
    """input validation of a public entry point: rays with NaN, infinite and zero directions, NaN origins and tmin > tmax give
    an unspecified colour, the call returns, and the good rays around them are shaded as without them"""
    if scene == "single":
        monkey_scene(gpu)
    else:
        cube, monkey = load("cube.obj"), load("monkey.obj")
        inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4), xf(0.3, 0.2, 2.4, (0.7, 0.7, 0.7), -1.0)],
                                 meshes=[1, 0, 1])
        gpu_scene(gpu, [cube, monkey], procedural_env(128, 64, seed=7), inst)
    _, M, cam = view_constants(0.9, 0.5, 64, 48)
    good = camera_rays(M, cam, 64, 48)
    p = rr.default_params(max_refract=11, max_reflect=3)
    gf, gu, gc = gpu.shade_rays(good, p, rgba8=True, ray_counts=True)
    assert (gc > 1).sum() > 100
    rays = good.copy()
    bad = np.arange(5, len(rays), 7)
    kinds = [(np.nan, np.nan, np.nan), (np.inf, 0.0, 0.0), (0.0, 0.0, 0.0), (-np.inf, np.inf, np.nan), (0.0, np.nan, 1.0),
             (1e38, 1e38, 1e38), (1e-45, 0.0, 0.0)]
    for j, i in enumerate(bad):
        k = j % (len(kinds) + 2)
        if k < len(kinds):
            rays["dir"][i] = kinds[k]
        elif k == len(kinds):
            rays["tmin"][i], rays["tmax"][i] = 10.0, 1.0
        else:
            rays["origin"][i] = (np.nan, 0.0, np.inf)
    f, u, c = gpu.shade_rays(rays, p, rgba8=True, ray_counts=True)
    keep = np.ones(len(rays), bool)
    keep[bad] = False
    assert f[keep].tobytes() == gf[keep].tobytes() and u[keep].tobytes() == gu[keep].tobytes() and np.array_equal(c[keep], gc[keep])
    # the tree of a bad ray is bounded like any other: at most 2^(max_reflect + 1) - 1 rays before the refraction chains,
    # each at most max_refract long
    assert c[bad].min() >= 1 and c[bad].max() <= (2 ** 4) * 12
