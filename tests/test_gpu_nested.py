"""GPU: nested media (Renderer.shade_rays_nested, render_nested; rr_shade_rays_nested[_device], rr_render_nested[_device]).

Three references.  tests/native/nested_ref.c (nested_helpers.py) restates the tree of include/rrdxr.h and is compared bit for bit --
float colours, RGBA8 and TraceRay counts -- on fixtures of shipped closed meshes inside and across each other, each of which meets a
condition read from the reference's tallies (test_nested_cpu.py prints them).  On closed, disjoint scenes the calls are their _materials
twins byte for byte.  And one ray through two concentric cubes has a closed form neither reference takes part in."""
import numpy as np
import pytest

import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from materials_helpers import H, W, view
from nested_helpers import FH, FW, OFF3, TABLE
from scenes import gpu, load, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import STAT_FIELDS, env_map, unorm8, view_constants
from test_gpu_capacity_edges import ENV as EDGE_ENV
from test_gpu_capacity_edges import EdgeScene, mesh
from test_gpu_samples import check
from test_gpu_stack_rungs import view as edge_view

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5


def same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rays(got, ref):
    """shade_rays_nested's (f32, u8, counts) against ref_shade's (rgb, rgba8, counts, tallies)"""
    f32, u8, cnt = got
    rgb, r8, rcnt, _ = ref
    assert np.all(f32[:, 3] == 1.0)
    mism = int((f32[:, :3].view(np.uint32) != rgb.view(np.uint32)).any(axis=-1).sum())
    assert mism == 0, "%d rays differ in their float bits" % mism
    assert np.array_equal(u8, r8)
    assert np.array_equal(cnt, rcnt)


# ------------------------------------------------------------------------------------------------- 1. the fixtures against the reference
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
@pytest.mark.parametrize("name", ["tumbler", "overlap", "five-deep", "twins", "mirrored", "monkey"])
def test_a_fixture_equals_the_reference(gpu, name, max_reflect):
    """monkey: the open mesh alone, a scene without a top level (its row travels as a kernel argument, and it has no instance flags)"""
    sc, rays, ref = NH.fixture_ref(name, max_reflect)
    assert NH.fixture_condition(name, ref[3]), ref[3]
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    kw = dict(max_refract=8, max_reflect=max_reflect)
    got = gpu.shade_rays_nested(rays, rr.default_params(**kw), rgba8=True, ray_counts=True)
    check_rays(got, ref)
    tm = gpu.shade_rays_nested(rays, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), rgba8=True)
    assert tm[0].tobytes() == got[0].tobytes() and np.array_equal(tm[1], unorm8(ref[0], True))


@pytest.mark.parametrize("name", ["tumbler", "overlap"])
def test_render_nested_is_the_fold_of_the_reference(gpu, name):
    sc = NH.FIXTURES[name]()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    cam = view(*NH.VIEW, FW, FH)
    kw = dict(max_refract=8, max_reflect=3)
    for samples in (4, OFF3):
        offs = rr.sample_pattern(4) if isinstance(samples, int) else samples
        rgb, cnt = NH.ref_frame(sc, cam, FW, FH, offs, TABLE, **kw)
        assert (cnt > len(offs)).mean() > 0.05
        check(gpu.render_nested(FW, FH, cam, samples, rr.default_params(**kw), rgba8=True, ray_counts=True), rgb, cnt, False)
    check(gpu.render_nested(FW, FH, cam, OFF3, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), rgba8=True, ray_counts=True), rgb, cnt, True)


@pytest.mark.parametrize("T", [32765, 32766])
def test_nested_at_the_16_bit_stack_entry_limit(gpu, T):
    """test_gpu_materials.py's two overlapping instances of one 32 765 / 32 766-triangle mesh (16-bit stack entries, or 32-bit ones)
    under the nested tree"""
    inst = rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], xf(0.45, 0.1, 0.25, (1, 1, 1), 0.5)], meshes=[0, 0], masks=[1, 1],
                             materials=[1, 2])
    sc = EdgeScene("edge-nested-%d" % T, [mesh("soup", T)], EDGE_ENV, inst)
    sc.load_gpu(gpu)
    assert sc.n_tris() == T and len(sc.tlas) == 1 and (T + 2 >= 32768) == (T == 32766)
    gpu.set_materials(TABLE)
    rays = rr.camera_rays(edge_view(-np.pi / 2, W, H), W, H)
    kw = dict(max_refract=5)
    ref = NH.ref_shade(sc, rays, TABLE, use_bvh=1, **kw)
    print("%d triangles twice: %d of %d rays hit; %s" % (T, int((ref[2] > 1).sum()), len(rays), ref[3]))
    assert (ref[2] > 1).sum() > 100 and ref[3].interfaces > 0
    check_rays(gpu.shade_rays_nested(rays, rr.default_params(**kw), rgba8=True, ray_counts=True), ref)


# ------------------------------------------------------------------------------------------------- 2. the reduction
@pytest.mark.parametrize("scene", ["sphere.obj", "cube.obj", "shell.obj", "disjoint"])
def test_nested_is_materials_on_closed_disjoint_instances(gpu, scene):
    """byte for byte: colours, RGBA8 and ray counts, of rays and of frames, under a uniform and a mixed table.  The views are those on
    which the reference's tallies show no ray for which culling would matter (nested_helpers.REDUCTION_VIEWS; asserted here again for
    the rays, and in test_nested_cpu.py for the frames)"""
    sc = NH.reduction_scene(scene)
    sc.load_gpu(gpu)
    rays = rr.camera_rays(view(*NH.REDUCTION_VIEWS[scene]), W, H)
    fv, fml = (NH.DISJOINT_FRAME["view"], NH.DISJOINT_FRAME["max_reflect"]) if scene == "disjoint" else (NH.REDUCTION_VIEWS[scene], 3)
    cam = view(*fv, FW, FH)
    for table in (MH.uniform(1.5, 3), MH.MIXED):
        gpu.set_materials(table)
        for ml in (2, 3):
            kw = dict(max_refract=8, max_reflect=ml)
            assert NH.reduction_holds(NH.ref_shade(sc, rays, table, **kw)[3])
            for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
                p = rr.default_params(flags=flags, **kw)
                want = gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True)
                assert (want[2] > 1).mean() > 0.05
                same(gpu.shade_rays_nested(rays, p, rgba8=True, ray_counts=True), want)
        p = rr.default_params(max_refract=8, max_reflect=fml)
        want = gpu.render_materials(FW, FH, cam, 4, p, rgba8=True, ray_counts=True)
        assert (want[2] > 4).mean() > 0.05
        same(gpu.render_nested(FW, FH, cam, 4, p, rgba8=True, ray_counts=True), want)


# ------------------------------------------------------------------------------------------------- 3. the closed-form ray
def test_the_closed_form_ray_on_the_gpu(gpu):
    """env * (1 - R)^4 * exp(-sigma_A d_A) * exp(-sigma_B d_B), relative tolerance 1e-5 (test_nested_cpu.py derives it); the material
    tree is off by more than 1e-3 on the same ray"""
    sc, ray, want = NH.closed_form()
    sc.load_gpu(gpu)
    gpu.set_materials(NH.CF_TABLE)
    p = rr.default_params(max_refract=8, max_reflect=0)
    f32, cnt = gpu.shade_rays_nested(ray, p, ray_counts=True)
    print("closed form %s, shade_rays_nested %s" % (want.tolist(), f32[0, :3].tolist()))
    assert cnt[0] == 5
    assert np.all(np.abs(f32[0, :3].astype(np.float64) - want) <= 1e-5 * want)
    mat = gpu.shade_rays_materials(ray, p)
    assert np.all(np.abs(mat[0, :3].astype(np.float64) - want) > 1e-3 * want)


# ------------------------------------------------------------------------------------------------- 4. the device path and the state
def test_the_device_variants_equal_the_host_path(gpu):
    import torch
    sc = NH.tumbler()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    cam = view(*NH.VIEW, FW, FH)
    p = rr.default_params(max_refract=8, max_reflect=3)
    host = gpu.render_nested(FW, FH, cam, OFF3, p, rgba8=True, ray_counts=True)
    rays = rr.camera_rays(cam, FW, FH)
    hf, hc = gpu.shade_rays_nested(rays, p, ray_counts=True)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_nested(FW, FH, cam, OFF3, p, rgba8=True, ray_counts=True, device=True)
        t = torch.from_numpy(rays.view(np.int32).reshape(-1, 12).copy()).to("cuda:%d" % gpu.device)
        rf, rc = gpu.shade_rays_nested(t, p, ray_counts=True)
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
        assert rf.cpu().numpy().tobytes() == hf.tobytes() and np.array_equal(rc.cpu().numpy().view(np.uint32), hc)
    finally:
        gpu.reset_stream()


def test_a_new_table_takes_effect_and_the_context_is_left_alone(gpu):
    import torch
    # the tumbler under two tables, no rebuild in between
    sc, rays, ref = NH.fixture_ref("tumbler", 2)
    sc.load_gpu(gpu)
    kw = dict(max_refract=8, max_reflect=2)
    p = rr.default_params(**kw)
    gpu.set_materials(TABLE)
    first = gpu.shade_rays_nested(rays, p, rgba8=True, ray_counts=True)
    check_rays(first, ref)
    other = TABLE[::-1].copy()
    gpu.set_materials(other)
    second = gpu.shade_rays_nested(rays, p, rgba8=True, ray_counts=True)
    check_rays(second, NH.ref_shade(sc, rays, other, **kw))
    assert second[0].tobytes() != first[0].tobytes()
    # read_frame and stats() stay the last dispatch's
    gpu.load_scene(*load("monkey.obj"), env_map())
    w, h = 160, 120
    cam0, _, _ = view_constants(0.3, 0.4, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(cam0)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    before = {k: getattr(st, k) for k in STAT_FIELDS}
    assert before["rays"] > w * h
    cam2, _, _ = view_constants(2.0, 0.2, 90, 50)
    gpu.render_nested(90, 50, cam2, 2, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.render_nested(90, 50, cam2, 2, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True, device=True)
    gpu.shade_rays_nested(rr.camera_rays(cam2, 90, 50), rgba8=True, ray_counts=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


# ------------------------------------------------------------------------------------------------- 5. errors
def test_what_the_nested_calls_refuse(gpu):
    sc = NH.tumbler()
    fresh = rr.Renderer(gpu.device)
    try:
        rays = rr.camera_rays(view(*NH.VIEW), W, H)
        cam = view(*NH.VIEW, 8, 8)
        calls = (lambda: fresh.shade_rays_nested(rays), lambda: fresh.render_nested(8, 8, cam, 1), lambda: fresh.render_nested(8, 8, cam, 1, device=True))
        fresh.set_materials(TABLE)
        for call in calls:
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_STATE               # no TLAS yet
        sc.load_gpu(fresh)
        fresh.set_materials(None)
        for call in calls:
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_STATE, "no table"
        fresh.set_materials(TABLE[:3])                          # the small cube is made of row 3
        for call in calls:
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_INVALID_ARGUMENT
        fresh.set_materials(TABLE)
        assert fresh.shade_rays_nested(rays[:0]).shape == (0, 4)                # zero rays
        # row 255 of a 300-row table: a list entry cannot hold it, the material tree can
        long = np.zeros(300, rr.MATERIAL_DTYPE)
        long["ior"] = 1.3
        fresh.set_materials(long)
        ids = [fresh.upload_mesh(*load("cube.obj"))]
        fresh.build_blas(ids[0])
        for row, ok in ((254, True), (255, False)):
            fresh.build_tlas(rr.make_instances(transforms=[xf(0, 0, 0), xf(3, 0, 0)], meshes=[ids[0], ids[0]], materials=[0, row]))
            assert fresh.render_materials(8, 8, cam, 1).shape == (8, 8, 4)
            if ok:
                assert fresh.render_nested(8, 8, cam, 1).shape == (8, 8, 4) and fresh.shade_rays_nested(rays).shape == (len(rays), 4)
            else:
                for call in calls:
                    with pytest.raises(rr.RRError) as e:
                        call()
                    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 6. the demo
def test_rrdemo_nested_writes_render_nested_frames(gpu, tmp_path):
    """rrdemo --spp 2 --materials ... --nested: drawFrameNested end to end, its PPM against render_nested's RGBA8 store"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("shell.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "n_%03d.ppm")]
    out = subprocess.run(args + ["--spp", "2", "--materials", "1.5:0.8,0.1,0.1", "--nested"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "with 1 materials (nested media)" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "n_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    gpu.load_scene(*load("shell.obj"), env_rt)
    gpu.set_materials([(1.5, (0.8, 0.1, 0.1))])
    _, u8 = gpu.render_nested(64, 48, rr.camera_orbit(0.01), 2, rgba8=True)
    assert np.array_equal(img, u8[..., :3])
    assert subprocess.run(args + ["--nested"], capture_output=True, text=True, timeout=120).returncode == 2     # needs --materials
