"""GPU: per-instance glass (Renderer.set_materials, shade_rays_materials, render_materials; rr_set_materials,
rr_shade_rays_materials[_device], rr_render_materials[_device]).

Two references.  With a table whose rows are all { ior, 0, 0, 0 } the calls are shade_rays / render_samples under that ior, byte for
byte: entry points that test_gpu_shade.py and test_gpu_samples.py pin to the CPU oracle.  With a mixed table -- three indices of
refraction, two of the glasses tinted -- the reference is tests/native/materials_ref.c (materials_helpers.py), which
test_materials_cpu.py proves against the oracle for uniform tables: float bits, RGBA8 and TraceRay counts of every ray, no tolerance."""
import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from materials_helpers import H, MIXED, VIEW3, W, monkey_scene, ref_frame, ref_shade, three_scene, uniform, view
from scenes import gpu, load, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import OFFP16, STAT_FIELDS, env_map, unorm8, view_constants
from test_gpu_capacity_edges import ENV as EDGE_ENV
from test_gpu_capacity_edges import EdgeScene, mesh
from test_gpu_samples import check
from test_gpu_stack_rungs import view as edge_view

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5
FW, FH = 50, 38                                             # not multiples of 8: partial blocks on two edges
OFF3 = np.array([[0.125, 0.75], [0.5, 0.0], [1.0, 0.4375]], np.float32)     # three offsets of the tests' own, the edges of the range among them


def same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_rays(got, ref):
    """shade_rays_materials' (f32, u8, counts) against ref_shade's (rgb, rgba8, counts, absorbed)"""
    f32, u8, cnt = got
    rgb, r8, rcnt, _ = ref
    assert np.all(f32[:, 3] == 1.0)
    mism = int((f32[:, :3].view(np.uint32) != rgb.view(np.uint32)).any(axis=-1).sum())
    assert mism == 0, "%d rays differ in their float bits" % mism
    assert np.array_equal(u8, r8)
    assert np.array_equal(cnt, rcnt)


# ------------------------------------------------------------------------------------------------- 1. a uniform table is the scalar call
@pytest.mark.parametrize("scene", ["monkey", "three"])
def test_uniform_table_shade_rays_materials_is_shade_rays(gpu, scene):
    sc = monkey_scene() if scene == "monkey" else three_scene()
    sc.load_gpu(gpu)
    rays = rr.camera_rays(view(*VIEW3), W, H)
    for ior in (1.3, 1.5):
        gpu.set_materials(uniform(ior, 3))
        for ml in (2, 3):
            for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
                want = gpu.shade_rays(rays, rr.default_params(flags=flags, max_refract=8, max_reflect=ml, ior=ior), rgba8=True, ray_counts=True)
                assert (want[2] > 1).mean() > 0.05
                # params.ior is ignored: left at its default, and at a value no glass has
                for pior in (1.3, 7.0):
                    got = gpu.shade_rays_materials(rays, rr.default_params(flags=flags, max_refract=8, max_reflect=ml, ior=pior), rgba8=True, ray_counts=True)
                    same(got, want)


@pytest.mark.parametrize("scene", ["monkey", "three"])
def test_uniform_table_render_materials_is_render_samples(gpu, scene):
    sc = monkey_scene() if scene == "monkey" else three_scene()
    sc.load_gpu(gpu)
    cam = view(*VIEW3, FW, FH)
    for ior in (1.3, 1.5):
        gpu.set_materials(uniform(ior, 3))
        for samples in (1, 4, OFF3):
            n = samples if isinstance(samples, int) else len(samples)
            for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
                p = rr.default_params(flags=flags, max_refract=8, max_reflect=3, ior=ior)
                want = gpu.render_samples(FW, FH, cam, samples, p, rgba8=True, ray_counts=True)
                assert (want[2] > n).mean() > 0.05
                same(gpu.render_materials(FW, FH, cam, samples, rr.default_params(flags=flags, max_refract=8, max_reflect=3), rgba8=True,
                                          ray_counts=True), want)


# ------------------------------------------------------------------------------------------------- 2. the mixed table against the reference
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
def test_mixed_table_equals_the_reference(gpu, max_reflect):
    sc = three_scene()
    sc.load_gpu(gpu)
    gpu.set_materials(MIXED)
    rays = rr.camera_rays(view(*VIEW3), W, H)
    kw = dict(max_refract=8, max_reflect=max_reflect)
    ref = ref_shade(sc, rays, MIXED, **kw)
    # the condition the view was chosen for (test_materials_cpu.py prints the figures): every glass absorbs, no uniform table explains the frame
    assert np.all(ref[3] >= 1), ref[3]
    for ior in MIXED["ior"]:
        assert (ref_shade(sc, rays, uniform(ior, 3), **kw)[2] != ref[2]).sum() >= 1
    got = gpu.shade_rays_materials(rays, rr.default_params(**kw), rgba8=True, ray_counts=True)
    check_rays(got, ref)
    tm = gpu.shade_rays_materials(rays, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), rgba8=True)
    assert tm[0].tobytes() == got[0].tobytes() and np.array_equal(tm[1], unorm8(ref[0], True))
    # the frame: four samples through the same trees
    cam = view(*VIEW3, FW, FH)
    rgb, cnt, _ = ref_frame(sc, cam, FW, FH, rr.sample_pattern(4), MIXED, **kw)
    check(gpu.render_materials(FW, FH, cam, 4, rr.default_params(**kw), rgba8=True, ray_counts=True), rgb, cnt, False)


def test_mixed_table_on_a_scene_without_a_top_level(gpu):
    """one identity instance made of row 2: the index travels as a kernel argument"""
    sc = monkey_scene(2)
    sc.load_gpu(gpu)
    gpu.set_materials(MIXED)
    rays = rr.camera_rays(view(*VIEW3), W, H)
    for ml in (2, 3):
        kw = dict(max_refract=8, max_reflect=ml)
        ref = ref_shade(sc, rays, MIXED, **kw)
        assert ref[3][2] > 100 and ref[3][0] == 0 and ref[3][1] == 0
        check_rays(gpu.shade_rays_materials(rays, rr.default_params(**kw), rgba8=True, ray_counts=True), ref)
        assert (ref[0] != ref_shade(monkey_scene(), rays, MIXED, **kw)[0]).any()        # row 2 is not row 0


@pytest.mark.parametrize("T", [32765, 32766])
def test_mixed_table_at_the_16_bit_stack_entry_limit(gpu, T):
    """two overlapping instances of one mesh, of different glass, whose pool holds 32 767 references (16-bit stack entries) or 32 768
    (32-bit ones): test_gpu_capacity_edges.py's scene with materials"""
    inst = rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], xf(0.45, 0.1, 0.25, (1, 1, 1), 0.5)], meshes=[0, 0], masks=[1, 1],
                             materials=[1, 2])
    sc = EdgeScene("edge-materials-%d" % T, [mesh("soup", T)], EDGE_ENV, inst)
    sc.load_gpu(gpu)
    assert sc.n_tris() == T and len(sc.tlas) == 1 and (T + 2 >= 32768) == (T == 32766)
    gpu.set_materials(MIXED)
    rays = rr.camera_rays(edge_view(-np.pi / 2, W, H), W, H)
    kw = dict(max_refract=5)
    ref = ref_shade(sc, rays, MIXED, use_bvh=1, **kw)
    print("%d triangles twice: %d of %d rays hit, inside hits absorbed at per material %s" % (T, int((ref[2] > 1).sum()), len(rays), ref[3].tolist()))
    assert (ref[2] > 1).sum() > 100 and ref[3][1] >= 1 and ref[3][2] >= 1 and ref[3][0] == 0
    check_rays(gpu.shade_rays_materials(rays, rr.default_params(**kw), rgba8=True, ray_counts=True), ref)


# ------------------------------------------------------------------------------------------------- 3. composition
def test_render_materials_is_the_fold_of_shade_rays_materials(gpu):
    import torch
    sc = three_scene()
    sc.load_gpu(gpu)
    gpu.set_materials(MIXED)
    cam = view(*VIEW3, FW, FH)
    offs = OFFP16[:5]
    host = None
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        p = rr.default_params(flags=flags, max_refract=8, max_reflect=3)
        cols, total = [], np.zeros(FW * FH, np.uint32)
        for ox, oy in offs:
            f, n = gpu.shade_rays_materials(rr.camera_rays(cam, FW, FH, float(ox), float(oy), p.tmin_primary, p.tmax_primary), p, ray_counts=True)
            cols.append(f[:, :3])
            total += n
        s = cols[0].copy()
        for c in cols[1:]:
            s = s + c
        rgb = (s / np.float32(len(cols))).reshape(FH, FW, 3)
        host = gpu.render_materials(FW, FH, cam, offs, p, rgba8=True, ray_counts=True)
        check(host, rgb, total.reshape(FH, FW), flags != 0)
    assert (host[2] > len(offs)).mean() > 0.05
    # the device variant on the renderer's stream, and device rays
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_materials(FW, FH, cam, offs, p, rgba8=True, ray_counts=True, device=True)
        rays = rr.camera_rays(cam, FW, FH)
        t = torch.from_numpy(rays.view(np.int32).reshape(-1, 12).copy()).to("cuda:%d" % gpu.device)
        rf, rc = gpu.shade_rays_materials(t, p, ray_counts=True)
        total = df.sum()                                        # queued behind the frame on the same stream
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
        hf, hc = gpu.shade_rays_materials(rays, p, ray_counts=True)
        assert rf.cpu().numpy().tobytes() == hf.tobytes() and np.array_equal(rc.cpu().numpy().view(np.uint32), hc)
        assert np.isfinite(float(total))
    finally:
        gpu.reset_stream()


# ------------------------------------------------------------------------------------------------- 4. state
def test_no_table_and_bad_tables_are_refused(gpu):
    sc = three_scene()
    fresh = rr.Renderer(gpu.device)
    try:
        rays = rr.camera_rays(view(*VIEW3), W, H)
        cam = view(*VIEW3, 8, 8)
        fresh.set_materials(MIXED)                              # a table may come before the scene
        for call in (lambda: fresh.shade_rays_materials(rays), lambda: fresh.render_materials(8, 8, cam, 1),
                     lambda: fresh.render_materials(8, 8, cam, 1, device=True)):
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_STATE               # no TLAS yet
        sc.load_gpu(fresh)
        ref = ref_shade(sc, rays, MIXED, max_refract=8)
        p = rr.default_params(max_refract=8)
        check_rays(fresh.shade_rays_materials(rays, p, rgba8=True, ray_counts=True), ref)       # the table set before the build is in force
        for clear in (None, MIXED[:0]):
            fresh.set_materials(clear)
            for call in (lambda: fresh.shade_rays_materials(rays), lambda: fresh.render_materials(8, 8, cam, 1),
                         lambda: fresh.render_materials(8, 8, cam, 1, device=True)):
                with pytest.raises(rr.RRError) as e:
                    call()
                assert e.value.status == RR_ERR_STATE, "no table"
            fresh.set_materials(MIXED)
        fresh.set_materials(MIXED[:2])                          # instance 2 is made of row 2
        for call in (lambda: fresh.shade_rays_materials(rays), lambda: fresh.render_materials(8, 8, cam, 1)):
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_INVALID_ARGUMENT
        fresh.set_materials(MIXED)
        nan, inf = float("nan"), float("inf")
        for field, k, bad in [("ior", None, v) for v in (0.0, -1.3, nan, inf, -inf)] + [("sigma_a", ch, v) for ch in range(3) for v in (-0.5, nan, inf, -inf)]:
            t = MIXED.copy()
            if k is None:
                t[field][1] = bad
            else:
                t[field][1, k] = bad
            with pytest.raises(rr.RRError) as e:
                fresh.set_materials(t)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, (field, k, bad)
        t = MIXED.copy()
        t["sigma_a"][0] = (-0.0, 0.0, 1e30)                     # a zero of either sign and a huge coefficient are allowed
        fresh.set_materials(t)
        fresh.set_materials(MIXED)
        assert rr.lib().rr_set_materials(fresh._h, None, 3) == RR_ERR_INVALID_ARGUMENT
        check_rays(fresh.shade_rays_materials(rays, p, rgba8=True, ray_counts=True), ref)       # a refused table leaves the one in force
    finally:
        fresh.close()


def test_a_new_table_and_a_refit_take_effect_without_a_rebuild(gpu):
    sc = three_scene()
    ids = []
    for v, i in sc.meshes:
        ids.append(gpu.upload_mesh(v, i))
        gpu.build_blas(ids[-1])
    inst = sc.instances.copy()
    inst["blas"] = [ids[int(b)] for b in sc.instances["blas"]]
    gpu.build_tlas(inst, allow_update=True)
    gpu.upload_envmap(sc.env)
    rays = rr.camera_rays(view(*VIEW3), W, H)
    kw = dict(max_refract=8, max_reflect=2)
    p = rr.default_params(**kw)
    gpu.set_materials(MIXED)
    first = gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True)
    check_rays(first, ref_shade(sc, rays, MIXED, **kw))
    # a second table: the next call sees it
    other = MIXED[::-1].copy()
    other["sigma_a"][1] = (0.0, 1.5, 0.25)
    gpu.set_materials(other)
    second = gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True)
    check_rays(second, ref_shade(sc, rays, other, **kw))
    assert second[0].tobytes() != first[0].tobytes() and (second[2] != first[2]).any()
    # a longer table after a shorter one (the device buffer grows)
    gpu.set_materials(uniform(1.3, 1)[:1])
    longer = np.concatenate([other, MIXED, other])
    gpu.set_materials(longer)
    check_rays(gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True), ref_shade(sc, rays, other, **kw))
    # a refit that changes nothing but the indices
    swapped = three_scene((2, 0, 1))
    assert np.array_equal(swapped.instances["transform"], sc.instances["transform"])
    inst["hitgroup_flags"] = swapped.instances["hitgroup_flags"]
    gpu.build_tlas(inst, update=True)
    third = gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True)
    check_rays(third, ref_shade(swapped, rays, longer, **kw))
    assert third[0].tobytes() != second[0].tobytes()
    inst["hitgroup_flags"] = (inst["hitgroup_flags"] & 0xff000000) | 9        # every instance made of row 9, past the table's nine rows
    gpu.build_tlas(inst, update=True)
    with pytest.raises(rr.RRError) as e:
        gpu.shade_rays_materials(rays, p)
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    inst["hitgroup_flags"] = (inst["hitgroup_flags"] & 0xff000000) | 8        # the last row
    gpu.build_tlas(inst, update=True)
    check_rays(gpu.shade_rays_materials(rays, p, rgba8=True, ray_counts=True), ref_shade(three_scene((8, 8, 8)), rays, longer, **kw))


def test_material_calls_leave_the_context_alone(gpu):
    import torch
    gpu.load_scene(*load("monkey.obj"), env_map())
    w, h = 160, 120
    sc, _, _ = view_constants(0.3, 0.4, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    before = {k: getattr(st, k) for k in STAT_FIELDS}
    assert before["rays"] > w * h
    gpu.set_materials(MIXED)
    sc2, _, _ = view_constants(2.0, 0.2, 90, 50)
    gpu.render_materials(90, 50, sc2, 2, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.render_materials(90, 50, sc2, 2, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True, device=True)
    gpu.shade_rays_materials(rr.camera_rays(sc2, 90, 50), rgba8=True, ray_counts=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before
    # and the scalar calls do not see the table
    rays = rr.camera_rays(sc2, 90, 50)
    plain = gpu.shade_rays(rays, rr.default_params(max_refract=8))
    gpu.set_materials(None)
    assert gpu.shade_rays(rays, rr.default_params(max_refract=8)).tobytes() == plain.tobytes()


# ------------------------------------------------------------------------------------------------- 5. the demo
def test_rrdemo_materials_writes_render_materials_frames(gpu, tmp_path):
    """rrdemo --spp 2 --materials ...: the C++ host's setMaterials and drawFrameMaterials end to end, its PPM against render_materials'
    RGBA8 store; the demo's one instance is made of row 0"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("cube.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "m_%03d.ppm")]
    out = subprocess.run(args + ["--spp", "2", "--materials", "1.5:0.8,0.1,0.1;1.3:0,0,0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "2 samples per pixel with 2 materials" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "m_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    gpu.load_scene(*load("cube.obj"), env_rt)
    gpu.set_materials([(1.5, (0.8, 0.1, 0.1)), (1.3, (0.0, 0.0, 0.0))])
    _, u8 = gpu.render_materials(64, 48, rr.camera_orbit(0.01), 2, rgba8=True)
    assert np.array_equal(img, u8[..., :3])
    _, plain = gpu.render_samples(64, 48, rr.camera_orbit(0.01), 2, rr.default_params(ior=1.5), rgba8=True)
    assert not np.array_equal(img, plain[..., :3])              # the tint shows
    for bad in (["--materials", ""], ["--materials", "1.5"], ["--materials", "0:0,0,0"], ["--materials", "1.5:-1,0,0"], ["--materials", "1.5:0,0,0;"
                 "x"], ["--materials", "1.5:0,0,0,0"], ["--spp", "4", "--lens", "0.2:5", "--materials", "1.5:0,0,0"],
                ["--dispersion", "4", "--materials", "1.5:0,0,0"], ["--pump", "--materials", "1.5:0,0,0"]):
        assert subprocess.run(args + bad, capture_output=True, text=True, timeout=120).returncode == 2, bad
