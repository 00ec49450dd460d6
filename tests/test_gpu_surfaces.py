"""GPU: opaque hit groups (Renderer.set_surfaces, set_lights, shade_rays_surfaces, render_surfaces; rr_set_surfaces, rr_set_lights,
rr_shade_rays_surfaces[_device], rr_render_surfaces[_device]).

tests/native/surfaces_ref.c (surfaces_helpers.py) restates the tree of include/rrdxr.h and is compared bit for bit -- float colours,
RGBA8 and TraceRay counts, shadow rays included -- on fixtures each of which meets a condition read from the reference's tallies
(test_surfaces_cpu.py prints them).  Without a surface table, or with every row glass, the calls are their _nested twins byte for
byte."""
import numpy as np
import pytest

import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
import surfaces_helpers as SH
from materials_helpers import H, W, view
from nested_helpers import FH, FW, OFF3, TABLE
from scenes import gpu, load, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import STAT_FIELDS, env_map, unorm8, view_constants
from test_gpu_capacity_edges import ENV as EDGE_ENV
from test_gpu_capacity_edges import EdgeScene, mesh
from test_gpu_nested import check_rays, same
from test_gpu_samples import check
from test_gpu_stack_rungs import view as edge_view

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5
OUT = dict(rgba8=True, ray_counts=True)


# ------------------------------------------------------------------------------------------------- 1. the fixtures against the reference
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
@pytest.mark.parametrize("name", sorted(SH.FIXTURES))
def test_a_fixture_equals_the_reference(gpu, name, max_reflect):
    """alone: the open mesh without a top level -- its row travels as a kernel argument and its shadow rays test shadow_mask & 1"""
    fx, rays, ref = SH.fixture_ref(name, max_reflect)
    assert SH.fixture_condition(name, ref[3]), ref[3]
    fx.load(gpu)
    kw = dict(max_refract=8, max_reflect=max_reflect)
    got = gpu.shade_rays_surfaces(rays, rr.default_params(**kw), **OUT)
    check_rays(got, ref)
    tm = gpu.shade_rays_surfaces(rays, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), rgba8=True)
    assert tm[0].tobytes() == got[0].tobytes() and np.array_equal(tm[1], unorm8(ref[0], True))


@pytest.mark.parametrize("name", ["table", "mirror"])
def test_render_surfaces_is_the_fold_of_the_reference(gpu, name):
    """the built-in four samples and three offsets of the tests' own; RR_DISPATCH_DEBUG_NO_CULL gives the same frame"""
    fx = SH.FIXTURES[name]()
    fx.load(gpu)
    cam = view(*SH.VIEW, FW, FH)
    kw = dict(max_refract=8, max_reflect=3)
    for samples in (4, OFF3):
        offs = rr.sample_pattern(4) if isinstance(samples, int) else samples
        rgb, cnt = fx.frame(cam, FW, FH, offs, **kw)
        assert (cnt > len(offs)).mean() > 0.05
        got = gpu.render_surfaces(FW, FH, cam, samples, rr.default_params(**kw), **OUT)
        check(got, rgb, cnt, False)
        same(gpu.render_surfaces(FW, FH, cam, samples, rr.default_params(flags=rr.DISPATCH_DEBUG_NO_CULL, **kw), **OUT), got)
    check(gpu.render_surfaces(FW, FH, cam, OFF3, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), **OUT), rgb, cnt, True)


# ------------------------------------------------------------------------------------------------- 2. the reduction
@pytest.mark.parametrize("name", ["tumbler", "overlap", "five-deep"])
def test_without_opaque_rows_it_is_the_nested_tree(gpu, name):
    """byte for byte -- colours, RGBA8 and ray counts, of rays and of frames: with no surface table, and with an all-glass table while
    lights are set"""
    sc = NH.FIXTURES[name]()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    rays = rr.camera_rays(view(*NH.VIEW), W, H)
    cam = view(*NH.VIEW, FW, FH)
    lts = SH.lights(rr.directional_light(SH.SUN, (1, 1, 1)), rr.point_light(SH.LAMP_AT, (2, 2, 2), 0x01))
    for surf, lt, amb in ((None, None, None), (SH.surfaces(*[rr.glass()] * len(TABLE)), lts, (0.5, 0.5, 0.5))):
        gpu.set_surfaces(surf)
        gpu.set_lights(lt, amb)
        for ml in (2, 3):
            for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
                p = rr.default_params(flags=flags, max_refract=8, max_reflect=ml)
                want = gpu.shade_rays_nested(rays, p, **OUT)
                assert (want[2] > 1).mean() > 0.05
                same(gpu.shade_rays_surfaces(rays, p, **OUT), want)
        p = rr.default_params(max_refract=8, max_reflect=3)
        for samples in (4, OFF3):
            want = gpu.render_nested(FW, FH, cam, samples, p, **OUT)
            assert (want[2] > len(OFF3) + 1).mean() > 0.05
            same(gpu.render_surfaces(FW, FH, cam, samples, p, **OUT), want)


# ------------------------------------------------------------------------------------------------- 3. the stacks the shadow rays walk on
@pytest.mark.parametrize("T", [32765, 32766])
def test_surfaces_at_the_16_bit_stack_entry_limit(gpu, T):
    """test_gpu_nested.py's two overlapping instances of one 32 765 / 32 766-triangle mesh (16-bit stack entries, or 32-bit ones): the
    second opaque and a mirror, lit by two lights whose shadow rays walk the same hierarchy"""
    inst = rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], xf(0.45, 0.1, 0.25, (1, 1, 1), 0.5)], meshes=[0, 0], masks=[1, 2],
                             materials=[1, 2])
    sc = EdgeScene("edge-surfaces-%d" % T, [mesh("soup", T)], EDGE_ENV, inst)
    surf = SH.surfaces(rr.glass(), rr.glass(), rr.opaque((0.6, 0.5, 0.4), specular=(0.4, 0.4, 0.4)))
    lts = SH.lights(rr.directional_light((0.2, 0.3, -1.0), (1.0, 0.9, 0.8), 0xff), rr.point_light((0.5, 2.0, 3.0), (4.0, 4.0, 4.0), 0x01))
    fx = SH.Fixture(sc, surf, lts, (0.02, 0.03, 0.04))
    fx.load(gpu)
    assert sc.n_tris() == T and len(sc.tlas) == 1 and (T + 2 >= 32768) == (T == 32766)
    rays = rr.camera_rays(edge_view(-np.pi / 2, W, H), W, H)
    kw = dict(max_refract=5)
    ref = fx.ref(rays, use_bvh=1, **kw)
    print("%d triangles twice: %d of %d rays hit; %s" % (T, int((ref[2] > 1).sum()), len(rays), ref[3]))
    assert (ref[2] > 1).sum() > 100 and ref[3].shadow_occluded > 0 and ref[3].shadow_lit > 0 and ref[3].specular_children > 0
    check_rays(gpu.shade_rays_surfaces(rays, rr.default_params(**kw), **OUT), ref)


def test_surfaces_on_either_side_of_a_stack_rung(gpu):
    """depth_meshes' chains, as test_gpu_stack_rungs.py builds them: a tree at the top of the 19-entry rung and one at the bottom of the
    next, without a top level, the one instance an opaque mirror.  The first light grazes the sheets: its shadow rays run along the
    stack and across the sheets in front of the one they start on; the second faces them and is never occluded"""
    from test_gpu_stack_rungs import DEEP, assert_rung, chain_scene
    from test_gpu_stack_rungs import view as rung_view
    w, h = 48, 32
    cam = rung_view(DEEP, w, h)
    rays = rr.camera_rays(cam, w, h)
    surf = SH.surfaces(rr.opaque((0.6, 0.5, 0.4), specular=(0.5, 0.5, 0.5)))
    lts = SH.lights(rr.directional_light((1.0, 0.2, -0.02), (1.0, 0.9, 0.8), 0x01), rr.directional_light((-0.3, 0.2, -1.0), (0.5, 0.6, 0.7), 0xff))
    kw = dict(max_refract=5, max_reflect=2)
    for need in (19, 20):
        sc = chain_scene(need)
        fx = SH.Fixture(sc, surf, lts, (0.01, 0.01, 0.01))
        fx.load(gpu)
        assert_rung(gpu, sc, need, rays)
        ref = fx.ref(rays, **kw)
        print(need, ref[3])
        assert ref[3].shadow_occluded > 0 and ref[3].shadow_lit > 0 and ref[3].light_used[0] > 0 and ref[3].light_used[1] > 0
        check_rays(gpu.shade_rays_surfaces(rays, rr.default_params(**kw), **OUT), ref)


# ------------------------------------------------------------------------------------------------- 4. the tables
def test_new_tables_take_effect_without_a_rebuild(gpu):
    """a second surface table and a second light set; zero lights; eight lights; a light no instance meets"""
    fx, rays, ref = SH.fixture_ref("table", 2)
    fx.load(gpu)
    kw = dict(max_refract=8, max_reflect=2)
    p = rr.default_params(**kw)
    first = gpu.shade_rays_surfaces(rays, p, **OUT)
    check_rays(first, ref)
    # the floor a mirror, the occluder glass
    surf2 = SH.surfaces(rr.opaque((0.1, 0.1, 0.1), specular=(0.7, 0.6, 0.5)), rr.glass(), rr.glass())
    gpu.set_surfaces(surf2)
    second = gpu.shade_rays_surfaces(rays, p, **OUT)
    check_rays(second, SH.ref_shade(fx.scene, rays, TABLE, surf2, fx.lights, fx.ambient, **kw))
    assert second[0].tobytes() != first[0].tobytes()
    # zero lights: the ambient term alone, and no shadow ray
    gpu.set_lights(None, fx.ambient)
    none = SH.ref_shade(fx.scene, rays, TABLE, surf2, None, fx.ambient, **kw)
    assert none[3].shadow_traced == 0 and none[3].opaque_hits > 0
    check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), none)
    # eight lights of both kinds and several masks, no ambient term
    rng = np.random.default_rng(5)
    eight = SH.lights(*[rr.directional_light(rng.normal(size=3) + (0, 1.5, 0), rng.uniform(0.1, 0.6, 3), m) if k % 2 else
                        rr.point_light(rng.uniform(-1.5, 1.5, 3) + (0, 2.0, 0), rng.uniform(0.5, 2.0, 3), m)
                        for k, m in enumerate((0xff, 0x01, 0x02, 0x03, 0x80, 0xff, 0x01, 0x02))])
    gpu.set_surfaces(fx.surf)
    gpu.set_lights(eight)
    many = SH.ref_shade(fx.scene, rays, TABLE, fx.surf, eight, None, **kw)
    assert all(many[3].light_used[k] > 0 for k in range(8)) and many[3].light_occluded[4] == 0
    check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), many)
    # a light no instance meets: every shadow ray is counted and none is occluded
    lone = fx.lights.copy()
    lone["shadow_mask"] = 0x80
    gpu.set_lights(lone, fx.ambient)
    got = SH.ref_shade(fx.scene, rays, TABLE, fx.surf, lone, fx.ambient, **kw)
    assert got[3].shadow_occluded == 0 and got[3].shadow_traced == ref[3].shadow_traced
    check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), got)


def test_a_light_the_one_instance_does_not_meet(gpu):
    """without a top level the instance's mask is 1: shadow_mask 0x02 passes nothing, 0x03 passes it"""
    fx, rays, ref = SH.fixture_ref("alone", 2)
    fx.load(gpu)
    kw = dict(max_refract=8, max_reflect=2)
    for mask in (0x02, 0x03):
        lts = fx.lights.copy()
        lts["shadow_mask"] = mask
        gpu.set_lights(lts, fx.ambient)
        want = fx.ref(rays, lts, **kw)
        assert (want[3].shadow_occluded == 0) == (mask == 0x02) and want[3].shadow_traced == ref[3].shadow_traced
        check_rays(gpu.shade_rays_surfaces(rays, rr.default_params(**kw), **OUT), want)


# ------------------------------------------------------------------------------------------------- 5. the device path and the state
def test_the_device_variants_equal_the_host_path(gpu):
    import torch
    fx = SH.table()
    fx.load(gpu)
    cam = view(*SH.VIEW, FW, FH)
    p = rr.default_params(max_refract=8, max_reflect=3)
    host = gpu.render_surfaces(FW, FH, cam, OFF3, p, **OUT)
    rays = rr.camera_rays(cam, FW, FH)
    hf, hc = gpu.shade_rays_surfaces(rays, p, ray_counts=True)
    assert (hc > 1).mean() > 0.05
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_surfaces(FW, FH, cam, OFF3, p, device=True, **OUT)
        t = torch.from_numpy(rays.view(np.int32).reshape(-1, 12).copy()).to("cuda:%d" % gpu.device)
        rf, rc = gpu.shade_rays_surfaces(t, p, ray_counts=True)
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
        assert rf.cpu().numpy().tobytes() == hf.tobytes() and np.array_equal(rc.cpu().numpy().view(np.uint32), hc)
    finally:
        gpu.reset_stream()


def test_the_context_and_the_other_calls_are_left_alone(gpu):
    """the dispatch state (read_frame, stats()) stays the last dispatch's, and the _nested and _materials calls give what they gave before
    a surface table and lights were set"""
    import torch
    fx = SH.table()
    fx.scene.load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_surfaces(None)
    gpu.set_lights(None)
    rays = rr.camera_rays(view(*SH.VIEW), W, H)
    cam = view(*SH.VIEW, FW, FH)
    p = rr.default_params(max_refract=8, max_reflect=2)
    before = (gpu.shade_rays_nested(rays, p, **OUT), gpu.render_nested(FW, FH, cam, 2, p, **OUT), gpu.shade_rays_materials(rays, p, **OUT),
              gpu.render_materials(FW, FH, cam, 2, p, **OUT))
    w, h = 160, 120
    cam0, _, _ = view_constants(0.3, 0.4, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(cam0)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    stats = {k: getattr(st, k) for k in STAT_FIELDS}
    assert stats["rays"] > w * h
    gpu.set_surfaces(fx.surf)
    gpu.set_lights(fx.lights, fx.ambient)
    lit = gpu.shade_rays_surfaces(rays, p, **OUT)
    assert lit[0].tobytes() != before[0][0].tobytes()
    gpu.render_surfaces(90, 50, cam, 2, rr.default_params(max_refract=3, max_reflect=3), **OUT)
    gpu.render_surfaces(90, 50, cam, 2, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), device=True, **OUT)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == stats
    after = (gpu.shade_rays_nested(rays, p, **OUT), gpu.render_nested(FW, FH, cam, 2, p, **OUT), gpu.shade_rays_materials(rays, p, **OUT),
             gpu.render_materials(FW, FH, cam, 2, p, **OUT))
    for a, b in zip(after, before):
        same(a, b)
    # rr_set_materials neither reads nor clears the surface table
    gpu.set_materials(TABLE)
    same(gpu.shade_rays_surfaces(rays, p, **OUT), lit)


# ------------------------------------------------------------------------------------------------- 6. errors
def refused(call, status=RR_ERR_INVALID_ARGUMENT):
    with pytest.raises(rr.RRError) as e:
        call()
    assert e.value.status == status


def test_what_the_setters_refuse(gpu):
    """each refusal leaves the table in force, and a valid call follows it"""
    fx, rays, ref = SH.fixture_ref("table", 2)
    fx.load(gpu)
    p = rr.default_params(max_refract=8, max_reflect=2)

    def still_valid():
        check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), ref)

    def row(**kw):
        r = SH.surfaces(rr.opaque((0.5, 0.5, 0.5)))
        for k, v in kw.items():
            r[k] = v
        return r

    for bad in (row(kind=2), row(albedo=(0.1, -0.1, 0.1)), row(albedo=(np.nan, 0, 0)), row(emission=(0, np.inf, 0)), row(specular=(0, 0, -1e-3)),
                row(specular=(0, np.nan, 0))):
        refused(lambda: gpu.set_surfaces(np.concatenate([fx.surf, bad])))
        still_valid()
    gpu.set_surfaces(np.concatenate([fx.surf, row(emission=(-0.5, 0, 0))]))        # a negative emission is allowed
    still_valid()

    def light(**kw):
        r = SH.lights(rr.directional_light((0, 1, 0), (1, 1, 1)))
        for k, v in kw.items():
            r[k] = v
        return r

    for bad in (light(kind=2), light(v=(0, 0, 0)), light(v=(np.nan, 1, 0)), light(radiance=(np.inf, 0, 0)), light(shadow_mask=0x100),
                light(kind=rr.LIGHT_POINT, v=(0, np.inf, 0))):
        refused(lambda: gpu.set_lights(bad, fx.ambient))
        still_valid()
    refused(lambda: gpu.set_lights(fx.lights, (0, np.nan, 0)))
    still_valid()
    refused(lambda: gpu.set_lights(np.concatenate([fx.lights] * 5), fx.ambient))    # ten lights
    still_valid()
    gpu.set_lights(light(radiance=(-1, 0, 0), kind=rr.LIGHT_POINT, v=(0, 0, 0)), fx.ambient)    # a negative radiance and a point at the origin are allowed
    gpu.set_lights(fx.lights, fx.ambient)
    still_valid()


def test_what_the_surface_calls_refuse(gpu):
    """the state rules of the nested calls"""
    sc = NH.tumbler()
    fresh = rr.Renderer(gpu.device)
    try:
        rays = rr.camera_rays(view(*NH.VIEW), W, H)
        cam = view(*NH.VIEW, 8, 8)
        calls = (lambda: fresh.shade_rays_surfaces(rays), lambda: fresh.render_surfaces(8, 8, cam, 1), lambda: fresh.render_surfaces(8, 8, cam, 1, device=True))
        fresh.set_materials(TABLE)
        fresh.set_surfaces(SH.surfaces(rr.glass(), rr.opaque((1, 1, 1))))        # the setters need no scene
        fresh.set_lights(SH.lights(rr.point_light((0, 3, 0), (1, 1, 1))))
        for call in calls:
            refused(call, RR_ERR_STATE)                         # no TLAS yet
        sc.load_gpu(fresh)
        fresh.set_materials(None)
        for call in calls:
            refused(call, RR_ERR_STATE)                         # no material table, whatever the surface table says
        fresh.set_materials(TABLE[:3])                          # the small cube is made of row 3
        for call in calls:
            refused(call)
        fresh.set_materials(TABLE)
        assert fresh.shade_rays_surfaces(rays[:0]).shape == (0, 4)                # zero rays
        assert fresh.shade_rays_surfaces(rays).shape == (len(rays), 4)
        long = np.zeros(300, rr.MATERIAL_DTYPE)
        long["ior"] = 1.3
        fresh.set_materials(long)
        ids = [fresh.upload_mesh(*load("cube.obj"))]
        fresh.build_blas(ids[0])
        for r_, ok in ((254, True), (255, False)):
            fresh.build_tlas(rr.make_instances(transforms=[xf(0, 0, 0), xf(3, 0, 0)], meshes=[ids[0], ids[0]], materials=[0, r_]))
            if ok:
                assert fresh.render_surfaces(8, 8, cam, 1).shape == (8, 8, 4) and fresh.shade_rays_surfaces(rays).shape == (len(rays), 4)
            else:
                for call in calls:
                    refused(call)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 7. the demo
def test_rrdemo_floor_and_lights_write_render_surfaces_frames(gpu, tmp_path):
    """rrdemo --spp 2 --materials ... --nested --floor ... --light ...: its PPM against render_surfaces' RGBA8 store of the same scene"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("sphere.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "s_%03d.ppm")]
    glassy = ["--spp", "2", "--materials", "1.5:0.8,0.1,0.1", "--nested"]
    switches = ["--floor", "0.7,0.6,0.5:0.25", "--light", "0.3,1,0.2:1.2,1.1,0.9", "--light", "@1.5,2.5,-1:6,6,7"]
    out = subprocess.run(args + glassy + switches, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "on a floor under 2 lights" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "s_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    sphere, cube = load("sphere.obj"), load("cube.obj")
    ymin = float(sphere[0]["position"][sphere[1].astype(np.int64)][:, 1].min())
    ids = [gpu.upload_mesh(*sphere), gpu.upload_mesh(*cube)]
    for i in ids:
        gpu.build_blas(i)
    floor = np.array([[4, 0, 0, 0], [0, 0.1, 0, np.float32(ymin) - np.float32(0.15)], [0, 0, 4, 0]], np.float32)
    gpu.build_tlas(rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], floor], meshes=ids, materials=[0, 1]))
    gpu.upload_envmap(env_rt)
    gpu.set_materials([(1.5, (0.8, 0.1, 0.1)), (1.0, (0, 0, 0))])
    gpu.set_surfaces([rr.glass(), rr.opaque((0.7, 0.6, 0.5), specular=(0.25, 0.25, 0.25))])
    gpu.set_lights([rr.directional_light((0.3, 1, 0.2), (1.2, 1.1, 0.9)), rr.point_light((1.5, 2.5, -1), (6, 6, 7))], (0.05, 0.05, 0.05))
    _, u8, cnt = gpu.render_surfaces(64, 48, rr.camera_orbit(0.01), 2, **OUT)
    assert (cnt > 4).mean() > 0.2
    assert np.array_equal(img, u8[..., :3])
    for bad in (args + glassy[:4] + switches, args + ["--spp", "2"] + switches, args + glassy + ["--compose"] + switches,
                args + glassy + ["--light", "0,0,0:1,1,1"], args + glassy + ["--floor", "1,1"]):
        assert subprocess.run(bad, capture_output=True, text=True, timeout=120).returncode == 2
