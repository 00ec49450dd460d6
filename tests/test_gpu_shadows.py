"""GPU: transparent shadows (Renderer.set_shadow_steps; rr_set_shadow_steps, read by rr_shade_rays_surfaces[_device],
rr_render_surfaces[_device] and rr_render_lit[_device]).

tests/native/shadows_ref.c (shadows_helpers.py) restates the walk of include/rrdxr.h and is compared bit for bit -- float colours,
RGBA8 and TraceRay counts, every call of a walk counted -- on fixtures each of which meets a condition read from the reference's
tallies (test_shadows_cpu.py prints them).  With the setting at 0 or 1, and wherever no shadow ray's first hit is glass, the calls
give what they gave before the setting existed.  Frames are materials_helpers' 48 x 36."""
import numpy as np
import pytest

import lit_helpers as LH
import refraction_raytracing_dxr_amd as rr
import shadows_helpers as S
import surfaces_helpers as SH
from materials_helpers import H, W, view
from nested_helpers import OFF3
from scenes import gpu  # noqa: F401  (a fixture)
from test_gpu_nested import check_rays, same
from test_gpu_samples import check

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT = 1
OUT = dict(rgba8=True, ray_counts=True)
KW = dict(max_refract=8, max_reflect=2)
OFF2 = OFF3[:2]
_frames = {}


def frame_ref(name):
    """(Fixture, camera, the reference's two-sample frame) of a fixture, once per process"""
    if name not in _frames:
        fx = S.FIXTURES[name]()
        cam = view(*SH.VIEW, W, H)
        _frames[name] = (fx, cam, fx.frame(cam, W, H, OFF2, **KW))
    return _frames[name]


# ------------------------------------------------------------------------------------------------- 1. the fixtures against the reference
@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_shade_rays_surfaces_walks_as_the_reference(gpu, name):
    """host arrays and device memory; the eight-slot builds too"""
    import torch
    for ml in (2, 3):
        fx, rays, ref = S.fixture_ref(name, ml)
        assert S.fixture_condition(name, ref[3]), ref[3]
        fx.load(gpu)
        assert gpu.shadow_steps() == fx.k
        p = rr.default_params(max_refract=8, max_reflect=ml)
        check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), ref)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        t = torch.from_numpy(rays.view(np.int32).reshape(-1, 12).copy()).to("cuda:%d" % gpu.device)
        f, u, c = gpu.shade_rays_surfaces(t, p, **OUT)
        torch.cuda.current_stream().synchronize()
        check_rays((f.cpu().numpy(), u.cpu().numpy(), c.cpu().numpy().view(np.uint32)), ref)
    finally:
        gpu.reset_stream()


@pytest.mark.parametrize("name", ["tinted", "drink", "capped"])
def test_render_surfaces_is_the_fold_of_the_reference(gpu, name):
    """two samples per pixel, host and device=True; RR_DISPATCH_DEBUG_NO_CULL gives the same frame"""
    import torch
    fx, cam, (rgb, cnt, tl) = frame_ref(name)
    assert tl.walks > 0 and sum(tl.walk_calls[2:]) > 0 and (cnt > len(OFF2)).mean() > 0.05
    fx.load(gpu)
    p = rr.default_params(**KW)
    got = gpu.render_surfaces(W, H, cam, OFF2, p, **OUT)
    check(got, rgb, cnt, False)
    same(gpu.render_surfaces(W, H, cam, OFF2, rr.default_params(flags=rr.DISPATCH_DEBUG_NO_CULL, **KW), **OUT), got)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_surfaces(W, H, cam, OFF2, p, device=True, **OUT)
        torch.cuda.current_stream().synchronize()
        same((df.cpu().numpy(), du.cpu().numpy(), dc.cpu().numpy().view(np.uint32)), got)
    finally:
        gpu.reset_stream()


def test_one_instance_without_a_top_level(gpu):
    """alone: the open monkey, opaque, without a top level -- there is no glass for a walk to cross, so K = 8 gives the reference's
    frame and the GPU's own K = 0 frame, rays and counts included; a light whose mask misses the instance walks one call and is lit"""
    fx, rays, ref = SH.fixture_ref("alone", 2)
    fx.load(gpu)
    p = rr.default_params(**KW)
    gpu.set_shadow_steps(0)
    base = gpu.shade_rays_surfaces(rays, p, **OUT)
    check_rays(base, ref)
    gpu.set_shadow_steps(8)
    got = gpu.shade_rays_surfaces(rays, p, **OUT)
    same(got, base)
    check_rays(got, S.ref_shade(fx.scene, rays, fx.table, fx.surf, fx.lights, fx.ambient, 8, **KW))
    lts = fx.lights.copy()
    lts["shadow_mask"] = 0x02
    gpu.set_lights(lts, fx.ambient)
    want = S.ref_shade(fx.scene, rays, fx.table, fx.surf, lts, fx.ambient, 8, **KW)
    assert want[3].shadow_occluded == 0 and want[3].walks > 0 and want[3].walk_calls[1] == want[3].walks
    check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), want)
    gpu.set_shadow_steps(0)


# ------------------------------------------------------------------------------------------------- 2. the lit frames
LIT_SHAPES = LH.shapes(rr.light_shape((0.05, 0.0, 0.0), (0.0, 0.0, 0.08)), rr.light_shape((0.15, 0.0, 0.0), (0.0, 0.1, 0.0)))
LIT_OFFSETS = np.array([[-1.0, 0.5], [-1.0, 0.5], [0.75, -1.0], [0.75, -1.0]], np.float32)


def test_render_lit_walks_towards_the_moved_lights(gpu):
    """tinted as key 0, four records at two positions under two light offsets, a small shape per light, K = 8: the fold of the
    reference under rr.moved_lights per sample, and not the frame of K = 0"""
    fx = S.tinted(8)
    cam = view(*SH.VIEW, W, H)
    recs = LH.records(np.repeat(OFF2, 2, axis=0)[[0, 2, 1, 3]], None, 0, 0, LIT_OFFSETS)
    rgb, cnt, _, extras = S.ref_lit([fx.scene], cam, W, H, recs, None, fx.table, fx.surf, fx.lights, LIT_SHAPES, fx.ambient, 8, **KW)
    assert all(e[2].walk_lit_glass[2] > 0 for e in extras) and sum(e[2].walk_occluded_after_glass for e in extras) > 0
    assert extras[0][0].tobytes() != extras[2][0].tobytes()     # the two light offsets give the same position two colours
    gpu.release_scene_key()
    gpu.set_material_bands(None)
    fx.load(gpu)
    gpu.set_light_shapes(LIT_SHAPES)
    gpu.capture_scene_key(0)
    p = rr.default_params(**KW)
    try:
        got = gpu.render_lit(W, H, cam, recs, params=p, **OUT)
        check(got, rgb, cnt, False)
        check(gpu.render_lit(W, H, cam, recs, params=rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **KW), **OUT), rgb, cnt, True)
        gpu.set_shadow_steps(0)
        black = gpu.render_lit(W, H, cam, recs, params=p, **OUT)
        assert black[0].tobytes() != got[0].tobytes()
        rgb0, cnt0, _, _ = S.ref_lit([fx.scene], cam, W, H, recs, None, fx.table, fx.surf, fx.lights, LIT_SHAPES, fx.ambient, 0, **KW)
        check(black, rgb0, cnt0, False)
    finally:
        gpu.set_shadow_steps(0)
        gpu.set_light_shapes(None)
        gpu.release_scene_key()


# ------------------------------------------------------------------------------------------------- 3. the reductions on the GPU
@pytest.mark.parametrize("name", ["table", "olive"])
def test_zero_and_one_call_are_the_first_hit_shadow_ray(gpu, name):
    """against the GPU's own K = 0 output, which the surfaces reference pins: K = 1 byte for byte in rays and frames -- on table the
    sun does not see the sphere and the lamp does, on olive every shadow ray stops in the glass round the olive; and K = 0 set again
    after a larger cap is K = 0"""
    fx, rays, ref = SH.fixture_ref(name, 2)
    fx.load(gpu)
    cam = view(*SH.VIEW, W, H)
    p = rr.default_params(**KW)
    gpu.set_shadow_steps(0)
    base = gpu.shade_rays_surfaces(rays, p, **OUT)
    check_rays(base, ref)
    frame = gpu.render_surfaces(W, H, cam, OFF2, p, **OUT)
    try:
        gpu.set_shadow_steps(1)
        same(gpu.shade_rays_surfaces(rays, p, **OUT), base)
        same(gpu.render_surfaces(W, H, cam, OFF2, p, **OUT), frame)
        gpu.set_shadow_steps(8)
        walked = gpu.shade_rays_surfaces(rays, p, **OUT)
        check_rays(walked, S.ref_shade(fx.scene, rays, fx.table, fx.surf, fx.lights, fx.ambient, 8, **KW))
        assert walked[0].tobytes() != base[0].tobytes()         # glass stood in the way of some shadow ray
        # the other setters leave the cap alone
        gpu.set_lights(fx.lights, fx.ambient)
        gpu.set_surfaces(fx.surf)
        gpu.set_materials(fx.table)
        assert gpu.shadow_steps() == 8
        same(gpu.shade_rays_surfaces(rays, p, **OUT), walked)
        gpu.set_shadow_steps(0)
        same(gpu.shade_rays_surfaces(rays, p, **OUT), base)
        same(gpu.render_surfaces(W, H, cam, OFF2, p, **OUT), frame)
    finally:
        gpu.set_shadow_steps(0)


def test_the_nested_and_materials_calls_do_not_read_the_cap(gpu):
    fx = S.tinted(8)
    fx.scene.load_gpu(gpu)
    gpu.set_materials(fx.table)
    gpu.set_surfaces(fx.surf)
    gpu.set_lights(fx.lights, fx.ambient)
    rays = rr.camera_rays(view(*SH.VIEW), W, H)
    p = rr.default_params(**KW)
    gpu.set_shadow_steps(0)
    before = (gpu.shade_rays_nested(rays, p, **OUT), gpu.shade_rays_materials(rays, p, **OUT))
    try:
        gpu.set_shadow_steps(8)
        same(gpu.shade_rays_nested(rays, p, **OUT), before[0])
        same(gpu.shade_rays_materials(rays, p, **OUT), before[1])
    finally:
        gpu.set_shadow_steps(0)


# ------------------------------------------------------------------------------------------------- 4. the refusal
def test_seventeen_steps_are_refused_and_the_cap_in_force_stays(gpu):
    fx, rays, ref = S.fixture_ref("tinted", 2)
    fx.load(gpu)
    p = rr.default_params(**KW)
    assert rr.SHADOW_MAX_STEPS == 16
    try:
        for bad in (17, 64, 0xffffffff):
            with pytest.raises(rr.RRError) as e:
                gpu.set_shadow_steps(bad)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT
            assert "rr_set_shadow_steps: need k <= RR_SHADOW_MAX_STEPS (16)" in str(e.value)
            assert gpu.shadow_steps() == fx.k == 8
            check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), ref)
        gpu.set_shadow_steps(16)                                # the largest cap: the same walks, none of them longer than three calls
        assert gpu.shadow_steps() == 16
        check_rays(gpu.shade_rays_surfaces(rays, p, **OUT), ref)
        fresh = rr.Renderer(gpu.device)
        try:
            assert fresh.shadow_steps() == 0                    # the setting after rr_create
        finally:
            fresh.close()
    finally:
        gpu.set_shadow_steps(0)
