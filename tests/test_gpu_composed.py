"""GPU: composed frames (Renderer.render_composed, set_material_bands; rr_render_composed[_device], rr_set_material_bands).

The contract is a fold: sample k is what shade_rays_nested gives the rays of lens_rays under band table T_band_k, weighted and summed
by render_spectral's rule.  It is checked bit for bit -- float colours, RGBA8 and TraceRay counts -- against that fold of the CPU
reference (tests/native/nested_ref.c through composed_helpers.py), against the same fold of the GPU's own shade_rays_nested, and
through its three reductions: to render_nested, and on a closed convex mesh to render_lens and render_spectral."""
import numpy as np
import pytest

import composed_helpers as CH
import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from composed_helpers import FH, FW, LENS
from materials_helpers import H, W, view
from nested_helpers import OFF3, TABLE
from scenes import gpu, load, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import STAT_FIELDS, env_map, view_constants
from test_gpu_samples import check

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5
OUT = dict(rgba8=True, ray_counts=True)


def same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def refused(call, status):
    with pytest.raises(rr.RRError) as e:
        call()
    assert e.value.status == status, e.value


# ------------------------------------------------------------------------------------------------- 1. the fold of the CPU reference
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
def test_composed_is_the_fold_of_the_reference(gpu, max_reflect):
    """the tumbler through a lens in two bands whose indices are out of order; the frame's last column of blocks lies outside the lens
    rectangle, so culled blocks are compared too"""
    sc, cam, recs, iors, weights, (rgb, cnt, _, tallies) = CH.tumbler_ref(max_reflect)
    assert (cnt > len(recs)).mean() > 0.05 and max(t.deepest for t in tallies) == 3
    assert rr.lens_screen_rect(sc.bounds, cam, LENS, FW, FH)[2] < FW
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    kw = dict(max_reflect=max_reflect, **CH.KW)
    got = gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    tm = gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), **OUT)
    check(tm, rgb, cnt, True)
    # the same samples through the other arguments: positions, paired band indices, the built-in lens points
    same(gpu.render_composed(FW, FH, cam, np.repeat(OFF3, 2, axis=0), lens=LENS, bands=CH.BAND_ORDER, paired=True, params=rr.default_params(**kw), **OUT), got)


def test_a_negative_weight(gpu):
    sc, cam, recs, iors, weights, (rgb, cnt, _, _) = CH.tumbler_ref(2, negative=True)
    assert weights[1, 2] < 0 and rgb.tobytes() != CH.tumbler_ref(2)[5][0].tobytes()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    check(gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=rr.default_params(max_reflect=2, **CH.KW), **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 2. the fold of the existing GPU calls
def test_composed_is_the_fold_of_shade_rays_nested(gpu):
    """the contract as the header words it, on two overlapping spheres: per sample set_materials(T_band), then shade_rays_nested on
    lens_rays"""
    sc = NH.overlap()
    sc.load_gpu(gpu)
    cam = view(*NH.VIEW, FW, FH)
    kw = dict(max_reflect=3, **CH.KW)
    p = rr.default_params(**kw)
    iors, weights = CH.fixture_bands()
    recs = CH.fixture_records()

    def shade(rays, t):
        gpu.set_materials(t)
        f, n = gpu.shade_rays_nested(rays, p, ray_counts=True)
        return f[:, :3], n, None
    rgb, cnt, cols, _ = CH.fold_samples(shade, cam, FW, FH, recs, LENS, TABLE, iors, weights, **kw)
    assert (cnt > len(recs)).mean() > 0.05 and cols[0].tobytes() != cols[1].tobytes()
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    check(gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=p, **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 3. a scene without a top level
def test_a_scene_without_a_top_level(gpu):
    """the open monkey alone: its row travels as a kernel argument, and every band's table is indexed with it"""
    sc = NH.alone("monkey.obj", 2)
    cam = view(*NH.VIEW, W, H)
    iors, weights = CH.fixture_bands()
    recs = CH.records(np.repeat(OFF3[:2], 2, axis=0), rr.lens_pattern(4), [1, 0, 0, 1])
    kw = dict(max_reflect=2, **CH.KW)
    rgb, cnt, cols, _ = CH.ref_composed(sc, cam, W, H, recs, LENS, TABLE, iors, weights, **kw)
    assert (cnt > len(recs)).mean() > 0.05 and cols[0].tobytes() != cols[1].tobytes()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    check(gpu.render_composed(W, H, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 4. the reductions
def test_without_lens_and_bands_it_is_render_nested(gpu):
    sc = NH.tumbler()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    cam = view(*NH.VIEW, FW, FH)
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        p = rr.default_params(max_refract=8, max_reflect=3, flags=flags)
        for samples in (4, OFF3):
            want = gpu.render_nested(FW, FH, cam, samples, p, **OUT)
            assert (want[2] > 4).mean() > 0.05
            gpu.set_material_bands(None)
            same(gpu.render_composed(FW, FH, cam, samples, params=p, **OUT), want)
            same(gpu.render_composed(FW, FH, cam, samples, lens=rr.Lens(0.0, 5.0), params=p, **OUT), want)      # radius 0: the pinhole
            gpu.set_material_bands(TABLE["ior"][None, :])       # one band that repeats the table, weights 1
            same(gpu.render_composed(FW, FH, cam, samples, params=p, **OUT), want)


def test_on_a_closed_convex_mesh_it_is_render_lens(gpu):
    """cube.obj of a clear row and no band set: render_lens under params.ior, byte for byte.  Culled and unculled TraceRay agree for
    every ray used: the reference's tallies say so"""
    recs = CH.cube_lens_records()
    assert all(NH.reduction_holds(t) for t in CH.cube_tallies(recs, LENS, None))
    sc = NH.reduction_scene("cube.obj")
    sc.load_gpu(gpu)
    gpu.set_materials(CH.CUBE_TABLE)
    cam = view(*CH.CUBE_VIEW, FW, FH)
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        want = gpu.render_lens(FW, FH, cam, LENS, 4, None, rr.default_params(ior=CH.CUBE_IOR, flags=flags, **CH.CUBE_KW), **OUT)
        assert (want[2] > 4).mean() > 0.05
        p = rr.default_params(flags=flags, **CH.CUBE_KW)
        same(gpu.render_composed(FW, FH, cam, 4, lens=LENS, params=p, **OUT), want)
        same(gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=p, **OUT), want)


def test_on_a_closed_convex_mesh_it_is_render_spectral(gpu):
    """the same cube, no lens, every row's index taken from rr_host_spectral_bands: render_spectral with that band table in the same
    sample order, byte for byte"""
    recs, bands, iors, weights = CH.cube_spectral()
    assert all(NH.reduction_holds(t) for t in CH.cube_tallies(recs, None, iors))
    sc = NH.reduction_scene("cube.obj")
    sc.load_gpu(gpu)
    gpu.set_materials(CH.CUBE_TABLE)
    gpu.set_material_bands(iors, weights)
    cam = view(*CH.CUBE_VIEW, FW, FH)
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        want = gpu.render_spectral(FW, FH, cam, 2, OFF3, rr.default_params(ior=CH.CUBE_IOR, flags=flags, **CH.CUBE_KW), abbe=CH.ABBE, **OUT)
        assert (want[2] > 6).mean() > 0.05
        p = rr.default_params(flags=flags, **CH.CUBE_KW)
        same(gpu.render_composed(FW, FH, cam, OFF3, bands=2, params=p, **OUT), want)
        same(gpu.render_composed(FW, FH, cam, recs, params=p, **OUT), want)
    gpu.set_material_bands(None)                                # and without the set the fringes are gone
    assert gpu.render_composed(FW, FH, cam, OFF3, params=p, **OUT)[0].tobytes() != want[0].tobytes()


# ------------------------------------------------------------------------------------------------- 5. culling
def test_culling_by_the_lens_rectangle_changes_no_byte(gpu):
    """a wide view in which the tumbler is a dozen pixels across: the lens rectangle, and the pinhole's, leave whole 8x8 blocks outside"""
    sc = NH.tumbler()
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    iors, weights = CH.fixture_bands()
    gpu.set_material_bands(iors, weights)
    cam = view(0.6, 2.0, FW, FH)
    lens = rr.Lens(0.6, 2.5)
    recs = CH.fixture_records()
    S = len(recs)
    rect = rr.lens_screen_rect(sc.bounds, cam, lens, FW, FH)
    pin = rr.lens_screen_rect(sc.bounds, cam, rr.Lens(0.0, 2.5), FW, FH)
    x0, y0 = (np.arange(FW) // 8) * 8, (np.arange(FH) // 8) * 8
    inside = ((y0 + 8 > rect[1]) & (y0 < rect[3]))[:, None] & ((x0 + 8 > rect[0]) & (x0 < rect[2]))[None, :]
    print("lens rectangle %s, pinhole rectangle %s: %d of %d pixels in culled blocks" % (rect, pin, int((~inside).sum()), FW * FH))
    assert (~inside).sum() >= 64 and inside.any()
    for lp, r in ((lens, rect), (None, pin)):
        culled = gpu.render_composed(FW, FH, cam, recs, lens=lp, params=rr.default_params(max_reflect=2, **CH.KW), **OUT)
        traced = gpu.render_composed(FW, FH, cam, recs, lens=lp, params=rr.default_params(max_reflect=2, flags=rr.DISPATCH_DEBUG_NO_CULL, **CH.KW), **OUT)
        same(culled, traced)
        ins = ((y0 + 8 > r[1]) & (y0 < r[3]))[:, None] & ((x0 + 8 > r[0]) & (x0 < r[2]))[None, :]
        assert np.all(culled[2][~ins] == S) and (culled[2] > S).any()       # one Miss per sample outside, the scene inside


# ------------------------------------------------------------------------------------------------- 6. the device path and the state
def test_the_device_variant_equals_the_host_path_and_the_context_is_left_alone(gpu):
    import torch
    sc, cam, recs, iors, weights, _ = CH.tumbler_ref(3)
    sc.load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    p = rr.default_params(max_reflect=3, **CH.KW)
    host = gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=p, **OUT)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_composed(FW, FH, cam, recs, lens=LENS, params=p, device=True, **OUT)
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
    finally:
        gpu.reset_stream()
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
    cam2, _, _ = view_constants(2.0, 0.2, W, H)
    gpu.set_materials(TABLE)
    gpu.set_tile_partition(1, 2)                                # ignored: the whole frame is rendered
    full = gpu.render_composed(W, H, cam2, 2, lens=LENS, params=rr.default_params(max_refract=3, max_reflect=3), **OUT)
    gpu.set_tile_partition(0, 1)
    same(gpu.render_composed(W, H, cam2, 2, lens=LENS, params=rr.default_params(max_refract=3, max_reflect=3), **OUT), full)
    gpu.render_composed(W, H, cam2, 2, params=rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), device=True, **OUT)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


# ------------------------------------------------------------------------------------------------- 7. state and refusals
def test_set_materials_clears_the_band_set(gpu):
    sc = NH.tumbler()
    sc.load_gpu(gpu)
    cam = view(*NH.VIEW, FW, FH)
    p = rr.default_params(max_reflect=2, **CH.KW)
    gpu.set_materials(TABLE)
    iors, weights = CH.fixture_bands()
    gpu.set_material_bands(iors, weights)
    assert gpu.render_composed(FW, FH, cam, OFF3, bands=[1, 1, 1], paired=True, params=p).shape == (FH, FW, 4)
    other = TABLE[::-1].copy()
    gpu.set_materials(other)
    refused(lambda: gpu.render_composed(FW, FH, cam, OFF3, bands=[0, 1, 0], paired=True, params=p), RR_ERR_INVALID_ARGUMENT)
    same(gpu.render_composed(FW, FH, cam, OFF3, params=p, **OUT), gpu.render_nested(FW, FH, cam, OFF3, p, **OUT))      # band 0: the new table
    # a set that is refused leaves the one in force alone
    gpu.set_material_bands(iors, weights)
    before = gpu.render_composed(FW, FH, cam, OFF3, bands=2, params=p, **OUT)
    for bad in (np.nan, np.inf, 0.0, -1.5):
        broken = iors.copy()
        broken[1, 3] = bad
        refused(lambda: gpu.set_material_bands(broken, weights), RR_ERR_INVALID_ARGUMENT)
    broken = weights.copy()
    broken[0, 1] = np.inf
    refused(lambda: gpu.set_material_bands(iors, broken), RR_ERR_INVALID_ARGUMENT)
    refused(lambda: gpu.set_material_bands(np.ones((65, len(TABLE)), np.float32)), RR_ERR_INVALID_ARGUMENT)
    same(gpu.render_composed(FW, FH, cam, OFF3, bands=2, params=p, **OUT), before)
    gpu.set_material_bands(None)                                # n_bands == 0 clears
    refused(lambda: gpu.render_composed(FW, FH, cam, OFF3, bands=2, params=p), RR_ERR_INVALID_ARGUMENT)


def test_what_the_composed_calls_refuse(gpu):
    sc = NH.tumbler()
    fresh = rr.Renderer(gpu.device)
    try:
        cam = view(*NH.VIEW, 8, 8)
        calls = (lambda: fresh.render_composed(8, 8, cam, 1), lambda: fresh.render_composed(8, 8, cam, 1, lens=LENS, device=True))
        refused(lambda: fresh.set_material_bands(np.ones((2, len(TABLE)), np.float32)), RR_ERR_STATE)      # no table
        fresh.set_materials(TABLE)
        for call in calls:
            refused(call, RR_ERR_STATE)                         # no TLAS yet
        sc.load_gpu(fresh)
        fresh.set_materials(None)
        for call in calls:
            refused(call, RR_ERR_STATE)                         # no table
        refused(lambda: fresh.set_material_bands(np.ones((2, len(TABLE)), np.float32)), RR_ERR_STATE)
        fresh.set_materials(TABLE[:3])                          # the small cube is made of row 3
        for call in calls:
            refused(call, RR_ERR_INVALID_ARGUMENT)
        fresh.set_materials(TABLE)
        iors, weights = CH.fixture_bands()
        fresh.set_material_bands(iors, weights)
        ok = CH.records(OFF3, rr.lens_pattern(3), [0, 1, 1])
        assert fresh.render_composed(8, 8, cam, ok, lens=LENS).shape == (8, 8, 4)

        def changed(field, k, value):
            r = ok.copy()
            r[field][k] = value
            return r
        refused(lambda: fresh.render_composed(8, 8, cam, changed("band", 2, 2), lens=LENS), RR_ERR_INVALID_ARGUMENT)      # a band beyond the set
        refused(lambda: fresh.render_composed(8, 8, cam, ok[:0], lens=LENS), RR_ERR_INVALID_ARGUMENT)
        refused(lambda: fresh.render_composed(8, 8, cam, np.zeros(65, rr.COMPOSED_SAMPLE_DTYPE), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        assert fresh.render_composed(8, 8, cam, np.zeros(64, rr.COMPOSED_SAMPLE_DTYPE), lens=LENS).shape == (8, 8, 4)
        for v in (-0.01, 1.01, np.nan):
            refused(lambda: fresh.render_composed(8, 8, cam, changed("offset", 1, (0.5, v)), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        for v in (-1.01, 1.01, np.nan):
            wide = changed("lens_offset", 1, (v, 0.0))
            refused(lambda: fresh.render_composed(8, 8, cam, wide, lens=LENS), RR_ERR_INVALID_ARGUMENT)
            # without a lens, or with radius 0, the lens offsets are not looked at; pad never is
            assert fresh.render_composed(8, 8, cam, wide).shape == (8, 8, 4)
            assert fresh.render_composed(8, 8, cam, wide, lens=rr.Lens(0.0, 5.0)).shape == (8, 8, 4)
        assert fresh.render_composed(8, 8, cam, changed("pad", 0, (7, 8, 9)), lens=LENS).tobytes() == fresh.render_composed(8, 8, cam, ok, lens=LENS).tobytes()
        refused(lambda: fresh.render_composed(8, 8, cam, ok, lens=rr.Lens(-1.0, 5.0)), RR_ERR_INVALID_ARGUMENT)
        refused(lambda: fresh.render_composed(8, 8, cam, ok, lens=rr.Lens(0.1, 0.0)), RR_ERR_INVALID_ARGUMENT)
        # row 255 of a 300-row table: a list entry cannot hold it
        long = np.zeros(300, rr.MATERIAL_DTYPE)
        long["ior"] = 1.3
        fresh.set_materials(long)
        ids = [fresh.upload_mesh(*load("cube.obj"))]
        fresh.build_blas(ids[0])
        for row, fine in ((254, True), (255, False)):
            fresh.build_tlas(rr.make_instances(transforms=[xf(0, 0, 0), xf(3, 0, 0)], meshes=[ids[0], ids[0]], materials=[0, row]))
            if fine:
                assert fresh.render_composed(8, 8, cam, 1).shape == (8, 8, 4)
            else:
                for call in calls:
                    refused(call, RR_ERR_INVALID_ARGUMENT)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 8. the demo
def test_rrdemo_compose_writes_render_composed_frames(gpu, tmp_path):
    """rrdemo --compose: drawFrameComposed end to end, its PPM against render_composed's RGBA8 store"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("shell.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "c_%03d.ppm")]
    out = subprocess.run(args + ["--compose", "--spp", "2", "--lens", "0.2:5", "--dispersion", "2:30", "--materials", "1.5:0.8,0.1,0.1", "--nested"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "composed frame: 2 positions x 2 bands" in out.stdout and "thin lens" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "c_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    gpu.load_scene(*load("shell.obj"), env_rt)
    table = [(1.5, (0.8, 0.1, 0.1))]
    gpu.set_materials(table)
    gpu.set_material_bands(*rr.material_bands(table, 30.0, 2))
    _, u8 = gpu.render_composed(64, 48, rr.camera_orbit(0.01), 2, lens=rr.Lens(0.2, 5.0), bands=2, rgba8=True)
    assert np.array_equal(img, u8[..., :3])
    assert subprocess.run(args + ["--compose", "--spp", "2", "--lens", "0.2:5"], capture_output=True, text=True, timeout=120).returncode == 2     # needs --materials
