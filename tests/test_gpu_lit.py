"""GPU: lit shutter frames (Renderer.set_light_shapes, render_lit; rr_set_light_shapes, rr_render_lit[_device]).

The contract is the shutter frame's fold over the surface tree with the lights of each sample: sample k is what shade_rays_surfaces
gives the rays of lens_rays in the scene captured as key_k under band table T_band_k, the surface table and ambient term in force and
the lights rr.moved_lights(lights, shapes, *light_offset_k), weighted and summed by render_shutter's rule.  It is checked bit for bit
-- float colours, RGBA8 (tone-mapped too) and TraceRay counts -- against that fold of the CPU reference (tests/native/surfaces_ref.c
through lit_helpers.py), against the same fold of the GPU's own shade_rays_surfaces in the live scenes, and through its reductions to
render_shutter and render_surfaces.  Frames are 48 x 36, or 50 x 38 where an edge block matters, with at most eight samples."""
import ctypes as C

import numpy as np
import pytest

import composed_helpers as CH
import lit_helpers as LH
import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as KH
import surfaces_helpers as SH
from composed_helpers import LENS
from lit_helpers import H, W
from nested_helpers import FH, FW, OFF3, TABLE
from scenes import Scene, gpu, load  # noqa: F401  (gpu: a fixture)
from spectral_helpers import weighted_fold
from test_gpu_samples import check
from test_gpu_shutter import refused, same, small_cube

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5
OUT = dict(rgba8=True, ray_counts=True)
REINHARD, NO_CULL = rr.DISPATCH_TONEMAP_REINHARD, rr.DISPATCH_DEBUG_NO_CULL


def clean(r):
    """the module's renderer without what an earlier test left: keys, bands, surfaces, lights and shapes"""
    r.release_scene_key()
    r.set_material_bands(None)
    r.set_surfaces(None)
    r.set_lights(None)


def key0(r, fx):
    clean(r)
    fx.load(r)
    r.capture_scene_key(0)


# ------------------------------------------------------------------------------------------------- 1. soft shadows, the CPU's fold
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
def test_soft_shadows_are_the_fold_of_the_reference(gpu, max_reflect):
    """the four corners of the lamp at the pixel centres: test_lit_cpu.py asserts that the reference has pixels occluded under some
    offsets and not under others, so a kernel that ignores the offsets cannot pass"""
    fx, cam, recs, (rgb, cnt, _, _) = LH.soft_ref(max_reflect)
    key0(gpu, fx)
    kw = dict(max_reflect=max_reflect, **LH.KW)
    got = gpu.render_lit(W, H, cam, recs, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    check(gpu.render_lit(W, H, cam, recs, params=rr.default_params(flags=REINHARD, **kw), **OUT), rgb, cnt, True)
    same(gpu.render_lit(W, H, cam, recs, params=rr.default_params(flags=NO_CULL, **kw), **OUT), got)
    # the same samples through the other arguments
    same(gpu.render_lit(W, H, cam, [(0.5, 0.5)] * 4, keys=[0] * 4, light_samples=LH.SOFT_OFFSETS, paired=True, params=rr.default_params(**kw), **OUT), got)
    # without the shapes the four samples are one, and it is render_surfaces' pixel centre
    gpu.set_light_shapes(None)
    same(gpu.render_lit(W, H, cam, recs, params=rr.default_params(**kw), **OUT),
         gpu.render_surfaces(W, H, cam, [(0.5, 0.5)] * 4, params=rr.default_params(**kw), **OUT))


@pytest.mark.parametrize("sun", [False, True])
def test_soft_shadows_through_a_lens_in_two_bands(gpu, sun):
    """a lens, two bands and four distinct positions, the records out of order, on the frame with partial blocks; sun: the table's
    directional light beside the lamp, with a shape of its own"""
    fx = LH.soft(sun)
    cam = LH.soft_view(FW, FH)
    iors, weights = CH.fixture_bands()
    pos = np.array([[0.125, 0.75], [0.5, 0.0], [1.0, 0.4375], [0.3, 0.9]], np.float32)
    order = [2, 0, 3, 1]
    recs = LH.records(pos[order], rr.lens_pattern(4)[[1, 3, 0, 2]], [1, 0, 0, 1], 0, LH.SOFT_OFFSETS[order])
    kw = dict(max_reflect=2, **LH.KW)
    rgb, cnt, _, extras = fx.lit(cam, FW, FH, recs, LENS, iors, weights, **kw)
    assert sum(e[2].shadow_occluded for e in extras) > 0 and sum(e[2].shadow_lit for e in extras) > 0
    if sun:
        assert all(e[2].light_used[0] > 0 and e[2].light_used[1] > 0 for e in extras)
    key0(gpu, fx)
    gpu.set_material_bands(iors, weights)
    got = gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    check(gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=REINHARD, **kw), **OUT), rgb, cnt, True)
    same(gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=NO_CULL, **kw), **OUT), got)


# ------------------------------------------------------------------------------------------------- 2. the fold of the GPU's own calls
def test_lit_is_the_fold_of_shade_rays_surfaces_in_the_live_scenes(gpu):
    """the contract as the header words it: per key the scene live, per sample set_materials(T_band), set_lights(moved_lights(...)) and
    shade_rays_surfaces on lens_rays; then the live scene becomes something else entirely and render_lit still gives that fold"""
    fx, scs = LH.moving_olive()
    cam = MH.view(*KH.VIEW, FW, FH)
    kw = dict(max_reflect=3, **LH.KW)
    p = rr.default_params(**kw)
    iors, weights = CH.fixture_bands()
    recs = LH.olive_records()
    recs["band"] = [1, 0, 0, 1, 1, 0]
    clean(gpu)
    gpu.set_surfaces(fx.surf)
    cols, total = [None] * len(recs), np.zeros(FW * FH, np.uint32)
    for j, sc in enumerate(scs):
        sc.load_gpu(gpu)
        for k, rec in enumerate(recs):
            if int(rec["key"]) != j:
                continue
            gpu.set_materials(CH.band_table(TABLE, iors, int(rec["band"])))
            gpu.set_lights(rr.moved_lights(fx.lights, fx.shapes, *rec["light_offset"]), fx.ambient)
            f, n = gpu.shade_rays_surfaces(CH.sample_rays(cam, FW, FH, rec, LENS, p), p, ray_counts=True)
            cols[k] = np.ascontiguousarray(f[:, :3]).reshape(FH, FW, 3)
            total += n
        gpu.capture_scene_key(j)
    rgb, cnt = weighted_fold(cols, [weights[int(r["band"])] for r in recs]), total.reshape(FH, FW)
    assert (cnt > len(recs)).mean() > 0.05 and cols[0].tobytes() != cols[1].tobytes()
    small_cube().load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    gpu.set_lights(fx.lights, fx.ambient)
    gpu.set_light_shapes(fx.shapes)
    check(gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=p, **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 3. the reductions
@pytest.mark.parametrize("fixture", ["tumbler", "moving"])
def test_without_opaque_rows_it_is_render_shutter(gpu, fixture):
    """no surface table, then a table of glass rows with lights and shapes set: render_shutter on the same records, byte for byte"""
    clean(gpu)
    iors, weights = CH.fixture_bands()
    if fixture == "tumbler":
        scs, cam, recs = [NH.tumbler()], MH.view(*NH.VIEW, FW, FH), CH.fixture_records()
        recs = KH.records(recs["offset"], recs["lens_offset"], recs["band"], 0)
    else:
        scs, cam, recs = KH.moving_keys(), MH.view(*KH.VIEW, FW, FH), KH.fixture_records()
    KH.capture_keys(gpu, scs)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    lit = LH.records(recs["offset"], recs["lens_offset"], recs["band"], recs["key"], np.linspace(-1, 1, 2 * len(recs)).reshape(-1, 2))
    for flags in (0, REINHARD):
        p = rr.default_params(max_reflect=3, flags=flags, **LH.KW)
        want = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT)
        assert (want[2] > len(recs)).mean() > 0.05
        same(gpu.render_lit(FW, FH, cam, lit, lens=LENS, params=p, **OUT), want)
        gpu.set_surfaces([rr.glass()] * 4)
        gpu.set_lights(LH.OLIVE_LIGHTS, LH.OLIVE_AMBIENT)
        gpu.set_light_shapes(LH.OLIVE_SHAPES)
        same(gpu.render_lit(FW, FH, cam, lit, lens=LENS, params=p, **OUT), want)
        gpu.set_surfaces(None)
        gpu.set_lights(None)


@pytest.mark.parametrize("name", ["table", "mirror", "deep-olive", "alone"])
def test_with_one_live_key_and_a_pinhole_it_is_render_surfaces(gpu, name):
    """one key that is a capture of the live scene, a pinhole, no band set: render_surfaces on the positions, byte for byte -- with
    no shape table, and with a table of zeros under non-zero offsets"""
    fx = SH.FIXTURES[name]()
    key0(gpu, fx)
    w, h = (MH.W, MH.H) if name == "alone" else (FW, FH)
    cam = MH.view(*SH.VIEW, w, h)
    zero = np.zeros(len(fx.lights), rr.LIGHT_SHAPE_DTYPE)
    for flags in (0, REINHARD):
        p = rr.default_params(max_reflect=3, flags=flags, **LH.KW)
        for samples in (4, OFF3):
            want = gpu.render_surfaces(w, h, cam, samples, params=p, **OUT)
            assert (want[2] > (4 if isinstance(samples, int) else 3)).mean() > 0.05
            gpu.set_light_shapes(None)
            same(gpu.render_lit(w, h, cam, samples, keys=1, params=p, **OUT), want)
            gpu.set_light_shapes(zero)
            same(gpu.render_lit(w, h, cam, samples, keys=1, params=p, **OUT), want)
            n = samples if isinstance(samples, int) else len(samples)
            same(gpu.render_lit(w, h, cam, samples, keys=1, light_samples=np.linspace(1, -1, 2 * n).reshape(n, 2), params=p, **OUT), want)


# ------------------------------------------------------------------------------------------------- 4. keys
def test_the_moving_olive_under_two_light_offsets(gpu):
    """three keys whose innermost cube is opaque, crossed with two light offsets, through a lens (test_lit_cpu.py asserts what the
    reference shows: opaque hits under a list of two media in every key, shadow rays lit and occluded)"""
    fx, scs = LH.moving_olive()
    cam = MH.view(*KH.VIEW, FW, FH)
    recs = LH.olive_records()
    kw = dict(max_reflect=2, **LH.KW)
    rgb, cnt, _, _ = fx.lit(cam, FW, FH, recs, LENS, scenes=scs, **kw)
    clean(gpu)
    KH.capture_keys(gpu, scs)
    gpu.set_materials(TABLE)
    gpu.set_surfaces(fx.surf)
    gpu.set_lights(fx.lights, fx.ambient)
    gpu.set_light_shapes(fx.shapes)
    got = gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    check(gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=REINHARD, **kw), **OUT), rgb, cnt, True)
    same(gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=NO_CULL, **kw), **OUT), got)


def test_lit_keys_of_a_refit_animation_without_a_top_level(gpu):
    """surfaces_helpers.alone -- the open monkey, opaque with a little specular, no top level -- under the README's sine, refitted and
    captured three times, under a shaped directional light"""
    fx = SH.alone()
    (v, i), = fx.scene.meshes
    clean(gpu)
    mid = gpu.upload_mesh(v, i)
    gpu.build_blas(mid, allow_update=True)
    inst = rr.make_instances(meshes=[mid], materials=[2])
    gpu.build_tlas(inst, allow_update=True)
    gpu.upload_envmap(fx.scene.env)
    gpu.set_tile_partition(0, 1)
    scs = []
    for j, t in enumerate((0, 12, 24)):
        moved = KH.sine(v, t)
        gpu.update_mesh_vertices(mid, moved)
        gpu.build_blas(mid, update=True)
        gpu.build_tlas(inst, update=True)
        gpu.capture_scene_key(j)
        assert gpu.scene_key_info(j).top_level == 0
        scs.append(Scene("monkey-lit-sine-%d" % t, [(moved, i)], fx.scene.env, rr.make_instances(meshes=[0], materials=[2])))
    cam = MH.view(*NH.VIEW, W, H)
    shapes = LH.shapes(rr.light_shape((0.3, 0.0, 0.0), (0.0, 0.0, 0.3)))
    recs = LH.records(OFF3, rr.lens_pattern(3), 0, [2, 0, 1], [[-1.0, 1.0], [0.5, -0.25], [1.0, 0.0]])
    kw = dict(max_reflect=2, **LH.KW)
    rgb, cnt, _, extras = LH.ref_lit(scs, cam, W, H, recs, LENS, fx.table, fx.surf, fx.lights, shapes, fx.ambient, **kw)
    assert all(e[2].shadow_lit > 0 and e[2].shadow_occluded > 0 for e in extras)
    gpu.set_materials(fx.table)
    gpu.set_surfaces(fx.surf)
    gpu.set_lights(fx.lights, fx.ambient)
    gpu.set_light_shapes(shapes)
    check(gpu.render_lit(W, H, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 5. the stack rung of the deepest key
@pytest.mark.parametrize("needs", [(19, 20), (19, 21)])
def test_the_stack_rung_comes_from_the_deepest_key_with_shadow_rays_on_it(gpu, needs):
    """depth_meshes' chains as test_gpu_shutter.py pairs them, opaque and lit from the side the deep rays travel to, so that shadow
    rays walk the deep tree on the stack the deepest key asks for"""
    from test_gpu_stack_rungs import DEEP, assert_rung, chain_scene, view
    w, h = 48, 32
    cam = view(DEEP, w, h)
    kw = dict(max_refract=5, max_reflect=2)
    p = rr.default_params(**kw)
    chains = [chain_scene(n) for n in needs]
    surf = SH.surfaces(rr.opaque((0.6, 0.5, 0.4), specular=(0.5, 0.5, 0.5)))
    lts = SH.lights(rr.directional_light((1.0, 0.2, -0.02), (1.0, 0.9, 0.8), 0x01), rr.directional_light((-0.3, 0.2, -1.0), (0.5, 0.6, 0.7), 0xff))
    shapes = LH.shapes(rr.light_shape((0.0, 0.05, 0.0), (0.0, 0.0, 0.05)), rr.light_shape((0.05, 0.0, 0.0), (0.0, 0.05, 0.0)))
    recs = LH.records(np.repeat(OFF3[:2], 2, axis=0), None, 0, [0, 1, 1, 0], [[1, -1], [-1, 1], [0.5, 0.5], [0, 0]])
    clean(gpu)
    gpu.set_materials(TABLE)
    gpu.set_surfaces(surf)
    gpu.set_lights(lts, (0.01, 0.01, 0.01))
    gpu.set_light_shapes(shapes)
    for order in ((0, 1), (1, 0)):
        scs = [chains[o] for o in order]
        for j, sc in enumerate(scs):
            sc.load_gpu(gpu)
            assert_rung(gpu, sc, needs[order[j]], CH.sample_rays(cam, w, h, recs[0], None, p))
            gpu.capture_scene_key(j)
        rgb, cnt, _, extras = LH.ref_lit(scs, cam, w, h, recs, None, TABLE, surf, lts, shapes, (0.01, 0.01, 0.01), **kw)
        assert all(e[2].shadow_traced > 0 for e in extras) and sum(e[2].shadow_occluded for e in extras) > 0
        check(gpu.render_lit(w, h, cam, recs, params=p, **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 6. state
def test_the_shape_table_and_what_the_calls_leave_alone(gpu):
    fx, cam, recs, _ = LH.soft_ref(2)
    key0(gpu, fx)
    p = rr.default_params(max_reflect=2, **LH.KW)
    gpu.set_camera(cam)
    gpu.dispatch_rays(W, H, p)
    frame, stats = gpu.read_frame(), gpu.stats()
    surfaces = gpu.render_surfaces(W, H, cam, 2, params=p, **OUT)
    shutter = gpu.render_shutter(W, H, cam, 2, keys=1, params=p, **OUT)
    soft = gpu.render_lit(W, H, cam, recs, params=p, **OUT)
    # set_lights clears the shapes: the four corners become one light, four times
    gpu.set_lights(fx.lights, fx.ambient)
    hard = gpu.render_lit(W, H, cam, recs, params=p, **OUT)
    assert hard[0].tobytes() != soft[0].tobytes()
    same(hard, gpu.render_surfaces(W, H, cam, [(0.5, 0.5)] * 4, params=p, **OUT))
    # a second table takes effect without a rebuild, and is the reference's again
    wide = LH.shapes(rr.light_shape((0.8, 0.0, 0.0), (0.0, 0.2, 0.4)))
    gpu.set_light_shapes(wide)
    rgb, cnt, _, _ = LH.ref_lit([fx.scene], cam, W, H, recs, None, fx.table, fx.surf, fx.lights, wide, fx.ambient, max_reflect=2, **LH.KW)
    assert rgb.tobytes() != soft[0][..., :3].tobytes()
    check(gpu.render_lit(W, H, cam, recs, params=p, **OUT), rgb, cnt, False)
    gpu.set_light_shapes(fx.shapes)
    same(gpu.render_lit(W, H, cam, recs, params=p, **OUT), soft)
    # zero lights: the ambient term alone, whatever the offsets; a shape table of length 0 is the only one that fits
    gpu.set_lights(None, (0.2, 0.3, 0.4))
    refused(lambda: gpu.set_light_shapes(fx.shapes), RR_ERR_INVALID_ARGUMENT)
    gpu.set_light_shapes(None)
    rgb, cnt, _, _ = LH.ref_lit([fx.scene], cam, W, H, recs, None, fx.table, fx.surf, SH.lights(), None, (0.2, 0.3, 0.4), max_reflect=2, **LH.KW)
    check(gpu.render_lit(W, H, cam, recs, params=p, **OUT), rgb, cnt, False)
    # eight shaped lights
    ring = [(np.cos(a), np.sin(a)) for a in np.arange(8) * (2 * np.pi / 8)]
    lts = SH.lights(*[rr.point_light((1.5 * c, 1.2 + 0.1 * k, 1.5 * s), (0.5, 0.4, 0.6), 0xff) for k, (c, s) in enumerate(ring)])
    eight = LH.shapes(*[rr.light_shape((0.05 * (k + 1), 0.0, 0.0), (0.0, 0.02 * k, 0.3)) for k in range(8)])
    gpu.set_lights(lts)
    gpu.set_light_shapes(eight)
    rgb, cnt, _, extras = LH.ref_lit([fx.scene], cam, W, H, recs, None, fx.table, fx.surf, lts, eight, None, max_reflect=2, **LH.KW)
    assert all(extras[0][2].light_used[k] > 0 for k in range(8))
    check(gpu.render_lit(W, H, cam, recs, params=p, **OUT), rgb, cnt, False)
    # nothing else moved: the dispatch state, the frame, the counters and the other frames' outputs
    assert gpu.read_frame().tobytes() == frame.tobytes()
    after = gpu.stats()
    assert all(getattr(after, f) == getattr(stats, f) for f, _ in rr._capi.Stats._fields_)
    gpu.set_lights(fx.lights, fx.ambient)
    same(gpu.render_surfaces(W, H, cam, 2, params=p, **OUT), surfaces)
    same(gpu.render_shutter(W, H, cam, 2, keys=1, params=p, **OUT), shutter)


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_what_the_lit_calls_refuse(gpu):
    fx = LH.soft(True)
    fresh = rr.Renderer(gpu.device)
    try:
        cam = LH.soft_view(8, 8)
        fx.scene.load_gpu(fresh)
        refused(lambda: fresh.render_lit(8, 8, cam, 1, keys=1), RR_ERR_STATE)              # no material table
        fx.load(fresh)
        refused(lambda: fresh.render_lit(8, 8, cam, 1, keys=1), RR_ERR_INVALID_ARGUMENT)    # no key, no frame
        fresh.capture_scene_key(0)
        fresh.capture_scene_key(1)
        ok = LH.records(OFF3, rr.lens_pattern(3), 0, [1, 0, 1], [[-1, 1], [0.5, 0], [1, -1]])
        want = LH.ref_lit([fx.scene] * 2, cam, 8, 8, ok, LENS, fx.table, fx.surf, fx.lights, fx.shapes, fx.ambient, **LH.KW)

        def good():
            check(fresh.render_lit(8, 8, cam, ok, lens=LENS, params=rr.default_params(**LH.KW), **OUT), want[0], want[1], False)
        good()

        def changed(field, k, value):
            r = ok.copy()
            r[field][k] = value
            return r
        # the shape table: n is not the number of lights, a shape that is not finite, a pad that is not zero; the one in force stays
        pad = fx.shapes.copy()
        pad["pad"][1] = (0, 1)
        nan = fx.shapes.copy()
        nan["ey"][0] = (0.0, np.nan, 0.0)
        inf = fx.shapes.copy()
        inf["ex"][1] = (np.inf, 0.0, 0.0)
        for bad in (fx.shapes[:1], np.concatenate([fx.shapes, fx.shapes[:1]]), pad, nan, inf):
            refused(lambda: fresh.set_light_shapes(bad), RR_ERR_INVALID_ARGUMENT)
            good()
        assert rr.lib().rr_set_light_shapes(fresh._h, None, 2) == RR_ERR_INVALID_ARGUMENT
        good()
        for bad in (changed("light_offset", 1, (1.5, 0.0)), changed("light_offset", 2, (0.0, np.nan)), changed("light_offset", 0, (-1.01, 0.0)),
                    changed("key", 2, rr.MAX_SCENE_KEYS), changed("key", 0, 2),              # a key out of range, an empty key
                    changed("band", 2, 1),                                                   # a band beyond the set
                    ok[:0], np.zeros(65, rr.LIT_SAMPLE_DTYPE),
                    changed("offset", 1, (0.5, 1.01)), changed("lens_offset", 1, (0.0, np.nan))):
            refused(lambda: fresh.render_lit(8, 8, cam, bad, lens=LENS), RR_ERR_INVALID_ARGUMENT)
            refused(lambda: fresh.render_lit(8, 8, cam, bad, lens=LENS, device=True), RR_ERR_INVALID_ARGUMENT)
            good()
        # the offsets are checked whether or not a shape table is set
        fresh.set_light_shapes(None)
        refused(lambda: fresh.render_lit(8, 8, cam, changed("light_offset", 1, (1.5, 0.0)), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        # a moved direction that becomes zero: the sun is v, its shape's ex is -v, and the offset (1, 0) takes it to (0, 0, 0) exactly
        v = fx.lights["v"][0]
        zero = fx.shapes.copy()
        zero["ex"][0], zero["ey"][0] = -v, (0.0, 0.0, 0.0)
        assert not rr.moved_lights(fx.lights, zero, 1.0, 0.0)["v"][0].any()
        fresh.set_light_shapes(zero)
        short = ok.copy()
        short["light_offset"] = [(-1.0, 1.0), (0.5, 0.0), (0.25, -1.0)]
        assert fresh.render_lit(8, 8, cam, short, lens=LENS).shape == (8, 8, 4)
        short["light_offset"][1] = (1.0, 0.0)
        refused(lambda: fresh.render_lit(8, 8, cam, short, lens=LENS), RR_ERR_INVALID_ARGUMENT)
        # a moved position that is not finite
        far = fx.shapes.copy()
        far["ex"][1] = (3.0e38, 0.0, 0.0)
        far["ey"][1] = (3.0e38, 0.0, 0.0)
        fresh.set_light_shapes(far)
        refused(lambda: fresh.render_lit(8, 8, cam, changed("light_offset", 0, (1.0, 1.0)), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        fresh.set_light_shapes(fx.shapes)
        good()
        with pytest.raises(ValueError):
            fresh.render_lit(8, 8, cam, OFF3)                                   # keys=None: there is no implicit key
        with pytest.raises(ValueError):
            fresh.render_lit(8, 8, cam, ok, light_samples=np.zeros((3, 2)))     # records carry their own light offsets
        with pytest.raises(ValueError):
            fresh.render_lit(8, 8, cam, OFF3, keys=1, light_samples=np.zeros((2, 2)))
        # a material row above the table, then no table
        fresh.set_materials(TABLE[:2])
        refused(lambda: fresh.render_lit(8, 8, cam, ok, lens=LENS), RR_ERR_INVALID_ARGUMENT)
        fresh.set_materials(None)
        refused(lambda: fresh.render_lit(8, 8, cam, ok, lens=LENS), RR_ERR_STATE)
        fresh.set_materials(TABLE)
        good()
        # keys of one frame that disagree on the top level: key 2 is a scene without one
        NH.alone("cube.obj", 1).load_gpu(fresh)
        fresh.capture_scene_key(2)
        refused(lambda: fresh.render_lit(8, 8, cam, changed("key", 0, 2), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        assert fresh.render_lit(8, 8, cam, OFF3, keys=[2, 2, 2], paired=True).shape == (8, 8, 4)
        good()
        # the device variant's pointers
        import torch
        L, P = rr.lib(), C.c_void_p
        dev = "cuda:%d" % fresh.device
        out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
        aux = torch.zeros(64 + 4, dtype=torch.int32, device=dev)
        a = (fresh._h, 8, 8, C.byref(cam), None, ok.ctypes.data, 3, None)
        assert L.rr_render_lit_device(*a, P(out.data_ptr()), P(aux.data_ptr()), P(aux.data_ptr())) == 0
        assert L.rr_render_lit_device(*a, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_lit_device(*a, P(out.data_ptr()), P(aux.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_lit_device(*a, None, None, P(aux.data_ptr())) == RR_ERR_INVALID_ARGUMENT
        fresh.wait()
        good()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 8. the device path
def test_the_device_variant_equals_the_host_path(gpu):
    import torch
    fx, scs = LH.moving_olive()
    cam = MH.view(*KH.VIEW, FW, FH)
    recs = LH.olive_records()
    clean(gpu)
    KH.capture_keys(gpu, scs)
    fx.load(gpu)
    p = rr.default_params(max_reflect=3, **LH.KW)
    host = gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=p, **OUT)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_lit(FW, FH, cam, recs, lens=LENS, params=p, device=True, **OUT)
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
    finally:
        gpu.reset_stream()


# ------------------------------------------------------------------------------------------------- 9. the demo
def test_rrdemo_lit_writes_render_lit_frames(gpu, tmp_path):
    """rrdemo --compose --lit --floor ... --light ... --soft 0.3: drawFrameLit end to end -- the sphere on the floor under a sun and a
    square lamp, through a lens in two bands; its PPM is render_lit's RGBA8 store of the same scene captured as key 0 with
    rr.light_pattern's offsets.  With --shutter the frame changes.  Without --lit the same switches are refused as before"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, SH.env_map())
    args = [exe, "--mesh", O.asset("sphere.obj"), "--env", hdr, "--size", "64x48", "--frames", "1"]
    glassy = ["--spp", "2", "--lens", "0.2:5", "--dispersion", "2:30", "--materials", "1.5:0.8,0.1,0.1", "--compose"]
    switches = ["--floor", "0.7,0.6,0.5:0.25", "--light", "0.3,1,0.2:1.2,1.1,0.9", "--light", "@1.5,2.5,-1:6,6,7", "--soft", "0.3"]
    images = []
    for k, more in enumerate(([], ["--shutter", "2:0.3"])):
        out = subprocess.run(args + glassy + ["--lit"] + switches + more + ["--out", str(tmp_path / ("s%d_%%03d.ppm" % k))], capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0 and "lit frame: 2 positions x %d keys" % (k + 1) in out.stdout and "under 2 lights, thin lens" in out.stdout, \
            out.stderr + out.stdout
        raw = open(tmp_path / ("s%d_000.ppm" % k), "rb").read()
        head = b"P6\n64 48\n255\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3))
    assert not np.array_equal(images[0], images[1])
    env_rt, _ = rr.load_texture(hdr, 3)
    sphere, cube = load("sphere.obj"), load("cube.obj")
    ymin = float(sphere[0]["position"][sphere[1].astype(np.int64)][:, 1].min())
    clean(gpu)
    ids = [gpu.upload_mesh(*sphere), gpu.upload_mesh(*cube)]
    for i in ids:
        gpu.build_blas(i)
    floor = np.array([[4, 0, 0, 0], [0, 0.1, 0, np.float32(ymin) - np.float32(0.15)], [0, 0, 4, 0]], np.float32)
    gpu.build_tlas(rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], floor], meshes=ids, materials=[0, 1]))
    gpu.upload_envmap(env_rt)
    gpu.capture_scene_key(0)
    table = [(1.5, (0.8, 0.1, 0.1)), (1.0, (0, 0, 0))]
    gpu.set_materials(table)
    gpu.set_material_bands(*rr.material_bands(table, 30.0, 2))
    gpu.set_surfaces([rr.glass(), rr.opaque((0.7, 0.6, 0.5), specular=(0.25, 0.25, 0.25))])
    gpu.set_lights([rr.directional_light((0.3, 1, 0.2), (1.2, 1.1, 0.9)), rr.point_light((1.5, 2.5, -1), (6, 6, 7))], (0.05, 0.05, 0.05))
    gpu.set_light_shapes([rr.light_shape((0, 0, 0), (0, 0, 0)), rr.light_shape((0.3, 0, 0), (0, 0, 0.3))])
    _, u8, cnt = gpu.render_lit(64, 48, rr.camera_orbit(0.01), 2, keys=1, lens=rr.Lens(0.2, 5.0), bands=2, **OUT)
    assert (cnt > 8).mean() > 0.2
    assert np.array_equal(images[0], u8[..., :3])
    hard = gpu.render_lit(64, 48, rr.camera_orbit(0.01), 2, keys=1, lens=rr.Lens(0.2, 5.0), bands=2, light_samples=np.zeros((2, 2), np.float32), **OUT)
    assert not np.array_equal(hard[1], u8)                   # the lamp's square shows
    for bad in (args + glassy + switches[:6], args + glassy + ["--shutter", "2:0.1"] + switches[:6],         # without --lit: as before
                args + glassy[:-1] + ["--lit"] + switches, args + glassy + switches):                        # --lit needs --compose, --soft needs --lit
        assert subprocess.run(bad, capture_output=True, text=True, timeout=120).returncode == 2


# ------------------------------------------------------------------------------------------------- 10. the README's example
def test_the_readme_example_renders(gpu):
    """the glass of water with ice on a lit table through a lens, as the README writes it: the tumbler's three nested instances over a
    flattened cube, the glass with a mask the sun's shadow rays do not see, the scene frozen as key 0, two bands, the lamp a square of
    half-edge 0.3 and the sun left a direction -- against the CPU fold"""
    t = NH.tumbler()
    floor = np.array([[2.5, 0, 0, 0], [0, 0.1, 0, -1.2], [0, 0, 2.5, 0]], np.float32)
    inst = rr.make_instances(transforms=list(t.instances["transform"].reshape(-1, 3, 4)) + [floor], meshes=[int(b) for b in t.instances["blas"]] + [0],
                             materials=[0, 1, 2, 3], masks=[0x02, 0x02, 0x02, 0x01])
    sc = Scene("readme-lit-table", t.meshes, t.env, inst)
    for k in range(3):
        SH.assert_disjoint(sc, k, 3)
    table = np.array([(1.5, (0.02, 0.02, 0.02)), (1.33, (0.05, 0.02, 0.01)), (1.31, (0, 0, 0)), (1.0, (0, 0, 0))], rr.MATERIAL_DTYPE)
    surf = SH.surfaces(rr.glass(), rr.glass(), rr.glass(), rr.opaque((0.7, 0.6, 0.5), specular=(0.1, 0.1, 0.1)))
    lts = SH.lights(rr.directional_light((-0.5, 1.0, -0.4), (1.2, 1.1, 0.9), shadow_mask=0x01), rr.point_light((1.5, 2.5, -1.0), (6, 6, 7)))
    shapes = LH.shapes(rr.light_shape((0, 0, 0), (0, 0, 0)), rr.light_shape((0.3, 0, 0), (0, 0, 0.3)))
    fx = LH.Lit(sc, surf, lts, (0.05, 0.05, 0.05), shapes, table)
    cam = MH.view(*NH.VIEW, W, H)
    iors, weights = rr.material_bands(table, abbe=30.0, n=2)
    recs = rr.lit_samples(2, 1, 2)
    rgb, cnt, _, extras = fx.lit(cam, W, H, recs, LENS, iors, weights, max_reflect=2, **LH.KW)
    assert sum(e[2].shadow_lit for e in extras) > 0 and sum(e[2].shadow_occluded for e in extras) > 0 and sum(e[2].specular_children for e in extras) > 0
    key0(gpu, fx)
    gpu.set_material_bands(iors, weights)
    got = gpu.render_lit(W, H, cam, samples=2, keys=1, lens=LENS, bands=2, params=rr.default_params(max_reflect=2, **LH.KW), **OUT)
    check(got, rgb, cnt, False)
