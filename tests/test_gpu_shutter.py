"""GPU: shutter frames (Renderer.capture_scene_key, release_scene_key, scene_key_info, render_shutter; rr_capture_scene_key,
rr_release_scene_key, rr_scene_key_info, rr_render_shutter[_device]).

The contract is composed's fold with one word added: sample k is what shade_rays_nested gives the rays of lens_rays in the scene
captured as key_k under band table T_band_k, weighted and summed by render_spectral's rule.  It is checked bit for bit -- float
colours, RGBA8 and TraceRay counts -- against that fold of the CPU reference (tests/native/nested_ref.c through
shutter_helpers.py, a key being just a Scene there), against the same fold of the GPU's own shade_rays_nested in the live scenes the
keys were captured from, and through its reduction to render_composed.  Every frame is about 50 x 38 with at most 8 samples."""
import ctypes as C

import numpy as np
import pytest

import composed_helpers as CH
import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as SH
from composed_helpers import LENS
from conftest import procedural_env
from nested_helpers import FH, FW, OFF3, TABLE
from scenes import Scene, gpu, load, xf  # noqa: F401  (gpu: a fixture)
from spectral_helpers import weighted_fold
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


def small_cube():
    """something else entirely: one cube a fifth of its size, off the middle"""
    return Scene("small-cube", [load("cube.obj")], SH.env_map(), rr.make_instances(transforms=[xf(0.3, -0.2, 0.1, (0.2, 0.2, 0.2), 0.3)], meshes=[0]))


# ------------------------------------------------------------------------------------------------- 1. the fold of the CPU reference
@pytest.mark.parametrize("max_reflect", [2, 3])             # 3: the builds with eight parked-ray slots
def test_shutter_is_the_fold_of_the_reference(gpu, max_reflect):
    """the moving tumbler through a lens: three keys and two bands, both out of order (test_shutter_cpu.py asserts what the fixture is
    for: blocks outside the union rectangle, and hits in blocks that only the union rectangle covers)"""
    scs, cam, recs, iors, weights, (rgb, cnt, _, _) = SH.moving_ref(max_reflect)
    SH.capture_keys(gpu, scs)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    kw = dict(max_reflect=max_reflect, **SH.KW)
    got = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    tm = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD, **kw), **OUT)
    check(tm, rgb, cnt, True)
    # culling by the union rectangle changes no byte
    same(gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=rr.default_params(flags=rr.DISPATCH_DEBUG_NO_CULL, **kw), **OUT), got)
    # the same samples through the other arguments: positions with paired key and band indices and the built-in lens points ...
    same(gpu.render_shutter(FW, FH, cam, np.repeat(OFF3, 2, axis=0), keys=SH.KEY_ORDER, lens=LENS, bands=SH.BAND_ORDER, paired=True,
                            params=rr.default_params(**kw), **OUT), got)
    # ... and crossed: rr.shutter_samples and the int arguments give one ordering, whose fold is the reference's again
    crossed = rr.shutter_samples(OFF3[:1], 3, 2)
    want = SH.ref_shutter(scs, cam, FW, FH, crossed, LENS, TABLE, iors, weights, **kw)
    by_records = gpu.render_shutter(FW, FH, cam, crossed, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(by_records, want[0], want[1], False)
    same(gpu.render_shutter(FW, FH, cam, OFF3[:1], keys=3, bands=2, lens=LENS, params=rr.default_params(**kw), **OUT), by_records)


# ------------------------------------------------------------------------------------------------- 2. the fold of the GPU's own calls
def test_shutter_is_the_fold_of_shade_rays_nested_in_the_live_scenes(gpu):
    """the contract as the header words it: per key the scene live, per sample set_materials(T_band) and shade_rays_nested on lens_rays;
    then the live scene becomes something else entirely and the keys still give that fold"""
    scs = SH.moving_keys()
    cam = MH.view(*SH.VIEW, FW, FH)
    kw = dict(max_reflect=3, **SH.KW)
    p = rr.default_params(**kw)
    iors, weights = CH.fixture_bands()
    recs = SH.fixture_records()
    cols, total = [None] * len(recs), np.zeros(FW * FH, np.uint32)
    for j, sc in enumerate(scs):
        sc.load_gpu(gpu)
        for k, rec in enumerate(recs):
            if int(rec["key"]) != j:
                continue
            gpu.set_materials(CH.band_table(TABLE, iors, int(rec["band"])))
            f, n = gpu.shade_rays_nested(CH.sample_rays(cam, FW, FH, rec, LENS, p), p, ray_counts=True)
            cols[k] = np.ascontiguousarray(f[:, :3]).reshape(FH, FW, 3)
            total += n
        gpu.capture_scene_key(j)
    rgb, cnt = weighted_fold(cols, [weights[int(r["band"])] for r in recs]), total.reshape(FH, FW)
    assert (cnt > len(recs)).mean() > 0.05 and cols[0].tobytes() != cols[1].tobytes()
    small_cube().load_gpu(gpu)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    check(gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT), rgb, cnt, False)
    assert gpu.render_composed(FW, FH, cam, 1, params=p).tobytes() != gpu.render_shutter(FW, FH, cam, 1, keys=1, params=p).tobytes()


# ------------------------------------------------------------------------------------------------- 3. the reduction
def test_with_every_key_the_live_scene_it_is_render_composed(gpu):
    sc = NH.tumbler()
    sc.load_gpu(gpu)
    gpu.capture_scene_key(0)
    gpu.capture_scene_key(5)
    gpu.set_materials(TABLE)
    cam = MH.view(*NH.VIEW, FW, FH)
    iors, weights = CH.fixture_bands()
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        p = rr.default_params(max_refract=8, max_reflect=3, flags=flags)
        for samples in (4, OFF3):
            gpu.set_material_bands(None)
            want = gpu.render_composed(FW, FH, cam, samples, params=p, **OUT)
            assert (want[2] > 4).mean() > 0.05
            same(gpu.render_shutter(FW, FH, cam, samples, keys=1, params=p, **OUT), want)
            gpu.set_material_bands(iors, weights)
            want = gpu.render_composed(FW, FH, cam, samples, lens=LENS, bands=2, params=p, **OUT)
            same(gpu.render_shutter(FW, FH, cam, samples, keys=1, lens=LENS, bands=2, params=p, **OUT), want)
        # two keys that hold the same scene, one per sample
        want = gpu.render_composed(FW, FH, cam, OFF3, lens=LENS, bands=[1, 0, 1], paired=True, params=p, **OUT)
        same(gpu.render_shutter(FW, FH, cam, OFF3, keys=[5, 0, 5], lens=LENS, bands=[1, 0, 1], paired=True, params=p, **OUT), want)


# ------------------------------------------------------------------------------------------------- 4. refit keys without a top level
def test_keys_of_a_refit_animation_without_a_top_level(gpu):
    """the open monkey alone under the README's sine: vertex update, BLAS refit, TLAS update, capture -- three times; then the live
    mesh moves on and no key follows"""
    sc = NH.alone("monkey.obj", 2)
    (v, i), = sc.meshes
    mid = gpu.upload_mesh(v, i)
    gpu.build_blas(mid, allow_update=True)
    inst = rr.make_instances(meshes=[mid], materials=[2])
    gpu.build_tlas(inst, allow_update=True)
    gpu.upload_envmap(sc.env)
    gpu.set_tile_partition(0, 1)
    scs = []
    for j, t in enumerate((0, 12, 24)):
        moved = SH.sine(v, t)
        gpu.update_mesh_vertices(mid, moved)
        gpu.build_blas(mid, update=True)
        gpu.build_tlas(inst, update=True)
        gpu.capture_scene_key(j)
        info = gpu.scene_key_info(j)
        assert info.captured == 1 and info.top_level == 0 and info.n_instances == 1 and info.n_triangles == len(i) // 3
        scs.append(Scene("monkey-sine-%d" % t, [(moved, i)], sc.env, rr.make_instances(meshes=[0], materials=[2])))
    cam = MH.view(*NH.VIEW, MH.W, MH.H)
    iors, weights = CH.fixture_bands()
    recs = SH.records(OFF3, rr.lens_pattern(3), [1, 0, 1], [2, 0, 1])
    kw = dict(max_reflect=2, **SH.KW)
    rgb, cnt, cols, _ = SH.ref_shutter(scs, cam, MH.W, MH.H, recs, LENS, TABLE, iors, weights, **kw)
    assert (cnt > len(recs)).mean() > 0.05
    one = CH.band_table(TABLE, iors, 0)
    rays = CH.sample_rays(cam, MH.W, MH.H, recs[0], LENS, rr.default_params(**kw))
    frames = [NH.ref_shade(s, rays, one, **kw)[0] for s in scs]
    assert all(frames[a].tobytes() != frames[b].tobytes() for a in range(3) for b in range(a + 1, 3))      # the keys differ
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    got = gpu.render_shutter(MH.W, MH.H, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT)
    check(got, rgb, cnt, False)
    gpu.update_mesh_vertices(mid, SH.sine(v, 40))               # the live mesh alone moves on: refitted in place, not captured
    same(gpu.render_shutter(MH.W, MH.H, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT), got)
    gpu.build_blas(mid, update=True)
    gpu.build_tlas(inst, update=True)
    same(gpu.render_shutter(MH.W, MH.H, cam, recs, lens=LENS, params=rr.default_params(**kw), **OUT), got)
    assert gpu.render_composed(MH.W, MH.H, cam, OFF3[:1], params=rr.default_params(**kw)).tobytes() != \
        gpu.render_shutter(MH.W, MH.H, cam, OFF3[:1], keys=[2], paired=True, params=rr.default_params(**kw)).tobytes()


# ------------------------------------------------------------------------------------------------- 5. the stack rung of the deepest key
@pytest.mark.parametrize("needs", [(19, 20), (19, 21)])
def test_the_stack_rung_comes_from_the_deepest_key(gpu, needs):
    """depth_meshes' chains, as test_gpu_stack_rungs.py builds them: a tree at the top of the 19-entry rung and one at the bottom of the
    next (and, since a rung has one entry to spare over its deepest tree, the tree one deeper, whose walk would overrun the 19-entry
    stack of a variant taken from the shallow key alone), in both capture orders"""
    from test_gpu_stack_rungs import DEEP, assert_rung, chain_scene, view
    w, h = 48, 32
    cam = view(DEEP, w, h)
    kw = dict(max_refract=5, max_reflect=2)
    p = rr.default_params(**kw)
    chains = [chain_scene(n) for n in needs]
    recs = SH.records(np.repeat(OFF3[:2], 2, axis=0), None, 0, [0, 1, 1, 0])
    gpu.set_materials(TABLE)
    for order in ((0, 1), (1, 0)):
        scs = [chains[o] for o in order]
        for j, sc in enumerate(scs):
            sc.load_gpu(gpu)
            need = needs[order[j]]
            assert_rung(gpu, sc, need, CH.sample_rays(cam, w, h, recs[0], None, p))
            gpu.capture_scene_key(j)
            info = gpu.scene_key_info(j)
            assert info.stack_need == need == gpu.stats().bvh_depth and info.top_level == 0
        rgb, cnt, _, _ = SH.ref_shutter(scs, cam, w, h, recs, None, TABLE, **kw)
        assert (cnt > len(recs)).mean() > 0.05
        check(gpu.render_shutter(w, h, cam, recs, params=p, **OUT), rgb, cnt, False)


# ------------------------------------------------------------------------------------------------- 6. lifecycle
def scene_box(gpu):
    """the live scene's world-space box as the library keeps it: the union of the top level's root's two child boxes"""
    root = gpu.download_tlas()[0][0]
    lo, hi = np.full(3, 3.0e38, np.float32), np.full(3, -3.0e38, np.float32)
    for k in range(2):
        if not root["lox"][k] <= root["hix"][k]:
            continue
        lo = np.minimum(lo, [root["lox"][k], root["loy"][k], root["loz"][k]])
        hi = np.maximum(hi, [root["hix"][k], root["hiy"][k], root["hiz"][k]])
    return np.concatenate([lo, hi]).astype(np.float32)


def test_the_life_of_a_key(gpu):
    three, five = NH.tumbler(), NH.five_deep()
    cam = MH.view(*NH.VIEW, FW, FH)
    kw = dict(max_reflect=2, **SH.KW)
    p = rr.default_params(**kw)
    recs = SH.records(np.repeat(OFF3[:2], 2, axis=0), rr.lens_pattern(4), 0, [0, 1, 1, 0])
    boxes = []
    gpu.release_scene_key()                                     # (the renderer is the module's: start from empty keys)
    for j, sc in enumerate((three, five)):                    # instance counts differ between the keys
        sc.load_gpu(gpu)
        boxes.append(scene_box(gpu))
        gpu.capture_scene_key(j)
    for j, (sc, n) in enumerate(((three, 3), (five, 5))):
        info = gpu.scene_key_info(j)
        assert info.captured == 1 and info.top_level == 1 and info.n_instances == n and info.bytes > 0 and info.max_material == n
        assert np.array(list(info.bounds), np.float32).tobytes() == boxes[j].tobytes()
        assert np.allclose(list(info.bounds), list(sc.bounds), atol=1e-3)
    assert gpu.scene_key_info(7).captured == 0 and gpu.scene_key_info(7).bytes == 0
    gpu.set_materials(TABLE)
    rgb, cnt, _, _ = SH.ref_shutter([three, five], cam, FW, FH, recs, LENS, TABLE, **kw)
    first = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT)
    check(first, rgb, cnt, False)
    # keys survive load_scene
    gpu.load_scene(*load("monkey.obj"), SH.env_map())
    same(gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT), first)
    # another environment map, of another size, and another table after the capture: both are the render call's
    env2 = procedural_env(64, 32, seed=11)
    table2 = TABLE[::-1].copy()
    gpu.upload_envmap(env2)
    gpu.set_materials(table2)
    moved = [Scene(sc.key + "-env2", sc.meshes, env2, sc.instances) for sc in (three, five)]
    rgb2, cnt2, _, _ = SH.ref_shutter(moved, cam, FW, FH, recs, LENS, table2, **kw)
    assert rgb2.tobytes() != rgb.tobytes()
    check(gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT), rgb2, cnt2, False)
    gpu.set_materials(TABLE)
    # recapture into a used key: a larger scene, then a smaller one; each time the key is the live scene, so the frame is composed's
    sizes = [gpu.scene_key_info(1).bytes]
    for sc in (MH.three_scene((1, 2, 3)), small_cube()):
        sc.load_gpu(gpu)
        gpu.capture_scene_key(1)
        sizes.append(gpu.scene_key_info(1).bytes)
        assert gpu.scene_key_info(1).n_instances == len(sc.instances)
        same(gpu.render_shutter(FW, FH, cam, OFF3, keys=[1, 1, 1], lens=LENS, paired=True, params=p, **OUT),
             gpu.render_composed(FW, FH, cam, OFF3, lens=LENS, params=p, **OUT))
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1]        # buffers grow, and are reused where they are large enough
    # release, then a render refuses; the other key still renders
    alone0 = gpu.render_shutter(FW, FH, cam, OFF3, keys=1, params=p, **OUT)
    gpu.release_scene_key(1)
    assert gpu.scene_key_info(1).captured == 0
    refused(lambda: gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p), RR_ERR_INVALID_ARGUMENT)
    same(gpu.render_shutter(FW, FH, cam, OFF3, keys=1, params=p, **OUT), alone0)
    gpu.release_scene_key()
    assert gpu.scene_key_info(0).captured == 0
    refused(lambda: gpu.render_shutter(FW, FH, cam, OFF3, keys=1, params=p), RR_ERR_INVALID_ARGUMENT)
    # destroying a renderer with keys held is clean
    other = rr.Renderer(gpu.device)
    three.load_gpu(other)
    other.capture_scene_key(3)
    other.set_materials(TABLE)
    assert other.render_shutter(8, 8, MH.view(*NH.VIEW, 8, 8), 1, keys=[3], paired=True).shape == (8, 8, 4)
    other.close()


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_what_the_shutter_calls_refuse(gpu):
    import torch
    sc = NH.tumbler()
    fresh = rr.Renderer(gpu.device)
    try:
        cam = MH.view(*NH.VIEW, 8, 8)
        refused(lambda: fresh.capture_scene_key(0), RR_ERR_STATE)              # nothing built
        fresh.set_materials(TABLE)
        refused(lambda: fresh.render_shutter(8, 8, cam, 1, keys=1), RR_ERR_INVALID_ARGUMENT)      # no key, no frame
        sc.load_gpu(fresh)
        refused(lambda: fresh.capture_scene_key(rr.MAX_SCENE_KEYS), RR_ERR_INVALID_ARGUMENT)
        refused(lambda: fresh.release_scene_key(rr.MAX_SCENE_KEYS), RR_ERR_INVALID_ARGUMENT)
        refused(lambda: fresh.scene_key_info(rr.MAX_SCENE_KEYS), RR_ERR_INVALID_ARGUMENT)
        fresh.capture_scene_key(0)
        fresh.capture_scene_key(1)
        iors, weights = CH.fixture_bands()
        fresh.set_material_bands(iors, weights)
        ok = SH.records(OFF3, rr.lens_pattern(3), [0, 1, 1], [1, 0, 1])

        def good():
            """the valid call, and it is correct: both keys hold the live scene, so it is composed's frame"""
            got = fresh.render_shutter(8, 8, cam, ok, lens=LENS, **OUT)
            same(got, fresh.render_composed(8, 8, cam, CH.records(OFF3, rr.lens_pattern(3), [0, 1, 1]), lens=LENS, **OUT))
        good()

        def changed(field, k, value):
            r = ok.copy()
            r[field][k] = value
            return r
        for bad in (changed("key", 2, rr.MAX_SCENE_KEYS), changed("key", 2, 0xffffffff),     # a key out of range
                    changed("key", 0, 2),                                                    # an empty key
                    changed("pad", 1, (0, 1)), changed("pad", 2, (7, 0)),                    # pad is not ignored here
                    changed("band", 2, 2),                                                   # a band beyond the set
                    ok[:0], np.zeros(65, rr.SHUTTER_SAMPLE_DTYPE),                           # 0 and 65 samples
                    changed("offset", 1, (0.5, 1.01)), changed("offset", 1, (np.nan, 0.5)),
                    changed("lens_offset", 1, (-1.01, 0.0)), changed("lens_offset", 1, (0.0, np.nan))):
            refused(lambda: fresh.render_shutter(8, 8, cam, bad, lens=LENS), RR_ERR_INVALID_ARGUMENT)
            refused(lambda: fresh.render_shutter(8, 8, cam, bad, lens=LENS, device=True), RR_ERR_INVALID_ARGUMENT)
            good()
        assert fresh.render_shutter(8, 8, cam, np.zeros(64, rr.SHUTTER_SAMPLE_DTYPE), lens=LENS).shape == (8, 8, 4)
        assert fresh.render_shutter(8, 8, cam, changed("lens_offset", 1, (-1.01, 0.0))).shape == (8, 8, 4)       # no lens: not looked at
        refused(lambda: fresh.render_shutter(8, 8, cam, ok, lens=rr.Lens(-1.0, 5.0)), RR_ERR_INVALID_ARGUMENT)
        with pytest.raises(ValueError):
            fresh.render_shutter(8, 8, cam, OFF3)                               # keys=None: there is no implicit key
        with pytest.raises(ValueError):
            fresh.render_shutter(8, 8, cam, ok, keys=2)                         # records carry their own keys
        with pytest.raises(ValueError):
            fresh.render_shutter(8, 8, cam, 16, keys=3, bands=2)                # 96 samples
        # a material row above the table: the small cube of the tumbler is made of row 3
        fresh.set_materials(TABLE[:3])
        refused(lambda: fresh.render_shutter(8, 8, cam, 1, keys=1), RR_ERR_INVALID_ARGUMENT)
        fresh.set_materials(None)
        refused(lambda: fresh.render_shutter(8, 8, cam, 1, keys=1), RR_ERR_STATE)      # no table
        fresh.set_materials(TABLE)
        fresh.set_material_bands(iors, weights)
        good()
        # keys of one frame that disagree on the top level: key 2 is a scene without one
        NH.alone("cube.obj", 1).load_gpu(fresh)
        fresh.capture_scene_key(2)
        assert fresh.scene_key_info(2).top_level == 0 and fresh.scene_key_info(0).top_level == 1
        refused(lambda: fresh.render_shutter(8, 8, cam, changed("key", 0, 2), lens=LENS), RR_ERR_INVALID_ARGUMENT)
        assert fresh.render_shutter(8, 8, cam, OFF3, keys=[2, 2, 2], paired=True).shape == (8, 8, 4)
        sc.load_gpu(fresh)
        good()
        # the device variant's pointers
        L, P = rr.lib(), C.c_void_p
        dev = "cuda:%d" % fresh.device
        out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
        aux = torch.zeros(64 + 4, dtype=torch.int32, device=dev)
        a = (fresh._h, 8, 8, C.byref(cam), None, ok.ctypes.data, 3, None)
        assert out.data_ptr() % 16 == 0 and aux.data_ptr() % 4 == 0
        assert L.rr_render_shutter_device(*a, P(out.data_ptr()), P(aux.data_ptr()), P(aux.data_ptr())) == 0
        assert L.rr_render_shutter_device(*a, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_shutter_device(*a, P(out.data_ptr()), P(aux.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_shutter_device(*a, P(out.data_ptr()), None, P(aux.data_ptr() + 1)) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_render_shutter_device(*a, None, None, P(aux.data_ptr())) == RR_ERR_INVALID_ARGUMENT
        fresh.wait()
        good()
        # a BLAS rebuilt since the TLAS: what render_nested refuses about the scene's state, capture refuses too
        mid = fresh.upload_mesh(*load("cube.obj"))
        fresh.build_blas(mid)
        refused(lambda: fresh.render_nested(8, 8, cam, 1), RR_ERR_STATE)
        refused(lambda: fresh.capture_scene_key(4), RR_ERR_STATE)
        assert fresh.scene_key_info(4).captured == 0
        good_keys = fresh.render_shutter(8, 8, cam, ok, lens=LENS)              # the live scene is not needed
        assert good_keys.shape == (8, 8, 4)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 9. the demo
def test_rrdemo_shutter_writes_render_shutter_frames(gpu, tmp_path):
    """rrdemo --compose --shutter: drawFrameShutter end to end.  With DT = 0 both keys hold the mesh where it is (under a top level: the
    demo's instance carries TRIANGLE_CULL_DISABLE), and its PPM is render_shutter's RGBA8 store; with DT > 0 the frame changes"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, SH.env_map())
    args = [exe, "--mesh", O.asset("shell.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--compose", "--spp", "2", "--lens", "0.2:5",
            "--dispersion", "2:30", "--materials", "1.5:0.8,0.1,0.1"]
    images = []
    for k, dt in enumerate(("0", "0.3")):
        out = subprocess.run(args + ["--shutter", "2:" + dt, "--out", str(tmp_path / ("s%d_%%03d.ppm" % k))], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "shutter frame: 2 positions x 2 keys" in out.stdout and "thin lens" in out.stdout, out.stderr + out.stdout
        raw = open(tmp_path / ("s%d_000.ppm" % k), "rb").read()
        head = b"P6\n64 48\n255\n"
        assert raw.startswith(head)
        images.append(np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3))
    assert not np.array_equal(images[0], images[1])
    env_rt, _ = rr.load_texture(hdr, 3)
    mid = gpu.load_scene(*load("shell.obj"), env_rt)
    gpu.build_tlas(rr.make_instances(meshes=[mid], flags=[rr._capi.INSTANCE_FLAG_CULL_DISABLE]))
    gpu.capture_scene_key(0)
    gpu.capture_scene_key(1)
    assert gpu.scene_key_info(0).top_level == 1
    table = [(1.5, (0.8, 0.1, 0.1))]
    gpu.set_materials(table)
    gpu.set_material_bands(*rr.material_bands(table, 30.0, 2))
    _, u8 = gpu.render_shutter(64, 48, rr.camera_orbit(0.01), 2, keys=2, lens=rr.Lens(0.2, 5.0), bands=2, rgba8=True)
    assert np.array_equal(images[0], u8[..., :3])
    assert subprocess.run(args[:9] + ["--spp", "2", "--shutter", "2:0.1"], capture_output=True, text=True, timeout=120).returncode == 2     # needs --compose


# ------------------------------------------------------------------------------------------------- 8. the device path
def test_the_device_variant_equals_the_host_path(gpu):
    import torch
    scs, cam, recs, iors, weights, _ = SH.moving_ref(3)
    SH.capture_keys(gpu, scs)
    gpu.set_materials(TABLE)
    gpu.set_material_bands(iors, weights)
    p = rr.default_params(max_reflect=3, **SH.KW)
    host = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, **OUT)
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_shutter(FW, FH, cam, recs, lens=LENS, params=p, device=True, **OUT)
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32 and df.device.index == gpu.device
        assert tuple(df.shape) == (FH, FW, 4) and tuple(du.shape) == (FH, FW, 4) and tuple(dc.shape) == (FH, FW)
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
    finally:
        gpu.reset_stream()
