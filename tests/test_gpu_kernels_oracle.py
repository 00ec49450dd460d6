"""Every render kernel, forced one at a time, against the CPU oracle.

The dispatch code picks one of four kernels for a launch (rr_stats.render_kernel): 0 k_render_fused, 1 k_render_lds,
2 k_render_paths, 7 k_stream_*.  The measured choice renders the first dispatch of a shape with k_render_fused, so tests that
dispatch each shape once only ever reach that kernel.  Here RR_DEBUG_KERNEL (read at rr_create) forces each kernel in turn and
every dispatch asserts which kernel rendered it: the forced one wherever it can render the launch, k_render_fused where it
cannot (the fall-back is silent).  Each compared frame is then held against the oracle's path-weight mode (the kernels'
summation order):
  * the float accumulator bit for bit (as uint32), the RGBA8 frame byte for byte;
  * the recursion's counters (rays, hits, misses, terminal hits, TIR) equal.  node_visits / tri_tests count visits of the
    GPU's own hierarchy, which the oracle does not build, so they are not compared here.
Batches are also checked slice by slice against single dispatches of the same kernel, and their counters against the sum.
"""
import collections
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from kernel_oracle_helpers import (check_launch,  # noqa: F401  (make_renderer: a fixture)
                                   check_slice, COUNTERS, counters, dispatch, FUSED, KERNEL_ID, make_renderer, oracle_frame, orbit, PATHS,
                                   report, STREAM)
from parity_cases import adversarial_constants, CULL_KINDS, CULL_SIZES, FRAME_CASES
from scenes import load, Scene, xf

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------- scenes


# ------------------------------------------------------------------------------------ which kernel can render a launch


# ------------------------------------------------------------------------------------------------- dispatch + compare


# --------------------------------------------------------------------------------- 1. single-mesh scenes (fused, lds, paths)
FLAG_CASES = [rr.DISPATCH_FLOAT_OUTPUT, 0, rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_TONEMAP_REINHARD]
SINGLE_MESH_VARIANTS = [("fused", {}), ("lds", {}), ("lds", {"RR_DEBUG_SHAPE": 1}), ("lds", {"RR_DEBUG_SHAPE": 2}),
                        ("lds", {"RR_DEBUG_TICKET": 19}), ("paths", {}), ("paths", {"RR_DEBUG_GROUP_TRACE": 0})]


@pytest.mark.parametrize("kernel,env", SINGLE_MESH_VARIANTS,
                         ids=["%s%s" % (k, "".join("-%s=%s" % (n[9:].lower(), v) for n, v in e.items())) for k, e in SINGLE_MESH_VARIANTS])
def test_single_mesh_frames_match_the_oracle(make_renderer, kernel, env):
    """FRAME_CASES (ragged sizes, parked rays, TIR on entry, no refraction, ...) plus float / RGBA8-only / tone-mapped output:
    24-slice batches on fused and LDS (every workgroup shape and ticket order), Depth 1 and 2 on paths (with and without
    group tracing)."""
    r = make_renderer(kernel, **env)
    shape = int(env.get("RR_DEBUG_SHAPE", 0))
    tally = collections.Counter()
    depths = (1, 2) if kernel == "paths" else (24,)
    cases = [(name, W, H, a, kw, rr.DISPATCH_FLOAT_OUTPUT) for name, W, H, a, kw in FRAME_CASES]
    cases += [("monkey.obj", 256, 192, 0.3, dict(max_refract=8), fl) for fl in FLAG_CASES[1:]]
    cases += [("sphere.obj", 160, 120, 0.9, dict(max_refract=6, max_reflect=1), FLAG_CASES[2])]
    scenes = {}
    n_forced = 0
    for name, W, H, angle, kw, flags in cases:
        if name not in scenes:
            scenes[name] = Scene(name, [load(name)], procedural_env(256, 128, seed=3))
        sc = scenes[name]
        sc.load_gpu(r)
        for depth in depths:
            got = check_launch(r, kernel, sc, W, H, orbit(angle, depth), kw, flags, tally, shape=shape,
                               tag="%s %s %dx%d depth %d %s flags %#x" % (kernel, name, W, H, depth, kw, flags))
            n_forced += got == KERNEL_ID[kernel]
    report("single mesh %s %s" % (kernel, env), tally)
    # the forced kernel really rendered the matrix: every case it supports (paths: all but max_reflect 3; lds: all but ott.obj
    # and meshes whose tree leaves no room beside the stacks)
    assert n_forced >= {"fused": len(cases), "lds": len(cases) - 4, "paths": 2 * (len(cases) - 1)}[kernel], (n_forced, len(cases), dict(tally))
    if kernel == "paths":
        assert tally[FUSED] >= 2          # max_reflect 3: the fall-back, asserted


def test_lds_does_not_render_what_it_cannot_hold(make_renderer):
    """the 15 472-triangle subdivided monkey does not fit LDS: forcing LDS renders it with k_render_fused (asserted), which
    still matches the oracle"""
    from refraction_raytracing_dxr_amd.synth import subdivide
    v, i = load("monkey.obj")
    v16, i16 = subdivide(v, 2)
    r = make_renderer("lds")
    sc = Scene("monkey16k", [(v16, i16)], procedural_env(128, 64, seed=5))
    sc.load_gpu(r)
    tally = collections.Counter()
    assert check_launch(r, "lds", sc, 128, 96, orbit(0.4, 3), dict(max_refract=8), rr.DISPATCH_FLOAT_OUTPUT, tally, tag="monkey16k") == FUSED
    report("lds monkey16k", tally)


# ------------------------------------------------------------------------------------ 2. two-level scenes (fused, stream)
def c4_scene():
    meshes = [load("shell.obj"), load("cube.obj"), load("ott.obj")]
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, -4.0), xf(0, 0, 4.0)], meshes=[0, 1, 2])
    return Scene("c4", meshes, procedural_env(256, 128, seed=4), inst)


def c5_scene(n_side=8, pitch=3.0, scale=0.9, key="c5"):
    xs = [xf(pitch * (i - (n_side - 1) / 2), 0, pitch * (j - (n_side - 1) / 2), (scale,) * 3) for i in range(n_side) for j in range(n_side)]
    return Scene(key, [load("monkey.obj")], procedural_env(256, 128, seed=5), rr.make_instances(transforms=xs, meshes=[0] * len(xs)))


def mixed_scene():
    """test_stream_renderer_renders_the_same_frames' first scene: rotations, non-uniform scale, cull flags, a zero mask"""
    meshes = [load("cube.obj"), load("monkey.obj"), load("sphere.obj")]
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4), xf(0.3, 0.2, 2.4, (0.7, 0.7, 0.7), -1.0),
                                         xf(0, 1.9, 0, (0.4, 0.4, 0.4), 0.2), xf(0, -1.8, 0.5, (0.5, 0.5, 0.5))],
                             meshes=[1, 0, 1, 2, 0], masks=[1, 1, 0xff, 1, 0], flags=[0, 0, 2, 1, 0])
    return Scene("mixed", meshes, procedural_env(256, 128, seed=9), inst)


def dense_scene():
    """the 100-monkey grid filling the frame"""
    xs = [xf(1.1 * (i - 4.5), 0.3 * ((i + j) % 3), 1.1 * (j - 4.5), (0.4, 0.4, 0.4), 0.3 * i) for i in range(10) for j in range(10)]
    return Scene("dense", [load("monkey.obj")], procedural_env(256, 128, seed=9), rr.make_instances(transforms=xs, meshes=[0] * 100))


def small_scene():
    """two small instances near the origin: a small screen rectangle, most tiles background"""
    inst = rr.make_instances(transforms=[xf(0.1, 0.05, 0, (0.12, 0.12, 0.12), 0.5), xf(-0.1, 0, 0.1, (0.08, 0.1, 0.08), 2.0)], meshes=[0, 1])
    return Scene("small", [load("monkey.obj"), load("sphere.obj")], procedural_env(256, 128, seed=9), inst)


# scene -> (W, H, start angle, orbit radius factor)
TWO_LEVEL = {"c4": (c4_scene, 240, 135, 0.01, 1.6), "c5": (c5_scene, 200, 112, 0.7, 5.0), "mixed": (mixed_scene, 211, 149, 0.3, 1.0),
             "dense": (dense_scene, 256, 192, 0.2, 1.0)}
BOUNCES = [(0, 0), (3, 0), (1, 2), (12, 2), (16, 2), (4, 3)]          # (max_refract, max_reflect); 4/3: stream cannot, fused renders


@pytest.mark.parametrize("scene_name", list(TWO_LEVEL))
@pytest.mark.parametrize("kernel", ["fused", "stream"])
def test_two_level_scenes_match_the_oracle(make_renderer, kernel, scene_name):
    """C4, the C5 8x8 grid, the mixed instanced scene and the dense 100-monkey grid at Depth 1, 3 and 16, every bounce limit,
    float / RGBA8-only / tone-mapped output; every stream pass without a queue overflow (dispatch() asserts
    traversal_overflow == 0 on each launch)"""
    make, W, H, angle, radius = TWO_LEVEL[scene_name]
    sc = make()
    r = make_renderer(kernel)
    sc.load_gpu(r)
    tally = collections.Counter()
    n_forced = n = 0
    for depth in (1, 3, 16):
        for bi, (refr, refl) in enumerate(BOUNCES):
            kw = dict(max_refract=refr, max_reflect=refl)
            flags = FLAG_CASES[(bi + depth) % 3]
            cams = orbit(angle + 0.05 * bi, depth, step=0.09, radius=radius)
            got = check_launch(r, kernel, sc, W, H, cams, kw, flags, tally,
                               tag="%s %s depth %d %s flags %#x" % (kernel, scene_name, depth, kw, flags))
            n += 1
            n_forced += got == KERNEL_ID[kernel]
    report("two-level %s %s" % (kernel, scene_name), tally)
    if kernel == "stream":
        assert n_forced == n - 3 and tally[FUSED] >= 3, (n_forced, n, dict(tally))   # all but the three 4/3 launches
    else:
        assert n_forced == n


@pytest.mark.parametrize("kernel", ["fused", "stream"])
def test_full_size_config5_window_matches_the_oracle(make_renderer, kernel):
    """C5 at full size (1 024 monkeys, 3840x2160, 16 bounces) on the forced kernel: an oracle window in the grid"""
    sc = c5_scene(n_side=32, scale=1.0, key="c5full")
    sc.env = procedural_env(512, 256, seed=6)
    r = make_renderer(kernel)
    sc.load_gpu(r)
    cam = rr.camera_orbit(0.4)
    for k in (0, 2):
        cam.camera_loc[k] *= 14.0
    cam.camera_loc[1] = 12.0
    W, H, kw = 3840, 2160, dict(max_refract=16)
    (frame, _), = dispatch(r, W, H, [cam], kw, 0)[0]
    st = r.stats()
    assert st.render_kernel == KERNEL_ID[kernel] and st.pixels == W * H
    for x0, y0 in ((1592, 1440), (2072, 1376)):         # windows on the grid's monkeys (the frame's centre falls between them)
        ref = oracle_frame(sc, cam, W, H, kw, region=(x0, y0, x0 + 48, y0 + 32))
        check_slice(frame[y0:y0 + 32, x0:x0 + 48], None, dict(rgba8=ref["rgba8"][y0:y0 + 32, x0:x0 + 48]), "c5 full %s (%d, %d)" % (kernel, x0, y0))
        assert ref["stats"].hits > 48 * 32 and ref["stats"].tir > 0
    report("c5 full %s" % kernel, collections.Counter({st.render_kernel: 2}))


# ----------------------------------------------------------------------------------------------- 3. sharded stream launches
def _alloc(n):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device="cuda:0")


def _orbit_angles(angle, n, step=0.01):
    """the angles rr_render_orbit* give its frames (float accumulation, as the C loop does)"""
    out, a = [], np.float32(angle)
    for _ in range(n):
        out.append(float(a))
        a = np.float32(a + np.float32(step))
    return out


@pytest.mark.parametrize("kernel", ["fused", "stream"])
def test_sharded_tile_partition_assembles_to_the_oracle(make_renderer, kernel):
    """world 3, round-robin tiles: every rank on the forced kernel (asserted), the gathered tiles assembled == the oracle, the
    ranks' counters summed == the oracle's"""
    import torch
    sc = mixed_scene()
    r = make_renderer(kernel)
    sc.load_gpu(r)
    W, H, world, kw = 211, 149, 3, dict(max_refract=6)
    cam = rr.camera_orbit(0.45)
    mx = rr.dist.max_local_tiles(W, H, world)
    gathered = _alloc(world * mx * 4096)
    total = np.zeros(len(COUNTERS), np.int64)
    r.set_camera(cam)
    for rank in range(world):
        r.set_tile_partition(rank, world)
        r.dispatch_rays(W, H, rr.default_params(flags=rr.DISPATCH_COLLECT_STATS, **kw))
        r.export_tiles(gathered.data_ptr() + rank * mx * 4096)
        r.wait()
        st = r.stats()
        assert st.render_kernel == KERNEL_ID[kernel] and st.traversal_overflow == 0
        total += counters(st)
    r.assemble_tiles(gathered.data_ptr(), world)
    r.wait()
    frame = r.read_frame()
    r.set_tile_partition(0, 1)
    ref = oracle_frame(sc, cam, W, H, kw)
    check_slice(frame, None, ref, "tiles world 3 %s" % kernel)
    assert tuple(total) == counters(ref["stats"])
    torch.cuda.synchronize()
    report("sharded tiles %s" % kernel, collections.Counter({KERNEL_ID[kernel]: 1}))


def mesh_sharded_frames(r, sc, W, H, F, angle, world, kw, no_cull=False):
    """every rank of a mesh-tile partitioned launch on this context, in turn, then the assembly -> (uint8 [F, H, W, 4], counters
    summed over the ranks, the kernels that rendered them, the partition)"""
    import torch
    flags = rr.DISPATCH_COLLECT_STATS | (rr.DISPATCH_DEBUG_NO_CULL if no_cull else 0)
    r.set_tile_partition(0, world)
    if no_cull:          # the whole-frame partition: what a NO_CULL launch renders and what its buffers are sized by
        part = rr._capi.MeshPartition()
        assert rr.lib().rr_host_mesh_partition(sc.bounds, None, F, W, H, world, C.byref(part)) == 0
    else:
        part = r.mesh_partition_for_orbit(W, H, F, angle=angle)
    fs, bs = max(part.max_mesh_tiles_per_rank, 1) * 3072, max(part.n_bg_tiles, 1) * 3072
    gat, bg, frames = _alloc(world * F * fs), _alloc(F * bs), _alloc(F * W * H * 4)
    torch.cuda.synchronize()
    total, kernels = np.zeros(len(COUNTERS), np.int64), []
    for rank in range(world):
        r.set_tile_partition(rank, world)
        r.render_orbit_mesh_sharded(W, H, F, C.c_void_p(gat.data_ptr() + rank * F * fs), fs, C.c_void_p(bg.data_ptr()) if rank == 0 else None, bs,
                                    angle=angle, params=rr.default_params(flags=flags, **kw))
        r.lane_join(0)
        r.wait()
        st = r.stats()
        assert st.traversal_overflow == 0
        kernels.append(st.render_kernel)
        total += counters(st)
    r.set_tile_partition(0, world)
    r.assemble_frames_mesh(C.c_void_p(gat.data_ptr()), F * fs, fs, C.c_void_p(bg.data_ptr()), bs, part, F, W, H, C.c_void_p(frames.data_ptr()), W * H * 4)
    r.wait()
    r.set_tile_partition(0, 1)
    out = frames.cpu().numpy().reshape(F, H, W, 4).copy()
    return out, total, kernels, part


@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("kernel", ["fused", "stream"])
def test_mesh_partition_assembles_to_the_oracle(make_renderer, kernel, world):
    """the mesh-tile partition at world 3 and 8, two frames per launch: assembled frames == the oracle's, counters too; and
    with RR_DISPATCH_DEBUG_NO_CULL (the whole-frame partition, buffers sized by it) the same frames"""
    sc = small_scene()
    r = make_renderer(kernel)
    sc.load_gpu(r)
    (W, H), F, angle, kw = ((211, 149) if world == 3 else (320, 200)), 2, 0.3, dict(max_refract=6)
    got, total, kernels, part = mesh_sharded_frames(r, sc, W, H, F, angle, world, kw)
    assert kernels == [KERNEL_ID[kernel]] * world, kernels
    assert part.rect_w > 0 and part.n_bg_tiles > 0           # a real rectangle: background tiles stay on rank 0
    ref_total = np.zeros(len(COUNTERS), np.int64)
    for k, a in enumerate(_orbit_angles(angle, F)):
        ref = oracle_frame(sc, rr.camera_orbit(a), W, H, kw)
        check_slice(got[k], None, ref, "mesh world %d %s frame %d" % (world, kernel, k))
        ref_total += counters(ref["stats"])
    assert np.array_equal(total, ref_total), (total, ref_total)
    nc, nc_total, nc_kernels, nc_part = mesh_sharded_frames(r, sc, W, H, F, angle, world, kw, no_cull=True)
    assert nc_part.rect_w == 0 and nc_part.n_bg_tiles == 0
    assert nc_kernels == [KERNEL_ID[kernel]] * world, nc_kernels
    assert np.array_equal(nc, got) and np.array_equal(nc_total, total)
    report("mesh partition world %d %s" % (world, kernel), collections.Counter({KERNEL_ID[kernel]: F}))


def test_no_cull_mesh_launch_refuses_buffers_sized_for_the_culled_partition(make_renderer):
    """RR_DISPATCH_DEBUG_NO_CULL renders the whole-frame partition: tile buffers sized from rr_mesh_partition_for_orbit (the
    culled one, fewer slots per rank) are refused before anything is launched -- the buffers keep their contents"""
    import torch
    sc = small_scene()
    r = make_renderer("stream")
    sc.load_gpu(r)
    W, H, F, world, angle = 320, 200, 2, 3, 0.3
    r.set_tile_partition(1, world)
    part = r.mesh_partition_for_orbit(W, H, F, angle=angle)
    whole = rr._capi.MeshPartition()
    assert rr.lib().rr_host_mesh_partition(sc.bounds, None, F, W, H, world, C.byref(whole)) == 0
    assert part.max_mesh_tiles_per_rank < whole.max_mesh_tiles_per_rank       # the two partitions differ
    fs = part.max_mesh_tiles_per_rank * 3072
    gat = torch.full((F * fs,), 0x5a, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(rr.RRError, match="RR_ERR_INVALID_ARGUMENT"):
        r.render_orbit_mesh_sharded(W, H, F, C.c_void_p(gat.data_ptr()), fs, None, 0, angle=angle,
                                    params=rr.default_params(flags=rr.DISPATCH_DEBUG_NO_CULL, max_refract=6))
    r.wait()
    torch.cuda.synchronize()
    assert bool((gat == 0x5a).all())
    # the same buffers without NO_CULL are the right size (rank 1 has no background buffer)
    r.render_orbit_mesh_sharded(W, H, F, C.c_void_p(gat.data_ptr()), fs, None, 0, angle=angle, params=rr.default_params(max_refract=6))
    r.lane_join(0)
    r.wait()
    r.set_tile_partition(0, 1)


# ------------------------------------------------------------------------------------------------- 4. culling on lds / stream
def _cull_case_bounds(scene):
    lo = np.array(scene.bounds[:3], np.float64)
    hi = np.array(scene.bounds[3:], np.float64)
    return lo, hi


@pytest.mark.parametrize("kernel", ["lds", "stream"])
def test_background_culling_on_the_lds_and_stream_kernels(make_renderer, kernel):
    """adversarial constants (test_background_culling_equals_tracing_every_primary_ray's) through k_render_lds -- 24-slice
    batches, which take the two-phase ticket order (rectangle strips, then background tiles) -- and through the stream renderer
    at Depth 1 and 3 (k_stream_background): every frame equals the same launch with RR_DISPATCH_DEBUG_NO_CULL, on the same
    kernel; a subset against the oracle"""
    if kernel == "lds":
        sc = Scene("monkey-cull", [load("monkey.obj")], procedural_env(128, 64, seed=21))
        plan = [(24, CULL_SIZES[k % len(CULL_SIZES)], k) for k in range(14)]
    else:
        sc = Scene("tlas-cull", [load("cube.obj"), load("monkey.obj")], procedural_env(128, 64, seed=21),
                   rr.make_instances(transforms=[xf(0, 0, 0, (0.6,) * 3), xf(1.2, 0.3, -0.8, (0.3,) * 3), xf(-0.9, -0.4, 0.7, (0.4,) * 3)],
                                     meshes=[1, 0, 1]))
        plan = [(1 if k % 2 == 0 else 3, CULL_SIZES[(k // 2) % len(CULL_SIZES)], k) for k in range(42)]
    r = make_renderer(kernel)
    sc.load_gpu(r)
    lo, hi = _cull_case_bounds(sc)
    rng = np.random.default_rng(31 if kernel == "lds" else 32)
    tally = collections.Counter()
    culled_cases = 0
    for depth, (W, H), k in plan:
        kind = CULL_KINDS[k % len(CULL_KINDS)]
        if depth >= 24:
            # one adversarial camera, moved a little per slice: the launch's rectangle is the union over its slices, which
            # independent cameras would spread over the whole frame (and no block would be culled)
            base, M, cam = adversarial_constants(rng, kind, lo, hi)
            cams = []
            for f in range(depth):
                cf = (cam * np.array([1.0 + 0.002 * f, 1.0, 1.0 - 0.001 * f, 1.0], np.float32)).astype(np.float32)
                cams.append((rr.scene_constants(M, cf), M, cf))
        else:
            cams = [adversarial_constants(rng, kind, lo, hi) for _ in range(depth)]
        kw = dict(max_refract=int(rng.choice([0, 2, 6])), max_reflect=int(rng.choice([0, 2])))
        tag = "%s case %d: %s %dx%d depth %d %s" % (kernel, k, kind, W, H, depth, kw)
        (fc, stc), (fn, stn) = [dispatch(r, W, H, [c[0] for c in cams], kw, rr.DISPATCH_FLOAT_OUTPUT | extra)
                                for extra in (0, rr.DISPATCH_DEBUG_NO_CULL)]
        assert stc.render_kernel == KERNEL_ID[kernel] and stn.render_kernel == KERNEL_ID[kernel], (tag, stc.render_kernel, stn.render_kernel)
        # the culled branch ran: more blocks shaded as one Miss than with every primary ray traced
        culled_cases += stc.background_waves > stn.background_waves
        assert counters(stc) == counters(stn), tag
        for f in range(depth):
            assert np.array_equal(fc[f][0], fn[f][0]), (tag, f)
            assert np.array_equal(fc[f][1].view(np.uint32), fn[f][1].view(np.uint32)), (tag, f)
        if W * H <= 40000:
            for f in sorted({0, depth - 1}):
                M, cam = cams[f][1].reshape(16), cams[f][2]
                ref = sc.oracle().render(M, cam, W, H, O.default_params(use_bvh=1, accum_mode=1, **kw))
                if np.isfinite(ref["rgb"]).all():
                    assert np.array_equal(fc[f][1][..., :3].view(np.uint32), ref["rgb"].view(np.uint32)), (tag, f)
                assert np.array_equal(fc[f][0], ref["rgba8"]), (tag, f)
                tally[stc.render_kernel] += 1
    report("culling %s" % kernel, tally)
    assert culled_cases >= len(plan) // 4, (culled_cases, len(plan))
    assert sum(tally.values()) >= 6


# ---------------------------------------------------------------------------------------------------- 5. after a refit
def test_refitted_two_instance_scene_on_stream_and_paths(make_renderer):
    """test_gpu_refit's two-instance scene, deformed: vertex update, BLAS update, TLAS update -- then stream (Depth 1, 3) and
    paths (Depth 1, 2) and fused render the deformed geometry as the oracle does"""
    from refit_helpers import _two_instances, deform
    verts, idx = load("monkey.obj")
    env = procedural_env(128, 64, seed=9)
    tally = collections.Counter()
    for kernel, depths in (("fused", (1, 3)), ("stream", (1, 3)), ("paths", (1, 2))):
        r = make_renderer(kernel)
        r.upload_envmap(env)
        mid = r.upload_mesh(verts, idx)
        r.build_blas(mid, allow_update=True)
        r.build_tlas(_two_instances(mid, 0.0), allow_update=True)
        r.set_tile_partition(0, 1)
        for step, kind in enumerate(("wave", "scale")):
            dv = deform(verts, kind, seed=step)
            if kind == "scale":
                dv["position"] = (dv["position"] - np.array([0.5, -0.25, 1.0], np.float32)) / np.float32(2.0)
            r.update_mesh_vertices(mid, dv)
            r.build_blas(mid, update=True)
            inst = _two_instances(mid, 0.3 * (step + 1))
            r.build_tlas(inst, update=True)
            o_inst = inst.copy()
            o_inst["blas"] = 0
            sc = Scene("refit-%d" % step, [(dv, idx)], env, o_inst)
            for depth in depths:
                for kw in (dict(max_refract=6), dict(max_refract=3, max_reflect=1)):
                    got = check_launch(r, kernel, sc, 200, 120, orbit(0.4 + step, depth), kw, rr.DISPATCH_FLOAT_OUTPUT, tally,
                                       tag="refit %s step %d depth %d %s" % (kernel, step, depth, kw))
                    assert got == KERNEL_ID[kernel]
        r.close()
    report("refit", tally)
    assert tally[STREAM] >= 8 and tally[PATHS] >= 8 and tally[FUSED] >= 8


# ------------------------------------------------------------------------------------- 6. the name of the kernel that rendered
# (scene, forced kernel, Depth) -> rr_stats.render_kernel_name without and with RR_DISPATCH_COLLECT_STATS.  The strings are a
# record: what the library reported while the stream renderer's name and the other kernels' names still had a buffer each.
RENDERED_BY = [
    ("monkey", "fused", 3, "k_render_fused<19, 2, false, false, false, unsigned int, 0>",
     "k_render_fused<19, 2, true, false, false, unsigned int, 0>"),
    ("monkey", "lds", 3, "k_render_lds<12, 2, false, false>",
     "k_render_lds<12, 2, true, false>"),
    ("monkey", "paths", 1, "k_render_paths<19, false, false, false>",
     "k_render_paths<19, true, false, false>"),
    ("small", "fused", 3, "k_render_fused<30, 2, false, true, false, unsigned short, 7>",
     "k_render_fused<30, 2, true, true, false, unsigned short, 7>"),
    ("small", "stream", 3, "k_stream_primary + k_stream_rays<30, false, unsigned short, 1|2, 6> x 2",
     "k_stream_primary + k_stream_rays<30, true, unsigned short, 1|2, 6> x 2"),
]


def test_every_renderer_reports_its_kernel_name(make_renderer):
    """monkey.obj on fused, lds and paths, then the two-instance scene on fused and stream, 64x48, each without and with the
    counters: after every launch rr_stats names the instantiation that rendered it -- one launcher after the other in one
    thread, so every name passes through the launchers' one name slot right after another renderer's"""
    scenes = {"monkey": Scene("monkey-names", [load("monkey.obj")], procedural_env(128, 64, seed=3)), "small": small_scene()}
    for scene, kernel, depth, plain, counted in RENDERED_BY:
        r = make_renderer(kernel)
        scenes[scene].load_gpu(r)
        for flags, want in ((0, plain), (rr.DISPATCH_COLLECT_STATS, counted)):
            cams = orbit(0.3, depth)
            if depth == 1:
                r.set_camera(cams[0])
                r.dispatch_rays(64, 48, rr.default_params(flags=flags))
            else:
                r.dispatch_rays_batch(64, 48, cams, rr.default_params(flags=flags))
            r.wait()
            st = r.stats()
            print("%s %s depth %d flags %#x: kernel %d %r" % (scene, kernel, depth, flags, st.render_kernel, st.render_kernel_name.decode()))
            assert st.render_kernel == KERNEL_ID[kernel], (scene, kernel, flags, st.render_kernel)
            assert st.render_kernel_name.decode() == want, (scene, kernel, flags, st.render_kernel_name)
        r.close()
