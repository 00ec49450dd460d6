"""GPU: indexed meshes -- every build, refit and consumer behind the index buffer.

Every other file of the suite uploads indices = 0..3T-1, so k_tri_boxes, k_pack_tris and k_refit_blas only ever gather through
the identity and n_verts == n_idx everywhere.  Here the meshes of tests/indexed_meshes.py (welded, shuffled, with unreferenced
far vertices, padded, smooth, with index-degenerate and duplicate triangles, natively indexed grids, one triangle over four
vertices) go through the builders, the queries, the render kernels and the update / refit path.  A mesh (V, I) is held against
  * its flat twin (V[I], arange) on the same renderer -- the form the rest of the suite proves correct -- byte for byte: the
    BLAS, hits, multi-hit slots, colours, frames, and the traversal counters (the hierarchy is the same, so is the walk);
  * the CPU oracle given (V, I) directly (tests/test_indexed_cpu.py pins that it honours the indices), bit for bit.
No tolerance anywhere: exact equality over all rays, pixels and bytes.
"""
import collections
import functools

import numpy as np
import pytest

import indexed_meshes as IM
import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from kernel_oracle_helpers import (FUSED, KERNEL_ID, LDS, PATHS, STREAM, check_launch, counters, dispatch,  # noqa: F401  (make_renderer: a fixture)
                                   make_renderer, orbit, report)
from refit_helpers import blas_bytes, deform
from scenes import Scene, build, check_closest, gpu, load, oracle_scene, random_rays, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import camera_rays, check_against_oracle, view_constants

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT = 1
WALK = ("node_visits", "tri_tests", "waves", "background_waves")     # equal between a mesh and its flat twin: same hierarchy bytes
ASSET_NAMES = ("cube.obj", "monkey.obj", "ott.obj")
CASES = [(n, v) for n in ASSET_NAMES for v in IM.VARIANTS] + [("grid%d" % n, "native") for n in IM.GRID_SIDES] + [("tri", "native")]
SMALL_CASES = [c for c in CASES if c[0] != "grid181"]                 # what the consumers run on (the 65 522-triangle grid: builds only)
CASE_IDS = ["%s-%s" % (n.replace(".obj", ""), v) for n, v in CASES]
SMALL_IDS = ["%s-%s" % (n.replace(".obj", ""), v) for n, v in SMALL_CASES]


@functools.lru_cache(maxsize=None)
def mesh(name, var):
    """-> (V, I) of a case"""
    if name == "tri":
        return IM.one_triangle()
    if name.startswith("grid"):
        return IM.heightfield(int(name[4:]), seed=2)
    return IM.variant(var, load(name)[0], seed=len(name))


def degenerate_ids(name):
    """(p, the index-degenerate triangles, the duplicate of p) of the `degenerate` variant of an asset"""
    return IM.degenerate_layout(len(load(name)[1]) // 3, seed=len(name))


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def show(gpu, mid):
    gpu.build_tlas(rr.make_instances(meshes=[mid]))


def blas_state(gpu, mid):
    """everything a build leaves: fp32 nodes, triangle records, traversal nodes, the six grid floats, the depth"""
    show(gpu, mid)
    return [x.tobytes() for x in blas_bytes(gpu, mid)] + [int(gpu.stats().bvh_depth)]


def aimed_rays(V, I, prims, n_each=6, seed=0):
    """rays through interior points of the given triangles, from both sides, with no culling"""
    rng = np.random.default_rng(seed)
    o, d = [], []
    for p in prims:
        tri = V["position"][I[3 * p:3 * p + 3]].astype(np.float64)
        nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        nrm = nrm / np.linalg.norm(nrm) if np.linalg.norm(nrm) > 0 else np.array([0.0, 0.0, 1.0])
        for k in range(n_each):
            w = rng.dirichlet([2.0, 2.0, 2.0])
            pt = w @ tri
            side = 1.0 if k % 2 == 0 else -1.0
            dirn = -side * nrm + 0.2 * rng.normal(size=3)
            dirn /= np.linalg.norm(dirn)
            o.append(pt - 3.0 * dirn)
            d.append(dirn)
    return rr.pack_rays(np.array(o), np.array(d), 1e-4, 100.0, flags=0)


def query_set(name, var, n):
    """random_rays plus the axis-aligned rays of test_trace_rays_bit_exact_vs_brute_force; for `degenerate`, rays through the
    duplicated triangle and along the index-degenerate ones"""
    rays = random_rays(n, seed=len(name) + len(var))
    rays["dir"][:8] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 0, 1)]
    rays["origin"][:8] = [(-5, 0, 0), (5, 0.25, 0.125), (0, -5, 0), (0.1, 5, 0.1), (0, 0, -5), (0.2, 0.1, 5), (-5, 1, 1), (1, -1, -5)]
    rays["tmax"][:8] = 100.0
    if var == "degenerate":
        V, I = mesh(name, var)
        p, deg, dup = degenerate_ids(name)
        rays = np.concatenate([aimed_rays(V, I, [p, dup], n_each=10), rays])
        # along the edge a-b that (a, a, b) and (a, b, a) collapse to, and through the point (a, a, a)
        a, b = (V["position"][k].astype(np.float64) for k in I[3 * p:3 * p + 2])
        ts = np.linspace(0.0, 1.0, 9)[:, None]
        pts = a + ts * (b - a)
        for org in ((0.3, 3.0, 0.2), (-2.5, -0.4, 1.7)):
            dirs = pts - np.array(org)
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            rays = np.concatenate([rr.pack_rays(np.tile(org, (len(pts), 1)), dirs, 1e-4, 100.0, flags=0), rays])
    return rays


# ============================================================================================== 1. the BLAS
@pytest.mark.parametrize("fast_build", [False, True], ids=["trace", "fast"])
@pytest.mark.parametrize("name,var", CASES, ids=CASE_IDS)
def test_indexed_mesh_builds_the_blas_of_its_flat_twin(gpu, name, var, fast_build):
    """nodes, triangle records, traversal nodes, grid and depth of (V, I) == those of (V[I], arange), both builders: a wrong
    gather in k_tri_boxes or k_pack_tris, or bounds / a grid widened by unreferenced vertices, changes a byte"""
    V, I = mesh(name, var)
    a = blas_state(gpu, build(gpu, V, I, fast_build=fast_build, tlas=False))
    b = blas_state(gpu, build(gpu, *IM.flat(V, I), fast_build=fast_build, tlas=False))
    for k, what in enumerate(("nodes", "triangle records", "qnodes", "grid origin", "grid cell", "depth")):
        assert a[k] == b[k], what
    nodes, tris = gpu.download_blas(build(gpu, V, I, fast_build=fast_build, tlas=False))
    T = len(I) // 3
    assert len(tris) == T and np.array_equal(np.sort(tris["prim"]), np.arange(T))
    P = V["position"][I].reshape(T, 3, 3)[tris["prim"]]
    assert same(tris["v0"], P[:, 0]) and same(tris["e1"], P[:, 1] - P[:, 0]) and same(tris["e2"], P[:, 2] - P[:, 0])
    # the grid spans the referenced vertices' bounds (holes / padded: the far ones do not show)
    _, org, cell = gpu.download_qnodes(build(gpu, V, I, fast_build=fast_build, tlas=False))
    ref = V["position"][I].astype(np.float64)
    org, cell = org.astype(np.float64), cell.astype(np.float64)
    assert np.all(org - 32768.0 * cell <= ref.min(0)) and np.all(org + 32768.0 * cell >= ref.max(0))
    ext, mag = ref.max(0) - ref.min(0), np.maximum(np.abs(ref.min(0)), np.abs(ref.max(0)))
    assert np.all(65530.0 * cell <= 1.001 * np.maximum(ext, 1e-6 * mag) + 1e-30)       # ... and no more than those (per axis)


# ============================================================================================== 2. queries
@pytest.mark.parametrize("name,var", SMALL_CASES, ids=SMALL_IDS)
def test_closest_hit_queries_on_an_indexed_mesh(gpu, name, var):
    """trace_rays and query_rays: hit, prim, t, u, v == the oracle's brute force over (V, I), and == the flat twin's bytes"""
    V, I = mesh(name, var)
    rays = query_set(name, var, 600 if name == "ott.obj" else 1500)
    show(gpu, build(gpu, V, I, tlas=False))
    t, q = gpu.trace_rays(rays), gpu.query_rays(rays)
    show(gpu, build(gpu, *IM.flat(V, I), tlas=False))
    assert same(t, gpu.trace_rays(rays)) and same(q, gpu.query_rays(rays))
    assert same(t, q)
    n_hit = check_closest(q, oracle_scene([(V, I)]), rays)
    assert n_hit > (len(rays) // 40 if name != "tri" else 5), n_hit
    if var == "degenerate":
        p, deg, dup = degenerate_ids(name)
        assert np.all(q["prim"][:18][q["hit"][:18] != 0] < deg[0])
        aimed = q[18:38]
        # an equal-t tie goes to the lower primitive: the duplicate is never the closest hit (at least a few of the 20 rays, which
        # all pass through the triangle, see it unoccluded)
        assert np.all(aimed["hit"] != 0) and np.sum(aimed["prim"] == p) >= 3 and not np.any(q["prim"][q["hit"] != 0] == dup)
        assert not np.isin(q["prim"][q["hit"] != 0], deg).any()


@pytest.mark.parametrize("name,var", SMALL_CASES, ids=SMALL_IDS)
def test_multi_hit_queries_on_an_indexed_mesh(gpu, name, var):
    """query_rays_multi with counts: slots and counts == the flat twin's; slot 0 == the closest-hit query (oracle-checked above);
    `degenerate`: the duplicate triangle is reported next to its original, an index-degenerate triangle never"""
    V, I = mesh(name, var)
    rays = query_set(name, var, 1500)
    show(gpu, build(gpu, V, I, tlas=False))
    hits, counts = gpu.query_rays_multi(rays, 16, counts=True)
    q = gpu.query_rays(rays)
    show(gpu, build(gpu, *IM.flat(V, I), tlas=False))
    fh, fc = gpu.query_rays_multi(rays, 16, counts=True)
    assert same(hits, fh) and same(counts, fc)
    assert np.array_equal(counts > 0, q["hit"] != 0)
    if name in ASSET_NAMES:
        assert (counts > 1).sum() > 10                   # closed meshes: rays cross more than one triangle
    for f in ("t", "u", "v", "prim", "inst"):
        assert same(hits[:, 0][f], q[f]), f
    if var == "degenerate":
        p, deg, dup = degenerate_ids(name)
        live = hits["hit"] != 0
        assert not np.isin(hits["prim"][live], deg).any()
        assert np.all(counts[:18] == np.sum(live[:18], axis=1))
        n_pairs = 0
        for r in range(len(rays)):
            h = hits[r, :min(int(counts[r]), 16)]
            at = np.flatnonzero(h["prim"] == p)
            twin = np.flatnonzero(h["prim"] == dup)
            if len(at) and at[0] < 15:              # (p in the last slot: its twin was truncated)
                assert len(twin) == 1 and twin[0] == at[0] + 1, r
                a, b = h[at[0]], h[twin[0]]
                assert all(same(a[f], b[f]) for f in ("t", "u", "v", "hit", "inst")), r
                n_pairs += 1
            elif not len(at):
                assert not len(twin), r
        assert n_pairs >= 15                         # the 20 aimed rays pass through its interior (a few may graze an edge in fp32)


@pytest.mark.parametrize("name,var", SMALL_CASES, ids=SMALL_IDS)
def test_radiance_queries_on_an_indexed_mesh(gpu, name, var):
    """shade_rays on a frame's primary rays == the oracle's frame of (V, I) (float bits, RGBA8, tone-mapped RGBA8, ray counts) and
    == the flat twin's colours: the normal records k_pack_tris gathers are what the shader interpolates"""
    V, I = mesh(name, var)
    w, h = 96, 72
    env = procedural_env(64, 32, seed=3)
    gpu.upload_envmap(env)
    s = oracle_scene([(V, I)])
    s.set_envmap(env)
    _, M, cam = view_constants(0.7, 0.45 if name != "ott.obj" else rr.FOV_Y, w, h)
    rays = camera_rays(M, cam, w, h)
    show(gpu, build(gpu, V, I, tlas=False))
    ref = check_against_oracle(gpu, s, M, cam, w, h, rays, max_refract=6)
    assert ref["stats"].hits > 100
    a = gpu.shade_rays(rays, rr.default_params(max_refract=6), rgba8=True, ray_counts=True)
    show(gpu, build(gpu, *IM.flat(V, I), tlas=False))
    b = gpu.shade_rays(rays, rr.default_params(max_refract=6), rgba8=True, ray_counts=True)
    assert all(same(x, y) for x, y in zip(a, b))


# ============================================================================================== 3. frames
def twin_scene(key, meshes, env, instances=None):
    return Scene(key, meshes, env, instances), Scene(key + "/flat", [IM.flat(V, I) for V, I in meshes], env, instances)


def check_against_flat_twin(r, sc, flat_sc, W, H, cams, kw, flags, tag):
    """the launch on (V, I) and on the flat twin: the same kernel, frame bytes, recursion counters and walk"""
    sc.load_gpu(r)
    fa, sa = dispatch(r, W, H, cams, kw, flags)
    flat_sc.load_gpu(r)
    fb, sb = dispatch(r, W, H, cams, kw, flags)
    assert sa.render_kernel == sb.render_kernel and sa.bvh_depth == sb.bvh_depth, tag
    for f in range(len(cams)):
        assert same(fa[f][0], fb[f][0]) and same(fa[f][1], fb[f][1]), (tag, f)
    assert counters(sa) == counters(sb), tag
    walk_a, walk_b = [int(getattr(sa, k)) for k in WALK], [int(getattr(sb, k)) for k in WALK]
    assert walk_a == walk_b, (tag, WALK, walk_a, walk_b)
    return sa


@pytest.mark.parametrize("kernel", ["fused", "lds", "paths"])
def test_frames_of_indexed_meshes_on_every_single_mesh_kernel(make_renderer, kernel):
    """every case on the forced kernel (asserted): float accumulator and RGBA8 == the oracle's path-weight frame of (V, I),
    recursion counters == the oracle's; frame, counters and walk == the flat twin's"""
    r = make_renderer(kernel)
    env = procedural_env(128, 64, seed=3)
    tally = collections.Counter()
    W, H, kw, flags = 160, 120, dict(max_refract=8), rr.DISPATCH_FLOAT_OUTPUT
    n_culled = 0
    for name, var in SMALL_CASES:
        if kernel == "lds" and name == "ott.obj":
            continue                                    # does not fit LDS (test_lds_does_not_render_what_it_cannot_hold)
        sc, flat_sc = twin_scene("idx-%s-%s" % (name, var), [mesh(name, var)], env)
        tag = "%s %s %s" % (kernel, name, var)
        for depth in ((1, 2) if kernel == "paths" else (1, 3)):
            cams = orbit(0.4, depth)
            sc.load_gpu(r)
            got = check_launch(r, kernel, sc, W, H, cams, kw, flags, tally, tag=tag)
            assert got == KERNEL_ID[kernel], (tag, got)
            st = check_against_flat_twin(r, sc, flat_sc, W, H, cams, kw, flags, tag)
            n_culled += st.background_waves > 0
    report("indexed single mesh %s" % kernel, tally)
    n_cases = len(SMALL_CASES) - (len(IM.VARIANTS) if kernel == "lds" else 0)
    assert tally[KERNEL_ID[kernel]] >= 3 * n_cases and sum(tally.values()) == tally[KERNEL_ID[kernel]], dict(tally)
    print("indexed single mesh %s: %d launches with background blocks" % (kernel, n_culled))
    if kernel != "paths":                                # (k_render_paths renders the rectangle only and counts no background waves)
        assert n_culled > 0                              # background blocks were shaded as one Miss: the far vertices did not spoil it


def _pair(shift=0.0):
    t0 = xf(-0.9, 0.0, 0.0)
    t1 = np.array([[0.0, 0.0, 0.7, 0.9 + shift], [0.0, 0.7, 0.0, 0.2 * shift], [-0.7, 0.0, 0.0, 0.0]], np.float32)
    return [t0, t1]


@pytest.mark.parametrize("kernel", ["fused", "stream"])
def test_frames_of_a_two_instance_scene_of_indexed_meshes(make_renderer, kernel):
    """two instances (one rotated and scaled) of every monkey variant, and a scene of two different indexed meshes, on fused and
    on the stream renderer (asserted), Depth 1 and 3: == the oracle, == the flat twin"""
    r = make_renderer(kernel)
    env = procedural_env(128, 64, seed=9)
    tally = collections.Counter()
    W, H, flags = 200, 120, rr.DISPATCH_FLOAT_OUTPUT
    scenes = [("monkey.obj-%s x2" % v, [mesh("monkey.obj", v)], [0, 0]) for v in IM.VARIANTS]
    scenes.append(("holes monkey + padded cube", [mesh("monkey.obj", "holes"), mesh("cube.obj", "padded")], [0, 1]))
    scenes.append(("grid8 + tri", [mesh("grid8", "native"), mesh("tri", "native")], [0, 1]))
    for key, meshes, which in scenes:
        inst = rr.make_instances(transforms=_pair(), meshes=which, masks=[1, 1], flags=[0, rr._capi.INSTANCE_FLAG_CULL_DISABLE])
        sc, flat_sc = twin_scene("idx2-" + key, meshes, env, inst)
        for depth, kw in ((1, dict(max_refract=6)), (3, dict(max_refract=3, max_reflect=1))):
            cams = orbit(0.4, depth)
            sc.load_gpu(r)
            got = check_launch(r, kernel, sc, W, H, cams, kw, flags, tally, tag="%s %s" % (kernel, key))
            assert got == KERNEL_ID[kernel], (key, got)
            check_against_flat_twin(r, sc, flat_sc, W, H, cams, kw, flags, "%s %s" % (kernel, key))
    report("indexed two-instance %s" % kernel, tally)
    assert tally[KERNEL_ID[kernel]] >= 4 * len(scenes)


def test_unreferenced_vertices_do_not_move_the_mesh_partition(gpu):
    """rr_mesh_partition_for_orbit (the screen rectangle of the scene's bounds, its mesh tiles and background tiles) of `holes`
    and `padded` == the flat twin's; the far vertices, projected, would cover the frame"""
    W, H, F, world = 320, 200, 2, 3
    for name, var in (("monkey.obj", "holes"), ("cube.obj", "holes"), ("monkey.obj", "padded")):
        V, I = mesh(name, var)
        parts = []
        for verts, idx in ((V, I), IM.flat(V, I)):
            mid = build(gpu, verts, idx, tlas=False)
            gpu.build_tlas(rr.make_instances(transforms=[xf(0.1, 0.05, 0, (0.2, 0.2, 0.2), 0.5)], meshes=[mid]))
            gpu.set_tile_partition(1, world)
            parts.append(gpu.mesh_partition_for_orbit(W, H, F, angle=0.3))
            gpu.set_tile_partition(0, 1)
        assert bytes(parts[0]) == bytes(parts[1]), (name, var)
        assert 0 < parts[0].rect_w < W and 0 < parts[0].rect_h < H and parts[0].n_bg_tiles > 0


# ============================================================================================== 4. updates and refits
def moved(V, kind, seed):
    """test_gpu_refit's deformation of a vertex array (unreferenced vertices move with the rest; their normals stay garbage)"""
    with np.errstate(all="ignore"):
        dv = deform(V, kind, seed=seed)
    if kind == "scale":                                  # x3 and translated -> x1.5 about the origin: bounds and grid move, still in view
        dv["position"] = (dv["position"] - np.array([0.5, -0.25, 1.0], np.float32)) / np.float32(2.0)
    return dv


def to_device(gpu, V):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(V).view(np.float32).reshape(-1, 8).copy()).to("cuda:%d" % gpu.device)
    torch.cuda.synchronize()
    return t


def frame_of(gpu, mid, angle=0.9, W=128, H=96, instances=None):
    gpu.build_tlas(rr.make_instances(meshes=[mid]) if instances is None else instances)
    gpu.set_tile_partition(0, 1)
    sc = rr.camera_orbit(angle)
    gpu.set_camera(sc)
    gpu.dispatch_rays(W, H, rr.default_params(max_refract=6, flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS))
    rgba, f32 = gpu.read_frame(want_float=True)
    st = gpu.stats()
    assert st.traversal_overflow == 0 and st.stats_valid
    return rgba, f32, counters(st), sc


def check_frame_against_oracle(frame, V, I, env, W=128, H=96, instances=None):
    rgba, f32, cnt, sc = frame
    s = oracle_scene([(V, I)], instances=instances)
    s.set_envmap(env)
    ref = s.render(np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32), W, H,
                   O.default_params(use_bvh=1, accum_mode=1, max_refract=6))
    assert np.array_equal(f32[..., :3].view(np.uint32), ref["rgb"].view(np.uint32)) and np.array_equal(rgba, ref["rgba8"])
    assert cnt == counters(ref["stats"])
    return ref


UPDATE_CASES = [("monkey.obj", "welded"), ("monkey.obj", "holes"), ("monkey.obj", "padded"), ("monkey.obj", "degenerate"),
                ("cube.obj", "shuffled"), ("ott.obj", "welded"), ("grid8", "native"), ("tri", "native")]


@pytest.mark.parametrize("fast_build", [False, True], ids=["trace", "fast"])
@pytest.mark.parametrize("name,var", UPDATE_CASES, ids=["%s-%s" % (n.replace(".obj", ""), v) for n, v in UPDATE_CASES])
def test_vertex_updates_and_refits_with_fewer_vertices_than_indices(gpu, name, var, fast_build):
    """update_mesh_vertices with n_verts != n_idx, from the host and from a [n_verts, 8] tensor, then build_blas(update=True):
    an identity update refits to the bytes of the build; a deformed V' refits to the bytes of the flat twin's refit to V'[I];
    traces and the frame == a fresh build's and the oracle's over (V', I)"""
    V, I = mesh(name, var)
    assert len(V) != len(I)
    env = procedural_env(64, 32, seed=5)
    gpu.upload_envmap(env)
    mid = build(gpu, V, I, fast_build=fast_build, allow_update=True, tlas=False)
    built = blas_state(gpu, mid)
    assert built == blas_state(gpu, build(gpu, V, I, fast_build=fast_build, tlas=False))
    for src in (V, to_device(gpu, V)):
        gpu.update_mesh_vertices(mid, src)
        gpu.build_blas(mid, update=True)
        assert blas_state(gpu, mid) == built
    twin = build(gpu, *IM.flat(V, I), fast_build=fast_build, allow_update=True, tlas=False)
    dev = build(gpu, V, I, fast_build=fast_build, allow_update=True, tlas=False)
    for step, kind in enumerate(("wave", "scale", "jitter")):
        dv = moved(V, kind, seed=step + len(name))
        gpu.update_mesh_vertices(mid, dv)
        gpu.build_blas(mid, update=True)
        gpu.update_mesh_vertices(twin, np.ascontiguousarray(dv[I]))
        gpu.build_blas(twin, update=True)
        gpu.update_mesh_vertices(dev, to_device(gpu, dv))
        gpu.build_blas(dev, update=True)
        a = blas_state(gpu, mid)
        assert a == blas_state(gpu, twin), kind
        assert a == blas_state(gpu, dev), kind
        # consumers: the refitted mesh against a fresh build of (V', I) and against the oracle
        P = dv["position"][I].astype(np.float64)
        c, rad = (P.min(0) + P.max(0)) / 2, np.abs(P.max(0) - P.min(0)).max() / 2
        rays = random_rays(500, seed=step, radius=4.0 * rad, extent=1.2 * rad)
        rays["origin"] += c.astype(np.float32)
        show(gpu, mid)
        hits = gpu.query_rays(rays)
        fresh = build(gpu, dv, I, fast_build=fast_build, tlas=False)
        show(gpu, fresh)
        assert same(hits, gpu.query_rays(rays)), kind
        assert check_closest(hits, oracle_scene([(dv, I)]), rays) > 0, kind
        fr = frame_of(gpu, mid)
        ff = frame_of(gpu, fresh)
        assert same(fr[0], ff[0]) and same(fr[1], ff[1]) and fr[2] == ff[2], kind
        ref = check_frame_against_oracle(fr, dv, I, env)
        assert ref["stats"].hits > 20


def test_moving_only_unreferenced_vertices_changes_nothing(gpu):
    """`holes`: the unreferenced vertices move (further out, into the mesh, onto the camera's side) -- bounds, grid, every BLAS
    byte and the frame stay"""
    V, I = mesh("monkey.obj", "holes")
    env = procedural_env(64, 32, seed=6)
    gpu.upload_envmap(env)
    mid = build(gpu, V, I, allow_update=True, tlas=False)
    built = blas_state(gpu, mid)
    frame = frame_of(gpu, mid)
    check_frame_against_oracle(frame, V, I, env)
    hm = IM.hole_mask(V, I)
    assert hm.sum() == 3 * IM.N_HOLES
    rng = np.random.default_rng(8)
    for step, make in enumerate((lambda n: rng.uniform(-3e6, 3e6, (n, 3)), lambda n: rng.uniform(-0.3, 0.3, (n, 3)),
                                 lambda n: np.tile([0.0, 0.0, 2.5], (n, 1)), lambda n: np.full((n, 3), 1e18))):
        dv = V.copy()
        dv["position"][hm] = make(int(hm.sum())).astype(np.float32)
        gpu.update_mesh_vertices(mid, dv if step % 2 == 0 else to_device(gpu, dv))
        gpu.build_blas(mid, update=True)
        assert blas_state(gpu, mid) == built, step
        again = frame_of(gpu, mid)
        assert same(again[0], frame[0]) and same(again[1], frame[1]) and again[2] == frame[2], step


def test_two_instance_scene_of_an_indexed_mesh_through_blas_and_tlas_updates(gpu):
    """vertex update (host, then device) -> BLAS update -> TLAS update of two instances of a shuffled mesh: the frame == the
    oracle's over (V', I) and == a fresh build's"""
    V, I = mesh("monkey.obj", "shuffled")
    env = procedural_env(128, 64, seed=9)
    gpu.upload_envmap(env)
    mid = build(gpu, V, I, allow_update=True, tlas=False)

    def inst_of(m, shift):
        return rr.make_instances(transforms=_pair(shift), meshes=[m, m], masks=[1, 1], flags=[0, rr._capi.INSTANCE_FLAG_CULL_DISABLE])
    gpu.build_tlas(inst_of(mid, 0.0), allow_update=True)
    for step, kind in enumerate(("wave", "jitter")):
        dv = moved(V, kind, seed=step)
        gpu.update_mesh_vertices(mid, dv if step == 0 else to_device(gpu, dv))
        gpu.build_blas(mid, update=True)
        gpu.build_tlas(inst_of(mid, 0.3 * (step + 1)), update=True)
        gpu.set_tile_partition(0, 1)
        sc = rr.camera_orbit(0.4 + step)
        gpu.set_camera(sc)
        p = rr.default_params(max_refract=6, flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS)
        gpu.dispatch_rays(200, 120, p)
        rgba, f32 = gpu.read_frame(want_float=True)
        st = gpu.stats()
        assert st.traversal_overflow == 0
        check_frame_against_oracle((rgba, f32, counters(st), sc), dv, I, env, 200, 120, inst_of(0, 0.3 * (step + 1)))
        fresh = build(gpu, dv, I, tlas=False)
        gpu.build_tlas(inst_of(fresh, 0.3 * (step + 1)))
        gpu.dispatch_rays(200, 120, p)
        r2, f2 = gpu.read_frame(want_float=True)
        assert same(rgba, r2) and same(f32, f2) and counters(st) == counters(gpu.stats())
        gpu.build_tlas(inst_of(mid, 0.3 * (step + 1)), allow_update=True)      # back to the updatable scene for the next step


def test_refusals_leave_an_indexed_mesh_as_it_was():
    """wrong vertex counts (n_idx among them), out-of-range indices and a non-finite unreferenced vertex -- at upload, on the host
    update path and on the device update path -- are RR_ERR_INVALID_ARGUMENT, and the mesh renders the frame it rendered before"""
    import torch
    gpu = rr.Renderer(0)
    try:
        V, I = mesh("monkey.obj", "holes")
        nv, ni = len(V), len(I)
        assert nv < ni
        gpu.upload_envmap(procedural_env(64, 32, seed=4))
        mid = build(gpu, V, I, allow_update=True, tlas=False)
        before_blas = blas_state(gpu, mid)
        before = frame_of(gpu, mid)

        def unchanged(what):
            assert blas_state(gpu, mid) == before_blas, what
            now = frame_of(gpu, mid)
            assert same(now[0], before[0]) and same(now[1], before[1]) and now[2] == before[2], what

        def refused(call, what):
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, what

        # ---- vertex counts: only n_verts is accepted (the flat twin's n_idx records are not)
        big = np.ascontiguousarray(np.concatenate([V, V, V, V, V, V])[:ni + 1])
        for n in (ni, nv - 1, nv + 1, 1, ni + 1):
            refused(lambda: gpu.update_mesh_vertices(mid, big[:n]), "host update with %d vertices" % n)
            t = to_device(gpu, big[:n])
            refused(lambda: gpu.update_mesh_vertices(mid, t), "device update with %d vertices" % n)
            gpu.wait()
        refused(lambda: gpu.update_mesh_vertices(mid, np.ascontiguousarray(V[I])), "host update with V[I]")
        gpu.build_blas(mid, update=True)                   # nothing is pending, nothing moved
        unchanged("after the refused counts")

        # ---- indices: n_verts and 0xffffffff
        n_meshes = gpu.upload_mesh(V[:3], np.arange(3, dtype=np.uint32))
        for bad_index in (nv, 0xffffffff):
            for at in (0, ni // 2, ni - 1):
                bad = I.copy()
                bad[at] = bad_index
                refused(lambda: gpu.upload_mesh(V, bad), "index %#x at %d" % (bad_index, at))
        assert gpu.upload_mesh(V[:3], np.arange(3, dtype=np.uint32)) == n_meshes + 1      # the refused uploads added no mesh
        unchanged("after the refused indices")

        # ---- a non-finite (or huge) unreferenced vertex: every position must be valid, referenced or not, on all three paths
        hole = int(np.flatnonzero(IM.hole_mask(V, I))[IM.N_HOLES])      # an inside one
        for val in (np.nan, np.inf, -np.inf, 1e19):
            bad = V.copy()
            bad["position"][hole, 1] = val
            refused(lambda: gpu.upload_mesh(bad, I), "upload with %r in an unreferenced vertex" % val)
            refused(lambda: gpu.update_mesh_vertices(mid, bad), "host update with %r" % val)
            unchanged("after the refused host update with %r" % val)
            t = to_device(gpu, bad)
            gpu.update_mesh_vertices(mid, t)                 # device path: found by the check kernel ...
            refused(lambda: gpu.build_blas(mid, update=True), "device update with %r" % val)   # ... reported by the next build
            gpu.build_blas(mid, update=True)                 # the verdict was taken: the mesh is as it was
            unchanged("after the refused device update with %r" % val)
        assert gpu.upload_mesh(V[:3], np.arange(3, dtype=np.uint32)) == n_meshes + 2
        torch.cuda.synchronize()
    finally:
        gpu.close()
