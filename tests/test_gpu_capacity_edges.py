"""GPU: scenes at the exact sizes where the builder and the stack entries switch.

A. BLAS builds at the sort's and the clustered builder's size edges (1024 / 1025: the second half of a sort run and k_ploc's chunk
   of 2; 2047 .. 2049 and 4096 / 4097: a key count at and just past a sort-run edge, half of the padded keys ~0; 32 768 / 32 769:
   PLOC_MAX_PRIMS and the first mesh past it), on three input families, with and without fast_build: the downloaded tree is the CPU
   model's (builder_models.py, depth_meshes.py) child ref for child ref, leaf for leaf, plane for plane; it is a tree with exact
   boxes; its quantised nodes contain it; 400 rays hit what the oracle says.
B. Top levels of 1025, 2049 and 4097 instances (the multi-block sort together with leaf_ref_prim, k_inst_boxes and k_keep_links over
   several blocks): rr_download_tlas against the radix-tree model over the instance-box model, then a refit of every instance.
C. One mesh of 32 767 triangles (the last that gets 16-bit stack entries) and of 32 768 (the first that does not).
D. Two instances of a mesh of 32 765 triangles (pool_refs 32 767: 16-bit entries, the stream renderer) and of 32 766 (32 768: neither).

Every case first asserts the shape it was built for -- the triangle or instance count, bvh_depth, which builder the tree is from, the
entry width by kernel name, and for C and D what pushed_refs says its own rays put on a stack -- and only then compares.  No
tolerance anywhere: trees are compared exactly, hits and frames bit for bit."""
import time

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from builder_models import (FAMILIES, aimed_rays, check_quantised, check_structure, check_tree, has_negative_zero, inst_world_box_model,
                            karras_model, karras_tlas_model, same_tree)
from conftest import procedural_env
from depth_meshes import ploc_model, pushed_refs, to_object_space, tree_depth
from kernel_oracle_helpers import check_slice, counters, dispatch, FUSED, make_renderer, oracle_frame, STREAM  # noqa: F401  (make_renderer: a fixture)
from scenes import build, check_closest, gpu, load, oracle_scene, Scene, xf  # noqa: F401  (gpu: a fixture)
from shading_helpers import check_against_oracle as check_shade
from test_gpu_query_multi import check_slots
from test_gpu_query_multi import expected as multi_expected
from test_gpu_stack_rungs import check_ray_trees, view
from test_kernel_choice import driver, run  # noqa: F401  (driver: a fixture)

pytestmark = pytest.mark.gpu

PLOC_MAX_PRIMS = 32768
FLOAT = rr.DISPATCH_FLOAT_OUTPUT
KW = dict(max_refract=5)
FW, FH = 64, 36
ENV = procedural_env(128, 64, seed=3)
_meshes = {}


def mesh(family, T):
    if (family, T) not in _meshes:
        verts, idx = FAMILIES[family](T)
        assert len(idx) == 3 * T and np.all(np.isfinite(verts["position"])) and not has_negative_zero(verts)
        _meshes[family, T] = (verts, idx)
    return _meshes[family, T]


def expected_tree(verts, idx, fast_build):
    """what rr_build_blas must build -> (model nodes, leaf order, depth, which builder)"""
    T = len(idx) // 3
    if not fast_build and T <= PLOC_MAX_PRIMS:
        m = ploc_model(verts, idx)
        if m[2] <= 64:
            return m + ("clustered",)
        return karras_model(verts, idx) + ("radix, the clustered tree being %d deep" % m[2],)
    return karras_model(verts, idx) + ("radix",)


# ------------------------------------------------------------------------------------------------------- A. builder sizes, BLAS
BLAS_CASES = [(f, T, fast) for T in (1024, 1025, 2047, 2048, 2049, 4096, 4097) for f in ("soup", "lattice", "line") for fast in (False, True)]
BLAS_CASES += [("soup", 32768, False), ("lattice", 32768, False), ("soup", 32769, False), ("lattice", 32769, False), ("soup", 32769, True)]


@pytest.mark.parametrize("family,T,fast_build", BLAS_CASES)
def test_blas_at_a_builder_size_edge(gpu, family, T, fast_build):
    t0 = time.time()
    verts, idx = mesh(family, T)
    model, order, depth, kind = expected_tree(verts, idx, fast_build)
    t_model = time.time() - t0
    assert kind.startswith("radix") or not fast_build and T <= PLOC_MAX_PRIMS
    mid = build(gpu, verts, idx, fast_build=fast_build)
    nodes, tris = gpu.download_blas(mid)
    st = gpu.stats()
    print("%s %d fast_build=%d: %s, depth %d (built %d), model %.2f s" % (family, T, fast_build, kind, depth, st.bvh_depth, t_model))
    assert len(tris) == T and len(nodes) == T - 1 and st.bvh_depth == depth == tree_depth(nodes)
    same_tree(nodes, model)
    assert np.array_equal(tris["prim"], order)
    check_structure(nodes, tris, verts, idx)
    if T > PLOC_MAX_PRIMS and not fast_build:                       # past PLOC_MAX_PRIMS the default build is the fast one, byte for byte
        fnodes, ftris = gpu.download_blas(build(gpu, verts, idx, fast_build=True))
        assert fnodes.tobytes() == nodes.tobytes() and ftris.tobytes() == tris.tobytes()
        build(gpu, verts, idx)
    if T == PLOC_MAX_PRIMS:                                         # PLOC_MAX_PRIMS itself is clustered: not the radix tree
        assert kind == "clustered" and not np.array_equal(karras_model(verts, idx)[0]["c"], nodes["c"])
    q, org, cell = gpu.download_qnodes(mid)
    P = verts["position"][idx].astype(np.float64)
    check_quantised(q, org, cell, nodes, P.min(0), P.max(0))
    rays = aimed_rays(verts, idx, 400, seed=T)
    n_hit = check_closest(gpu.trace_rays(rays), oracle_scene([(verts, idx)]), rays, use_bvh=1 if T >= 32768 else 0)
    assert n_hit >= 100, n_hit


# ------------------------------------------------------------------------------------------------------- B. builder sizes, TLAS
MASKS = (1, 2, 4, 0x80, 0x81, 0xff)
RAY_MASKS = (0xff, 1, 2, 0x84)


def instance_grid(N, seed):
    """N transforms on a jittered cubic grid, each rotated about y and scaled unevenly (all scales positive); instance N // 2 is
    the identity, moved to no grid point; mixed masks"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(N ** (1.0 / 3.0)))
    k = np.arange(N)
    pos = np.stack([k % side, (k // side) % side, k // (side * side)], -1) * 3.0 + 1.5 + rng.uniform(-0.5, 0.5, (N, 3))
    scale = rng.uniform(0.4, 1.1, (N, 3))
    rot = rng.uniform(-np.pi, np.pi, N)
    T = [xf(*pos[i], tuple(scale[i]), rot[i]) for i in range(N)]
    T[N // 2] = np.eye(4, dtype=np.float32)[:3]
    return rr.make_instances(transforms=T, meshes=[0] * N, masks=[int(m) for m in rng.choice(MASKS, N)])


def tlas_rays(inst, n, seed):
    """seeded rays from outside the grid towards instance centres, with mixed InstanceInclusionMasks"""
    rng = np.random.default_rng(seed)
    c = inst["transform"].reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
    lo, hi = c.min(0), c.max(0)
    o = rng.normal(size=(n, 3))
    o = (lo + hi) / 2 + o / np.linalg.norm(o, axis=1, keepdims=True) * float((hi - lo).max())
    d = c[rng.integers(0, len(c), n)] + rng.uniform(-0.3, 0.3, (n, 3)) - o
    return rr.pack_rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), 1e-4, 1000.0, instance_mask=rng.choice(RAY_MASKS, n))


def check_masked(gpu, cube, inst, rays):
    """query_rays == the oracle's brute force over the instances each ray's mask selects: hit, instance, primitive, t / u / v bits"""
    q = gpu.query_rays(rays)
    inst_masks = inst["instance_id_mask"] >> 24
    n_hit = 0
    for rm in RAY_MASKS:
        sel = np.flatnonzero(rays["instance_mask"] == rm)
        keep = np.flatnonzero(inst_masks & rm & 0xff)
        assert len(sel) and len(keep)
        hits = check_closest(q, oracle_scene([cube], instances=inst[keep]), rays, sel=sel, inst_map=keep)
        assert hits > 0, hex(rm)
        n_hit += hits
    return n_hit, q


def check_tlas(gpu, inst, bounds, leaf_base, want_c=None):
    """rr_download_tlas against the models -> the downloaded fp32 nodes"""
    N = len(inst)
    boxes = inst_world_box_model(inst["transform"], np.tile(bounds, (N, 1)))
    model, order, depth = karras_tlas_model(boxes, leaf_base)
    nodes, q, org, cell = gpu.download_tlas()
    assert len(nodes) == N - 1 == len(q)
    if want_c is None:
        same_tree(nodes, model)
    else:                                                           # a refit: the kept topology over the new boxes
        assert np.array_equal(nodes["c"], want_c)
    check_tree(nodes, boxes, leaf_base)
    check_quantised(q, org, cell, nodes, boxes[:, :3].min(0), boxes[:, 3:].max(0))
    return nodes, depth


@pytest.mark.parametrize("N", [1025, 2049, 4097])
def test_tlas_at_a_builder_size_edge(gpu, N):
    cube = load("cube.obj")
    leaf_base = len(cube[1]) // 3
    P = cube[0]["position"][cube[1]]
    bounds = np.concatenate([P.min(0), P.max(0)]).astype(np.float32)
    cube_depth = ploc_model(*cube)[2]
    mid = gpu.upload_mesh(*cube)
    gpu.build_blas(mid)
    inst = instance_grid(N, seed=N)
    assert len(inst) == N and np.array_equal(inst["transform"][N // 2], np.eye(4, dtype=np.float32)[:3].reshape(12))
    assert len(set((inst["instance_id_mask"] >> 24).tolist())) == len(MASKS)
    on_gpu = inst.copy()
    on_gpu["blas"] = mid
    gpu.build_tlas(on_gpu, allow_update=True)
    nodes, depth = check_tlas(gpu, inst, bounds, leaf_base)
    assert gpu.stats().bvh_depth == depth + cube_depth and tree_depth(nodes) == depth
    rays = tlas_rays(inst, 400, seed=N + 1)
    n_hit, _ = check_masked(gpu, cube, inst, rays)
    print("%d instances: top level %d deep, %d of 400 rays hit" % (N, depth, n_hit))
    assert n_hit >= 100
    # every instance moves: a refit keeps the child refs, takes the new boxes and answers as a fresh build does
    moved = instance_grid(N, seed=N + 7)
    moved["instance_id_mask"] = inst["instance_id_mask"]
    assert not np.any(np.all(moved["transform"] == inst["transform"], axis=1) & (np.arange(N) != N // 2))
    moved["transform"][N // 2] = xf(-2.0, -1.0, -3.0, (0.9, 0.7, 1.2), 0.3).reshape(12)
    on_gpu["transform"] = moved["transform"]
    gpu.build_tlas(on_gpu, update=True)
    check_tlas(gpu, moved, bounds, leaf_base, want_c=nodes["c"])
    rays = tlas_rays(moved, 400, seed=N + 2)
    n_hit, q_refit = check_masked(gpu, cube, moved, rays)
    assert n_hit >= 100
    gpu.build_tlas(on_gpu)
    check_tlas(gpu, moved, bounds, leaf_base)
    assert gpu.query_rays(rays).tobytes() == q_refit.tobytes()


# ---------------------------------------------------------------------------------------- C, D. 16-bit stack entries at their limit
class EdgeScene(Scene):
    """a Scene of one mesh that keeps what it built: the mesh id, the downloaded fp32 hierarchy and, two-level, the top level"""

    def __init__(self, key, meshes, env, instances=None, **build_kw):
        super().__init__(key, meshes, env, instances)
        self.build_kw = build_kw

    def load_gpu(self, r):
        (v, i), = self.meshes
        self.mid = r.upload_mesh(v, i)
        r.build_blas(self.mid, **self.build_kw)
        inst = rr.make_instances(meshes=[self.mid]) if self.instances is None else self.instances.copy()
        inst["blas"] = self.mid
        r.build_tlas(inst)
        r.upload_envmap(self.env)
        r.set_tile_partition(0, 1)
        self.nodes = r.download_blas(self.mid)[0]
        self.tlas = None if self.instances is None else r.download_tlas()[0]


_scenes = {}
TWO = rr.make_instances(transforms=[np.eye(4, dtype=np.float32)[:3], xf(0.45, 0.1, 0.25, (1, 1, 1), 0.5)], meshes=[0, 0], masks=[1, 1])


def edge_scene(T, two_level):
    """soup(T): one identity instance over its radix tree (bvh_depth 20 or 21: inside 20..39, where one instance gets 16-bit
    entries), or two instances -- one where the mesh is, one moved and rotated about y, overlapping it -- over its clustered tree"""
    key = "edge-%d-%d" % (T, two_level)
    if key not in _scenes:
        _scenes[key] = EdgeScene(key, [mesh("soup", T)], ENV, TWO.copy()) if two_level else EdgeScene(key, [mesh("soup", T)], ENV, fast_build=True)
    return _scenes[key]


def policy(driver, sc, need, depth, max_reflect=2, tlas32=0):  # noqa: F811
    """The choice policy (rr_choice.cpp, compiled into the driver from the sources the library is built from) fed this scene's
    facts -> (k_render_fused takes 16-bit stack entries for a launch of `depth` slices, the stack-entry width in bits of the
    ray-tree kernels' instantiation).  Asked before anything is launched: a policy that grants 16-bit entries to a scene whose
    refs do not fit them fails the test here, not on the GPU."""
    T = sc.n_tris()
    n_inst = 1 if sc.single else len(sc.instances)
    facts = "%d %d %d %d %d 0" % (sc.single, need, T if sc.single else 0, max(n_inst - 1, 1) + T - 1, T + n_inst)
    f_launch, f_tree = run(driver, ["fused %s %d %d 0 0 %d" % (facts, depth, max_reflect, tlas32), "fused %s 64 %d 0 0 %d" % (facts, max_reflect, tlas32)])
    bits = int(run(driver, ["tree %d %s" % (sc.single, f_tree)])[0].split()[3])
    return f_launch.split()[2] == "1", bits


def launch(r, sc, cams, kw, want_kernel, oracle_slices, tag):
    """one launch of len(cams) slices: the kernel that rendered it, the slices in oracle_slices against the oracle bit for bit
    (float accumulator and RGBA8), depth 1 also the counters -> (frames, the kernel's name)"""
    frames, st = dispatch(r, FW, FH, cams, kw, FLOAT)
    name = st.render_kernel_name.decode()
    assert st.render_kernel == want_kernel, "%s: rendered by kernel %d (%s), expected %d" % (tag, st.render_kernel, name, want_kernel)
    for f in oracle_slices:
        ref = oracle_frame(sc, cams[f], FW, FH, kw)
        check_slice(frames[f][0], frames[f][1], ref, "%s slice %d" % (tag, f))
        assert ref["stats"].hits > 0
        if len(cams) == 1:
            assert counters(st) == counters(ref["stats"]), (tag, counters(st), counters(ref["stats"]))
    return frames, name


def last_leaves_rays(sc, n, seed):
    """rays aimed, from every side, at the triangles in the last 512 leaf positions of the scene's mesh"""
    (v, i), = sc.meshes
    order = karras_model(v, i)[1] if sc.build_kw.get("fast_build") else ploc_model(v, i)[1]
    return aimed_rays(v, i, n, seed, prims=order[-512:])


def multi_expected_near(m, rays):
    """test_gpu_query_multi's expected() for a mesh too large for its one oracle scene per triangle per ray: the oracle is asked
    only about the triangles a float64 test cannot rule out for some ray -- barycentrics more than 0.01 outside the triangle, where
    an fp32 test's error is a few 1e-7 of the triangle's size, unless the ray is within 1e-6 of the triangle's plane, and no
    bound on t at all -- so every triangle the oracle would accept is among them; primitive ids mapped back"""
    verts, idx = m
    P = verts["position"][idx].reshape(-1, 3, 3).astype(np.float64)
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    near = np.zeros(len(P), bool)
    for k in range(len(rays)):
        o, d = rays["origin"][k].astype(np.float64), rays["dir"][k].astype(np.float64)
        pv = np.cross(d, e2)
        det = np.einsum("nc,nc->n", e1, pv)
        flat = np.abs(det) <= 1e-6 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) * np.linalg.norm(d)
        inv = 1.0 / np.where(flat, 1.0, det)
        tv = o - P[:, 0]
        u = np.einsum("nc,nc->n", tv, pv) * inv
        v = np.einsum("nc,c->n", np.cross(tv, e1), d) * inv
        near |= flat | ((u >= -0.01) & (v >= -0.01) & (u + v <= 1.01))
    cand = np.flatnonzero(near)
    sub = np.ascontiguousarray(verts[idx.reshape(-1, 3)[cand].reshape(-1)])
    exp = multi_expected([(sub, np.arange(len(sub), dtype=np.uint32))], None, rays)
    return [[(a[0], a[1], int(cand[a[2]])) + a[3:] for a in acc] for acc in exp]


@pytest.mark.parametrize("T", [32767, 32768])
def test_one_mesh_at_the_16_bit_limit(make_renderer, driver, T):  # noqa: F811
    t0, lap = time.time(), []
    sc = edge_scene(T, False)
    r = make_renderer("fused")
    sc.load_gpu(r)
    need = r.stats().bvh_depth
    wide = T >= 32768
    lap.append(('build', time.time() - t0))
    assert sc.n_tris() == T == len(sc.nodes) + 1 and need == tree_depth(sc.nodes) == karras_model(*sc.meshes[0])[2] and 20 <= need <= 39
    cams = [view(a, FW, FH) for a in (-np.pi / 2, np.pi / 2, -1.0, 2.2)]
    cam_rays = np.concatenate([rr.camera_rays(c, FW, FH) for c in cams])
    q_rays = np.concatenate([last_leaves_rays(sc, 300, seed=T), cam_rays[::23]])
    for what, rays in (("camera rays", cam_rays), ("query rays", q_rays)):
        high, top_node, top_leaf = pushed_refs(sc.nodes, rays)
        print("%d triangles, %s: deepest stack %d of need %d, largest internal ref pushed %d, largest leaf ref pushed %d" %
              (T, what, high.max(), need, top_node, top_leaf))
        assert top_node >= 32000 and top_leaf >= 32000 and high.max() < need
    lap.append(('walks', time.time() - t0))
    # the policy first: 16-bit entries up to 32 767 triangles, 32-bit ones from 32 768, for dispatches and ray-tree queries alike
    s16, bits = policy(driver, sc, need, 4)
    print("%d triangles: the policy gives Depth 4 %d-bit and the ray-tree kernels %d-bit stack entries" % (T, 16 if s16 else 32, bits))
    assert s16 == (not wide) and bits == (32 if wide else 16)
    # dispatches: Depth 4 on k_render_fused -- the 39-entry rung with 16-bit entries, or the 32-bit ladder
    _, name = launch(r, sc, cams, KW, FUSED, range(4), "one mesh %d" % T)
    rung = next(s for s in (22, 26, 31, 39) if need <= s)
    lap.append(('frames', time.time() - t0))
    print("%d triangles: Depth 4 ran %s" % (T, name))
    assert name.startswith("k_render_fused<%d, 2, " % (rung if wide else 39)) and ("unsigned short" in name) == (not wide), name
    # the ray-tree queries (their width is the policy's, asserted above): the colours from the oracle
    cam = cams[0]
    ref = check_shade(r, sc.oracle(), np.array(cam.proj_inv, np.float32), np.array(cam.camera_loc, np.float32), FW, FH, rr.camera_rays(cam, FW, FH), **KW)
    assert ref["stats"].hits > 0
    lap.append(('shade', time.time() - t0))
    check_ray_trees(r, sc, KW, angles=(-np.pi / 2, 2.2))
    lap.append(('ray trees', time.time() - t0))
    # closest-hit and multi-hit queries against brute force
    s = sc.oracle()
    assert check_closest(r.query_rays(q_rays), s, q_rays) >= 150        # three in four of the 300 aimed rays end inside a triangle
    few = q_rays[:90]
    hits, counts = r.query_rays_multi(few, 4, counts=True)
    exp = multi_expected_near(sc.meshes[0], few)
    check_slots(hits, counts, exp, few, 4)
    assert max(len(a) for a in exp) >= 2 and sum(len(a) for a in exp) >= 90
    lap.append(("queries", time.time() - t0))
    print("%d triangles, seconds since the start after each part: %s" % (T, ", ".join("%s %.2f" % x for x in lap)))


@pytest.mark.parametrize("T", [32765, 32766])
def test_two_instances_at_the_16_bit_limit(make_renderer, driver, T):  # noqa: F811
    sc = edge_scene(T, True)
    pool_refs = T + 2
    wide = pool_refs >= 32768
    cams1, cams16 = [view(-np.pi / 2, FW, FH)], [view(c, FW, FH) for c in np.linspace(-np.pi, np.pi, 16, endpoint=False)]
    frames = {}
    for kernel, env in (("fused", {}), ("stream", {})) + (() if wide else (("fused", {"RR_DEBUG_TLAS32": 1}),)):
        r = make_renderer(kernel, **env)
        sc.load_gpu(r)
        need = r.stats().bvh_depth
        tag = "two instances of %d, %s %s" % (T, kernel, env)
        assert sc.n_tris() == T and len(sc.tlas) == 1 and need == tree_depth(sc.nodes) + 2 <= 30
        assert sorted((~sc.tlas["c"][0]).tolist()) == [T, T + 1]             # the instance leaves: the highest refs of the pool
        rays = rr.camera_rays(cams1[0], FW, FH)
        high, top_node, top_leaf = pushed_refs(sc.tlas, rays)
        assert int(high.sum()) >= 100 and top_node == -1 and top_leaf >= T   # rays that enter both instance boxes push an instance leaf
        blas_top = [pushed_refs(sc.nodes, to_object_space(rays, t))[1:] for t in sc.instances["transform"]]
        tlas32 = bool(env)
        s16 = not wide and not tlas32
        for depth in (1, 16):                                                # the policy first, before anything is launched
            assert policy(driver, sc, need, depth, tlas32=int(tlas32)) == (s16, 16 if s16 else 32), (tag, depth)
        want = STREAM if kernel == "stream" and not wide else FUSED
        got1, name1 = launch(r, sc, cams1, KW, FUSED if kernel == "fused" or wide else STREAM, [0], tag + " Depth 1")
        got16, name16 = launch(r, sc, cams16, KW, want, (0, 5, 10, 15), tag + " Depth 16")
        print("%s: pool_refs %d, need %d; %d rays push an instance leaf, the largest %d; BLAS refs pushed (node, leaf) %s; Depth 1 %s; Depth 16 %s" %
              (tag, pool_refs, need, int(high.sum()), top_leaf, blas_top, name1, name16))
        if want == FUSED:
            for name in (name1, name16):
                assert name.startswith("k_render_fused<%d, 2, " % (30 if s16 else next(s for s in (22, 26, 31) if need <= s))), name
                assert ("unsigned short" in name) == s16, name
        frames[kernel, tlas32] = [f[1].tobytes() + f[0].tobytes() for f in got1 + got16]
        if kernel == "fused":
            cam = cams1[0]
            check_shade(r, sc.oracle(), np.array(cam.proj_inv, np.float32), np.array(cam.camera_loc, np.float32), FW, FH, rays, **KW)
            q_rays = np.concatenate([last_leaves_rays(sc, 200, seed=T), rays[::11]])
            assert check_closest(r.query_rays(q_rays), sc.oracle(), q_rays) >= 100    # three in four of the 200 aimed rays end inside a triangle
    assert len(set(map(tuple, frames.values()))) == 1                         # every kernel and entry width: the same frames
