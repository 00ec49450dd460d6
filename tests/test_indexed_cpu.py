"""CPU: the indexed-mesh generators (tests/indexed_meshes.py) and the oracle on what they make.

tests/test_gpu_indexed.py holds the GPU against the oracle given an indexed mesh (V, I) and against the GPU's own results on the
flat twin (V[I], arange).  Both references rest on what is pinned here: the generators keep the geometry they claim to keep, and
the oracle -- which gathers through the index buffer for boxes, triangles and normals -- renders and traces (V, I) exactly as it
does the flat twin.
"""
import numpy as np
import pytest

import indexed_meshes as IM
import oracle as O
from refraction_raytracing_dxr_amd.synth import procedural_env
from scenes import load, oracle_scene

ASSETS = ["cube.obj", "sphere.obj", "monkey.obj", "shell.obj", "ott.obj"]
# vertices of the shipped meshes welded on whole 32-byte records / on positions alone
WELDED = {"cube.obj": 24, "sphere.obj": 441, "monkey.obj": 556, "shell.obj": 882, "ott.obj": 8255}


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------------------------------------- 1. the generators
@pytest.mark.parametrize("name", ASSETS)
def test_variants_keep_the_geometry_and_have_the_stated_counts(name):
    verts, idx = load(name)
    T, nw = len(idx) // 3, WELDED[name]
    for var in ("welded", "shuffled", "holes", "padded"):
        V, I = IM.variant(var, verts, seed=3)
        assert V.dtype == IM.VERTEX_DTYPE and I.dtype == np.uint32 and len(I) == 3 * T
        assert I.max() < len(V)
        assert same_bytes(V[I], verts), var                                   # V[I] is the source, byte for byte
        fv, fi = IM.flat(V, I)
        assert same_bytes(fv, verts) and np.array_equal(fi, idx)
        assert len(V) == {"welded": nw, "shuffled": nw, "holes": nw + 3 * IM.N_HOLES, "padded": 3 * T + IM.N_PAD_EXTRA}[var], var
        assert int(IM.hole_mask(V, I).sum()) == len(V) - nw
    assert nw < 3 * T                                                          # n_verts != n_idx in every welded variant
    W, WI = IM.welded(verts)
    assert len(np.unique(W.view(np.uint32).reshape(-1, 8), axis=0)) == len(W)
    S, SI = IM.shuffled(verts, seed=3)
    assert not np.array_equal(SI, WI) and same_bytes(np.sort(S.view(np.uint32).reshape(-1, 8), axis=0), np.sort(W.view(np.uint32).reshape(-1, 8), axis=0))
    assert not np.array_equal(IM.shuffled(verts, seed=4)[1], SI)               # seeded ...
    assert all(same_bytes(a, b) for a, b in zip(IM.holes(verts, seed=3), IM.holes(verts, seed=3)))    # ... and repeatable
    # holes: unreferenced vertices first, last and in between, far away but finite, with garbage normals
    H, HI = IM.holes(verts, seed=3)
    hm = IM.hole_mask(H, HI)
    assert hm[:IM.N_HOLES].all() and hm[-IM.N_HOLES:].all() and int(hm[IM.N_HOLES:-IM.N_HOLES].sum()) == IM.N_HOLES
    assert not hm[IM.N_HOLES] and not hm[-IM.N_HOLES - 1]
    for V, I in ((H, HI), IM.padded(verts, seed=3)):
        far = V["position"][IM.hole_mask(V, I)]
        assert np.isfinite(far).all() and np.abs(far).min() >= 4e5 and np.abs(far).max() <= 1e18
        assert not np.isfinite(V["norm"][IM.hole_mask(V, I)]).all()
    P, PI = IM.padded(verts, seed=3)
    assert len(P) >= len(PI) and IM.hole_mask(P, PI)[nw:].all() and same_bytes(P[:nw], W) and np.array_equal(PI, WI)


@pytest.mark.parametrize("name", ASSETS)
def test_smooth_and_degenerate_variants(name):
    verts, idx = load(name)
    T = len(idx) // 3
    V, I = IM.smooth(verts)
    n_pos = len(np.unique(verts["position"].view(np.uint32).reshape(-1, 3), axis=0))
    assert len(V) == n_pos <= WELDED[name] and len(I) == 3 * T and I.max() == len(V) - 1
    assert same_bytes(V["position"][I], verts["position"])                     # the same triangles ...
    assert np.allclose(np.linalg.norm(V["norm"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    if n_pos < WELDED[name]:
        assert not same_bytes(V["norm"][I], verts["norm"])                      # ... another shading input
    # a vertex's normal is the mean of its corners' normals
    k = int(I[len(I) // 2])
    mean = verts["norm"][I == k].astype(np.float64).sum(0)
    assert np.allclose(V["norm"][k], mean / np.linalg.norm(mean), atol=1e-6)

    S, SI = IM.shuffled(verts, seed=5)
    D, DI = IM.degenerate(verts, seed=5)
    p, deg, dup = IM.degenerate_layout(T, seed=5)
    assert same_bytes(D, S) and np.array_equal(DI[:3 * T], SI) and len(DI) == 3 * (T + 4) and DI.max() < len(D)
    a, b, c = SI[3 * p:3 * p + 3]
    assert len({a, b, c}) == 3
    assert [tuple(DI[3 * t:3 * t + 3]) for t in deg] == [(a, a, b), (a, b, a), (a, a, a)]
    assert tuple(DI[3 * dup:3 * dup + 3]) == (a, b, c) and dup == T + 3


def test_grids_and_the_single_triangle():
    for n in IM.GRID_SIDES:
        V, I = IM.heightfield(n, seed=1)
        assert len(V) == (n + 1) ** 2 and len(I) == 6 * n * n and I.dtype == np.uint32
        assert np.array_equal(np.unique(I), np.arange(len(V)))                 # every vertex referenced, none out of range
        tri = V["position"][I].reshape(-1, 3, 3).astype(np.float64)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert np.all(nrm @ IM.GRID_UP > 0)                                     # no degenerate cell, all facing the same side
        assert np.allclose(np.linalg.norm(V["norm"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert len(IM.heightfield(181)[1]) // 3 == 65522 > 32768
    V, I = IM.one_triangle()
    assert len(V) == 4 and tuple(I) == (2, 0, 1) and np.isfinite(V["position"]).all()


# ------------------------------------------------------------------------------------------------- 2. the oracle
STAT_FIELDS = [f for f, _ in O.Stats._fields_]


def stat_tuple(st):
    return tuple(tuple(getattr(st, f)) if f == "rays_per_level" else int(getattr(st, f)) for f in STAT_FIELDS)


def trace_rays(n, seed, centre, radius):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = centre + o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.0, 4.0 * radius, (n, 1))
    d = centre + rng.uniform(-1.2 * radius, 1.2 * radius, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32), rng.choice([O.CULL_BACK, O.CULL_FRONT, 0], n)


def assert_oracle_equal(V, I, W=96, H=72, angle=0.4, n_rays=200, seed=0, tag=""):
    """the oracle on (V, I) == the oracle on the flat twin: path-weight frame (float bits, RGBA8, per-pixel ray counts, every
    Stats counter), and brute-force and BVH traces of random rays"""
    env = procedural_env(64, 32, seed=7)
    a, b = oracle_scene([(V, I)], env), oracle_scene([IM.flat(V, I)], env)
    M, cam = O.camera(angle)
    p = O.default_params(use_bvh=1, accum_mode=1, max_refract=8)
    ra, rb = a.render(M, cam, W, H, p, want_rays=True), b.render(M, cam, W, H, p, want_rays=True)
    assert np.array_equal(ra["rgb"].view(np.uint32), rb["rgb"].view(np.uint32)), tag
    assert np.array_equal(ra["rgba8"], rb["rgba8"]) and np.array_equal(ra["rays"], rb["rays"]), tag
    assert stat_tuple(ra["stats"]) == stat_tuple(rb["stats"]), tag
    ref = V["position"][I].astype(np.float64)
    centre, radius = (ref.min(0) + ref.max(0)) / 2, float(np.abs(ref.max(0) - ref.min(0)).max()) / 2
    o, d, fl = trace_rays(n_rays, seed, centre, radius)
    n_hit = 0
    for k in range(n_rays):
        for use_bvh in (0, 1):
            ha = a.trace(o[k], d[k], 1e-4, 100.0, int(fl[k]), use_bvh=use_bvh)
            hb = b.trace(o[k], d[k], 1e-4, 100.0, int(fl[k]), use_bvh=use_bvh)
            assert bytes(ha) == bytes(hb), (tag, k, use_bvh)
        n_hit += bool(ha.hit)
    return ra, n_hit


@pytest.mark.parametrize("var", IM.VARIANTS)
@pytest.mark.parametrize("name", ASSETS)
def test_oracle_renders_and_traces_a_variant_as_its_flat_twin(name, var):
    verts, idx = load(name)
    V, I = IM.variant(var, verts, seed=len(name))
    ra, n_hit = assert_oracle_equal(V, I, n_rays=200 if name != "ott.obj" else 60, seed=len(var), tag="%s %s" % (name, var))
    assert ra["stats"].hits > 100 and n_hit > 5                                # the mesh is in view and in the rays' way
    if var in ("welded", "shuffled", "holes", "padded"):
        # ... and as the un-indexed source itself
        src = oracle_scene([(verts, idx)], procedural_env(64, 32, seed=7)).render(*O.camera(0.4), 96, 72, O.default_params(use_bvh=1, accum_mode=1, max_refract=8))
        assert np.array_equal(ra["rgb"].view(np.uint32), src["rgb"].view(np.uint32))
        assert stat_tuple(ra["stats"])[:8] == stat_tuple(src["stats"])[:8]


@pytest.mark.parametrize("n", IM.GRID_SIDES)
def test_oracle_renders_and_traces_a_grid_as_its_flat_twin(n):
    V, I = IM.heightfield(n, seed=2)
    ra, n_hit = assert_oracle_equal(V, I, W=64, H=48, n_rays=100 if n < 100 else 30, tag="grid %d" % n)
    assert ra["stats"].hits > 50 and n_hit > 5


def test_oracle_on_the_single_triangle_and_the_degenerate_additions():
    V, I = IM.one_triangle()
    ra, _ = assert_oracle_equal(V, I, tag="one triangle")
    assert ra["stats"].hits > 20
    # the duplicate of triangle p is hit exactly where p is; an index-degenerate triangle is never hit
    verts, idx = load("monkey.obj")
    D, DI = IM.degenerate(verts, seed=5)
    p, deg, dup = IM.degenerate_layout(len(idx) // 3, seed=5)
    tri = D["position"][DI[3 * p:3 * p + 3]].astype(np.float64)
    c, nrm = tri.mean(0), np.cross(tri[1] - tri[0], tri[2] - tri[0])
    nrm /= np.linalg.norm(nrm)
    env = procedural_env(16, 8)
    for t in [p, dup] + deg:
        one = oracle_scene([(D, np.ascontiguousarray(DI[3 * t:3 * t + 3]))], env)
        for sign in (1.0, -1.0):
            h = one.trace(c + sign * 0.5 * nrm, -sign * nrm, 1e-4, 100.0, 0, use_bvh=0)
            assert bool(h.hit) == (t in (p, dup)), t
