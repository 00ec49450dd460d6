"""What the tests share about scenes, rays and frames, each defined once: meshes, a scene on the GPU and its twin in the oracle,
seeded rays and triangle soups, the closest-hit and whole-frame checks against the oracle, the device-tensor round trip and the
module-scoped renderer fixture.  A mesh is a (verts, indices) pair everywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr

FLOAT_TOL = 1e-4


@pytest.fixture(scope="module")
def gpu():
    r = rr.Renderer(0)
    yield r
    r.close()


# ------------------------------------------------------------------------------- meshes
def load(name):
    m = rr.Mesh()
    assert m.load(O.asset(name))
    return m.verts, m.indices


def procedural_mesh(n_side, seed=0):
    """bumpy unit-ish sphere patch grid: 2*n_side*n_side triangles with smooth normals"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0.02, np.pi - 0.02, n_side + 1), np.linspace(0, 2 * np.pi, n_side + 1), indexing="ij")
    rad = 1.0 + 0.08 * np.sin(7 * u) * np.cos(5 * v) + 0.01 * rng.standard_normal(u.shape)
    P = np.stack([rad * np.sin(u) * np.cos(v), rad * np.cos(u), rad * np.sin(u) * np.sin(v)], -1).astype(np.float32)
    N = P / np.linalg.norm(P, axis=-1, keepdims=True)
    idx = np.arange((n_side + 1) * (n_side + 1)).reshape(n_side + 1, n_side + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tri = np.concatenate([np.stack([a, c, b], 1), np.stack([a, d, c], 1)]).astype(np.int64)    # outward winding
    verts = np.zeros(tri.size, rr.VERTEX_DTYPE)
    verts["position"] = P.reshape(-1, 3)[tri.ravel()]
    verts["norm"] = N.reshape(-1, 3)[tri.ravel()].astype(np.float32)
    return verts, np.arange(tri.size, dtype=np.uint32)


def soup(kind, n, seed, collinear=True):
    """awkward geometry for the builder and the quantised boxes (vertex records, identity indices)"""
    rng = np.random.default_rng(seed)
    if kind == "flat":                     # every triangle in the plane z = 0.25: zero extent on one axis
        P = rng.uniform(-2, 2, (n, 3, 3)); P[..., 2] = 0.25
    elif kind == "far":                    # small mesh far from the origin: coordinates ~1e3, extent ~1
        P = rng.uniform(-0.5, 0.5, (n, 3, 3)) * 0.2 + rng.uniform(-0.5, 0.5, (n, 1, 3)) + np.array([1000.0, -2000.0, 500.0])
    elif kind == "mixed":                  # huge and tiny triangles, slivers, a few degenerate ones
        c = rng.uniform(-3, 3, (n, 1, 3))
        P = c + rng.normal(size=(n, 3, 3)) * rng.choice([1e-4, 1e-2, 0.3, 2.0], (n, 1, 1))
        P[::17, 1] = P[::17, 0]            # zero-area: two equal vertices
        if collinear:
            P[5::29, 2] = (P[5::29, 0] + P[5::29, 1]) / 2      # zero-area: collinear
    else:                                  # "line": all centroids on one line (Morton codes collide massively)
        t = rng.uniform(-2, 2, (n, 1, 1))
        P = t * np.array([1.0, 1.0, 1.0]) + rng.normal(size=(n, 3, 3)) * 0.01
    v = np.zeros(n * 3, rr.VERTEX_DTYPE)
    v["position"] = P.reshape(-1, 3).astype(np.float32)
    v["norm"] = (0, 0, 1)
    return v, np.arange(n * 3, dtype=np.uint32)


def xf(tx, ty, tz, s=(1, 1, 1), rot=0.0):
    c, sn = np.cos(rot), np.sin(rot)
    R = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], np.float32) * np.array(s, np.float32)
    return np.concatenate([R, np.array([[tx], [ty], [tz]], np.float32)], axis=1)


# ------------------------------------------------------------------------------- scenes on both sides
def oracle_instances(instances):
    """rr.INSTANCE_DTYPE records -> the oracle's"""
    inst = np.zeros(len(instances), O.INSTANCE_DTYPE)
    inst["transform"] = instances["transform"]
    inst["id_mask"] = instances["instance_id_mask"]
    inst["hitgroup_flags"] = instances["hitgroup_flags"]
    inst["blas"] = instances["blas"]
    return inst


def oracle_scene(meshes, env=None, instances=None):
    """instances["blas"] index `meshes` (None: the reference's one identity instance); env=None: no environment map"""
    s = O.Scene()
    for verts, idx in meshes:
        s.add_mesh(verts, idx)
    if instances is not None:
        s.set_instances(oracle_instances(instances))
    if env is not None:
        s.set_envmap(env)
    return s


def gpu_scene(gpu, meshes, env=None, instances=None):
    """uploads + builds; instances["blas"] index `meshes`; -> mesh ids"""
    ids = []
    for verts, idx in meshes:
        mid = gpu.upload_mesh(verts, idx)
        gpu.build_blas(mid)
        ids.append(mid)
    if instances is None:
        instances = rr.make_instances(meshes=[ids[0]])
    else:
        instances = instances.copy()
        instances["blas"] = [ids[int(b)] for b in instances["blas"]]
    gpu.build_tlas(instances)
    if env is not None:
        gpu.upload_envmap(env)
    return ids


def build(gpu, verts, idx, tlas=True, **kw):
    """upload + BLAS (+ a one-instance TLAS) -> mesh id"""
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, **kw)
    if tlas:
        gpu.build_tlas(rr.make_instances(meshes=[mid]))
    return mid


class Scene:
    """meshes [(verts, indices)], instances (blas = index into meshes; None: the reference's one identity instance), env"""

    def __init__(self, key, meshes, env, instances=None):
        self.key, self.meshes, self.env, self.instances = key, meshes, env, instances
        self._oracle = None
        self.single = instances is None
        lo, hi = [], []
        for k in range(1 if instances is None else len(instances)):
            V, I = meshes[0 if instances is None else int(instances["blas"][k])]
            P = V["position"][np.asarray(I, np.int64)].astype(np.float64)      # the referenced vertices: what the BLAS bounds
            if instances is not None:
                T = instances["transform"][k].reshape(3, 4).astype(np.float64)
                P = P @ T[:, :3].T + T[:, 3]
            lo.append(P.min(axis=0)); hi.append(P.max(axis=0))
        self.bounds = (C.c_float * 6)(*[float(v) for v in np.min(lo, axis=0)], *[float(v) for v in np.max(hi, axis=0)])

    def load_gpu(self, r):
        gpu_scene(r, self.meshes, self.env, self.instances)
        r.set_tile_partition(0, 1)

    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_scene(self.meshes, self.env, self.instances)
        return self._oracle

    def n_tris(self):
        return len(self.meshes[0][1]) // 3


# ------------------------------------------------------------------------------- rays and closest hits
def random_rays(n, seed, radius=4.0, extent=1.2, masks=(0xff,), any_frac=0.0, cull_p=(0.35, 0.35, 0.3)):
    """origins within `radius` of the origin, aimed into the cube of half-side `extent`; cull_p: the odds of cull-back / cull-front /
    no culling"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.0, radius, (n, 1))
    d = rng.uniform(-extent, extent, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmin = np.where(rng.random(n) < 0.5, 1e-4, 1e-3)
    tmax = rng.choice([100.0, 1000.0, 3.0], n)
    flags = rng.choice([rr.RAY_FLAG_CULL_BACK, rr.RAY_FLAG_CULL_FRONT, 0], n, p=list(cull_p))
    flags = flags | np.where(rng.random(n) < any_frac, rr.RAY_FLAG_ACCEPT_FIRST_HIT, 0)
    return rr.pack_rays(o, d, tmin, tmax, flags=flags, instance_mask=rng.choice(list(masks), n))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def oracle_trace(s, rays, k, use_bvh=0):
    return s.trace(rays["origin"][k], rays["dir"][k], float(rays["tmin"][k]), float(rays["tmax"][k]), int(rays["flags"][k]) & 0x30,
                   use_bvh=use_bvh)


def check_closest(hits, s, rays, sel=None, inst_map=None, use_bvh=0):
    """hits[k] == the oracle's brute-force closest hit for every k in sel (use_bvh=1: through the oracle's own hierarchy, for
    meshes of tens of thousands of triangles); inst_map: oracle instance -> GPU instance"""
    n_hit = 0
    for k in (range(len(rays)) if sel is None else sel):
        h = oracle_trace(s, rays, k, use_bvh)
        g = hits[k]
        assert bool(g["hit"]) == bool(h.hit), "ray %d" % k
        if h.hit:
            n_hit += 1
            assert g["prim"] == h.prim, "ray %d" % k
            assert g["inst"] == (h.inst if inst_map is None else inst_map[h.inst]), "ray %d" % k
            assert bits(g["t"]) == bits(h.t) and bits(g["u"]) == bits(h.u) and bits(g["v"]) == bits(h.v), "ray %d" % k
    return n_hit


def to_dev(rays, gpu, dtype="int32"):
    import torch
    a = rays.view(np.int32).reshape(-1, 12).copy()
    t = torch.from_numpy(a).to("cuda:%d" % gpu.device)
    return t.view(torch.float32) if dtype == "float32" else t


def from_dev(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).view(rr.HIT_DTYPE).reshape(-1)


# ------------------------------------------------------------------------------- frames
def render_both(gpu, s, angle, W, H, stats=True, **kw):
    sc = rr.camera_orbit(angle)
    M, cam = np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)
    flags = rr.DISPATCH_FLOAT_OUTPUT | (rr.DISPATCH_COLLECT_STATS if stats else 0)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(W, H, rr.default_params(flags=flags, **kw))
    rgba, f32 = gpu.read_frame(want_float=True)
    st = gpu.stats()
    lit = s.render(M, cam, W, H, O.default_params(use_bvh=1, **kw))
    pw = s.render(M, cam, W, H, O.default_params(use_bvh=1, accum_mode=1, **kw))
    return rgba, f32, st, lit, pw


def check_frame(rgba, f32, st, lit, pw):
    assert st.traversal_overflow == 0
    o = lit["stats"]
    assert st.rays == o.rays and st.primary == o.primary and st.secondary == o.secondary
    if st.stats_valid:
        assert (st.hits, st.misses, st.terminal_hits, st.tir) == (o.hits, o.misses, o.terminal_hits, o.tir)
    assert np.all(f32[..., 3] == 1.0) and np.all(rgba[..., 3] == 255)
    # literal recursive oracle: stated tolerance on every pixel
    d = np.abs(f32[..., :3] - lit["rgb"])
    assert d.max() <= FLOAT_TOL, "max |d| %.3g at %s" % (d.max(), np.unravel_index(d.argmax(), d.shape))
    assert np.abs(rgba.astype(int) - lit["rgba8"].astype(int)).max() <= 1
    # path-weight oracle (same summation order as the kernel): bit-exact
    assert np.array_equal(f32[..., :3].view(np.uint32), pw["rgb"].view(np.uint32))
    assert np.array_equal(rgba, pw["rgba8"])
