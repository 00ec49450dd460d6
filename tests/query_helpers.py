"""What the ray-query tests share (test_gpu_query.py, test_gpu_query_multi.py, test_gpu_indexed.py): meshes, scenes on both sides,
seeded rays, the closest-hit check against the oracle's brute force, and the device-tensor round trip."""
import numpy as np

import oracle as O
import refraction_raytracing_dxr_amd as rr

ANY = rr.RAY_FLAG_ACCEPT_FIRST_HIT
CULLS = [rr.RAY_FLAG_CULL_BACK, rr.RAY_FLAG_CULL_FRONT, 0]


def load(name):
    m = rr.Mesh()
    assert m.load(O.asset(name))
    return m.verts, m.indices


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def oracle_scene(meshes, instances=None):
    s = O.Scene()
    for verts, idx in meshes:
        s.add_mesh(verts, idx)
    if instances is not None:
        inst = np.zeros(len(instances), O.INSTANCE_DTYPE)
        inst["transform"] = instances["transform"]
        inst["id_mask"] = instances["instance_id_mask"]
        inst["hitgroup_flags"] = instances["hitgroup_flags"]
        inst["blas"] = instances["blas"]
        s.set_instances(inst)
    return s


def gpu_scene(gpu, meshes, instances=None):
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
    return ids


def random_rays(n, seed, radius=4.0, extent=1.2, masks=(0xff,), any_frac=0.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.0, radius, (n, 1))
    d = rng.uniform(-extent, extent, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmin = np.where(rng.random(n) < 0.5, 1e-4, 1e-3)
    tmax = rng.choice([100.0, 1000.0, 3.0], n)
    flags = rng.choice(CULLS, n, p=[0.35, 0.35, 0.3]) | np.where(rng.random(n) < any_frac, ANY, 0)
    return rr.pack_rays(o, d, tmin, tmax, flags=flags, instance_mask=rng.choice(list(masks), n))


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


def _soup(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        P = rng.uniform(-2, 2, (n, 3, 3)); P[..., 2] = 0.25
    elif kind == "mixed":
        c = rng.uniform(-3, 3, (n, 1, 3))
        P = c + rng.normal(size=(n, 3, 3)) * rng.choice([1e-4, 1e-2, 0.3, 2.0], (n, 1, 1))
        P[::17, 1] = P[::17, 0]
    else:                                  # "line"
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


MASKED_INSTANCES = dict(
    transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4), xf(0.3, 0.2, 2.4, (0.7, 0.7, 0.7), -1.0),
                xf(0, 1.9, 0, (0.4, 0.4, 0.4), 0.2), xf(0, 0, 0, (1, 1, 1), 0.9), xf(0, -1.8, 0.5, (0.5, 0.5, 0.5)),
                xf(-2.2, 0, 0, (0.6, 0.6, 0.6))],
    meshes=[1, 0, 1, 0, 1, 0, 0], masks=[1, 2, 4, 0x80, 0x81, 0x06, 0], flags=[0, 0, 0, 1, 0, 2, 0])
# instance 4 is a rotated copy of instance 0 at the same place; instance 6 has InstanceMask 0 and is never visited
RAY_MASKS = [0xff, 1, 2, 4, 0x80, 0x81, 0x7f, 0x06, 0x102, 0]


def to_dev(rays, gpu, dtype="int32"):
    import torch
    a = rays.view(np.int32).reshape(-1, 12).copy()
    t = torch.from_numpy(a).to("cuda:%d" % gpu.device)
    return t.view(torch.float32) if dtype == "float32" else t


def from_dev(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32).view(rr.HIT_DTYPE).reshape(-1)
