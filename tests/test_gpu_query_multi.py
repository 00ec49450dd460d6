"""GPU: multi-hit ray queries (rr_query_rays_multi[_device], Renderer.query_rays_multi) against the CPU oracle and the closest-hit
query.

The expectation of a ray is built as tests/test_gpu_query.py checks first hits: one oracle scene per triangle (the triangle alone,
with its instance's transform and flags), brute-force trace.  That says, per (ray, triangle), whether the closest-hit test accepts
it and with which t/u/v bits; the multi-hit result must be that set sorted by (t, inst, prim), bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from query_helpers import MASKED_INSTANCES, RAY_MASKS
from scenes import bits, from_dev, gpu, gpu_scene, load, oracle_scene, random_rays, soup, to_dev, xf  # noqa: F401  (gpu: a fixture)

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5
ANY = rr.RAY_FLAG_ACCEPT_FIRST_HIT
FRONT, BACK = rr.HIT_KIND_FRONT_FACE, rr.HIT_KIND_BACK_FACE


def tri_scenes(meshes, instances=None, clear_cull_disable=False):
    """[(inst, prim, InstanceMask, oracle scene of that one triangle)] over every instance's triangles"""
    out = []
    if instances is None:
        verts, idx = meshes[0]
        for p in range(len(idx) // 3):
            tri = np.ascontiguousarray(verts[idx[3 * p:3 * p + 3]])
            out.append((0, p, 0xff, oracle_scene([(tri, np.arange(3, dtype=np.uint32))])))
        return out
    for i in range(len(instances)):
        verts, idx = meshes[int(instances["blas"][i])]
        one = instances[i:i + 1].copy()
        one["blas"] = 0
        one["instance_id_mask"] = 1 << 24
        if clear_cull_disable:
            one["hitgroup_flags"] &= ~np.uint32(1 << 24)
        for p in range(len(idx) // 3):
            tri = np.ascontiguousarray(verts[idx[3 * p:3 * p + 3]])
            out.append((i, p, int(instances["instance_id_mask"][i]) >> 24, oracle_scene([(tri, np.arange(3, dtype=np.uint32))], instances=one)))
    return out


def expected(meshes, instances, rays):
    """per ray: the accepted triangles as (t, inst, prim, t_bits, u_bits, v_bits, hit_kind), sorted by (t, inst, prim)"""
    scenes = tri_scenes(meshes, instances)
    facing = tri_scenes(meshes, instances, clear_cull_disable=True)
    res = []
    for k in range(len(rays)):
        o, d = rays["origin"][k], rays["dir"][k]
        tmin, tmax, fl, rm = float(rays["tmin"][k]), float(rays["tmax"][k]), int(rays["flags"][k]) & 0x30, int(rays["instance_mask"][k])
        acc = []
        for j, (inst, prim, imask, s) in enumerate(scenes):
            if not (imask & rm & 0xff):
                continue
            h = s.trace(o, d, tmin, tmax, fl, use_bvh=0)
            if h.hit:
                front = facing[j][3].trace(o, d, tmin, tmax, rr.RAY_FLAG_CULL_BACK, use_bvh=0).hit
                acc.append((np.float32(h.t), inst, prim, bits(h.t), bits(h.u), bits(h.v), FRONT if front else BACK))
        acc.sort(key=lambda a: (a[0], a[1], a[2]))
        res.append(acc)
    return res


def check_slots(hits, counts, exp, rays, k):
    """hits: [n, k] HIT_DTYPE, counts: [n] or None; exp: expected()"""
    for r, acc in enumerate(exp):
        if counts is not None:
            assert counts[r] == len(acc), "ray %d: %d != %d" % (r, counts[r], len(acc))
        for j in range(k):
            g = hits[r, j]
            if j < len(acc):
                a = acc[j]
                assert (g["inst"], g["prim"], g["hit"]) == (a[1], a[2], a[6]), "ray %d slot %d" % (r, j)
                assert (bits(g["t"]), bits(g["u"]), bits(g["v"])) == (a[3], a[4], a[5]), "ray %d slot %d" % (r, j)
            else:
                assert g["hit"] == 0 and bits(g["t"]) == bits(rays["tmax"][r]), "ray %d slot %d" % (r, j)
                assert g["u"] == 0 and g["v"] == 0 and g["prim"] == 0 and g["inst"] == 0, "ray %d slot %d" % (r, j)


def instanced_scene(gpu, name):
    """-> (meshes, instances) built on the GPU"""
    if name == "masked":
        meshes, inst = [load("cube.obj"), load("monkey.obj")], rr.make_instances(**MASKED_INSTANCES)
    elif name == "facing":      # FRONT_COUNTERCLOCKWISE, mirrored (negative determinant) transforms and CULL_DISABLE
        mir = np.diag([-1.0, 1.0, 1.0]).astype(np.float32)
        T = [xf(-2.5, 0, 0), xf(0, 0, 0), xf(2.5, 0, 0), np.concatenate([mir, [[0], [2.5], [0]]], 1).astype(np.float32),
             np.concatenate([mir * 0.8, [[0], [-2.5], [0]]], 1).astype(np.float32), xf(0, 0, 2.5, (0.7, 0.7, 0.7), 0.5)]
        meshes = [load("cube.obj"), load("monkey.obj")]
        inst = rr.make_instances(transforms=T, meshes=[1, 0, 1, 1, 0, 0], masks=[1] * 6, flags=[0, 2, 1, 0, 2, 3])
    else:                       # "row": 24 cubes along x, so rays along the row cross far more than 16 triangles
        meshes = [load("cube.obj")]
        inst = rr.make_instances(transforms=[xf(3.0 * i - 34.5, 0, 0, (0.6, 0.6, 0.6), 0.1 * i) for i in range(24)], meshes=[0] * 24,
                                 masks=[1] * 24)
    gpu_scene(gpu, meshes, instances=inst)
    return meshes, inst


def row_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = np.stack([np.full(n, -40.0), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-0.002, 0.002, n), rng.uniform(-0.002, 0.002, n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rr.pack_rays(o, d, 1e-4, 1000.0, flags=rng.choice([0, 0x10, 0x20], n))


def soup_rays(verts, n, seed):
    P = verts["position"].astype(np.float64)
    ctr, ext = (P.min(0) + P.max(0)) / 2, max(float((P.max(0) - P.min(0)).max()), 1e-3)
    rng = np.random.default_rng(seed)
    o = ctr + rng.normal(size=(n, 3)) * ext
    d = P[rng.integers(0, len(P), n)] + rng.normal(size=(n, 3)) * ext * 0.02 - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rr.pack_rays(o, d, 1e-4, 1e6, flags=rng.choice([0, 0x10, 0x20], n))


# ------------------------------------------------------------------------------------------------- 1. complete and exact
@pytest.mark.parametrize("name", ["cube.obj", "sphere.obj", "monkey.obj", "soup-flat", "soup-mixed", "masked", "facing", "row"])
def test_slots_and_counts_are_the_oracles_sorted_set(gpu, name):
    if name.endswith(".obj"):
        meshes, inst = [load(name)], None
        gpu_scene(gpu, meshes)
        rays = random_rays(300, seed=len(name))
    elif name.startswith("soup"):
        m = soup(name[5:], 150, seed=7, collinear=False)
        meshes, inst = [m], None
        gpu_scene(gpu, meshes)
        rays = soup_rays(m[0], 300, seed=8)
    else:
        meshes, inst = instanced_scene(gpu, name)
        rays = row_rays(40, seed=9) if name == "row" else random_rays(150, seed=11, radius=5.0, extent=2.5,
                                                                        masks=RAY_MASKS if name == "masked" else (0xff,))
    hits, counts = gpu.query_rays_multi(rays, 16, counts=True)
    assert hits.shape == (len(rays), 16) and hits.dtype == rr.HIT_DTYPE and counts.dtype == np.uint32
    exp = expected(meshes, inst, rays)
    check_slots(hits, counts, exp, rays, 16)
    assert sum(len(a) > 0 for a in exp) >= len(rays) // 10
    if name == "row":
        assert min(len(a) for a in exp) > 16                       # truncation exercised on every ray
    if name == "facing":
        kinds = {(int(h["inst"]), int(h["hit"])) for h in hits.reshape(-1) if h["hit"]}
        assert {FRONT, BACK} <= {kk for _, kk in kinds} and len({i for i, _ in kinds}) >= 4


# ------------------------------------------------------------------------------------------------- 2. k = 1 is the closest hit
@pytest.mark.parametrize("name", ["cube.obj", "sphere.obj", "monkey.obj", "shell.obj", "ott.obj", "masked", "facing"])
def test_k1_is_the_closest_hit_query(gpu, name):
    if name.endswith(".obj"):
        gpu_scene(gpu, [load(name)])
        rays = random_rays(4000, seed=3)
    else:
        instanced_scene(gpu, name)
        rays = random_rays(4000, seed=4, radius=5.0, extent=2.5, masks=RAY_MASKS)
    q = gpu.query_rays(rays)
    for counts in (False, True):
        m = gpu.query_rays_multi(rays, 1, counts=counts)
        m = (m[0] if counts else m)[:, 0]
        for f in ("t", "u", "v", "prim", "inst"):
            assert m[f].tobytes() == q[f].tobytes(), f
        assert np.array_equal(m["hit"] != 0, q["hit"] != 0)
    assert q["hit"].sum() > 200


# ------------------------------------------------------------------------------------------------- 3. pruned == unpruned
@pytest.mark.parametrize("name", ["monkey.obj", "masked"])
def test_pruned_slots_equal_the_counted_run(gpu, name):
    if name == "masked":
        instanced_scene(gpu, name)
        rays = random_rays(20000, seed=5, radius=5.0, extent=2.5, masks=RAY_MASKS)
    else:
        gpu_scene(gpu, [load(name)])
        rays = random_rays(20000, seed=6)
    full, counts = gpu.query_rays_multi(rays, 16, counts=True)
    assert (counts > 4).sum() > 50
    for k in (1, 2, 3, 8, 16):
        assert gpu.query_rays_multi(rays, k).tobytes() == np.ascontiguousarray(full[:, :k]).tobytes(), k
        h, c = gpu.query_rays_multi(rays, k, counts=True)
        assert h.tobytes() == np.ascontiguousarray(full[:, :k]).tobytes() and np.array_equal(c, counts), k
    _, c0 = gpu.query_rays_multi(rays, 0, counts=True)
    assert np.array_equal(c0, counts)


# ------------------------------------------------------------------------------------------------- 4. coincident surfaces
def test_coincident_surfaces_return_both_twins_in_order(gpu):
    verts, idx = load("monkey.obj")
    n_tri = len(idx) // 3
    rays = random_rays(3000, seed=12, masks=(0xff,))
    # two instances of monkey with the same transform
    gpu_scene(gpu, [(verts, idx)], instances=rr.make_instances(transforms=[xf(0, 0, 0, (1, 1, 1), 0.3)] * 2, meshes=[0, 0], masks=[1, 1]))
    for twin_of in ("inst", "prim"):
        if twin_of == "prim":          # one mesh whose every triangle appears twice (prim p and p + n_tri)
            gpu_scene(gpu, [(verts, np.concatenate([idx, idx]))])
        hits, counts = gpu.query_rays_multi(rays, 16, counts=True)
        assert np.all(counts % 2 == 0) and (counts > 0).sum() > 200
        checked = 0
        for r in np.flatnonzero((counts > 0) & (counts <= 16)):
            h = hits[r, :int(counts[r])]
            key = [(int(x["inst"]), int(x["prim"])) for x in h]
            tb = bits(h["t"])
            for t0 in np.unique(tb):                                        # every equal-t group holds whole twin pairs, in order
                g = [key[j] for j in np.flatnonzero(tb == t0)]
                assert len(g) % 2 == 0 and g == sorted(g), (r, g)
                if twin_of == "inst":
                    assert [p for i, p in g if i == 0] == [p for i, p in g if i == 1], (r, g)
                else:
                    assert sorted(p % n_tri for _, p in g) == sorted(2 * [p for _, p in g if p < n_tri]), (r, g)
                checked += 1
        assert checked > 500
        # the workaround this replaces -- closest-hit queries that advance tmin to the last t -- returns one of each twin pair
        loop, cur = [], rays.copy()
        for _ in range(4):
            q = gpu.query_rays(cur)
            loop.append(q)
            cur["tmin"] = np.where(q["hit"] != 0, q["t"], cur["tmin"])
        sel = np.flatnonzero(counts >= 8)
        assert len(sel) > 20
        for r in sel:
            distinct = np.unique(hits[r, :min(int(counts[r]), 16)]["t"])
            assert [float(q["t"][r]) for q in loop] == [float(x) for x in distinct[:4]], r


# ------------------------------------------------------------------------------------------------- 6. masks and flags
def test_masks_flags_and_determinism(gpu):
    instanced_scene(gpu, "masked")
    rays = random_rays(20000, seed=13, radius=5.0, extent=2.5, masks=RAY_MASKS)
    hits, counts = gpu.query_rays_multi(rays, 8, counts=True)
    zero = (rays["instance_mask"] & 0xff) == 0
    assert zero.sum() > 100 and np.all(counts[zero] == 0) and np.all(hits[zero]["hit"] == 0)
    assert np.all(bits(hits[zero]["t"]) == bits(rays["tmax"][zero])[:, None])
    for extra in (ANY, 0x8, ANY | 0x8):
        r = rays.copy()
        r["flags"] |= extra
        h2, c2 = gpu.query_rays_multi(r, 8, counts=True)
        assert h2.tobytes() == hits.tobytes() and np.array_equal(c2, counts), hex(extra)
    h3, c3 = gpu.query_rays_multi(rays, 8, counts=True)
    assert h3.tobytes() == hits.tobytes() and np.array_equal(c3, counts)


# ------------------------------------------------------------------------------------------------- 7. device path
def test_device_multi_equals_host(gpu):
    import torch
    instanced_scene(gpu, "masked")
    rays = random_rays(20000, seed=14, radius=5.0, extent=2.5, masks=RAY_MASKS, any_frac=0.3)
    for k in (0, 1, 5, 16):
        host_c = None
        if k:
            host_h, host_c = gpu.query_rays_multi(rays, k, counts=True)
            host_p = gpu.query_rays_multi(rays, k)
            assert host_p.tobytes() == host_h.tobytes()
        else:
            _, host_c = gpu.query_rays_multi(rays, 0, counts=True)
        for dt in ("int32", "float32"):
            t = to_dev(rays, gpu, dt)
            torch.cuda.synchronize()
            h, c = gpu.query_rays_multi(t, k, counts=True)
            p = gpu.query_rays_multi(t, k) if k else None
            gpu.wait()
            assert h.dtype == t.dtype and h.device == t.device and tuple(h.shape) == (len(rays), k, 6)
            assert c.dtype == torch.int32 and tuple(c.shape) == (len(rays),)
            assert np.array_equal(c.cpu().numpy().view(np.uint32), host_c), (k, dt)
            if k:
                assert from_dev(h).tobytes() == host_h.tobytes() and from_dev(p).tobytes() == host_h.tobytes(), (k, dt)


def test_device_multi_of_1m_rays(gpu):
    import torch
    gpu_scene(gpu, [load("monkey.obj")])
    n = 1024 * 1024 + 17
    rays = random_rays(n, seed=15, masks=(0xff, 1, 2), any_frac=0.5)
    host = gpu.query_rays_multi(rays, 4)
    assert (host[:, 0]["hit"] != 0).sum() > n // 10
    t = to_dev(rays, gpu)
    torch.cuda.synchronize()
    out = gpu.query_rays_multi(t, 4)
    gpu.wait()
    assert from_dev(out).tobytes() == host.tobytes()


def test_device_multi_is_ordered_on_torch_stream(gpu):
    import torch
    instanced_scene(gpu, "masked")
    dev = "cuda:%d" % gpu.device
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        torch.cuda.synchronize()
        g = torch.Generator(device=dev)
        g.manual_seed(17)
        n = 1 << 19
        big = torch.randn((4096, 4096), device=dev, generator=g)
        big = big @ big                                     # queue work ahead of the rays on the same stream
        o = torch.randn((n, 3), device=dev, generator=g) * 3.0 + big[0, 0] * 0.0
        d = torch.rand((n, 3), device=dev, generator=g) * 2.4 - 1.2 - o
        d = d / d.norm(dim=1, keepdim=True)
        masks = torch.tensor(RAY_MASKS, device=dev)[torch.randint(0, len(RAY_MASKS), (n,), device=dev, generator=g)]
        t = rr.pack_rays(o, d, 1e-4, 100.0, flags=0, instance_mask=masks)
        out, cnt = gpu.query_rays_multi(t, 4, counts=True)  # no synchronisation between producing the rays and the query
        torch.cuda.current_stream().synchronize()
        rays = np.ascontiguousarray(t.cpu().numpy()).view(rr.RAY_DTYPE).reshape(-1)
        host, hc = gpu.query_rays_multi(rays, 4, counts=True)
        assert hc.sum() > n // 10
        assert from_dev(out).tobytes() == host.tobytes() and np.array_equal(cnt.cpu().numpy().view(np.uint32), hc)
    finally:
        gpu.reset_stream()


def test_multi_errors(gpu):
    import torch
    dev = "cuda:%d" % gpu.device
    L = rr.lib()
    fresh = rr.Renderer(gpu.device)
    try:
        rays = random_rays(64, seed=1)
        t = to_dev(rays, fresh)
        for call in (lambda: fresh.query_rays_multi(rays, 4), lambda: fresh.query_rays_multi(t, 4, counts=True)):
            with pytest.raises(rr.RRError) as e:
                call()                                                          # nothing built
            assert e.value.status == RR_ERR_STATE
        verts, idx = load("cube.obj")
        mid = fresh.upload_mesh(verts, idx)
        fresh.build_blas(mid, allow_update=True)
        with pytest.raises(rr.RRError) as e:
            fresh.query_rays_multi(t, 2)                                        # BLAS built, no TLAS yet
        assert e.value.status == RR_ERR_STATE
        fresh.build_tlas(rr.make_instances(meshes=[mid]), allow_update=True)
        fresh.query_rays_multi(t, 2)
        fresh.update_mesh_vertices(mid, verts)
        fresh.build_blas(mid, update=True)
        for call in (lambda: fresh.query_rays_multi(t, 2), lambda: fresh.query_rays_multi(rays, 2, counts=True)):
            with pytest.raises(rr.RRError) as e:
                call()                                                          # BLAS updated, TLAS not
            assert e.value.status == RR_ERR_STATE
        fresh.build_tlas(rr.make_instances(meshes=[mid]), update=True)
        ok = from_dev(fresh.query_rays_multi(t, 2))
        fresh.wait()
        assert ok.tobytes() == fresh.query_rays_multi(rays, 2).tobytes()
        # k out of range, k == 0 without counts: the C ABI and the Python checks
        hits = torch.zeros(64 * 17 * 6 + 8, dtype=torch.int32, device=dev)
        cnt = torch.zeros(64 + 8, dtype=torch.int32, device=dev)
        hp, cp, rp = hits.data_ptr(), cnt.data_ptr(), t.data_ptr()
        for k, c in ((17, cp), (0, 0), (100, 0)):
            assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp), 64, k, C.c_void_p(hp), C.c_void_p(c or None)) == RR_ERR_INVALID_ARGUMENT
            hh = np.zeros(64 * 17, rr.HIT_DTYPE)
            cc = np.zeros(64, np.uint32)
            assert L.rr_query_rays_multi(fresh._h, rays.ctypes.data, 64, k, hh.ctypes.data, cc.ctypes.data if c else None) == RR_ERR_INVALID_ARGUMENT
        for k, c in ((17, True), (0, False), (-1, True)):
            with pytest.raises(ValueError):
                fresh.query_rays_multi(rays, k, counts=c)
        # misaligned rays, hits or counts; n == 0 is RR_OK
        assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp + 4), 8, 2, C.c_void_p(hp), C.c_void_p(cp)) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp), 64, 2, C.c_void_p(hp + 2), C.c_void_p(cp)) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp), 64, 2, C.c_void_p(hp), C.c_void_p(cp + 1)) == RR_ERR_INVALID_ARGUMENT
        assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp), 0, 2, C.c_void_p(hp + 2), C.c_void_p(cp + 1)) == 0
        assert L.rr_query_rays_multi_device(fresh._h, C.c_void_p(rp), 64, 2, C.c_void_p(hp + 4), C.c_void_p(cp + 4)) == 0
        fresh.wait()
        # wrong device, shape, dtype, layout
        for bad in (t.cpu(), t[:, :8].contiguous(), t.reshape(-1), t.to(torch.float64),
                    torch.zeros((64, 16), dtype=torch.int32, device=dev)[:, :12]):
            with pytest.raises(ValueError):
                fresh.query_rays_multi(bad, 4)
        e = fresh.query_rays_multi(torch.empty((0, 12), dtype=torch.int32, device=dev), 3, counts=True)
        assert tuple(e[0].shape) == (0, 3, 6) and tuple(e[1].shape) == (0,)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 8. after a refit
def test_multi_after_refit_equals_a_fresh_build(gpu):
    verts, idx = load("monkey.obj")
    P = verts["position"].astype(np.float64)
    dv = verts.copy()
    P[:, 1] += 0.15 * np.sin(4.0 * P[:, 0]) * np.cos(3.0 * P[:, 2])
    dv["position"] = P.astype(np.float32)
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0.4, 0.1, -2.2, (0.6, 0.6, 0.6), 0.7)], meshes=[0, 0], masks=[1, 2])
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, allow_update=True)
    ii = inst.copy()
    ii["blas"] = mid
    gpu.build_tlas(ii, allow_update=True)
    gpu.update_mesh_vertices(mid, dv)
    gpu.build_blas(mid, update=True)
    gpu.build_tlas(ii, update=True)
    rays = random_rays(6000, seed=51, radius=5.0, extent=2.0, masks=(0xff, 1, 2, 3, 0))
    refit = [gpu.query_rays_multi(rays, 16, counts=True), gpu.query_rays_multi(rays, 3)]
    gpu_scene(gpu, [(dv, idx)], instances=inst)
    fresh = [gpu.query_rays_multi(rays, 16, counts=True), gpu.query_rays_multi(rays, 3)]
    assert refit[0][0].tobytes() == fresh[0][0].tobytes() and np.array_equal(refit[0][1], fresh[0][1])
    assert refit[1].tobytes() == fresh[1].tobytes()
    assert (fresh[0][1] >= 2).sum() > 200


# ------------------------------------------------------------------------------------------------- 9. user-level sanity
def _dirs(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize("name", ["sphere.obj", "cube.obj"])
def test_crossing_parity_inside_and_outside(gpu, name):
    gpu_scene(gpu, [load(name)])
    n = 4096
    rng = np.random.default_rng(16)
    inside = rng.uniform(-0.5, 0.5, (n, 3))
    outside = _dirs(n, 17) * rng.uniform(2.5, 4.0, (n, 1))
    for pts, parity in ((inside, 1), (outside, 0)):
        _, c = gpu.query_rays_multi(rr.pack_rays(pts, _dirs(n, 18), 0.0, 1e6), 0, counts=True)
        # Moller-Trumbore is not watertight: a ray through a shared edge may count it twice or not at all (none expected here)
        assert np.mean(c % 2 == parity) >= 0.999, (name, parity, np.bincount(c))
    _, c = gpu.query_rays_multi(rr.pack_rays(inside, _dirs(n, 19), 0.0, 1e6), 0, counts=True)
    assert np.mean(c == 1) >= 0.999          # convex: exactly one exit


def test_sphere_chord_length(gpu):
    verts, idx = load("sphere.obj")
    gpu_scene(gpu, [(verts, idx)])
    P = verts["position"].astype(np.float64)
    R = float(np.linalg.norm(P, axis=1).max())
    T = P[idx].reshape(-1, 3, 3)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    r_in = float(np.min(np.abs(np.einsum("ij,ij->i", nrm / np.linalg.norm(nrm, axis=1, keepdims=True), T[:, 0]))))
    n = 2000
    rng = np.random.default_rng(20)
    d = _dirs(n, 21)
    b = rng.uniform(0.0, 1.2, n)                         # offset of the ray from the centre
    perp = np.cross(d, _dirs(n, 22))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    o = perp * b[:, None] - d * 5.0
    hits = gpu.query_rays_multi(rr.pack_rays(o, d, 1e-4, 100.0), 2)
    ok = (hits[:, 0]["hit"] != 0) & (hits[:, 1]["hit"] != 0) & (hits[:, 0]["hit"] != hits[:, 1]["hit"])     # in and out: a front/back pair
    assert ok.mean() >= 0.999
    chord = (hits[:, 1]["t"] - hits[:, 0]["t"]).astype(np.float64)[ok]
    lo = 2.0 * np.sqrt(r_in ** 2 - b[ok] ** 2) - 1e-4
    hi = 2.0 * np.sqrt(R ** 2 - b[ok] ** 2) + 1e-4
    assert np.all((chord >= lo) & (chord <= hi))
