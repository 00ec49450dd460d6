"""GPU: update builds (DXR ALLOW_UPDATE / PERFORM_UPDATE) -- vertex updates, BLAS refit and TLAS refit against the CPU oracle.

A refit keeps the hierarchy and recomputes every box, triangle / normal record, bound and grid from the new vertices; the
hierarchy never changes a traced hit or a pixel, so everything below is compared bit-exactly: against the oracle's brute
force (TraceRay), the oracle's path-weight render (frames) and fresh builds of the same vertices.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from refit_helpers import blas_bytes, deform, _two_instances
from scenes import check_closest, check_frame, gpu, load, oracle_scene, procedural_mesh, random_rays, render_both  # noqa: F401  (gpu: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE = 1, 5


def gpu_refit_scene(gpu, verts, idx, deformed, fast_build=False):
    """upload + ALLOW_UPDATE build of `verts`, then the vertices replaced by `deformed` and the BLAS refitted; -> mesh id"""
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, fast_build=fast_build, allow_update=True)
    gpu.update_mesh_vertices(mid, deformed)
    gpu.build_blas(mid, update=True)
    gpu.build_tlas(rr.make_instances(meshes=[mid]))
    return mid


# ----------------------------------------------------------------------------------------- 1. identity refit
@pytest.mark.parametrize("fast_build", [True, False])
@pytest.mark.parametrize("name", ["cube.obj", "monkey.obj", "ott.obj"])
def test_identity_refit_reproduces_the_build_byte_for_byte(gpu, name, fast_build):
    verts, idx = load(name)
    plain = gpu.upload_mesh(verts, idx)
    gpu.build_blas(plain, fast_build=fast_build)
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, fast_build=fast_build, allow_update=True)
    built = blas_bytes(gpu, mid)
    for a, b in zip(blas_bytes(gpu, plain), built):                     # ALLOW_UPDATE builds the same nodes
        assert a.tobytes() == b.tobytes()
    gpu.update_mesh_vertices(mid, verts)
    gpu.build_blas(mid, update=True)
    for a, b in zip(built, blas_bytes(gpu, mid)):
        assert a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------------------- 2. deformed meshes trace exactly
@pytest.mark.parametrize("kind", ["wave", "scale", "jitter", "permute"])
@pytest.mark.parametrize("name", ["monkey.obj", "ott.obj"])
def test_refitted_mesh_traces_bit_exact_vs_brute_force(gpu, name, kind):
    verts, idx = load(name)
    dv = deform(verts, kind, seed=len(name))
    gpu_refit_scene(gpu, verts, idx, dv)
    s = oracle_scene([(dv, idx)], procedural_env(32, 16))
    P = dv["position"].astype(np.float64)
    c, r = (P.min(0) + P.max(0)) / 2, np.abs(P.max(0) - P.min(0)).max() / 2
    rays = random_rays(3000 if name == "monkey.obj" else 1500, seed=len(name) + len(kind), radius=4.0 * r, extent=1.2 * r,
                       cull_p=(0.45, 0.45, 0.1))
    rays["origin"] += c.astype(np.float32)
    assert check_closest(gpu.trace_rays(rays), s, rays) > len(rays) // 20


def test_refitted_large_mesh_traces_bit_exact(gpu):
    """131 072 triangles: the refit climb across thousands of workgroups on every XCD"""
    verts, idx = procedural_mesh(256, seed=3)
    assert len(idx) // 3 == 131072
    dv = deform(verts, "wave", seed=5)
    mid = gpu_refit_scene(gpu, verts, idx, dv, fast_build=True)
    s = oracle_scene([(dv, idx)], procedural_env(32, 16))
    rays = random_rays(400, seed=41, radius=3.0, cull_p=(0.45, 0.45, 0.1))
    assert check_closest(gpu.trace_rays(rays), s, rays) > 40
    # the same refit equals a fresh build of the deformed vertices wherever the hierarchy does not show: triangle records
    # per primitive, bounds
    fresh = gpu.upload_mesh(dv, idx)
    gpu.build_blas(fresh, fast_build=True)
    _, t_ref = gpu.download_blas(mid)
    _, t_new = gpu.download_blas(fresh)
    assert np.array_equal(t_ref[np.argsort(t_ref["prim"])].view(np.uint8), t_new[np.argsort(t_new["prim"])].view(np.uint8))
    _, o1, c1 = gpu.download_qnodes(mid)
    _, o2, c2 = gpu.download_qnodes(fresh)
    assert o1.tobytes() == o2.tobytes() and c1.tobytes() == c2.tobytes()


# ----------------------------------------------------------------------------------------- 3. the refitted tree is sound
@pytest.mark.parametrize("kind", ["scale", "permute"])
@pytest.mark.parametrize("name", ["cube.obj", "monkey.obj", "ott.obj"])
def test_refitted_tree_is_sound(gpu, name, kind):
    verts, idx = load(name)
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, allow_update=True)
    gpu.build_tlas(rr.make_instances(meshes=[mid]))
    depth0 = gpu.stats().bvh_depth
    nodes0, _ = gpu.download_blas(mid)
    dv = deform(verts, kind, seed=7)
    gpu.update_mesh_vertices(mid, dv)
    gpu.build_blas(mid, update=True)
    gpu.build_tlas(rr.make_instances(meshes=[mid]))
    assert gpu.stats().bvh_depth == depth0
    nodes, tris = gpu.download_blas(mid)
    q, org, cell = gpu.download_qnodes(mid)
    assert np.array_equal(nodes["c"], nodes0["c"]) and np.array_equal(nodes["pad"], nodes0["pad"])
    # quantised boxes contain the fp32 boxes (the bounds of the parity suite's check)
    org, cell = org.astype(np.float64), cell.astype(np.float64)
    for ax, (lo, hi) in enumerate((("lox", "hix"), ("loy", "hiy"), ("loz", "hiz"))):
        qlo = org[ax] + q[lo].astype(np.float64) * cell[ax]
        qhi = org[ax] + q[hi].astype(np.float64) * cell[ax]
        flo, fhi = nodes[lo].astype(np.float64), nodes[hi].astype(np.float64)
        real = flo <= fhi
        assert np.all(np.abs(q[lo][real].astype(np.float64)) <= 32768) and np.all(np.abs(q[hi][real].astype(np.float64)) <= 32768)
        assert np.all(qlo[real] <= flo[real]) and np.all(qhi[real] >= fhi[real])
        assert np.all(flo[real] - qlo[real] <= 18 * cell[ax]) and np.all(qhi[real] - fhi[real] <= 18 * cell[ax])
    c, qc = nodes["c"], q["c"]
    assert np.array_equal(qc[c < 0], c[c < 0]) and np.array_equal(qc[c >= 0], c[c >= 0] * 32)
    # every triangle lies inside its leaf's slot of the parent box, every internal slot is the union of its children
    T = len(tris)
    P = dv["position"][idx].reshape(T, 3, 3)[tris["prim"]]
    assert np.array_equal(tris["v0"], P[:, 0]) and np.array_equal(tris["e1"], P[:, 1] - P[:, 0])
    lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], -1)
    hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], -1)
    node_lo, node_hi = lo.min(1), hi.max(1)
    for k in (0, 1):
        ck = nodes["c"][:, k]
        leaf = ck < 0
        if T == 1 and k == 1:
            continue
        exp_lo = np.where(leaf[:, None], P.min(1)[np.where(leaf, ~ck, 0)], node_lo[np.where(leaf, 0, ck)])
        exp_hi = np.where(leaf[:, None], P.max(1)[np.where(leaf, ~ck, 0)], node_hi[np.where(leaf, 0, ck)])
        assert np.array_equal(lo[:, k], exp_lo) and np.array_equal(hi[:, k], exp_hi)
    # the grid is over the new bounds
    Pall = dv["position"][idx].astype(np.float64)
    assert np.all(org - 32768 * cell <= Pall.min(0)) and np.all(org + 32768 * cell >= Pall.max(0))


# ----------------------------------------------------------------------------------------- 4. frames
def test_refitted_frame_matches_the_oracle(gpu):
    verts, idx = load("monkey.obj")
    env = procedural_env(256, 128, seed=3)
    dv = deform(verts, "wave", seed=2)
    gpu_refit_scene(gpu, verts, idx, dv)
    gpu.upload_envmap(env)
    check_frame(*render_both(gpu, oracle_scene([(dv, idx)], env), 0.01, 240, 136, max_refract=8))


def test_refitted_frames_of_a_deep_batch_on_the_lds_kernel(gpu, tmp_path):
    """a 24-slice DispatchRays(W, H, 24) on k_render_lds (BLAS nodes in LDS) over refitted nodes, every slice against the oracle"""
    verts, idx = load("monkey.obj")
    dv = deform(verts, "jitter", seed=4)
    env = procedural_env(64, 32, seed=5)
    np.savez(tmp_path / "in.npz", verts=verts, idx=idx, dv=dv, env=env)
    W, H, D = 64, 48, 24
    code = ("import sys, json, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "import refraction_raytracing_dxr_amd as rr\n"
            "d = np.load(sys.argv[1])\n"
            "r = rr.Renderer(0)\n"
            "mid = r.upload_mesh(d['verts'], d['idx'])\n"
            "r.build_blas(mid, allow_update=True)\n"
            "r.update_mesh_vertices(mid, d['dv'])\n"
            "r.build_blas(mid, update=True)\n"
            "r.build_tlas(rr.make_instances(meshes=[mid]))\n"
            "r.upload_envmap(d['env'])\n"
            "r.set_tile_partition(0, 1)\n"
            "cams = [rr.camera_orbit(0.01 + 0.26 * k) for k in range(%d)]\n"
            "r.dispatch_rays_batch(%d, %d, cams, rr.default_params(max_refract=6, flags=rr.DISPATCH_FLOAT_OUTPUT))\n"
            "st = r.stats()\n"
            "out = np.stack([r.read_frame(want_float=True, slice=k)[1] for k in range(%d)])\n"
            "np.save(sys.argv[2], out)\n"
            "print(json.dumps({'kernel': st.render_kernel, 'name': st.render_kernel_name.decode(), 'overflow': st.traversal_overflow}))\n"
            "r.close()\n") % (ROOT, D, W, H, D)
    p = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "out.npy")], capture_output=True,
                       text=True, env=dict(os.environ, RR_DEBUG_KERNEL="lds"), timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["kernel"] == 1 and info["overflow"] == 0, info
    out = np.load(tmp_path / "out.npy")
    s = oracle_scene([(dv, idx)], env)
    for k in range(D):
        sc = rr.camera_orbit(0.01 + 0.26 * k)
        pw = s.render(np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32), W, H,
                      O.default_params(use_bvh=1, accum_mode=1, max_refract=6))
        assert np.array_equal(out[k][..., :3].view(np.uint32), pw["rgb"].view(np.uint32)), "slice %d" % k


def test_two_instance_scene_after_blas_and_tlas_updates_matches_the_oracle(gpu):
    verts, idx = load("monkey.obj")
    env = procedural_env(128, 64, seed=9)
    gpu.upload_envmap(env)
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, allow_update=True)
    gpu.build_tlas(_two_instances(mid, 0.0), allow_update=True)
    for step, kind in enumerate(("wave", "scale")):
        dv = deform(verts, kind, seed=step)
        if kind == "scale":
            dv["position"] = (dv["position"] - np.array([0.5, -0.25, 1.0], np.float32)) / np.float32(2.0)   # x1.5, still in view
        gpu.update_mesh_vertices(mid, dv)
        gpu.build_blas(mid, update=True)
        inst = _two_instances(mid, 0.3 * (step + 1))
        gpu.build_tlas(inst, update=True)
        o_inst = inst.copy()
        o_inst["blas"] = 0
        check_frame(*render_both(gpu, oracle_scene([(dv, idx)], env, o_inst), 0.4 + step, 200, 120, max_refract=6))


# ----------------------------------------------------------------------------------------- 5. animation
def test_animation_through_refits_equals_fresh_builds(gpu):
    verts, idx = load("monkey.obj")
    env = procedural_env(128, 64, seed=21)
    gpu.upload_envmap(env)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(rr.camera_orbit(0.9))
    p = rr.default_params(max_refract=8, flags=rr.DISPATCH_FLOAT_OUTPUT)
    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, allow_update=True)
    gpu.build_tlas(rr.make_instances(meshes=[mid]), allow_update=True)
    kinds = ["wave", "jitter", "wave", "scale", "jitter", "wave", "permute", "wave"]
    refit_frames = []
    n_meshes = None
    for f, kind in enumerate(kinds):
        gpu.update_mesh_vertices(mid, deform(verts, kind, seed=f, amount=0.5 + 0.1 * f))
        gpu.build_blas(mid, update=True)
        gpu.build_tlas(rr.make_instances(meshes=[mid]), update=True)
        probe = gpu.upload_mesh(verts[:3], np.arange(3, dtype=np.uint32))     # the next mesh id tells how many exist
        if n_meshes is None:
            n_meshes = probe
        assert probe == n_meshes + f                                       # only the probes add meshes: the refit adds none
        gpu.dispatch_rays(320, 180, p)
        refit_frames.append(gpu.read_frame(want_float=True)[1].copy())
    for f, kind in enumerate(kinds):
        fresh = gpu.upload_mesh(deform(verts, kind, seed=f, amount=0.5 + 0.1 * f), idx)
        gpu.build_blas(fresh)
        gpu.build_tlas(rr.make_instances(meshes=[fresh]))
        gpu.dispatch_rays(320, 180, p)
        assert np.array_equal(gpu.read_frame(want_float=True)[1].view(np.uint32), refit_frames[f].view(np.uint32)), "frame %d" % f


# ----------------------------------------------------------------------------------------- 6. device path
def test_device_vertex_update_equals_the_host_path(gpu):
    import torch
    verts, idx = load("monkey.obj")
    dv = deform(verts, "wave", seed=11)
    env = procedural_env(64, 32, seed=2)
    gpu.upload_envmap(env)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(rr.camera_orbit(2.0))
    p = rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT)
    out = []
    for device_path in (False, True):
        mid = gpu.upload_mesh(verts, idx)
        gpu.build_blas(mid, allow_update=True)
        if device_path:
            t = torch.from_numpy(dv.view(np.float32).reshape(-1, 8).copy()).to("cuda:%d" % gpu.device)
            torch.cuda.synchronize()
            gpu.update_mesh_vertices(mid, t)
        else:
            gpu.update_mesh_vertices(mid, dv)
        gpu.build_blas(mid, update=True)
        gpu.build_tlas(rr.make_instances(meshes=[mid]))
        gpu.dispatch_rays(160, 120, p)
        out.append([x.tobytes() for x in blas_bytes(gpu, mid)] + [gpu.read_frame(want_float=True)[1].tobytes()])
    assert out[0] == out[1]


# ----------------------------------------------------------------------------------------- 7. errors
def test_update_errors(gpu):
    import torch
    verts, idx = load("cube.obj")
    gpu.upload_envmap(procedural_env(32, 16))
    plain = gpu.upload_mesh(verts, idx)
    gpu.build_blas(plain)
    with pytest.raises(rr.RRError) as e:
        gpu.build_blas(plain, update=True)                                 # no ALLOW_UPDATE
    assert e.value.status == RR_ERR_STATE

    mid = gpu.upload_mesh(verts, idx)
    gpu.build_blas(mid, allow_update=True)
    before = [x.tobytes() for x in blas_bytes(gpu, mid)]
    with pytest.raises(rr.RRError) as e:
        gpu.update_mesh_vertices(mid, verts[:-1])                          # wrong count
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    bad = verts.copy()
    bad["position"][3, 1] = np.nan
    with pytest.raises(rr.RRError) as e:
        gpu.update_mesh_vertices(mid, bad)                                 # non-finite, host path: refused at once
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    gpu.build_blas(mid, update=True)                                       # the mesh kept its vertices
    assert [x.tobytes() for x in blas_bytes(gpu, mid)] == before
    bad["position"][3, 1] = 1e30
    t = torch.from_numpy(bad.view(np.float32).reshape(-1, 8).copy()).to("cuda:%d" % gpu.device)
    torch.cuda.synchronize()
    gpu.update_mesh_vertices(mid, t)                                       # device path: found by the check kernel ...
    with pytest.raises(rr.RRError) as e:
        gpu.build_blas(mid, update=True)                                   # ... and reported by the next build
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    assert [x.tobytes() for x in blas_bytes(gpu, mid)] == before
    gpu.build_blas(mid, update=True)                                       # the verdict was taken: the mesh is usable as it was
    assert [x.tobytes() for x in blas_bytes(gpu, mid)] == before

    # a dispatch after a BLAS update and before a TLAS build / update
    gpu.build_tlas(rr.make_instances(meshes=[mid, mid], transforms=[np.eye(4)[:3], np.eye(4)[:3] * 0.5]), allow_update=True)
    gpu.set_camera(rr.camera_orbit(0.5))
    gpu.dispatch_rays(32, 32)
    gpu.update_mesh_vertices(mid, deform(verts, "wave"))
    with pytest.raises(rr.RRError) as e:
        gpu.build_tlas(rr.make_instances(meshes=[mid, mid], transforms=[np.eye(4)[:3]] * 2), update=True)  # stale BLAS
    assert e.value.status == RR_ERR_STATE
    gpu.build_blas(mid, update=True)
    with pytest.raises(rr.RRError) as e:
        gpu.dispatch_rays(32, 32)
    assert e.value.status == RR_ERR_STATE
    # a TLAS update with another instance count or another BLAS in a slot
    with pytest.raises(rr.RRError) as e:
        gpu.build_tlas(rr.make_instances(meshes=[mid]), update=True)
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    with pytest.raises(rr.RRError) as e:
        gpu.build_tlas(rr.make_instances(meshes=[mid, plain], transforms=[np.eye(4)[:3]] * 2), update=True)
    assert e.value.status == RR_ERR_INVALID_ARGUMENT
    gpu.build_tlas(rr.make_instances(meshes=[mid, mid], transforms=[np.eye(4)[:3]] * 2), update=True)
    gpu.dispatch_rays(32, 32)
    # a TLAS built without ALLOW_UPDATE cannot be updated
    gpu.build_tlas(rr.make_instances(meshes=[mid]))
    with pytest.raises(rr.RRError) as e:
        gpu.build_tlas(rr.make_instances(meshes=[mid]), update=True)
    assert e.value.status == RR_ERR_STATE
