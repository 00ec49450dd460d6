"""Ray queries, closest hit against first hit: python tools/bench_query.py [--reps N] [--json out.json]

Times rr_query_rays (host arrays: upload, kernel, download, synchronise) and rr_query_rays_device (rays already in device memory,
a torch tensor; the kernel alone) with HIP events on the context's stream (rr_timing_begin / rr_timing_end around the call), on
monkey.obj, ott.obj, the 131 072-triangle procedural sphere and C4 (shell.obj + cube.obj + ott.obj under one TLAS), for three
ray sets of one 1920x1080 frame's worth of rays each:
  * coherent:   the camera's primary rays (camera_orbit(0.01), tmin 1e-4, tmax 100),
  * incoherent: random rays through the scene's box (as in the parity tests),
  * shadow:     from the closest hits of the primary rays towards a point light (tmin 1e-3, tmax = the light's distance): the
                occlusion rays first-hit termination is for.
No culling.  Each set is traced as closest-hit rays and as RAY_FLAG_ACCEPT_FIRST_HIT rays; results in Mrays/s (median).  Under
rocprofv3 --kernel-trace the k_query_rays launches give the kernel times alone.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import asset  # noqa: E402
from bench_refit import sphere_grid  # noqa: E402

W, H = 1920, 1080
LIGHT = np.array([5.0, 8.0, -6.0])


def load(name):
    m = rr.Mesh()
    assert m.load(asset(name))
    return m.verts, m.indices


def xf(tx, ty, tz):
    m = np.eye(4, dtype=np.float32)[:3].copy()
    m[:, 3] = (tx, ty, tz)
    return m


def primary_rays():
    sc = rr.camera_orbit(0.01)
    M = np.array(sc.proj_inv, np.float32)
    cam = np.array(sc.camera_loc, np.float32)[:3]
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    sx = (x + np.float32(0.5)) / np.float32(W) * np.float32(2) - np.float32(1)
    sy = -((y + np.float32(0.5)) / np.float32(H) * np.float32(2) - np.float32(1))
    R = np.stack([(sx * M[0] + sy * M[1]) + M[3], (sx * M[4] + sy * M[5]) + M[7], (sx * M[8] + sy * M[9]) + M[11]], -1).reshape(-1, 3)
    R /= np.linalg.norm(R, axis=1, keepdims=True)
    return rr.pack_rays(np.broadcast_to(cam, R.shape), R, 1e-4, 100.0)


def random_rays(n, lo, hi, seed=0):
    rng = np.random.default_rng(seed)
    ctr, ext = (lo + hi) / 2, float((hi - lo).max()) / 2
    o = rng.normal(size=(n, 3))
    o = ctr + o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.0, 3.0 * ext, (n, 1))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rr.pack_rays(o, d, 1e-4, 1000.0)


def shadow_rays(prim, hits):
    h = hits["hit"] != 0
    p = prim["origin"][h].astype(np.float64) + prim["dir"][h].astype(np.float64) * hits["t"][h, None]
    d = LIGHT - p
    dist = np.linalg.norm(d, axis=1)
    return rr.pack_rays(p, d / dist[:, None], 1e-3, dist)


def timed(r, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        r.wait()
        r.timing_begin()
        fn()
        ts.append(r.timing_end())
    return float(np.median(ts))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    scenes = [("monkey.obj", [load("monkey.obj")], None), ("ott.obj", [load("ott.obj")], None),
              ("sphere grid 131072", [sphere_grid(256)], None),
              ("C4", [load("shell.obj"), load("cube.obj"), load("ott.obj")], rr.make_instances(
                  transforms=[xf(0, 0, 0), xf(0, 0, -4.0), xf(0, 0, 4.0)], meshes=[0, 1, 2]))]
    out = {"unit": "Mrays/s (median of %d reps, HIP events)" % a.reps, "frame": [W, H], "scenes": {}}
    prim = primary_rays()
    print("%-20s %-10s %9s | %-21s | %-21s | %s" % ("scene", "rays", "n", "host closest / first", "device closest / first",
                                                    "first-hit t > closest t"), flush=True)
    for name, meshes, inst in scenes:
        ids = []
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for k, (v, i) in enumerate(meshes):
            mid = r.upload_mesh(v, i)
            r.build_blas(mid)
            ids.append(mid)
            off = inst["transform"][k].reshape(3, 4)[:, 3] if inst is not None else 0.0
            lo = np.minimum(lo, v["position"].min(0) + off)
            hi = np.maximum(hi, v["position"].max(0) + off)
        ii = rr.make_instances(meshes=[ids[0]]) if inst is None else inst.copy()
        if inst is not None:
            ii["blas"] = [ids[int(b)] for b in inst["blas"]]
        r.build_tlas(ii)
        sets = {"coherent": prim, "incoherent": random_rays(W * H, lo, hi)}
        sets["shadow"] = shadow_rays(prim, r.query_rays(prim))
        row = {}
        for sname, rays in sets.items():
            first = rays.copy()
            first["flags"] |= rr.RAY_FLAG_ACCEPT_FIRST_HIT
            n = len(rays)
            if n == 0:
                continue
            res = {"n": n}
            for mode, rs in (("closest", rays), ("first", first)):
                res["host_" + mode] = n / timed(r, lambda: r.query_rays(rs), a.reps) / 1e3
                t = torch.from_numpy(rs.view(np.int32).reshape(-1, 12).copy()).to(dev)
                torch.cuda.synchronize()
                res["device_" + mode] = n / timed(r, lambda: r.query_rays(t), a.reps) / 1e3
                del t
            hc, hf = r.query_rays(rays), r.query_rays(first)
            assert np.array_equal(hc["hit"], hf["hit"])
            h = hc["hit"] != 0
            res["hit_fraction"] = float(h.mean())
            res["first_further_fraction"] = float((hf["t"][h] > hc["t"][h]).mean()) if h.any() else 0.0
            row[sname] = res
            print("%-20s %-10s %9d | %9.0f / %9.0f | %9.0f / %9.0f | %.3f of hits (%.2f hit)"
                  % (name, sname, n, res["host_closest"], res["host_first"], res["device_closest"], res["device_first"],
                     res["first_further_fraction"], res["hit_fraction"]), flush=True)
        out["scenes"][name] = row
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
