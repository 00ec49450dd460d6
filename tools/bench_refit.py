"""Update builds against full rebuilds: python tools/bench_refit.py [--reps N] [--json out.json]

Times, with HIP events on the context's stream (rr_timing_begin / rr_timing_end around the call, which includes the call's
own host synchronisation), for monkey.obj, ott.obj and the 131 072-triangle procedural sphere:
  * a full BLAS build (PREFER_FAST_TRACE: PLOC up to 32 768 triangles, the Morton LBVH above; and PREFER_FAST_BUILD),
  * a BLAS refit (PERFORM_UPDATE) over moved vertices, and the host vertex upload in front of it,
  * a TLAS update against a TLAS build of the same one-instance scene.
Then renders C2's shape on monkey.obj (1920x1080, 4 refraction / 2 reflection bounces, Depth 16) after a moderate
deformation, once through the refitted tree and once through a fresh build of the same vertices, to show what refitting
costs in tree quality (node visits per ray, kernel time); the frames must be identical.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import asset, procedural_env  # noqa: E402


def sphere_grid(n_side, seed=3):
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(0.02, np.pi - 0.02, n_side + 1), np.linspace(0, 2 * np.pi, n_side + 1), indexing="ij")
    rad = 1.0 + 0.08 * np.sin(7 * u) * np.cos(5 * v) + 0.01 * rng.standard_normal(u.shape)
    P = np.stack([rad * np.sin(u) * np.cos(v), rad * np.cos(u), rad * np.sin(u) * np.sin(v)], -1).astype(np.float32)
    N = P / np.linalg.norm(P, axis=-1, keepdims=True)
    idx = np.arange((n_side + 1) * (n_side + 1)).reshape(n_side + 1, n_side + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tri = np.concatenate([np.stack([a, c, b], 1), np.stack([a, d, c], 1)]).astype(np.int64)
    verts = np.zeros(tri.size, rr.VERTEX_DTYPE)
    verts["position"] = P.reshape(-1, 3)[tri.ravel()]
    verts["norm"] = N.reshape(-1, 3)[tri.ravel()].astype(np.float32)
    return verts, np.arange(tri.size, dtype=np.uint32)


def wave(verts, phase, amp=0.1):
    v = verts.copy()
    P = v["position"]
    P[:, 1] += (amp * np.sin(4.0 * P[:, 0] + phase) * np.cos(3.0 * P[:, 2])).astype(np.float32)
    return v


def timed(r, fn, reps):
    ts = []
    for _ in range(reps):
        r.wait()
        r.timing_begin()
        fn()
        ts.append(r.timing_end())
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    out = {"unit": "ms (median, min) over %d reps, HIP events" % a.reps, "meshes": {}}
    cases = []
    for name in ("monkey.obj", "ott.obj"):
        m = rr.Mesh()
        m.load(asset(name))
        cases.append((name, m.verts, m.indices))
    v, i = sphere_grid(256)
    cases.append(("sphere grid 131072", v, i))
    for name, verts, idx in cases:
        dv = wave(verts, 0.5)
        row = {"tris": len(idx) // 3}
        mid = r.upload_mesh(verts, idx)
        row["build_fast_trace"] = timed(r, lambda: r.build_blas(mid), a.reps)
        row["build_fast_build"] = timed(r, lambda: r.build_blas(mid, fast_build=True), a.reps)
        r.build_blas(mid, allow_update=True)
        row["build_fast_trace_allow_update"] = timed(r, lambda: r.build_blas(mid, allow_update=True), a.reps)
        row["vertex_upload_host"] = timed(r, lambda: r.update_mesh_vertices(mid, dv), a.reps)
        row["refit"] = timed(r, lambda: r.build_blas(mid, update=True), a.reps)
        inst = rr.make_instances(meshes=[mid])
        row["tlas_build"] = timed(r, lambda: r.build_tlas(inst, allow_update=True), a.reps)
        row["tlas_update"] = timed(r, lambda: r.build_tlas(inst, update=True), a.reps)
        out["meshes"][name] = row
        print("%-20s %7d tris | build %.3f ms (fast_build %.3f) | refit %.3f ms | vertex upload %.3f ms | TLAS build %.3f / update %.3f ms"
              % (name, row["tris"], row["build_fast_trace"][0], row["build_fast_build"][0], row["refit"][0],
                 row["vertex_upload_host"][0], row["tlas_build"][0], row["tlas_update"][0]), flush=True)

    # tree quality: C2's shape on monkey.obj after a moderate deformation, refitted vs rebuilt
    m = rr.Mesh()
    m.load(asset("monkey.obj"))
    r.upload_envmap(procedural_env(2048, 1024, seed=1))
    dv = wave(m.verts, 1.0, amp=0.15)
    W, H, D = 1920, 1080, 16
    cams = [rr.camera_orbit(0.01 * (k + 1)) for k in range(D)]
    p = rr.default_params(max_refract=4, max_reflect=2)
    res = {}
    for how in ("refit", "rebuild"):
        if how == "refit":
            mid = r.upload_mesh(m.verts, m.indices)
            r.build_blas(mid, allow_update=True)
            r.update_mesh_vertices(mid, dv)
            r.build_blas(mid, update=True)
        else:
            mid = r.upload_mesh(dv, m.indices)
            r.build_blas(mid)
        r.build_tlas(rr.make_instances(meshes=[mid]))
        r.set_tile_partition(0, 1)
        r.dispatch_rays_batch(W, H, cams, rr.default_params(max_refract=4, max_reflect=2, flags=rr.DISPATCH_COLLECT_STATS))
        st = r.stats()
        visits = st.node_visits / max(st.rays, 1)
        for _ in range(3):
            r.dispatch_rays_batch(W, H, cams, p)
        ts = []
        for _ in range(a.reps):
            r.timing_begin()
            r.dispatch_rays_batch(W, H, cams, p)
            ts.append(r.timing_end())
        frame = r.read_frame(slice=D - 1).copy()
        res[how] = {"node_visits_per_ray": visits, "ms_per_frame": float(np.median(ts)) / D, "frame": frame,
                    "kernel": r.stats().render_kernel_name.decode()}
    same = bool(np.array_equal(res["refit"].pop("frame"), res["rebuild"].pop("frame")))
    out["c2_shape_monkey"] = {"workload": "monkey.obj 1920x1080, 4 refraction / 2 reflection bounces, Depth 16, wave amp 0.15",
                              "refit": res["refit"], "rebuild": res["rebuild"], "frames_identical": same}
    print("monkey 1920x1080 (C2's shape): refit %.4f ms/frame, %.2f node visits/ray | rebuild %.4f ms/frame, %.2f node visits/ray | frames identical: %s"
          % (res["refit"]["ms_per_frame"], res["refit"]["node_visits_per_ray"], res["rebuild"]["ms_per_frame"],
             res["rebuild"]["node_visits_per_ray"], same), flush=True)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
