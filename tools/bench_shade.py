"""Radiance queries against the dispatch that shades the same rays: python tools/bench_shade.py [--reps N] [--json out.json]

Times rr_shade_rays_device (rays in device memory, a torch tensor; float, RGBA8 and count outputs) with HIP events on the context's
stream (rr_timing_begin / rr_timing_end around the call, median of --reps) on monkey.obj, ott.obj and C4 (shell.obj + cube.obj +
ott.obj under one TLAS) with the reference's bounce limits, on the primary rays of one 1920x1080 orbit frame (camera_orbit(0.01),
tmin 1e-4, tmax 100) in three orders:
  * blocks:    8x8 pixel blocks, row-major, Morton lane order inside a block -- the 64 rays a k_render_fused wave holds,
  * row-major: the frame's raster order (a wave is 64 pixels of one row),
  * permuted:  a random permutation (what incoherence costs a lock-step wave: information, not a target).
Next to them the kernel time of rr_dispatch_rays for the same frame with FLOAT_OUTPUT | DEBUG_NO_CULL | TIME_KERNEL (every
primary ray traced, as a radiance query must) under RR_DEBUG_KERNEL=fused, which this tool sets: k_render_fused's way of shading
the same rays.  Results: input rays per second and traced rays (TraceRay calls) per second.
"""
import argparse
import json
import os
import sys

import numpy as np

os.environ["RR_DEBUG_KERNEL"] = "fused"            # read at rr_create: the dispatches below run k_render_fused
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import procedural_env  # noqa: E402
from bench_query import W, H, load, primary_rays, timed, xf  # noqa: E402


def block_order():
    """pixel index (row-major) of ray j when the frame is walked in 8x8 blocks, Morton order inside a block"""
    lane = np.arange(64)

    def compact(v):
        v = v & 0x55
        v = (v ^ (v >> 1)) & 0x33
        return (v ^ (v >> 2)) & 0x0f
    lx, ly = compact(lane), compact(lane >> 1)
    bx, by = np.meshgrid(np.arange(W // 8), np.arange(H // 8))
    x = (bx.reshape(-1, 1) * 8 + lx[None, :]).reshape(-1)
    y = (by.reshape(-1, 1) * 8 + ly[None, :]).reshape(-1)
    return y * W + x


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert W % 8 == 0 and H % 8 == 0
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    scenes = [("monkey.obj", [load("monkey.obj")], None), ("ott.obj", [load("ott.obj")], None),
              ("C4", [load("shell.obj"), load("cube.obj"), load("ott.obj")], rr.make_instances(
                  transforms=[xf(0, 0, 0), xf(0, 0, -4.0), xf(0, 0, 4.0)], meshes=[0, 1, 2]))]
    prim = primary_rays()
    n = len(prim)
    orders = {"blocks": block_order(), "row-major": np.arange(n), "permuted": np.random.default_rng(0).permutation(n)}
    env = procedural_env(512, 256, seed=0)
    p = rr.default_params()
    sc = rr.camera_orbit(0.01)
    out = {"unit": "ms (median of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "scenes": {}}
    print("%-11s %-10s %9s %9s %12s %13s" % ("scene", "rays", "ms", "traced", "input Mray/s", "traced Mray/s"), flush=True)
    for name, meshes, inst in scenes:
        ids = []
        for v, i in meshes:
            mid = r.upload_mesh(v, i)
            r.build_blas(mid)
            ids.append(mid)
        ii = rr.make_instances(meshes=[ids[0]]) if inst is None else inst.copy()
        if inst is not None:
            ii["blas"] = [ids[int(b)] for b in inst["blas"]]
        r.build_tlas(ii)
        r.upload_envmap(env)
        row = {}
        # the dispatch: k_render_fused on the same primary rays, none culled
        r.set_camera(sc)
        dp = rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_DEBUG_NO_CULL | rr.DISPATCH_TIME_KERNEL)
        r.dispatch_rays(W, H, dp)
        r.kernel_time()
        ts = []
        for _ in range(a.reps):
            r.dispatch_rays(W, H, dp)
            ts.append(r.kernel_time()[0])
        st = r.stats()
        traced = int(st.rays)
        ms = float(np.median(ts))
        row["dispatch"] = {"ms": ms, "traced": traced, "kernel": st.render_kernel_name.decode()}
        _, frame = r.read_frame(want_float=True)
        frame = frame.reshape(-1, 4).copy()
        print("%-11s %-10s %9.3f %9d %12.0f %13.0f   %s" % (name, "dispatch", ms, traced, n / ms / 1e3, traced / ms / 1e3,
                                                           row["dispatch"]["kernel"]), flush=True)
        for oname, perm in orders.items():
            t = torch.from_numpy(prim[perm].view(np.int32).reshape(-1, 12).copy()).to(dev)
            torch.cuda.synchronize()
            f32, _, cnt = r.shade_rays(t, p, rgba8=True, ray_counts=True)
            r.wait()
            # (the rays are numpy's restatement of GenerateCameraRay, a rounding away from the kernel's: equal trees, close colours)
            traced = int(cnt.sum().item())
            diff = float(np.abs(f32.cpu().numpy() - frame[perm]).max())
            ms = timed(r, lambda: r.shade_rays(t, p, rgba8=True, ray_counts=True), a.reps)
            row[oname] = {"ms": ms, "traced": traced, "max_abs_diff_to_dispatch": diff}
            print("%-11s %-10s %9.3f %9d %12.0f %13.0f   max |shade - dispatch| %.3g" % (name, oname, ms, traced, n / ms / 1e3, traced / ms / 1e3, diff),
                  flush=True)
            del t
        out["scenes"][name] = row
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
