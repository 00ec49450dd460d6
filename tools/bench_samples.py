"""Supersampled frames against the radiance queries that shade the same samples:
python tools/bench_samples.py [--reps N] [--json out.json]

monkey.obj at 1920x1080 (camera_orbit(0.01), the reference's bounce limits), S = 4 and 16 samples per pixel of the built-in
patterns.  Two ways to the same colours, both with float, RGBA8 and count outputs in device memory:
  * render_samples(device=True): one launch of k_render_samples, the samples generated and resolved in registers;
  * S shade_rays calls on the samples' rays, generated beforehand (rr.camera_rays, row-major) and already in device memory:
    S launches of k_shade_rays.  Neither the ray generation nor the reduction of the S colour arrays is timed -- the comparison
    is between the launches alone, which favours this side.
The outputs of both are allocated before the timing and the C entry points are called directly, so a timed call holds no allocation.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the two alternating, median of --reps after a
warm-up of each; the outputs are compared bit for bit first.  Mrays/s: TraceRay calls (ray_counts) per microsecond.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import procedural_env  # noqa: E402
from bench_query import W, H, load  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    v, i = load("monkey.obj")
    r.load_scene(v, i, procedural_env(512, 256, seed=0))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params()
    out = {"unit": "ms (median of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "scene": "monkey.obj", "samples": {}}
    print("%-3s %-15s %9s %11s %9s" % ("S", "path", "ms", "traced", "Mrays/s"), flush=True)
    for S in (4, 16):
        rays = [torch.from_numpy(rr.camera_rays(sc, W, H, float(ox), float(oy), p.tmin_primary, p.tmax_primary).view(np.int32)
                                 .reshape(-1, 12)).to(dev) for ox, oy in rr.sample_pattern(S)]
        torch.cuda.synchronize()

        # every output is allocated here, outside the timed calls, and the entry points are called directly: a timed call
        # is the launches and nothing else
        n = W * H
        P = C.c_void_p
        L = rr.lib()
        f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        cnt = torch.empty((H, W), dtype=torch.int32, device=dev)
        q = [(torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.uint8, device=dev),
              torch.empty((n,), dtype=torch.int32, device=dev)) for _ in rays]
        torch.cuda.synchronize()

        def samples():
            rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p), None, S, P(f32.data_ptr()), P(u8.data_ptr()), P(cnt.data_ptr()))
            assert rc == 0, rc

        def queries():
            for t, (qf, qu, qc) in zip(rays, q):
                rc = L.rr_shade_rays_device(r._h, P(t.data_ptr()), n, C.byref(p), P(qf.data_ptr()), P(qu.data_ptr()), P(qc.data_ptr()))
                assert rc == 0, rc
        # warm-up of both, and the two must agree: ((c_0 + c_1) + ...) / S in fp32
        samples()
        queries()
        r.wait()
        acc = q[0][0][:, :3].clone()
        for f, _, _ in q[1:]:
            acc = acc + f[:, :3]
        same = bool(torch.equal((acc / float(S)).view(torch.int32), f32.reshape(-1, 4)[:, :3].contiguous().view(torch.int32)))
        traced = int(cnt.sum().item())
        same_n = traced == sum(int(c.sum().item()) for _, _, c in q)
        del acc
        ts, tq = [], []
        for _ in range(a.reps):                     # alternating: what else the machine does hits both alike
            r.wait()
            r.timing_begin()
            samples()
            ts.append(r.timing_end())
            r.wait()
            r.timing_begin()
            queries()
            tq.append(r.timing_end())
        ms_s, ms_q = float(np.median(ts)), float(np.median(tq))
        out["samples"][S] = {"render_samples_ms": ms_s, "shade_rays_ms": ms_q, "traced": traced, "equal_colours": same, "equal_counts": same_n,
                             "render_samples_all_ms": ts, "shade_rays_all_ms": tq}
        print("%-3d %-15s %9.3f %11d %9.0f" % (S, "render_samples", ms_s, traced, traced / ms_s / 1e3), flush=True)
        print("%-3d %-15s %9.3f %11d %9.0f   colours equal: %s, counts equal: %s" % (S, "S x shade_rays", ms_q, traced, traced / ms_q / 1e3, same, same_n),
              flush=True)
        del rays, q
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
