"""Transparent shadows against the first-hit shadow ray: python tools/bench_shadows.py [--reps N] [--steps 0 8] [--json out.json]

What rr_set_shadow_steps costs.  The README's tumbler on a table from shipped meshes: a glass cube (the tumbler) holding a sphere of
tinted water holding a small cube of ice, standing on a flattened opaque cube under the README's sun and lamp, both of which see the
glass (shadow_mask 0xff).  rr_render_surfaces_device at 1920x1080, camera_orbit(0.01), the reference's bounce limits, 4 samples per
pixel, float, RGBA8 and count outputs in device memory, allocated before the timing; the C entry point is called directly.  One
variant per --steps value K: K = 0 launches k_render_surfaces, the kernel that rendered the scene before the setting existed; K >= 1
launches k_render_shadows, whose shadow rays walk through the glass in at most K closest-hit calls.  The frames must differ (the
shadow is no longer black) and the K >= 1 frame must trace more rays.  Timed with HIP events on the context's stream
(rr_timing_begin / rr_timing_end), the variants taking turns, median and range of --reps after a warm-up of each (a first launch also
loads the code object).  Mrays/s: TraceRay calls per microsecond.  With --steps 0 alone the setter is never called: that run needs
nothing but rr_render_surfaces_device."""
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

S = 4
TABLE = [(1.5, (0.02, 0.02, 0.02)), (1.33, (0.9, 0.3, 0.1)), (1.31, (0, 0, 0)), (1.0, (0, 0, 0))]      # glass, a tinted drink, ice; row 3 is the table's
LIGHTS = [rr.directional_light((-0.5, 1.0, -0.4), (1.2, 1.1, 0.9), 0xff), rr.point_light((1.5, 2.5, -1.0), (6, 6, 7), 0xff)]
AMBIENT = (0.05, 0.05, 0.05)


def xf(t, s):
    m = np.zeros((3, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2] = s
    m[:, 3] = t
    return m


def scene(r):
    """the tumbler (cube, half side 0.6), the water (sphere.obj inside it), the ice (a cube inside the water) and the table"""
    cube, sphere = (r.upload_mesh(*load(n)) for n in ("cube.obj", "sphere.obj"))
    r.build_blas(cube)
    r.build_blas(sphere)
    top = -0.62
    r.build_tlas(rr.make_instances(transforms=[xf((0, 0, 0), (0.6, 0.6, 0.6)), xf((0.02, -0.02, 0.02), (0.3, 0.3, 0.3)), xf((0.05, 0.03, -0.01), (0.12, 0.12, 0.12)),
                                               xf((0, top - 0.1, 0), (3.0, 0.1, 3.0))], meshes=[cube, sphere, cube, cube], materials=[0, 1, 2, 3]))
    r.upload_envmap(procedural_env(512, 256, seed=0))
    r.set_materials(TABLE)
    r.set_surfaces([rr.glass(), rr.glass(), rr.glass(), rr.opaque((0.7, 0.6, 0.5), specular=(0.1, 0.1, 0.1))])
    r.set_lights(LIGHTS, AMBIENT)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    f32, u8, cnt = (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
                    torch.empty((H, W), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    scene(r)
    L, Pt = rr.lib(), C.c_void_p
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    sc, p = rr.camera_orbit(0.01), rr.default_params()
    pos = rr.sample_pattern(S)
    set_steps = a.steps != [0]

    def frame(k):
        if set_steps:
            r.set_shadow_steps(k)                               # (host state that travels with the launch: outside the timed interval)
        r.wait()
        r.timing_begin()
        rc = L.rr_render_surfaces_device(r._h, W, H, C.byref(sc), C.byref(p), pos.ctypes.data, S, *outs)
        ms = r.timing_end()
        assert rc == 0, rc
        return ms

    traced, frames = {}, {}
    for k in a.steps:                                               # warm-up, and what each traces
        frame(k)
        r.wait()
        torch.cuda.synchronize()
        traced[k] = int(cnt.sum().item())
        frames[k] = f32.cpu().numpy().copy()
    times = {k: [] for k in a.steps}
    for _ in range(a.reps):                                         # taking turns: what else the machine does hits all alike
        for k in a.steps:
            times[k].append(frame(k))
    base = float(np.median(times[a.steps[0]]))
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "samples": S, "variants": {}}
    print("the tumbler on a table, %dx%d, %d samples per pixel" % (W, H, S), flush=True)
    print("  %-18s %9s %19s %14s %9s %8s" % ("shadow_steps", "ms", "range", "rays per frame", "Mrays/s", "x first"), flush=True)
    for k in a.steps:
        t = times[k]
        ms = float(np.median(t))
        out["variants"]["K = %d" % k] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[k], "all_ms": t, "ratio": ms / base}
        print("  %-18s %9.3f %8.3f - %8.3f %14d %9.0f %8.3f" % ("K = %d" % k, ms, min(t), max(t), traced[k], traced[k] / ms / 1e3, ms / base), flush=True)
    walked = [k for k in a.steps if k >= 2]
    if 0 in a.steps and walked:
        k = walked[0]
        differ = int((frames[0].view(np.uint32) != frames[k].view(np.uint32)).any(axis=-1).sum())
        print("  %d of %d pixels differ between K = 0 and K = %d" % (differ, W * H, k), flush=True)
        assert differ > 0 and traced[k] > traced[0], "the walks changed nothing: is the glass between the table and a light?"
        out["pixels_differing"] = differ
    if set_steps:
        r.set_shadow_steps(0)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
