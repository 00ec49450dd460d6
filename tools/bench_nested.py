"""Nested media against per-instance glass with the same table: python tools/bench_nested.py [--reps N] [--json out.json]

What unculled traversal, the medium list and the eleven-word parked ray cost.  1920x1080, camera_orbit(0.01), the reference's bounce
limits, S = 16 samples per pixel, float, RGBA8 and count outputs in device memory, allocated before the timing; the C entry points are
called directly.  Two scenes of closed meshes, on which the two trees agree wherever culled and unculled TraceRay find the same hits:
  * shell.obj, one identity instance (the builds without a top level), one tinted row;
  * sphere + cube + shell, three disjoint instances under one top level (the two-level builds), the mixed table.
Before the timing the two frames are compared and the pixels that differ are counted: the shipped sphere and shell are smooth-shaded,
and at a silhouette a child direction built from the shading normal can dip under the faceted surface, where the unculled ray meets a
back face the culled one never sees (include/rrdxr.h, "Reduction").  Such a pixel costs the nested tree one more TraceRay.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the two calls taking turns, median and range of
--reps after a warm-up of each (a first launch also loads the code object).  Mrays/s: TraceRay calls per microsecond.
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
from bench_materials import MIXED, moved, table  # noqa: E402
from bench_query import W, H, load  # noqa: E402

S = 16


def run_scene(r, name, tab, reps, bufs):
    import torch
    f32, u8, cnt = bufs
    L, Pt = rr.lib(), C.c_void_p
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params()
    calls = {"render_materials": L.rr_render_materials_device, "render_nested": L.rr_render_nested_device}
    r.set_materials(tab)
    traced, frames = {}, {}
    for label, f in calls.items():                                  # warm-up, and what each traces
        rc = f(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
        assert rc == 0, rc
        r.wait()
        torch.cuda.synchronize()
        traced[label] = int(cnt.sum().item())
        frames[label] = (f32.cpu().numpy().copy(), u8.cpu().numpy().copy(), cnt.cpu().numpy().copy())
    a, b = frames["render_materials"], frames["render_nested"]
    d_colour = int((a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=-1).sum())
    d_count = int((a[2] != b[2]).sum())
    times = {label: [] for label in calls}
    for _ in range(reps):                                           # taking turns: what else the machine does hits both alike
        for label, f in calls.items():
            r.wait()
            r.timing_begin()
            rc = f(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
            times[label].append(r.timing_end())
            assert rc == 0, rc
    base = float(np.median(times["render_materials"]))
    out = {"pixels_differing_in_colour": d_colour, "pixels_differing_in_count": d_count, "variants": {}}
    print("%s" % name, flush=True)
    print("  %-20s %9s %19s %11s %9s %11s" % ("path", "ms", "range", "traced", "Mrays/s", "x materials"), flush=True)
    for label in calls:
        t = times[label]
        ms = float(np.median(t))
        out["variants"][label] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[label], "all_ms": t}
        print("  %-20s %9.3f %8.3f - %8.3f %11d %9.0f %11.3f" % (label, ms, min(t), max(t), traced[label], traced[label] / ms / 1e3, ms / base), flush=True)
    print("  of %d pixels, %d differ in colour and %d in their TraceRay count" % (W * H, d_colour, d_count), flush=True)
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    bufs = (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
            torch.empty((H, W), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    env = procedural_env(512, 256, seed=0)
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "samples": S, "scenes": {}}
    r.load_scene(*load("shell.obj"), env)
    out["scenes"]["shell.obj"] = run_scene(r, "shell.obj, one identity instance", table([(1.5, (0.8, 0.1, 0.1))]), a.reps, bufs)
    ids = []
    for name in ("sphere.obj", "cube.obj", "shell.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])
    r.build_tlas(rr.make_instances(transforms=[moved(0.0), moved(-4.0), moved(4.0)], meshes=ids, materials=[0, 1, 2]))
    out["scenes"]["sphere + cube + shell"] = run_scene(r, "sphere + cube + shell, three disjoint instances", MIXED, a.reps, bufs)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
