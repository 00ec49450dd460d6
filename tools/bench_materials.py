"""Per-instance glass against the scalar frames with the same S: python tools/bench_materials.py [--reps N] [--json out.json]

What the RGB path weight, the material fetch and the absorption cost.  1920x1080, camera_orbit(0.01), the reference's bounce limits,
S = 16 samples per pixel, float, RGBA8 and count outputs in device memory, allocated before the timing; the C entry points are
called directly.  Two scenes:
  * monkey.obj, one identity instance (the builds without a top level):
      render_samples at ior 1.3, the yardstick;
      render_materials with the table { 1.3, 0, 0, 0 } -- the same rays and, checked first, the same bytes;
      render_materials with { 1.3, 0.8, 0.1, 0.1 }: the same rays again, every inside hit absorbs;
  * shell + cube + ott, three BLASes under one top level (the two-level builds):
      render_samples at ior 1.3;
      render_materials with three rows { 1.3, 0, 0, 0 }, compared with it byte for byte;
      render_materials with the mixed table { 1.3, 0,0,0 }, { 1.5, 0.8,0.1,0.1 }, { 1.1, 0.05,0.4,2.0 }: other rays.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), a scene's variants taking turns, median and range of
--reps after a warm-up of each.  Mrays/s: TraceRay calls per microsecond.
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

S, IOR = 16, 1.3
MIXED = np.array([(1.3, (0.0, 0.0, 0.0)), (1.5, (0.8, 0.1, 0.1)), (1.1, (0.05, 0.4, 2.0))], rr.MATERIAL_DTYPE)


def table(rows):
    return np.array(rows, rr.MATERIAL_DTYPE)


def moved(tz):
    m = np.eye(4, dtype=np.float32)[:3].copy()
    m[2, 3] = tz
    return m


def run_scene(r, name, variants, reps, bufs):
    """variants: [(label, table or None for render_samples)] -> {label: figures}; the first is the yardstick, the second must equal it"""
    import torch
    f32, u8, cnt = bufs
    L, Pt = rr.lib(), C.c_void_p
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params(ior=IOR)

    def call(tab):
        if tab is None:
            rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
        else:
            rc = L.rr_render_materials_device(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
        assert rc == 0, rc
    traced, frames = {}, {}
    for label, tab in variants:                                     # warm-up, and what each traces
        if tab is not None:
            r.set_materials(tab)
        call(tab)
        r.wait()
        torch.cuda.synchronize()
        traced[label] = int(cnt.sum().item())
        frames[label] = (f32.cpu().numpy().tobytes(), u8.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes())
    same = frames[variants[0][0]] == frames[variants[1][0]]
    times = {label: [] for label, _ in variants}
    for _ in range(reps):                                           # taking turns: what else the machine does hits all alike
        for label, tab in variants:
            if tab is not None:
                r.set_materials(tab)                                # (outside the timed interval)
            r.wait()
            r.timing_begin()
            call(tab)
            times[label].append(r.timing_end())
    base = float(np.median(times[variants[0][0]]))
    out = {"uniform_table_equals_render_samples": same, "variants": {}}
    print("%s" % name, flush=True)
    print("  %-34s %9s %19s %11s %9s %9s" % ("path", "ms", "range", "traced", "Mrays/s", "x samples"), flush=True)
    for label, _ in variants:
        t = times[label]
        ms = float(np.median(t))
        out["variants"][label] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[label], "all_ms": t}
        print("  %-34s %9.3f %8.3f - %8.3f %11d %9.0f %9.3f" % (label, ms, min(t), max(t), traced[label], traced[label] / ms / 1e3, ms / base), flush=True)
    print("  uniform table equals render_samples byte for byte: %s" % same, flush=True)
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
    r.load_scene(*load("monkey.obj"), env)
    out["scenes"]["monkey.obj"] = run_scene(r, "monkey.obj, one identity instance", [
        ("render_samples", None), ("render_materials uniform", table([(IOR, (0, 0, 0))])), ("render_materials tinted", table([(IOR, (0.8, 0.1, 0.1))]))],
        a.reps, bufs)
    ids = []
    for name in ("shell.obj", "cube.obj", "ott.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])
    r.build_tlas(rr.make_instances(transforms=[moved(0.0), moved(-4.0), moved(4.0)], meshes=ids, materials=[0, 1, 2]))
    out["scenes"]["shell + cube + ott"] = run_scene(r, "shell + cube + ott, three instances", [
        ("render_samples", None), ("render_materials uniform", table([(IOR, (0, 0, 0))] * 3)), ("render_materials mixed", MIXED)], a.reps, bufs)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if all(s["uniform_table_equals_render_samples"] for s in out["scenes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
