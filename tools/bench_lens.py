"""Thin-lens frames against supersampled frames with the same S: python tools/bench_lens.py [--reps N] [--json out.json]

monkey.obj at 1920x1080 (camera_orbit(0.01), the reference's bounce limits), S = 4 and 16 samples per pixel of the built-in
patterns, float, RGBA8 and count outputs in device memory, allocated before the timing; the C entry points are called directly:
  * render_samples: one launch of k_render_samples, every sample from the pinhole;
  * render_lens with radius 0: k_render_lens on the pinhole path (the same rays: what the extra kernel arguments and the branch cost);
  * render_lens with an open aperture, focused at the mesh (5 units) for radii 0.05, 0.2 and 0.8: the 64 rays of a wave start on one
    lens point and fan out, the primary rays lose coherence and the lens rectangle grows with the radius.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the variants taking turns, median of --reps after a
warm-up of each.  The radius-0 frame is compared with render_samples' byte for byte first.  Mrays/s: TraceRay calls per microsecond.
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

FOCUS = 5.0
RADII = (0.0, 0.05, 0.2, 0.8)


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
    P = v["position"][i]
    bounds = np.concatenate([P.min(axis=0), P.max(axis=0)])
    sc = rr.camera_orbit(0.01)
    p = rr.default_params()
    L = rr.lib()
    Pt = C.c_void_p
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    cnt = torch.empty((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    out = {"unit": "ms (median of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "scene": "monkey.obj", "focus": FOCUS, "samples": {}}
    print("%-3s %-22s %9s %11s %9s %8s  %s" % ("S", "path", "ms", "traced", "Mrays/s", "x pinhole", "rectangle"), flush=True)
    for S in (4, 16):
        def samples():
            rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
            assert rc == 0, rc

        def lens_call(lens):
            def call():
                rc = L.rr_render_lens_device(r._h, W, H, C.byref(sc), C.byref(p), None, None, S, C.byref(lens), *outs)
                assert rc == 0, rc
            return call
        variants = [("render_samples", samples, None)] + [("render_lens r=%g" % rad, lens_call(rr.Lens(rad, FOCUS)), rr.Lens(rad, FOCUS)) for rad in RADII]
        traced, frames = {}, {}
        for name, call, _ in variants:                              # warm-up, and what each traces
            call()
            r.wait()
            traced[name] = int(cnt.sum().item())
            frames[name] = (f32.cpu().numpy().tobytes(), u8.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes())
        same = frames["render_samples"] == frames["render_lens r=0"]
        times = {name: [] for name, _, _ in variants}
        for _ in range(a.reps):                                     # taking turns: what else the machine does hits all alike
            for name, call, _ in variants:
                r.wait()
                r.timing_begin()
                call()
                times[name].append(r.timing_end())
        base = float(np.median(times["render_samples"]))
        res = {"radius0_equals_render_samples": same}
        for name, _, lens in variants:
            ms = float(np.median(times[name]))
            rect = rr.lens_screen_rect(bounds, sc, lens, W, H) if lens is not None else rr.lens_screen_rect(bounds, sc, rr.Lens(0.0, FOCUS), W, H)
            res[name] = {"ms": ms, "traced": traced[name], "all_ms": times[name], "rect": rect}
            print("%-3d %-22s %9.3f %11d %9.0f %8.3f  %s" % (S, name, ms, traced[name], traced[name] / ms / 1e3, ms / base, rect), flush=True)
        print("%-3d radius 0 equals render_samples byte for byte: %s" % (S, same), flush=True)
        out["samples"][S] = res
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
