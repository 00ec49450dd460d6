"""Adaptive supersampling against the supersampled frames it is composed of:
python tools/bench_adaptive.py [--reps N] [--thresholds a,b,c] [--samples BASE,MAX] [--once] [--json out.json]

monkey.obj at 1920x1080 (camera_orbit(0.01), the reference's bounce limits, procedural 512x256 environment map), the built-in
pattern of MAX samples.  Three paths, all with float, RGBA8 and count outputs in device memory allocated before the timing, the C
entry points called directly:
  * render_samples on the first BASE and on all MAX samples of that pattern: k_render_samples, the yardsticks;
  * render_adaptive(BASE, MAX) at each threshold: base, classify, scan, list and refine on a pre-allocated workspace.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the paths alternating, medians and ranges of
--reps after a warm-up of each.  f is the refined share of the frame's pixels; the linear model is what the sample counts alone
would cost, t_base + f * (t_max - t_base), and the overhead is the adaptive time over it.  Before the timing every pixel is
compared with render_samples(BASE) or render_samples(MAX) according to its sample count.
--once: one untimed adaptive call per threshold and nothing else (for a kernel trace of the stages).
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--thresholds", default="%g,%g,%g" % (rr.ADAPTIVE_THRESHOLD / 2, rr.ADAPTIVE_THRESHOLD, rr.ADAPTIVE_THRESHOLD * 2))
    ap.add_argument("--samples", default="4,16")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n_base, n_max = (int(s) for s in a.samples.split(","))
    thresholds = [float(t) for t in a.thresholds.split(",")]
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    v, i = load("monkey.obj")
    r.load_scene(v, i, procedural_env(512, 256, seed=0))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params()
    P = C.c_void_p
    L = rr.lib()

    def outputs():
        return (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
                torch.empty((H, W), dtype=torch.int32, device=dev))
    lo, hi, ad = outputs(), outputs(), outputs()
    taken = torch.empty((H, W), dtype=torch.int32, device=dev)
    ws_bytes = int(L.rr_host_adaptive_workspace_bytes(W, H))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    pattern = rr.sample_pattern(n_max)              # the base samples are its first n_base, not the built-in pattern of n_base

    def samples(S, o):
        rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p), pattern.ctypes.data, S, P(o[0].data_ptr()), P(o[1].data_ptr()), P(o[2].data_ptr()))
        assert rc == 0, rc

    def adaptive(t):
        rc = L.rr_render_adaptive_device(r._h, W, H, C.byref(sc), C.byref(p), None, n_base, n_max, t, P(ad[0].data_ptr()), P(ad[1].data_ptr()),
                                         P(ad[2].data_ptr()), P(taken.data_ptr()), P(ws.data_ptr()), ws_bytes)
        assert rc == 0, rc

    if a.once:
        for t in thresholds:
            adaptive(t)
        r.wait()
        r.close()
        return
    # warm-up of every path, and the composition: each pixel is that pixel of one of the two supersampled frames
    samples(n_base, lo)
    samples(n_max, hi)
    share, equal = {}, {}
    for t in thresholds:
        adaptive(t)
        r.wait()
        m = taken == n_max
        share[t] = float(m.float().mean().item())
        equal[t] = all(bool(torch.equal(g, torch.where(m.reshape(m.shape + (1,) * (g.dim() - 2)), h, l))) for g, l, h in zip(ad, lo, hi)) and \
            bool(((taken == n_base) | m).all().item())
    paths = [("samples_base", lambda: samples(n_base, lo)), ("samples_max", lambda: samples(n_max, hi))] + \
            [("adaptive_%g" % t, (lambda t=t: adaptive(t))) for t in thresholds]
    times = {name: [] for name, _ in paths}
    for _ in range(a.reps):                         # alternating: what else the machine does hits all alike
        for name, call in paths:
            r.wait()
            r.timing_begin()
            call()
            times[name].append(r.timing_end())
    med = {k: float(np.median(v)) for k, v in times.items()}
    rng = {k: (float(min(v)), float(max(v))) for k, v in times.items()}
    t_lo, t_hi = med["samples_base"], med["samples_max"]
    out = {"unit": "ms (median of %d reps, HIP events)" % a.reps, "frame": [W, H], "scene": "monkey.obj", "samples": [n_base, n_max],
           "render_samples_ms": {n_base: t_lo, n_max: t_hi}, "all_ms": times, "thresholds": {}}
    print("%-22s %8s %17s" % ("path", "ms", "range"), flush=True)
    for S, k in ((n_base, "samples_base"), (n_max, "samples_max")):
        print("%-22s %8.3f %8.3f-%8.3f" % ("render_samples(%d)" % S, med[k], rng[k][0], rng[k][1]), flush=True)
    for t in thresholds:
        k = "adaptive_%g" % t
        f = share[t]
        model = t_lo + f * (t_hi - t_lo)
        out["thresholds"][t] = {"refined_share": f, "adaptive_ms": med[k], "range_ms": rng[k], "linear_model_ms": model,
                                "overhead_ms": med[k] - model, "composition_holds": equal[t]}
        print("%-22s %8.3f %8.3f-%8.3f   f = %.4f, linear model %.3f ms, overhead %+.3f ms (%+.1f %%), composition holds: %s"
              % ("adaptive t=%g" % t, med[k], rng[k][0], rng[k][1], f, model, med[k] - model, 100.0 * (med[k] - model) / model, equal[t]), flush=True)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
