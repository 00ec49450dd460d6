"""Spectral frames against supersampled frames with the same S: python tools/bench_spectral.py [--reps N] [--json out.json]

monkey.obj at 1920x1080 (camera_orbit(0.01), the reference's bounce limits), S = 16 samples per pixel, float, RGBA8 and count
outputs in device memory, allocated before the timing; the C entry points are called directly:
  * render_samples: one launch of k_render_samples, the yardstick;
  * render_spectral with bands = NULL: k_render_spectral with sixteen times (ior, 1, 1, 1) -- the same rays, so what the band table's
    scalar loads and the three multiplications per sample cost; compared with render_samples' frame byte for byte first;
  * render_spectral with spectral_bands(16, 1.3, 30) paired with the built-in sixteen positions;
  * render_spectral with 4 positions x 4 bands crossed (spectral_bands(4, 1.3, 30));
  * the emulation the entry point replaces: 4 render_samples calls of 4 samples, one per band's ior, and a weighted sum of the four
    float frames in torch (its result is not the same frame: it resolves per band first).
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end; torch works on that stream too), the variants taking
turns, median and range of --reps after a warm-up of each.  Mrays/s: TraceRay calls per microsecond.
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

S, IOR, ABBE = 16, 1.3, 30.0


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    v, i = load("monkey.obj")
    r.load_scene(v, i, procedural_env(512, 256, seed=0))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params(ior=IOR)
    L = rr.lib()
    Pt = C.c_void_p
    f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    cnt = torch.empty((H, W), dtype=torch.int32, device=dev)
    band_f32 = torch.empty((4, H, W, 4), dtype=torch.float32, device=dev)        # the emulation's per-band frames
    band_cnt = torch.empty((4, H, W), dtype=torch.int32, device=dev)
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    b16 = rr.spectral_bands(S, IOR, ABBE)
    b4 = rr.spectral_bands(4, IOR, ABBE)
    off44 = np.ascontiguousarray(np.repeat(rr.sample_pattern(4), 4, axis=0))     # sample a * 4 + b: position a, band b
    b44 = np.ascontiguousarray(np.tile(b4, 4))
    w4 = torch.cat([torch.from_numpy(b4["weight"].copy()), torch.zeros(4, 1)], dim=1).to(dev)     # [band, rgba]; alpha is set afterwards
    p4 = [rr.default_params(ior=float(b["ior"])) for b in b4]
    torch.cuda.synchronize()
    r.set_stream(torch.cuda.current_stream().cuda_stream)                       # torch's weighted sum runs between the same two events

    def samples():
        rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
        assert rc == 0, rc

    def spectral(offsets, bands):
        op = offsets.ctypes.data if offsets is not None else None
        bp = bands.ctypes.data if bands is not None else None

        def call():
            rc = L.rr_render_spectral_device(r._h, W, H, C.byref(sc), C.byref(p), op, bp, S, *outs)
            assert rc == 0, rc
        return call

    def emulation():
        for b in range(4):
            rc = L.rr_render_samples_device(r._h, W, H, C.byref(sc), C.byref(p4[b]), None, 4, Pt(band_f32[b].data_ptr()), None,
                                            Pt(band_cnt[b].data_ptr()))
            assert rc == 0, rc
        torch.sum(band_f32 * w4[:, None, None, :], dim=0, out=f32)
        f32.mul_(0.25)
        f32[..., 3] = 1.0
        torch.sum(band_cnt, dim=0, out=cnt)

    variants = [("render_samples", samples), ("spectral bands=NULL", spectral(None, None)), ("spectral 16 bands", spectral(None, b16)),
                ("spectral 4 pos x 4 bands", spectral(off44, b44)), ("4 x render_samples + torch", emulation)]
    traced, frames = {}, {}
    for name, call in variants:                                     # warm-up, and what each traces
        call()
        r.wait()
        torch.cuda.synchronize()
        traced[name] = int(cnt.sum().item())
        frames[name] = (f32.cpu().numpy().tobytes(), u8.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes())
    same = frames["render_samples"] == frames["spectral bands=NULL"]
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):                                         # taking turns: what else the machine does hits all alike
        for name, call in variants:
            r.wait()
            r.timing_begin()
            call()
            times[name].append(r.timing_end())
    base = float(np.median(times["render_samples"]))
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "scene": "monkey.obj", "samples": S,
           "ior_d": IOR, "abbe": ABBE, "uniform_bands_equal_render_samples": same, "variants": {}}
    print("%-28s %9s %19s %11s %9s %9s" % ("path", "ms", "range", "traced", "Mrays/s", "x samples"), flush=True)
    for name, _ in variants:
        t = times[name]
        ms = float(np.median(t))
        out["variants"][name] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[name], "all_ms": t}
        print("%-28s %9.3f %8.3f - %8.3f %11d %9.0f %9.3f" % (name, ms, min(t), max(t), traced[name], traced[name] / ms / 1e3, ms / base), flush=True)
    print("uniform bands equal render_samples byte for byte: %s" % same, flush=True)
    r.reset_stream()
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
