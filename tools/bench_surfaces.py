"""Opaque hit groups against the nested-media tree: python tools/bench_surfaces.py [--reps N] [--json out.json]

Two questions.  (i) What the second hit group costs when it is not used: rr_render_surfaces under an all-glass surface table with two
lights set against rr_render_nested, on the two scenes of tools/bench_nested.py -- shell.obj as one identity instance (the builds
without a top level) and sphere + cube + shell under one top level.  The two frames are compared first: they must be equal byte for
byte.  (ii) What lighting costs: a glass sphere on an opaque floor beside a small opaque cube with 0, 1 and 2 lights, with the
TraceRay totals (shadow rays included).
1920x1080, camera_orbit(0.01), the reference's bounce limits, S = 16 samples per pixel, float, RGBA8 and count outputs in device
memory, allocated before the timing; the C entry points are called directly.  Timed with HIP events on the context's stream
(rr_timing_begin / rr_timing_end), the calls taking turns, median and range of --reps after a warm-up of each (a first launch also
loads the code object).  Mrays/s: TraceRay calls per microsecond.
The library is measured as it was built.  The other form of the shadow ray (csrc/rr_render_surfaces.h) is a build with
RR_EXTRA_DEFINES=-DRR_SURFACES_ONE_SITE in the environment; render_nested is the same code in both builds and serves as the baseline of
either run.
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
LIGHTS = [rr.directional_light((-0.5, 1.0, -0.4), (1.2, 1.1, 0.9), 0x01), rr.point_light((-0.6, 1.6, 0.5), (2.0, 2.2, 2.6), 0xff)]
AMBIENT = (0.05, 0.06, 0.08)


def timed(r, calls, reps, bufs):
    """{label: C entry point} -> {label: (times, traced, frame)}: a warm-up of each, then reps rounds in which they take turns"""
    import torch
    f32, u8, cnt = bufs
    Pt = C.c_void_p
    outs = (Pt(f32.data_ptr()), Pt(u8.data_ptr()), Pt(cnt.data_ptr()))
    sc = rr.camera_orbit(0.01)
    p = rr.default_params()
    traced, frames = {}, {}
    for label, (before, f) in calls.items():
        before()
        rc = f(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
        assert rc == 0, rc
        r.wait()
        torch.cuda.synchronize()
        traced[label] = int(cnt.sum().item())
        frames[label] = (f32.cpu().numpy().copy(), u8.cpu().numpy().copy(), cnt.cpu().numpy().copy())
    times = {label: [] for label in calls}
    for _ in range(reps):                                           # taking turns: what else the machine does hits all alike
        for label, (before, f) in calls.items():
            before()                                                # (a setter: outside the timed interval)
            r.wait()
            r.timing_begin()
            rc = f(r._h, W, H, C.byref(sc), C.byref(p), None, S, *outs)
            times[label].append(r.timing_end())
            assert rc == 0, rc
    return times, traced, frames


def report(name, times, traced, base_label, extra=""):
    base = float(np.median(times[base_label]))
    out = {}
    print("%s" % name, flush=True)
    print("  %-28s %9s %19s %12s %9s %9s" % ("path", "ms", "range", "traced", "Mrays/s", "x " + base_label[:14]), flush=True)
    for label, t in times.items():
        ms = float(np.median(t))
        out[label] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[label], "all_ms": t, "ratio": ms / base}
        print("  %-28s %9.3f %8.3f - %8.3f %12d %9.0f %9.3f" % (label, ms, min(t), max(t), traced[label], traced[label] / ms / 1e3, ms / base), flush=True)
    if extra:
        print("  " + extra, flush=True)
    return out


def unused(r, name, tab, reps, bufs):
    """case (i): an all-glass table with lights set against render_nested"""
    L = rr.lib()
    r.set_materials(tab)
    r.set_surfaces([rr.glass()] * len(tab))
    r.set_lights(LIGHTS, AMBIENT)
    nothing = lambda: None  # noqa: E731
    calls = {"render_nested": (nothing, L.rr_render_nested_device), "render_surfaces, all glass": (nothing, L.rr_render_surfaces_device)}
    times, traced, frames = timed(r, calls, reps, bufs)
    a, b = frames["render_nested"], frames["render_surfaces, all glass"]
    equal = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert equal, "the all-glass frame differs from render_nested's"
    n, s = times["render_nested"], times["render_surfaces, all glass"]
    overlap = min(s) <= max(n) and min(n) <= max(s)
    out = report(name, times, traced, "render_nested", "frames equal byte for byte; the ranges %s" % ("overlap" if overlap else "do not overlap"))
    out["ranges_overlap"] = overlap
    return out


def lit(r, reps, bufs):
    """case (ii): the table scene with 0, 1 and 2 lights"""
    L = rr.lib()
    ids = []
    for name in ("cube.obj", "sphere.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])

    def xf(t, s):
        m = np.zeros((3, 4), np.float32)
        m[0, 0], m[1, 1], m[2, 2] = s
        m[:, 3] = t
        return m
    top = -0.8
    r.build_tlas(rr.make_instances(transforms=[xf((0, top - 0.1, 0), (2.5, 0.1, 2.5)), xf((0, top + 0.05 + 0.3 * 3.0 ** 0.5, 0), (0.3, 0.3, 0.3)),
                                               xf((0.9, top + 0.25, 0.8), (0.2, 0.2, 0.2))], meshes=[ids[0], ids[1], ids[0]], materials=[0, 1, 2],
                                   masks=[0x01, 0x02, 0x01]))
    r.set_materials(MIXED)
    r.set_surfaces([rr.opaque((0.7, 0.6, 0.5)), rr.glass(), rr.opaque((0.2, 0.5, 0.8), emission=(0.02, 0.0, 0.0))])
    calls = {"render_nested (all glass)": (lambda: None, L.rr_render_nested_device)}
    for n in (0, 1, 2):
        calls["render_surfaces, %d lights" % n] = ((lambda k=n: r.set_lights(LIGHTS[:k], AMBIENT)), L.rr_render_surfaces_device)
    times, traced, _ = timed(r, calls, reps, bufs)
    return report("floor + glass sphere + cube", times, traced, "render_nested (all glass)")


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
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "samples": S, "unused": {}, "lit": {}}
    r.load_scene(*load("shell.obj"), env)
    out["unused"]["shell.obj"] = unused(r, "shell.obj, one identity instance", table([(1.5, (0.8, 0.1, 0.1))]), a.reps, bufs)
    ids = []
    for name in ("sphere.obj", "cube.obj", "shell.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])
    r.build_tlas(rr.make_instances(transforms=[moved(0.0), moved(-4.0), moved(4.0)], meshes=ids, materials=[0, 1, 2]))
    out["unused"]["sphere + cube + shell"] = unused(r, "sphere + cube + shell, three disjoint instances", MIXED, a.reps, bufs)
    out["lit"] = lit(r, a.reps, bufs)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
