"""Lit shutter frames against their yardsticks: python tools/bench_lit.py [--reps N] [--json out.json]

What rr_render_lit costs beside the two calls it joins.  1920x1080, camera_orbit(0.01), the reference's bounce limits, S = 16 samples
per pixel, float, RGBA8 and count outputs in device memory, allocated before the timing; the C entry points are called directly.
  1. sphere + cube + shell under one top level (bench_shutter.py's scene), every sample in key 0, through a lens, an all-glass
     surface table with two lights and their shapes set: render_lit against render_shutter on the same records.  The frames are
     equal byte for byte (asserted): the cost of the unused hit group behind the key indirection.
  2. the table scene of bench_surfaces.py -- a glass sphere on an opaque floor beside a small opaque cube, two lights -- as key 0, a
     pinhole, no shapes: render_lit against render_surfaces on the live scene.  Equal byte for byte (asserted): the cost of the
     sample tables and the key record.
  3. the same scene through a lens with the lamp a square of half-edge 0.4 over the 16 offsets of rr.light_pattern: render_lit
     beside the call of 2, with the TraceRay totals.  The frames differ; this is the price of the picture, not of the kernel.
  4. four keys of the sliding three-instance scene on a lit floor (sample k in key k % 4), lens and shaped lamp as in 3, beside the
     same call with every sample in the last key.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the calls of a group taking turns, median and range
of --reps after a warm-up of each (bench_composed.run_group).  Mrays/s: TraceRay calls per microsecond.
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
from bench_composed import run_group  # noqa: E402
from bench_materials import MIXED, moved  # noqa: E402
from bench_query import W, H, load  # noqa: E402
from bench_surfaces import AMBIENT, LIGHTS  # noqa: E402

S, FOCUS, RADIUS, K = 16, 5.0, 0.2, 4
SHAPES = [rr.light_shape((0.05, 0.0, 0.0), (0.0, 0.0, 0.05)), rr.light_shape((0.4, 0.0, 0.0), (0.0, 0.0, 0.4))]


def records(dtype, positions, lens_offsets, keys, light_offsets=None):
    rec = np.zeros(len(positions), dtype)
    rec["offset"], rec["lens_offset"], rec["key"] = positions, lens_offsets, keys
    if light_offsets is not None:
        rec["light_offset"] = light_offsets
    return rec


def xf(t, s):
    m = np.zeros((3, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2] = s
    m[:, 3] = t
    return m


def overlap(group, a, b):
    va, vb = group["variants"][a], group["variants"][b]
    yes = va["min"] <= vb["max"] and vb["min"] <= va["max"]
    print("  the ranges of %s and %s %s" % (a, b, "overlap" if yes else "do not overlap"), flush=True)
    group["ranges_overlap"] = yes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "samples": S, "keys": K, "groups": {}}
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    bufs = (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
            torch.empty((H, W), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    L, Pt = rr.lib(), C.c_void_p
    outs = tuple(Pt(t.data_ptr()) for t in bufs)
    sc = rr.camera_orbit(0.01)
    pos, lpos, gpos = rr.sample_pattern(S), rr.lens_pattern(S), rr.light_pattern(S)
    lens = rr.Lens(RADIUS, FOCUS)
    p = rr.default_params()

    def frame(f, rec, with_lens):
        def go():
            rc = f(r._h, W, H, C.byref(sc), C.byref(p), rec.ctypes.data, S, C.byref(lens) if with_lens else None, *outs)
            assert rc == 0, rc
        return go

    def surfaces():
        rc = L.rr_render_surfaces_device(r._h, W, H, C.byref(sc), C.byref(p), pos.ctypes.data, S, *outs)
        assert rc == 0, rc

    r.upload_envmap(procedural_env(512, 256, seed=0))
    # 1. the unused hit group behind the key indirection
    ids = []
    for name in ("sphere.obj", "cube.obj", "shell.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])
    r.build_tlas(rr.make_instances(transforms=[moved(0.0), moved(-4.0), moved(4.0)], meshes=ids, materials=[0, 1, 2]))
    r.capture_scene_key(0)
    r.set_materials(MIXED)
    r.set_surfaces([rr.glass()] * len(MIXED))
    r.set_lights(LIGHTS, AMBIENT)
    r.set_light_shapes(SHAPES)
    shutter = records(rr.SHUTTER_SAMPLE_DTYPE, pos, lpos, 0)
    lit = records(rr.LIT_SAMPLE_DTYPE, pos, lpos, 0, gpos)
    calls = [("render_shutter", frame(L.rr_render_shutter_device, shutter, True)), ("render_lit, all glass", frame(L.rr_render_lit_device, lit, True))]
    g = out["groups"]["1 all glass"] = run_group(r, "1. sphere + cube + shell, all glass, lights set: the unused hit group", calls, a.reps, bufs, True)
    overlap(g, "render_shutter", "render_lit, all glass")

    # 2. the table scene as key 0 from a pinhole: the sample tables and the key record
    cube, sphere = ids[1], ids[0]
    top = -0.8

    def table_scene(dx=0.0):
        return rr.make_instances(transforms=[xf((0, top - 0.1, 0), (2.5, 0.1, 2.5)), xf((dx, top + 0.05 + 0.3 * 3.0 ** 0.5, 0), (0.3, 0.3, 0.3)),
                                             xf((0.9 - dx, top + 0.25, 0.8), (0.2, 0.2, 0.2))], meshes=[cube, sphere, cube], materials=[0, 1, 2],
                                 masks=[0x01, 0x02, 0x01])
    r.build_tlas(table_scene(), allow_update=True)
    r.capture_scene_key(0)
    r.set_surfaces([rr.opaque((0.7, 0.6, 0.5)), rr.glass(), rr.opaque((0.2, 0.5, 0.8), emission=(0.02, 0.0, 0.0))])
    r.set_light_shapes(None)
    pinhole = records(rr.LIT_SAMPLE_DTYPE, pos, lpos, 0, gpos)
    calls = [("render_surfaces", surfaces), ("render_lit, pinhole, no shapes", frame(L.rr_render_lit_device, pinhole, False))]
    g = out["groups"]["2 table, pinhole"] = run_group(r, "2. floor + glass sphere + cube, two lights, key 0 from a pinhole: the sample tables", calls, a.reps,
                                                      bufs, True)
    overlap(g, "render_surfaces", "render_lit, pinhole, no shapes")

    # 3. a lens and a shaped lamp over 16 offsets, beside 2
    r.set_light_shapes(SHAPES)
    calls = [("render_lit, pinhole, point lights", frame(L.rr_render_lit_device, records(rr.LIT_SAMPLE_DTYPE, pos, lpos, 0), False)),
             ("render_lit, lens, shaped lamp", frame(L.rr_render_lit_device, lit, True))]
    out["groups"]["3 table, lens and soft lamp"] = run_group(r, "3. the same scene through a lens under a lamp of half-edge 0.4", calls, a.reps, bufs, False)

    # 4. four keys: the sphere and the cube slide towards each other on the lit floor
    for j in range(K):
        r.build_tlas(table_scene(0.1 * j), update=True)
        r.capture_scene_key(j)
    dealt = records(rr.LIT_SAMPLE_DTYPE, pos, lpos, np.arange(S) % K, gpos)
    last = records(rr.LIT_SAMPLE_DTYPE, pos, lpos, K - 1, gpos)
    calls = [("render_lit, the last key alone", frame(L.rr_render_lit_device, last, True)), ("render_lit, 4 distinct keys", frame(L.rr_render_lit_device, dealt, True))]
    out["groups"]["4 four keys"] = run_group(r, "4. four keys of the sliding scene on the lit floor", calls, a.reps, bufs, False)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
