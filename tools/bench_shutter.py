"""Shutter frames against composed frames: python tools/bench_shutter.py [--reps N] [--json out.json]

What the scene-key indirection costs, and what a frame over distinct keys costs.  1920x1080, camera_orbit(0.01), the reference's
bounce limits, S = 16 samples per pixel through a lens (radius 0.2, focus 5), no band set; float, RGBA8 and count outputs in device
memory, allocated before the timing; the C entry points are called directly.  On the two scenes of bench_nested.py and
bench_composed.py (shell.obj alone, built with ALLOW_UPDATE; sphere + cube + shell under one top level built with ALLOW_UPDATE):
  * render_composed on the live scene, the yardstick, against render_shutter with the same samples
      - every sample in key 0, a capture of that scene,
      - the samples dealt over four keys (sample k in key k % 4) that are all captures of that scene.
    The frames are the same byte for byte (asserted), so the difference is the indirection: the record behind a scalar address,
    fetched once per sample, instead of a SceneDev in the kernel arguments.
  * then four DISTINCT keys of a refit animation -- shell.obj under the README's sine (vertex update, BLAS refit, TLAS update,
    capture, four times), the outer two of the three instances sliding inwards (TLAS update, capture, four times) -- and render_shutter with sample k in
    key k % 4, beside render_composed on the last instant alone.  The frames differ (the pixels that do are counted) and so does the
    work: the rectangle is the union's and every key has its own rays, so this ratio is a cost of the motion, not of the kernel.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import procedural_env  # noqa: E402
from bench_composed import composed_records, run_group  # noqa: E402
from bench_materials import MIXED, moved, table  # noqa: E402
from bench_query import W, H, load  # noqa: E402

S, FOCUS, RADIUS, K = 16, 5.0, 0.2, 4


def shutter_records(positions, lens_offsets, keys):
    rec = np.zeros(len(positions), rr.SHUTTER_SAMPLE_DTYPE)
    rec["offset"], rec["lens_offset"], rec["key"] = positions, lens_offsets, keys
    return rec


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
    env = procedural_env(512, 256, seed=0)
    pos, lpos = rr.sample_pattern(S), rr.lens_pattern(S)
    lens = rr.Lens(RADIUS, FOCUS)
    p = rr.default_params()
    live = composed_records(pos, lpos, 0)
    one_key = shutter_records(pos, lpos, 0)
    dealt = shutter_records(pos, lpos, np.arange(S) % K)

    def call(f, rec):
        def go():
            rc = f(r._h, W, H, C.byref(sc), C.byref(p), rec.ctypes.data, S, C.byref(lens), *outs)
            assert rc == 0, rc
        return go

    def groups(name, title, animate):
        """the live scene captured four times, then animate(j) for j = 0 .. 3, each followed by a capture"""
        for j in range(K):
            r.capture_scene_key(j)
        calls = [("render_composed", call(L.rr_render_composed_device, live)),
                 ("render_shutter, every sample in key 0", call(L.rr_render_shutter_device, one_key)),
                 ("render_shutter, 4 keys of one scene", call(L.rr_render_shutter_device, dealt))]
        out["groups"][name + ", same scene"] = run_group(r, title + ": every key the live scene", calls, a.reps, bufs, True)
        for j in range(K):
            animate(j)
            r.capture_scene_key(j)
        calls = [("render_composed, the last instant", call(L.rr_render_composed_device, live)),
                 ("render_shutter, 4 distinct keys", call(L.rr_render_shutter_device, dealt))]
        out["groups"][name + ", refit animation"] = run_group(r, title + ": four keys of a refit animation", calls, a.reps, bufs, False)
        out["groups"][name + ", refit animation"]["key_bytes"] = [int(r.scene_key_info(j).bytes) for j in range(K)]

    # shell.obj alone: no top level; the README's sine
    verts, idx = load("shell.obj")
    mid = r.upload_mesh(verts, idx)
    r.build_blas(mid, allow_update=True)
    inst = rr.make_instances(meshes=[mid])
    r.build_tlas(inst, allow_update=True)
    r.upload_envmap(env)
    r.set_materials(table([(1.5, (0.8, 0.1, 0.1))]))

    def sine(j):
        v = verts.copy()
        v["position"][:, 1] += (0.1 * np.sin(4 * v["position"][:, 0] + 1.0 * j)).astype(np.float32)
        r.update_mesh_vertices(mid, v)
        r.build_blas(mid, update=True)
        r.build_tlas(inst, update=True)
    groups("shell.obj", "shell.obj, one identity instance", sine)

    # sphere + cube + shell: the outer two slide towards the middle one (away from the camera; they stay disjoint)
    ids = []
    for name in ("sphere.obj", "cube.obj", "shell.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])

    def three(j):
        return rr.make_instances(transforms=[moved(0.0), moved(-4.0 + 0.15 * j), moved(4.0 - 0.15 * j)], meshes=ids, materials=[0, 1, 2])
    r.build_tlas(three(0), allow_update=True)
    r.set_materials(MIXED)
    groups("sphere + cube + shell", "sphere + cube + shell, three disjoint instances", lambda j: r.build_tlas(three(j), update=True))
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
