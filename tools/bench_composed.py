"""Composed frames against the frames they are composed of: python tools/bench_composed.py [--reps N] [--json out.json] [--codegen-only]

What the composition costs.  1920x1080, camera_orbit(0.01), the reference's bounce limits, S = 16 samples per pixel, float, RGBA8 and
count outputs in device memory, allocated before the timing; the C entry points are called directly.  Three yardsticks, none of
which the composed kernel touches:
  * render_nested against render_composed without a lens and without a band set, on the two scenes of bench_nested.py (shell.obj
    alone; sphere + cube + shell under one top level).  The frames are the same byte for byte (asserted), so the difference is the
    new kernel's overhead: the lens branch, the band index, the weights from memory, the table behind a computed base.
  * render_lens (radius 0.2, focus 5) on monkey.obj, the single-mesh headline view, against render_composed with that lens and a
    one-row clear table of the same index.
  * render_spectral (4 positions x 4 bands) on the same view against render_composed with the band set of those bands.
  The monkey is an open mesh, so in the last two the nested tree sees back faces the scalar tree culls: the frames differ where
  that happens, the pixels that differ are counted, and the ratio includes what unculled traversal costs (bench_nested.py has that
  alone).
Before any timing the code object is read: scratch instructions (llvm-objdump), VGPRs and private segment bytes (the kernels' notes)
of k_render_composed and k_render_nested for every launchable instantiation; --codegen-only stops there and needs no GPU.
Timed with HIP events on the context's stream (rr_timing_begin / rr_timing_end), the calls of a group taking turns, median and range
of --reps after a warm-up of each (a first launch also loads the code object).  Mrays/s: TraceRay calls per microsecond.
"""
import argparse
import ctypes as C
import json
import os
import pathlib
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refraction_raytracing_dxr_amd as rr  # noqa: E402
from refraction_raytracing_dxr_amd.synth import procedural_env  # noqa: E402
from bench_materials import MIXED, moved, table  # noqa: E402
from bench_query import W, H, load  # noqa: E402
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, OBJDUMP, kernels, template_args  # noqa: E402

S, IOR, ABBE, FOCUS, RADIUS = 16, 1.3, 30.0, 5.0, 0.2


def codegen():
    """{instantiation: {kernel: {"scratch", "vgprs", "private_bytes"}}} for k_render_composed and k_render_nested"""
    if not HAVE_OBJDUMP:
        print("llvm-objdump of the ROCm toolchain not found: no code-object figures", flush=True)
        return {}
    tools = os.path.dirname(OBJDUMP)
    out = {}
    with tempfile.TemporaryDirectory(prefix="bench_composed") as d:
        k = kernels(pathlib.Path(d))
        notes = {}
        for f in sorted((pathlib.Path(d) / "co").iterdir()):
            if "gfx950" not in f.name:
                continue
            text = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", str(f)], check=True, capture_output=True, text=True).stdout
            for block in text.split("- .agpr_count:")[1:]:          # one block per kernel of amdhsa.kernels
                name = re.search(r"\.name:\s+(\S+)", block)
                vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
                priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
                if name and vgpr and priv:
                    notes[name.group(1)] = (int(vgpr.group(1)), int(priv.group(1)))
        print("%-46s %28s %28s" % ("instantiation", "k_render_composed", "k_render_nested"), flush=True)
        print("%-46s %28s %28s" % ("", "scratch ins / VGPRs / bytes", "scratch ins / VGPRs / bytes"), flush=True)
        for variant in LAUNCHABLE:
            args = template_args(*variant)
            # the notes name kernels as the linker does: <39, 2, true, unsigned short> is ILi39ELi2ELb1EtE
            mangled = "ILi%dELi%dELb%dE%sE" % (variant[0], variant[1], variant[2], "t" if variant[3] == "unsigned short" else "j")
            row = {}
            for kern in ("k_render_composed", "k_render_nested"):
                sym = [n for n in k if kern + args in n]
                meta = [v for n, v in notes.items() if kern + mangled in n]
                assert len(sym) == 1 and len(meta) == 1, (kern, args, sym)
                row[kern] = {"scratch": k[sym[0]]["scratch"], "vgprs": meta[0][0], "private_bytes": meta[0][1]}
            out[args] = row
            print("%-46s %28s %28s" % (args, *["%d / %d / %d" % (row[n]["scratch"], row[n]["vgprs"], row[n]["private_bytes"]) for n in row]), flush=True)
    return out


def composed_records(positions, lens_offsets, bands):
    rec = np.zeros(len(positions), rr.COMPOSED_SAMPLE_DTYPE)
    rec["offset"] = positions
    if lens_offsets is not None:
        rec["lens_offset"] = lens_offsets
    rec["band"] = bands
    return rec


def run_group(r, title, calls, reps, bufs, must_equal):
    """calls: [(label, callable)], the first being the yardstick.  Warm-up, the frames compared, then the calls taking turns"""
    import torch
    f32, u8, cnt = bufs
    traced, frames = {}, {}
    for label, f in calls:                                          # warm-up, and what each traces
        f()
        r.wait()
        torch.cuda.synchronize()
        traced[label] = int(cnt.sum().item())
        frames[label] = (f32.cpu().numpy().copy(), u8.cpu().numpy().copy(), cnt.cpu().numpy().copy())
    base_label = calls[0][0]
    a = frames[base_label]
    diffs = {}
    for label, _ in calls[1:]:
        b = frames[label]
        diffs[label] = (int((a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=-1).sum()), int((a[2] != b[2]).sum()))
        if must_equal:
            assert diffs[label] == (0, 0) and a[1].tobytes() == b[1].tobytes(), "%s differs from %s: %s" % (label, base_label, diffs[label])
    times = {label: [] for label, _ in calls}
    for _ in range(reps):                                           # taking turns: what else the machine does hits all alike
        for label, f in calls:
            r.wait()
            r.timing_begin()
            f()
            times[label].append(r.timing_end())
    base = float(np.median(times[base_label]))
    out = {"variants": {}, "pixels_differing": {k: {"colour": v[0], "count": v[1]} for k, v in diffs.items()}}
    print(title, flush=True)
    print("  %-34s %9s %19s %11s %9s %11s" % ("path", "ms", "range", "traced", "Mrays/s", "x yardstick"), flush=True)
    for label, _ in calls:
        t = times[label]
        ms = float(np.median(t))
        out["variants"][label] = {"ms": ms, "min": min(t), "max": max(t), "traced": traced[label], "all_ms": t}
        print("  %-34s %9.3f %8.3f - %8.3f %11d %9.0f %11.3f" % (label, ms, min(t), max(t), traced[label], traced[label] / ms / 1e3, ms / base), flush=True)
    for label, (dc, dn) in diffs.items():
        print("  %s: of %d pixels, %d differ from %s in colour and %d in their TraceRay count" % (label, W * H, dc, base_label, dn), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    ap.add_argument("--codegen-only", action="store_true")
    a = ap.parse_args()
    out = {"unit": "ms (median and range of %d reps, HIP events), Mrays/s" % a.reps, "frame": [W, H], "samples": S, "codegen": codegen(), "groups": {}}
    if a.codegen_only:
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return 0
    import torch
    r = rr.Renderer(0)
    dev = "cuda:%d" % r.device
    bufs = (torch.empty((H, W, 4), dtype=torch.float32, device=dev), torch.empty((H, W, 4), dtype=torch.uint8, device=dev),
            torch.empty((H, W), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    L, Pt = rr.lib(), C.c_void_p
    outs = tuple(Pt(t.data_ptr()) for t in bufs)
    sc = rr.camera_orbit(0.01)
    env = procedural_env(512, 256, seed=0)
    pos16 = rr.sample_pattern(S)

    def call(f, *args):
        def go():
            rc = f(r._h, W, H, C.byref(sc), *args, *outs)
            assert rc == 0, rc
        return go

    # 1. the new kernel's overhead: render_nested against the degenerate composed frame
    p = rr.default_params()
    plain = composed_records(pos16, None, 0)
    degenerate = [("render_nested", call(L.rr_render_nested_device, C.byref(p), None, S)),
                  ("render_composed, no lens, no bands", call(L.rr_render_composed_device, C.byref(p), plain.ctypes.data, S, None))]
    r.load_scene(*load("shell.obj"), env)
    r.set_materials(table([(1.5, (0.8, 0.1, 0.1))]))
    out["groups"]["shell.obj"] = run_group(r, "shell.obj, one identity instance", degenerate, a.reps, bufs, True)
    ids = []
    for name in ("sphere.obj", "cube.obj", "shell.obj"):
        ids.append(r.upload_mesh(*load(name)))
        r.build_blas(ids[-1])
    r.build_tlas(rr.make_instances(transforms=[moved(0.0), moved(-4.0), moved(4.0)], meshes=ids, materials=[0, 1, 2]))
    r.set_materials(MIXED)
    out["groups"]["sphere + cube + shell"] = run_group(r, "sphere + cube + shell, three disjoint instances", degenerate, a.reps, bufs, True)

    # 2. and 3. the lens and spectral frames of the single-mesh headline view against their composed equivalents
    r.load_scene(*load("monkey.obj"), env)
    pi = rr.default_params(ior=IOR)
    r.set_materials(table([(IOR, (0.0, 0.0, 0.0))]))
    lens = rr.Lens(RADIUS, FOCUS)
    with_lens = composed_records(pos16, rr.lens_pattern(S), 0)
    out["groups"]["lens"] = run_group(r, "monkey.obj through a lens of radius %g focused at %g" % (RADIUS, FOCUS),
                                      [("render_lens", call(L.rr_render_lens_device, C.byref(pi), None, None, S, C.byref(lens))),
                                       ("render_composed, lens", call(L.rr_render_composed_device, C.byref(pi), with_lens.ctypes.data, S, C.byref(lens)))],
                                      a.reps, bufs, False)
    b4 = rr.spectral_bands(4, IOR, ABBE)
    off44 = np.ascontiguousarray(np.repeat(rr.sample_pattern(4), 4, axis=0))     # sample a * 4 + b: position a, band b
    b44 = np.ascontiguousarray(np.tile(b4, 4))
    in_bands = composed_records(off44, None, np.tile(np.arange(4), 4))
    r.set_material_bands(*rr.material_bands(table([(IOR, (0.0, 0.0, 0.0))]), ABBE, 4))
    out["groups"]["spectral"] = run_group(r, "monkey.obj, 4 positions x 4 bands of Abbe number %g" % ABBE,
                                          [("render_spectral", call(L.rr_render_spectral_device, C.byref(pi), off44.ctypes.data, b44.ctypes.data, S)),
                                           ("render_composed, 4 bands", call(L.rr_render_composed_device, C.byref(pi), in_bands.ctypes.data, S, None))],
                                          a.reps, bufs, False)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
