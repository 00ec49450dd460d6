"""GPU: what the caller-ray entry points refuse, in which order and in which words (rr_shade_rays*, rr_render_* and their _device
variants: 28 entry points of two families).

Each entry point walks a ladder: the first call is wrong in every respect the entry point checks, (status, rr_last_error) is
recorded, exactly the thing that text names is repaired, and so on until the call succeeds.  The list of texts is the entry point's
whole refusal order, so a reordering, a reworded text or a changed status shows as a different list.  The transcript is compared
with tests/golden/refusal_texts.json, which `python tests/test_gpu_refusal_texts.py <file>` writes.  Every recorded call is refused
on the host before any launch, or succeeds: 8 x 8 frames, 4 rays, one Renderer.

The rays family has a second ladder per entry point, "<name> [n = 0]": with no rays the call succeeds once the scene's state is in
order, which pins where that return stands among the refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from nested_helpers import TABLE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusal_texts.json")
W = H = 8
N_RAYS = 4
RAYS = ("rr_shade_rays", "rr_shade_rays_materials", "rr_shade_rays_nested", "rr_shade_rays_surfaces")
FRAMES = ("rr_render_samples", "rr_render_adaptive", "rr_render_lens", "rr_render_spectral", "rr_render_materials", "rr_render_nested",
          "rr_render_surfaces", "rr_render_composed", "rr_render_shutter", "rr_render_lit")
NAMES = tuple(n + d for n in RAYS + FRAMES for d in ("", "_device"))
BIG = np.tile(TABLE, 51)[:301]                              # a table long enough for row 300
BAD_ROW = 300                                               # above the short table's length and above NESTED_MAX_MATERIAL
KEY_BAD, KEY_FLAT, KEY_EMPTY = 3, 2, 5                      # keys 0 and 1: the tumbler; 3: with BAD_ROW; 2: no top level; 5: never captured


class Args:
    """the arguments of one ladder's call, which the repairs change in place"""


def record():
    """-> { entry point or "<entry point> [n = 0]": [[status, text], ...] }, the last rung being [0, ""]"""
    import torch
    L = rr.lib()
    r = rr.Renderer(0)
    try:
        return _record(L, r, torch)
    finally:
        r.close()


def _record(L, r, torch):
    h = r._h
    tumbler, flat = NH.tumbler(), NH.alone("cube.obj", 1)
    ids = [r.upload_mesh(v, i) for v, i in tumbler.meshes]
    flat_id = r.upload_mesh(*flat.meshes[0])
    for m in ids + [flat_id]:
        r.build_blas(m)
    r.upload_envmap(tumbler.env)
    good = tumbler.instances.copy()
    good["blas"] = [ids[int(b)] for b in good["blas"]]
    bad = good.copy()
    bad["hitgroup_flags"][2] = BAD_ROW
    flat_inst = flat.instances.copy()
    flat_inst["blas"] = flat_id
    for inst, keys in ((bad, (KEY_BAD,)), (good, (0, 1)), (flat_inst, (KEY_FLAT,))):
        r.build_tlas(inst)
        for k in keys:
            r.capture_scene_key(k)
    cam = rr.camera_orbit(0.6)
    rays = rr.camera_rays(cam, 2, 2)
    assert len(rays) == N_RAYS

    # the memory the calls write to and read from: host arrays, and device tensors with room for a pointer moved off its alignment
    host = dict(f32=np.zeros((W * H, 4), np.float32), rgba8=np.zeros((W * H, 4), np.uint8), n=np.zeros(W * H, np.uint32),
                taken=np.zeros(W * H, np.uint32))
    dev = dict(f32=torch.zeros((W * H + 1, 4), dtype=torch.float32, device="cuda:0"), rgba8=torch.zeros(W * H + 4, dtype=torch.int32, device="cuda:0"),
               n=torch.zeros(W * H + 4, dtype=torch.int32, device="cuda:0"), taken=torch.zeros(W * H + 4, dtype=torch.int32, device="cuda:0"),
               rays=torch.from_numpy(np.concatenate([rays, rays[:1]]).view(np.int32).reshape(-1, 12)).to("cuda:0"))
    ws_bytes = int(L.rr_host_adaptive_workspace_bytes(W, H))
    dev["ws"] = torch.zeros(ws_bytes // 4 + 8, dtype=torch.int32, device="cuda:0")
    n_refined = C.c_uint64(0)

    def ptr(device, what):
        return dev[what].data_ptr() if device else host[what].ctypes.data

    sun = rr.directional_light((0.0, 0.0, 1.0), (1.0, 1.0, 1.0))
    lights, shapes = np.zeros(2, rr.LIGHT_DTYPE), np.zeros(2, rr.LIGHT_SHAPE_DTYPE)
    lights[0], lights[1] = rr.point_light((0.0, 3.0, 0.0), (2.0, 2.0, 2.0)), sun
    # under the light offset (1, 1): the point light goes to infinity, the sun's direction to zero
    shapes[0], shapes[1] = rr.light_shape((3.0e38, 0, 0), (3.0e38, 0, 0)), rr.light_shape(-sun["v"], (0, 0, 0))

    def reset():
        """nothing built, no table, no band set; the lights and the shapes that the lit ladder trips over"""
        r.build_blas(ids[0])
        r.set_materials(None)
        r.set_surfaces(None)
        r.set_lights(lights)
        r.set_light_shapes(shapes)
        shapes_now[:] = shapes

    shapes_now = shapes.copy()

    def shape(i, ex, ey):
        shapes_now["ex"][i], shapes_now["ey"][i] = ex, ey
        r.set_light_shapes(shapes_now)

    def fresh_args(device, kind):
        a = Args()
        a.device, a.kind = device, kind
        a.rays, a.n = None, N_RAYS
        a.w, a.h, a.cam = 0, H, None
        a.params = rr.default_params(max_refract=-1, max_reflect=9, ior=0.0)
        a.f32 = a.rgba8 = a.n_rays = a.taken = None
        a.offsets, a.n_samples = None, 3
        a.off = np.array([[0.5, 0.5], [0.25, 1.01], [np.nan, 0.75]], np.float32)
        a.n_base, a.threshold = 5, float("nan")
        a.ws, a.ws_bytes = None, ws_bytes
        a.lens, a.loff = None, np.array([[0.0, 0.0], [-1.01, 0.0], [0.5, 0.5]], np.float32)
        a.bands = np.array([(1.3, (1, 1, 1)), (0.0, (1, 1, 1)), (1.4, (1, np.inf, 1))], rr.BAND_DTYPE)
        if kind in ("composed", "shutter", "lit"):
            a.samples, a.n_samples = None, 0
            a.rec = np.zeros(3, {"composed": rr.COMPOSED_SAMPLE_DTYPE, "shutter": rr.SHUTTER_SAMPLE_DTYPE, "lit": rr.LIT_SAMPLE_DTYPE}[kind])
            a.rec["offset"], a.rec["lens_offset"], a.rec["band"] = a.off, a.loff, (0, 1, 0)
            a.lens = rr.Lens(-1.0, 2.0)
            if kind != "composed":
                a.rec["key"] = rr.MAX_SCENE_KEYS
            if kind == "shutter":
                a.rec["pad"][1] = (0, 1)
            if kind == "lit":
                a.rec["light_offset"][0] = (1.01, 0.0)
        return a

    def outputs(a):
        return [C.c_void_p(p) for p in (a.f32, a.rgba8, a.n_rays)]

    def call(name, a):
        fn = getattr(L, name)
        pp = C.byref(a.params)
        if a.kind == "rays":
            return fn(h, C.c_void_p(a.rays), a.n, pp, *outputs(a))
        head = (h, a.w, a.h, C.byref(a.cam) if a.cam is not None else None, pp)
        offp = a.off.ctypes.data if a.offsets else None
        lens = C.byref(a.lens) if a.lens is not None else None
        if a.kind == "adaptive":
            tail = (C.c_void_p(a.taken), C.c_void_p(a.ws), a.ws_bytes) if a.device else (C.c_void_p(a.taken), C.byref(n_refined))
            return fn(*head, offp, a.n_base, a.n_samples, a.threshold, *outputs(a), *tail)
        if a.kind == "lens":
            return fn(*head, offp, a.loff.ctypes.data, a.n_samples, lens, *outputs(a))
        if a.kind == "spectral":
            return fn(*head, offp, a.bands.ctypes.data, a.n_samples, *outputs(a))
        if a.kind in ("composed", "shutter", "lit"):
            return fn(*head, a.rec.ctypes.data if a.samples else None, a.n_samples, lens, *outputs(a))
        return fn(*head, offp, a.n_samples, *outputs(a))

    # ---- the repairs: what a text names -> what mends it, one entry per time the text may come
    def set_(**kw):
        return lambda a: [setattr(a, k, v) for k, v in kw.items()]

    def colour(a):
        # the host variants get their arrays; the device variants get every pointer off its alignment first
        off4, off1 = (4, 1) if a.device else (0, 0)
        a.f32, a.rgba8, a.n_rays = ptr(a.device, "f32") + off4, ptr(a.device, "rgba8") + off1, ptr(a.device, "n") + off1
        if a.kind == "adaptive":
            a.taken = ptr(a.device, "taken") + off1

    def aligned(what, field):
        return lambda a: setattr(a, field, ptr(True, what))

    def rec(field, k, value):
        def fix(a):
            a.rec[field][k] = value
        return fix

    def off(k, value):
        def fix(a):
            a.off[k] = value
            if hasattr(a, "rec"):
                a.rec["offset"][k] = value
        return fix

    def loff(a):
        a.loff[1] = (-1.0, 0.0)
        if hasattr(a, "rec"):
            a.rec["lens_offset"][1] = (-1.0, 0.0)

    def keys(*ks):
        def fix(a):
            a.rec["key"] = ks
        return fix

    def band(k, field, value):
        def fix(a):
            a.bands[field][k] = value
        return fix

    out_align = [aligned("f32", "f32"), aligned("rgba8", "rgba8"), aligned("n", "n_rays"), aligned("taken", "taken")]
    need_n = [set_(n_samples=65), set_(n_samples=3)]
    repairs = {
        "build the BLAS and TLAS first": [lambda a: r.build_tlas(bad)],
        "set a material table first (rr_set_materials)": [lambda a: r.set_materials(TABLE)],
        "an instance's hit-group index is not below the material table's length": [lambda a: r.set_materials(BIG)],
        "an instance's hit-group index is above RR_NESTED_MAX_MATERIAL (254)": [lambda a: r.build_tlas(good)],
        "need rgba32f or rgba8": [colour],
        "need d_rgba32f or d_rgba8": [colour],
        "null rays": [lambda a: setattr(a, "rays", rays.ctypes.data)],
        "need 16-byte aligned ray and float pointers and 4-byte aligned rgba8 and count pointers":
            [lambda a: setattr(a, "rays", ptr(True, "rays") + 8), aligned("rays", "rays")] + out_align[:3],
        "need a 16-byte aligned float pointer and 4-byte aligned rgba8 and count pointers": out_align,
        "negative bounce limit": [lambda a: setattr(a.params, "max_refract", 3)],
        "max_reflect > 8 (parked-ray registers)": [lambda a: setattr(a.params, "max_reflect", 1)],
        "ior must be > 0": [lambda a: setattr(a.params, "ior", 1.3)],
        "null constants": [set_(cam=cam)],
        "width and height must be 1..32768": [set_(w=W)],
        "the built-in patterns have 1, 2, 4, 8 or 16 samples": [set_(offsets=True, n_samples=0)],
        "need 1 <= n_samples <= 64": need_n,
        "offsets must lie in [0, 1]": [off(1, (0.25, 1.0)), off(2, (0.0, 0.75))],
        "need 1 <= n_base <= n_max": [set_(n_base=2)],
        "threshold must be finite and >= 0": [set_(threshold=0.05)],
        "need a 16-byte aligned workspace of at least rr_host_adaptive_workspace_bytes(width, height) bytes":
            [lambda a: setattr(a, "ws", ptr(True, "ws") + 4), lambda a: [setattr(a, "ws", ptr(True, "ws")), setattr(a, "ws_bytes", ws_bytes - 1)],
             set_(ws_bytes=ws_bytes)],
        "null lens": [set_(lens=rr.Lens(-1.0, 2.0))],
        "need a finite radius >= 0, a finite focus_distance > 0 and proj_inv columns of finite non-zero length": [set_(lens=rr.Lens(0.05, 2.0))],
        "lens offsets must lie in [-1, 1]": [loff],
        "every band's ior must be finite and > 0": [band(1, "ior", 1.35)],
        "every band's weights must be finite": [band(2, "weight", (1, 0.5, 1))],
        # (rr_render_lit says this of a sample count out of range too: it hands rr_render_shutter's check no records then)
        "null samples": [set_(samples=True)] + need_n,
        "a sample's band is not below the number of bands in force (1 without rr_set_material_bands)": [rec("band", 1, 0)],
        "a sample's pad must be zero": [rec("pad", 1, (0, 0))],
        "a sample's key is not a captured scene key (rr_capture_scene_key)": [keys(KEY_EMPTY, KEY_EMPTY, KEY_EMPTY), keys(KEY_BAD, KEY_FLAT, KEY_BAD)],
        "a key's hit-group index is not below the material table's length": [lambda a: r.set_materials(BIG)],
        "a key's hit-group index is above RR_NESTED_MAX_MATERIAL (254)": [keys(0, KEY_FLAT, 0)],
        "the keys of one frame must all have a top level or all be without one": [keys(0, 1, 0)],
        "light offsets must lie in [-1, 1]": [rec("light_offset", 0, (1.0, 1.0))],
        "a light moved by a sample's offset has a position or direction that is not finite": [lambda a: shape(0, (0.2, 0, 0), (0, 0, 0.2))],
        "a directional light moved by a sample's offset has the direction zero": [lambda a: shape(1, (0.1, 0, 0), (0, 0.1, 0))],
    }

    def ladder(name, a):
        reset()
        rungs, seen = [], {}
        while len(rungs) < 64:
            status = call(name, a)
            rungs.append([status, L.rr_last_error(h).decode() if status else ""])
            if status == 0:
                r.wait()
                return rungs
            what = rungs[-1][1].split(": ", 1)[1]
            k = seen[what] = seen.get(what, -1) + 1
            assert what in repairs and k < len(repairs[what]), "%s, rung %d: no repair for %r" % (name, len(rungs), rungs[-1])
            repairs[what][k](a)
        raise AssertionError("%s: the ladder does not end: %r" % (name, rungs[-3:]))

    out = {}
    for name in NAMES:
        device = name.endswith("_device")
        base = name[:-len("_device")] if device else name
        kind = "rays" if base in RAYS else base[len("rr_render_"):]
        out[name] = ladder(name, fresh_args(device, kind))
        if kind == "rays":
            a = fresh_args(device, kind)
            a.n = 0
            out[name + " [n = 0]"] = ladder(name, a)
    return out


def test_every_refusal_keeps_its_status_text_and_place():
    got = record()
    for name, rungs in got.items():
        for status, text in rungs:
            print("%-40s %d %s" % (name, status, text))
        assert rungs[-1] == [0, ""], name
    for name in NAMES:
        assert name in got and len(got[name]) >= 3, (name, got.get(name))
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], name


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")
