"""What the shutter-frame tests share (test_shutter_cpu.py, test_gpu_shutter.py): the moving tumbler -- three instants of the nested
tumbler of nested_helpers.py, one Scene per scene key --, the sample records of the fixtures, and the contract of rr_render_shutter
on the CPU: sample k is nested_helpers.ref_shade of composed_helpers.sample_rays in the Scene of key_k under T_band_k, resolved by
spectral_helpers.weighted_fold.  A key on the CPU side is just a Scene.  Each reference is computed once per process."""
import ctypes as C

import numpy as np

import composed_helpers as CH
import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from composed_helpers import LENS
from nested_helpers import FH, FW, MESHES, OFF3, TABLE
from scenes import Scene, load, xf
from shading_helpers import env_map
from spectral_helpers import weighted_fold

KEY_ORDER = [2, 0, 1, 1, 0, 2]                              # the key of each of the six samples, deliberately not 0, 1, 2, 0, 1, 2
BAND_ORDER = CH.BAND_ORDER                                  # [1, 0, 0, 1, 1, 0]
KW = CH.KW
N_KEYS = 3
# Key 2: the outer cube, and with it the scene's box, moves by SHIFT -- across the screen of VIEW, and far enough that pixels hit it in
# 8x8 blocks outside key 0's own screen rectangle (the rectangles are those of the boxes seen from the whole lens disk, plus a margin of
# 8 pixels: a small step stays inside it), while a column of blocks stays outside the union's.  nested_helpers.VIEW's angle with a
# wider field of view: at its 0.9 the rectangles cover the frame.  test_shutter_cpu.py asserts all of it.
SHIFT = (2.0, 0.0, -2.0)
VIEW = (NH.VIEW[0], 1.5)

_scenes = {}


def moving_tumbler(j):
    """instant j of 0, 1, 2: the tumbler with the inner cube turning (rot 0.4, 1.0, 1.6) and drifting, the sphere shifting by 0.03 per
    key (towards the cube's middle: it fills the cube to within 0.13), and in key 2 the outer cube translated by SHIFT with what
    it holds.  The three stay nested in every key"""
    key = "moving-tumbler-%d" % j
    if key not in _scenes:
        sx, sy, sz = SHIFT if j == 2 else (0.0, 0.0, 0.0)
        inst = rr.make_instances(transforms=[xf(sx, sy, sz), xf(sx + 0.05 - 0.03 * j, sy - 0.03, sz + 0.04, (0.5, 0.5, 0.5)),
                                             xf(sx + 0.1 + 0.02 * j, sy + 0.05 - 0.01 * j, sz - 0.02, (0.3, 0.3, 0.3), 0.4 + 0.6 * j)],
                                 meshes=[0, 1, 0], materials=[1, 2, 3])
        _scenes[key] = Scene(key, [load(m) for m in MESHES], env_map(), inst)
    sc = _scenes[key]
    NH.assert_inside(sc, 1, 0)
    NH.assert_inside(sc, 2, 1)
    return sc


def moving_keys():
    return [moving_tumbler(j) for j in range(N_KEYS)]


def union_bounds(scenes):
    """(lo xyz, hi xyz) of the boxes of several Scenes, as ctypes floats"""
    b = np.array([list(s.bounds) for s in scenes], np.float32)
    return (C.c_float * 6)(*[float(v) for v in b[:, :3].min(axis=0)], *[float(v) for v in b[:, 3:].max(axis=0)])


def records(positions, lens_offsets, bands, keys):
    """SHUTTER_SAMPLE_DTYPE [S]: sample k has positions[k], lens_offsets[k] (None: zeros), bands[k] and keys[k]"""
    rec = np.zeros(len(positions), rr.SHUTTER_SAMPLE_DTYPE)
    rec["offset"] = np.asarray(positions, np.float32)
    if lens_offsets is not None:
        rec["lens_offset"] = np.asarray(lens_offsets, np.float32)
    rec["band"] = bands
    rec["key"] = keys
    return rec


def fixture_records():
    """the six samples of the moving tumbler: position k // 2 of OFF3, key KEY_ORDER[k], band BAND_ORDER[k], lens point k of
    lens_pattern(6)"""
    return records(np.repeat(OFF3, 2, axis=0), rr.lens_pattern(6), BAND_ORDER, KEY_ORDER)


def fold_keys(shade, camera, w, h, recs, lens, table, iors, weights, **kw):
    """composed_helpers.fold_samples with the key: shade(key, rays, T_band) -> (rgb [n, 3], counts [n], extra) gives c_k ->
    (rgb [h, w, 3], counts [h, w], the unweighted colours [S, h, w, 3], the extras)"""
    p = rr.default_params(**kw)
    iors = np.asarray(table["ior"], np.float32)[None, :] if iors is None else iors
    weights = np.ones((len(iors), 3), np.float32) if weights is None else np.asarray(weights, np.float32)
    cols, total, extras = [], np.zeros(w * h, np.uint32), []
    for rec in recs:
        rgb, cnt, extra = shade(int(rec["key"]), CH.sample_rays(camera, w, h, rec, lens, p), CH.band_table(table, iors, int(rec["band"])))
        cols.append(np.ascontiguousarray(rgb, np.float32).reshape(h, w, 3))
        total += cnt
        extras.append(extra)
    return weighted_fold(cols, [weights[int(r["band"])] for r in recs]), total.reshape(h, w), np.stack(cols), extras


def ref_shutter(scenes, camera, w, h, recs, lens, table, iors=None, weights=None, **kw):
    """rr_render_shutter's contract on the CPU: scenes[key] is the Scene of a key; the extras are the nested reference's tallies"""
    def shade(key, rays, t):
        rgb, _, cnt, tl = NH.ref_shade(scenes[key], rays, t, **kw)
        return rgb, cnt, tl
    return fold_keys(shade, camera, w, h, recs, lens, table, iors, weights, **kw)


_refs = {}


def moving_ref(max_reflect):
    """(scenes, camera, records, iors, weights, ref_shutter's result) of the moving tumbler at FW x FH through LENS"""
    if max_reflect not in _refs:
        scs = moving_keys()
        cam = MH.view(*VIEW, FW, FH)
        iors, weights = CH.fixture_bands()
        recs = fixture_records()
        _refs[max_reflect] = (scs, cam, recs, iors, weights, ref_shutter(scs, cam, FW, FH, recs, LENS, TABLE, iors, weights, max_reflect=max_reflect, **KW))
    return _refs[max_reflect]


def blocks_inside(rect, w=FW, h=FH):
    """bool [h, w]: the pixel's 8x8 block touches the rectangle (x0, y0, x1, y1), the kernels' own test"""
    x0, y0 = (np.arange(w) // 8) * 8, (np.arange(h) // 8) * 8
    return ((y0 + 8 > rect[1]) & (y0 < rect[3]))[:, None] & ((x0 + 8 > rect[0]) & (x0 < rect[2]))[None, :]


def capture_keys(gpu, scenes):
    """loads every Scene live in turn and captures it as the key of its index"""
    for j, sc in enumerate(scenes):
        sc.load_gpu(gpu)
        gpu.capture_scene_key(j)


def sine(verts, t):
    """the README's deformation of a mesh at step t"""
    v = verts.copy()
    v["position"][:, 1] += (0.1 * np.sin(4 * v["position"][:, 0] + 0.1 * t)).astype(np.float32)
    return v
