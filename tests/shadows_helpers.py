"""The reference of the ray tree with transparent shadows (test_shadows_cpu.py, test_gpu_shadows.py, test_gpu_shadows_tree_matrix.py):
tests/native/shadows_ref.c, compiled when first asked for with the C compiler and the floating-point flags the oracle is built with,
and loaded with ctypes beside oracle/librr_oracle.so, whose rro_trace and rro_env_lookup it calls -- as surfaces_helpers.py loads
surfaces_ref.c.  rro_trace has no instance mask: for every distinct shadow_mask the helper builds one more oracle scene of the
instances whose InstanceMask meets it.  That scene numbers its instances anew, and a walk needs the row, the winding flag and the
object space of what it hits, so the helper hands the reference the map back to the whole scene's numbering, per light.  The lit
frames' per-sample moved lights go through the same reference: ref_lit is lit_helpers.ref_lit with a cap."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import lit_helpers as LH
import nested_helpers as NH
import oracle as O
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as KH
import surfaces_helpers as SH
from materials_helpers import _Mesh, scene_instances
from nested_helpers import TABLE
from scenes import Scene, load, oracle_instances, oracle_scene, xf
from shading_helpers import fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "shadows_ref.c")
MAX_STEPS = 16


class Tallies(C.Structure):
    """surfaces_helpers.Tallies and the walks'"""
    _fields_ = SH.Tallies._fields_ + [("walks", C.c_uint64), ("walk_calls", C.c_uint64 * (MAX_STEPS + 1)), ("walk_start_media", C.c_uint64 * 5),
                                      ("walk_capped", C.c_uint64), ("walk_ended_by_fs", C.c_uint64), ("walk_lit_glass", C.c_uint64 * 3),
                                      ("walk_occluded_after_glass", C.c_uint64), ("walk_absorbed", C.c_uint64)]

    def __repr__(self):
        return ("opaque hits %d, TraceRay calls of shadow rays %d = %d occluded + %d lit walks or rays (per light %s, occluded %s), lights skipped %d; "
                "walks %d, by calls %s, by the list they start with %s, capped %d, ended by fs %d, lit through 0 / 1 / >= 2 glass hits %s, "
                "occluded after glass %d, glass hits that absorbed %d") % (
            self.opaque_hits, self.shadow_traced, self.shadow_occluded, self.shadow_lit, list(self.light_used), list(self.light_occluded),
            self.lights_skipped, self.walks, list(self.walk_calls), list(self.walk_start_media), self.walk_capped, self.walk_ended_by_fs,
            list(self.walk_lit_glass), self.walk_occluded_after_glass, self.walk_absorbed)


_lib = None
_dir = None


def lib():
    """shadows_ref.c as a shared object in a temporary directory of this process"""
    global _lib, _dir
    if _lib is None:
        O.lib()                                                 # builds oracle/librr_oracle.so if it is missing
        _dir = tempfile.TemporaryDirectory(prefix="shadows_ref")
        so = os.path.join(_dir.name, "libshadows_ref.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.run([cc, "-O2", "-g0", "-std=gnu11", "-fPIC", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                        "-shared", "-o", so, SRC, "-L" + O.ORACLE_DIR, "-l:librr_oracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-lm"], check=True)
        L = C.CDLL(so)
        L.shref_shade.restype = C.c_int
        L.shref_shade.argtypes = [C.c_void_p, C.POINTER(_Mesh), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(O.Params), C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Tallies)]
        _lib = L
    return _lib


_shadow = {}


def shadow_scene(sc, mask):
    """(the oracle scene a shadow ray of shadow_mask `mask` is traced in, the index in sc of each of its instances as uint32 or None
    where the numbering is sc's own): sc's own scene where every instance meets the mask, (None, None) where none does"""
    key = (sc.key, int(mask))
    if key not in _shadow:
        inst = scene_instances(sc)
        keep = ((inst["instance_id_mask"] >> 24) & int(mask)) != 0
        if keep.all():
            _shadow[key] = (sc.oracle(), None)
        elif not keep.any():
            _shadow[key] = (None, None)
        else:
            _shadow[key] = (oracle_scene(sc.meshes, None, inst[keep]), np.ascontiguousarray(np.flatnonzero(keep), np.uint32))
    return _shadow[key]


def ref_shade(sc, rays, table, surf=None, lts=None, ambient=None, k=0, use_bvh=0, **kw):
    """surfaces_helpers.ref_shade under shadow_steps k -> (rgb float32 [n, 3], rgba8 uint8 [n, 4], TraceRay calls uint32 [n], Tallies)"""
    L = lib()
    table = np.ascontiguousarray(table, rr.MATERIAL_DTYPE)
    surf = SH.surfaces() if surf is None else np.ascontiguousarray(surf, rr.SURFACE_DTYPE).reshape(-1)
    lts = SH.lights() if lts is None else np.ascontiguousarray(lts, rr.LIGHT_DTYPE).reshape(-1)
    amb = np.zeros(3, np.float32) if ambient is None else np.ascontiguousarray(ambient, np.float32).reshape(3)
    inst = np.ascontiguousarray(oracle_instances(scene_instances(sc)))
    keep = [(np.ascontiguousarray(v), np.ascontiguousarray(i, np.uint32)) for v, i in sc.meshes]
    meshes = (_Mesh * len(keep))(*[_Mesh(v.ctypes.data, i.ctypes.data) for v, i in keep])
    held = [shadow_scene(sc, m) for m in lts["shadow_mask"]]
    shadow = (C.c_void_p * max(1, len(lts)))(*[None if s is None else s.h for s, _ in held])
    maps = (C.c_void_p * max(1, len(lts)))(*[None if m is None else m.ctypes.data for _, m in held])
    n = len(rays)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7], r8[:, 7] = rays["origin"], rays["tmin"], rays["dir"], rays["tmax"]
    rgb, u8, cnt = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint32)
    tl = Tallies()
    p = O.default_params(use_bvh=use_bvh, use_libm=0, accum_mode=1, **kw)
    rc = L.shref_shade(sc.oracle().h, meshes, inst.ctypes.data, len(inst), table.ctypes.data, len(table), surf.ctypes.data if len(surf) else None,
                       len(surf), lts.ctypes.data if len(lts) else None, len(lts), amb.ctypes.data, shadow, maps, int(k), C.byref(p), r8.ctypes.data, n,
                       rgb.ctypes.data, u8.ctypes.data, cnt.ctypes.data, C.byref(tl))
    assert rc == 0, "shref_shade refused the scene"
    return rgb, u8, cnt, tl


def add_tallies(a, b):
    """a += b, field by field"""
    for name, typ in Tallies._fields_:
        if name == "deepest":
            a.deepest = max(a.deepest, b.deepest)
        elif typ is C.c_uint64:
            setattr(a, name, getattr(a, name) + getattr(b, name))
        else:
            arr, other = getattr(a, name), getattr(b, name)
            for i in range(len(arr)):
                arr[i] += other[i]
    return a


def ref_frame(sc, camera, w, h, offsets, table, surf=None, lts=None, ambient=None, k=0, use_bvh=0, **kw):
    """render_surfaces' contract under shadow_steps k -> (rgb [h, w, 3], counts [h, w], the samples' Tallies summed)"""
    p = rr.default_params(**kw)
    cols, total, tl = [], np.zeros(w * h, np.uint32), Tallies()
    for ox, oy in np.asarray(offsets, np.float32):
        rgb, _, cnt, t = ref_shade(sc, rr.camera_rays(camera, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), table, surf, lts, ambient,
                                   k, use_bvh, **kw)
        cols.append(rgb)
        total += cnt
        add_tallies(tl, t)
    return fold(cols).reshape(h, w, 3), total.reshape(h, w), tl


def ref_lit(scenes, camera, w, h, recs, lens, table, surf, lts, shapes, ambient, k, iors=None, weights=None, **kw):
    """lit_helpers.ref_lit under shadow_steps k: per sample the lights are rr.moved_lights(lts, shapes, *light_offset) -> (rgb [h, w, 3],
    counts [h, w], the unweighted colours [S, h, w, 3], per sample (colour, counts, Tallies))"""
    j = [0]

    def shade(key, rays, t):
        rec = recs[j[0]]
        j[0] += 1
        moved = rr.moved_lights(lts, shapes, *(float(v) for v in rec["light_offset"]))
        rgb, _, cnt, tl = ref_shade(scenes[key], rays, t, surf, moved, ambient, k, **kw)
        return rgb, cnt, (rgb.reshape(h, w, 3).copy(), cnt.reshape(h, w).copy(), tl)
    return KH.fold_keys(shade, camera, w, h, recs, lens, table, iors, weights, **kw)


# ------------------------------------------------------------------------------------------------- fixtures
class Fixture(SH.Fixture):
    """a surfaces fixture with the cap its shadow walks run under"""

    def __init__(self, scene, surf, lts, ambient, k, table=TABLE):
        super().__init__(scene, surf, lts, ambient, table)
        self.k = k

    def load(self, r):
        super().load(r)
        r.set_shadow_steps(self.k)

    def ref(self, rays, lts=None, k=None, **kw):
        return ref_shade(self.scene, rays, self.table, self.surf, self.lights if lts is None else lts, self.ambient, self.k if k is None else k, **kw)

    def frame(self, camera, w, h, offsets, k=None, **kw):
        return ref_frame(self.scene, camera, w, h, offsets, self.table, self.surf, self.lights, self.ambient, self.k if k is None else k, **kw)


def with_cap(fx, k):
    """a surfaces_helpers.Fixture as a Fixture under cap k"""
    return Fixture(fx.scene, fx.surf, fx.lights, fx.ambient, k, fx.table)


# the sphere's glass: TABLE's row 1 with a tint strong enough to see, red passing best
TINTED_TABLE = TABLE.copy()
TINTED_TABLE["sigma_a"][1] = (0.2, 0.9, 1.6)
# The lamp of `tinted` stands low beyond the occluder as the sphere sees it, so that the floor on the sphere's far side is reached by
# walks that cross the sphere (two glass hits) and then stop on the occluder; the sun is surfaces_helpers.table()'s.  Both see everything
LOW_LAMP = (2.0, -0.3, 1.8)


def tinted(k=8):
    """surfaces_helpers._floor_scene's floor, sphere and occluder (the scene of surfaces_helpers.table()); the sphere is tinted glass,
    and both lights' shadow rays see it (shadow_mask 0xff)"""
    t = SH.table()
    lts = SH.lights(rr.directional_light(SH.SUN, (1.2, 1.1, 0.9), 0xff), rr.point_light(LOW_LAMP, (2.0, 2.2, 2.6), 0xff))
    return Fixture(t.scene, t.surf, lts, SH.AMBIENT, k, TINTED_TABLE)


def capped():
    """tinted under a cap of two calls: a walk that crosses the sphere and would leave it lit ends occluded at its second glass hit"""
    return tinted(2)


def drink(deep=False, k=8):
    """surfaces_helpers.olive() / deep_olive(): the opaque olive inside two (deep: three) glass instances, so its walks start with a
    list of that length and leave through the glass they are in"""
    return with_cap(SH.deep_olive() if deep else SH.olive(), k)


FIXTURES = {"tinted": tinted, "capped": capped, "drink": drink, "deep-drink": lambda: drink(True)}


def fixture_condition(name, tl):
    """what a fixture is for, as a condition on the tallies of the reference"""
    if name == "tinted":
        return tl.walk_lit_glass[2] > 0 and tl.walk_occluded_after_glass > 0 and tl.walk_calls[1] > 0 and tl.walk_absorbed > 0 and tl.walk_capped == 0
    if name == "capped":
        return tl.walk_capped > 0 and tl.walk_calls[2] > 0 and sum(tl.walk_calls[3:]) == 0
    if name == "drink":
        return tl.walk_start_media[2] > 0 and tl.walk_lit_glass[2] > 0
    if name == "deep-drink":
        return tl.walk_start_media[3] > 0 and tl.walk_lit_glass[2] > 0
    raise KeyError(name)


_refs = {}


def fixture_ref(name, max_reflect=2):
    """(Fixture, rays, ref_shade's result) of a fixture at max_refract 8 on materials_helpers' W x H view, computed once per process"""
    from materials_helpers import H, W, view
    key = (name, max_reflect)
    if key not in _refs:
        fx = FIXTURES[name]()
        rays = rr.camera_rays(view(*SH.VIEW), W, H)
        _refs[key] = (fx, rays, fx.ref(rays, max_refract=8, max_reflect=max_reflect))
    return _refs[key]


# ------------------------------------------------------------------------------------------------- closed forms
CF_SIGMA = (1.0, 2.0, 4.0)
CF_TABLE = np.array([(1.0, (0.0, 0.0, 0.0)), (1.5, CF_SIGMA)], rr.MATERIAL_DTYPE)


def cf_glass_cube(albedo=(0.7, 0.6, 0.5)):
    """surfaces_helpers.cf_floor() with the hovering cube (side 0.4, over x = 1) a glass row of sigma_a CF_SIGMA -> (Scene, surface
    table, material table)"""
    sc, _ = SH.cf_floor()
    return sc, SH.surfaces(rr.opaque(albedo), rr.glass()), CF_TABLE
