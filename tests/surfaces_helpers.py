"""The reference of the ray tree with opaque hit groups (test_surfaces_cpu.py, test_gpu_surfaces.py): tests/native/surfaces_ref.c,
compiled when first asked for with the C compiler and the floating-point flags the oracle is built with, and loaded with ctypes beside
oracle/librr_oracle.so, whose rro_trace and rro_env_lookup it calls -- as nested_helpers.py loads nested_ref.c.  rro_trace has no
instance mask: for every distinct shadow_mask the helper builds one more oracle scene of the instances whose InstanceMask meets it,
and hands none where no instance does.  The fixtures are shipped closed meshes (and the open monkey, alone) under instance
transforms; what each claims about its geometry is asserted here from the transformed vertices, with nested_helpers' margin."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import nested_helpers as NH
import oracle as O
import refraction_raytracing_dxr_amd as rr
from materials_helpers import _Mesh, scene_instances
from nested_helpers import MARGIN, TABLE, assert_disjoint, assert_inside, world_triangles
from scenes import Scene, load, oracle_instances, oracle_scene, xf
from shading_helpers import env_map, fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "surfaces_ref.c")


class Tallies(C.Structure):
    _fields_ = [("interfaces", C.c_uint64), ("passes", C.c_uint64), ("deepest", C.c_uint64), ("opaque_hits", C.c_uint64),
                ("shadow_traced", C.c_uint64), ("shadow_occluded", C.c_uint64), ("shadow_lit", C.c_uint64), ("lights_skipped", C.c_uint64),
                ("specular_children", C.c_uint64), ("specular_then_refracted", C.c_uint64), ("opaque_in_media", C.c_uint64 * 5),
                ("opaque_back", C.c_uint64), ("light_used", C.c_uint64 * 8), ("light_occluded", C.c_uint64 * 8)]

    def __repr__(self):
        return ("interfaces %d, passes %d, deepest list %d, opaque hits %d (by list length %s, back faces %d), shadow rays %d = %d occluded + %d lit "
                "(per light %s, occluded %s), lights skipped %d, specular children %d, interfaces below them %d") % (
            self.interfaces, self.passes, self.deepest, self.opaque_hits, list(self.opaque_in_media), self.opaque_back, self.shadow_traced,
            self.shadow_occluded, self.shadow_lit, list(self.light_used), list(self.light_occluded), self.lights_skipped, self.specular_children,
            self.specular_then_refracted)


_lib = None
_dir = None


def lib():
    """surfaces_ref.c as a shared object in a temporary directory of this process"""
    global _lib, _dir
    if _lib is None:
        O.lib()                                                 # builds oracle/librr_oracle.so if it is missing
        _dir = tempfile.TemporaryDirectory(prefix="surfaces_ref")
        so = os.path.join(_dir.name, "libsurfaces_ref.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.run([cc, "-O2", "-g0", "-std=gnu11", "-fPIC", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                        "-shared", "-o", so, SRC, "-L" + O.ORACLE_DIR, "-l:librr_oracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-lm"], check=True)
        L = C.CDLL(so)
        L.sref_shade.restype = C.c_int
        L.sref_shade.argtypes = [C.c_void_p, C.POINTER(_Mesh), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(O.Params), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(Tallies)]
        _lib = L
    return _lib


def surfaces(*rows):
    return np.array(list(rows), rr.SURFACE_DTYPE) if rows else np.zeros(0, rr.SURFACE_DTYPE)


def lights(*rows):
    return np.array(list(rows), rr.LIGHT_DTYPE) if rows else np.zeros(0, rr.LIGHT_DTYPE)


_shadow = {}


def shadow_scene(sc, mask):
    """the oracle scene a shadow ray of shadow_mask `mask` is traced in: sc's own where every instance meets the mask, one of the
    instances that do otherwise, None where none does"""
    key = (sc.key, int(mask))
    if key not in _shadow:
        inst = scene_instances(sc)
        keep = ((inst["instance_id_mask"] >> 24) & int(mask)) != 0
        if keep.all():
            _shadow[key] = sc.oracle()
        elif not keep.any():
            _shadow[key] = None
        else:
            _shadow[key] = oracle_scene(sc.meshes, None, inst[keep])
    return _shadow[key]


def ref_shade(sc, rays, table, surf=None, lts=None, ambient=None, use_bvh=0, **kw):
    """the ray trees of RAY_DTYPE rays in Scene sc under the material table, the surface table, the lights and the ambient term ->
    (rgb float32 [n, 3], rgba8 uint8 [n, 4], TraceRay calls uint32 [n], Tallies); kw: max_refract, max_reflect, tmin_secondary,
    tmax_secondary"""
    L = lib()
    table = np.ascontiguousarray(table, rr.MATERIAL_DTYPE)
    surf = surfaces() if surf is None else np.ascontiguousarray(surf, rr.SURFACE_DTYPE).reshape(-1)
    lts = lights() if lts is None else np.ascontiguousarray(lts, rr.LIGHT_DTYPE).reshape(-1)
    amb = np.zeros(3, np.float32) if ambient is None else np.ascontiguousarray(ambient, np.float32).reshape(3)
    inst = np.ascontiguousarray(oracle_instances(scene_instances(sc)))
    keep = [(np.ascontiguousarray(v), np.ascontiguousarray(i, np.uint32)) for v, i in sc.meshes]
    meshes = (_Mesh * len(keep))(*[_Mesh(v.ctypes.data, i.ctypes.data) for v, i in keep])
    held = [shadow_scene(sc, m) for m in lts["shadow_mask"]]
    shadow = (C.c_void_p * max(1, len(lts)))(*[None if s is None else s.h for s in held])
    n = len(rays)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7], r8[:, 7] = rays["origin"], rays["tmin"], rays["dir"], rays["tmax"]
    rgb, u8, cnt = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint32)
    tl = Tallies()
    p = O.default_params(use_bvh=use_bvh, use_libm=0, accum_mode=1, **kw)
    rc = L.sref_shade(sc.oracle().h, meshes, inst.ctypes.data, len(inst), table.ctypes.data, len(table), surf.ctypes.data if len(surf) else None,
                      len(surf), lts.ctypes.data if len(lts) else None, len(lts), amb.ctypes.data, shadow, C.byref(p), r8.ctypes.data, n,
                      rgb.ctypes.data, u8.ctypes.data, cnt.ctypes.data, C.byref(tl))
    assert rc == 0, "sref_shade refused the scene"
    return rgb, u8, cnt, tl


def ref_frame(sc, camera, w, h, offsets, table, surf=None, lts=None, ambient=None, use_bvh=0, **kw):
    """render_surfaces' contract on the CPU: sample s is ref_shade of rr.camera_rays(camera, w, h, *offsets[s]), resolved by
    shading_helpers.fold -> (rgb [h, w, 3], counts [h, w])"""
    p = rr.default_params(**kw)
    cols, total = [], np.zeros(w * h, np.uint32)
    for ox, oy in np.asarray(offsets, np.float32):
        rgb, _, cnt, _ = ref_shade(sc, rr.camera_rays(camera, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), table, surf, lts, ambient,
                                   use_bvh, **kw)
        cols.append(rgb)
        total += cnt
    return fold(cols).reshape(h, w, 3), total.reshape(h, w)


# ------------------------------------------------------------------------------------------------- fixtures
class Fixture:
    """a scene with what the four calls read beside it"""

    def __init__(self, scene, surf, lts=None, ambient=None, table=TABLE):
        self.scene, self.table, self.surf, self.lights, self.ambient = scene, table, surf, lights() if lts is None else lts, ambient

    def load(self, r):
        self.scene.load_gpu(r)
        r.set_materials(self.table)
        r.set_surfaces(self.surf)
        r.set_lights(self.lights, self.ambient)

    def ref(self, rays, lts=None, **kw):
        return ref_shade(self.scene, rays, self.table, self.surf, self.lights if lts is None else lts, self.ambient, **kw)

    def frame(self, camera, w, h, offsets, **kw):
        return ref_frame(self.scene, camera, w, h, offsets, self.table, self.surf, self.lights, self.ambient, **kw)


FLOOR_TOP = -0.8
AMBIENT = (0.05, 0.06, 0.08)
SUN = (-0.5, 1.0, -0.4)                                     # towards the light: behind the things as the camera of VIEW sees them
LAMP_AT = (-0.6, 1.6, 0.5)
VIEW = NH.VIEW


def _floor_scene(key, occluder):
    """a flattened cube as the floor (row 0, mask 0x01), a sphere resting above it (row 1, mask 0x02) and, with `occluder`, a small cube
    standing beside it (row 2, mask 0x01): pairwise apart by more than MARGIN, the floor's top face the plane y = FLOOR_TOP"""
    t = [xf(0, FLOOR_TOP - 0.1, 0, (2.5, 0.1, 2.5)), xf(0, FLOOR_TOP + 0.05 + 0.3 * 3.0 ** 0.5, 0, (0.3, 0.3, 0.3))]
    if occluder:
        t.append(xf(0.9, FLOOR_TOP + 0.05 + 0.2, 0.8, (0.2, 0.2, 0.2), 0.5))
    k = len(t)
    sc = NH._scene(key, transforms=t, meshes=[0, 1, 0][:k], materials=[0, 1, 2][:k], masks=[0x01, 0x02, 0x01][:k])
    top = world_triangles(sc, 0).reshape(-1, 3)[:, 1].max()
    assert abs(top - FLOOR_TOP) < 1e-6
    for a in range(k):
        for b in range(a + 1, k):
            assert_disjoint(sc, a, b)
        if a:
            assert world_triangles(sc, a).reshape(-1, 3)[:, 1].min() > FLOOR_TOP + MARGIN       # above the floor, not in it
    return sc


def table(sun_mask=0x01):
    """the floor, the glass sphere and the occluder under a directional light that does not see the glass (shadow_mask 0x01) and a
    point light that does (0xff), with an ambient term"""
    surf = surfaces(rr.opaque((0.7, 0.6, 0.5)), rr.glass(), rr.opaque((0.2, 0.5, 0.8), emission=(0.02, 0.0, 0.0)))
    lts = lights(rr.directional_light(SUN, (1.2, 1.1, 0.9), sun_mask), rr.point_light(LAMP_AT, (2.0, 2.2, 2.6), 0xff))
    return Fixture(_floor_scene("table", True), surf, lts, AMBIENT)


def mirror():
    """the floor as a mirror with a small albedo, the glass sphere above it"""
    surf = surfaces(rr.opaque((0.05, 0.05, 0.05), specular=(0.8, 0.8, 0.8)), rr.glass())
    return Fixture(_floor_scene("mirror", False), surf, lights(rr.directional_light(SUN, (1.0, 1.0, 1.0), 0xff)), (0.1, 0.1, 0.1))


def olive():
    """nested_helpers.tumbler() with its innermost cube (row 3) opaque and emissive, under one point light outside the glass"""
    surf = surfaces(rr.glass(), rr.glass(), rr.glass(), rr.opaque((0.4, 0.5, 0.1), emission=(0.1, 0.2, 0.05)))
    return Fixture(NH.tumbler(), surf, lights(rr.point_light((2.0, 2.5, 1.0), (6.0, 6.0, 6.0), 0xff)), (0.02, 0.02, 0.02))


def deep_olive():
    """the tumbler's three instances inside one more glass sphere (row 4): the opaque, emissive innermost cube is reached with a list
    of three media.  The glass has mask 0x02 and the olive 0x01, so the point light's shadow rays (shadow_mask 0x01) reach it through
    the glass and the olive is lit as well as dimmed"""
    sc = NH._scene("deep-olive", transforms=[xf(0, 0, 0, (1.2, 1.2, 1.2)), xf(0, 0, 0), xf(0.05, -0.03, 0.04, (0.5, 0.5, 0.5)),
                                             xf(0.1, 0.05, -0.02, (0.3, 0.3, 0.3), 0.4)],
                   meshes=[1, 0, 1, 0], materials=[4, 1, 2, 3], masks=[0x02, 0x02, 0x02, 0x01])
    for k in range(3):
        assert_inside(sc, k + 1, k)
    surf = surfaces(rr.glass(), rr.glass(), rr.glass(), rr.opaque((0.4, 0.5, 0.1), emission=(0.1, 0.2, 0.05), specular=(0.2, 0.2, 0.2)))
    return Fixture(sc, surf, lights(rr.point_light((2.0, 2.5, 1.0), (6.0, 6.0, 6.0), 0x01), rr.directional_light((0.8, 0.6, 0.5), (0.5, 0.5, 0.5), 0xff)),
                   (0.02, 0.02, 0.02))


def lamp():
    """an emissive opaque sphere (row 2) inside a glass cube (row 1): no light but its own"""
    sc = NH._scene("lamp", transforms=[xf(0, 0, 0), xf(0.1, 0.0, -0.1, (0.3, 0.3, 0.3))], meshes=[0, 1], materials=[1, 2])
    assert_inside(sc, 1, 0)
    return Fixture(sc, surfaces(rr.glass(), rr.glass(), rr.opaque((0.0, 0.0, 0.0), emission=(1.5, 1.2, 0.6))))


def alone():
    """monkey.obj without a top level, made of the opaque row 2 (it travels as a kernel argument), one directional light; a little
    specular, so that mirror children meet the open mesh from behind"""
    surf = surfaces(rr.glass(), rr.glass(), rr.opaque((0.8, 0.7, 0.6), specular=(0.3, 0.3, 0.3)))
    return Fixture(NH.alone("monkey.obj", 2), surf, lights(rr.directional_light((0.6, 0.7, 0.4), (1.0, 0.9, 0.8), 0x01)), (0.03, 0.03, 0.03))


FIXTURES = {"table": table, "mirror": mirror, "olive": olive, "deep-olive": deep_olive, "lamp": lamp, "alone": alone}


def fixture_condition(name, tl):
    """what a fixture is for, as a condition on the tallies of the reference"""
    if name == "table":
        return (tl.shadow_occluded > 0 and tl.shadow_lit > 0 and tl.lights_skipped > 0 and tl.light_used[0] > 0 and tl.light_used[1] > 0
                and tl.light_occluded[0] > 0 and tl.light_occluded[1] > 0)
    if name == "mirror":
        return tl.specular_children > 0 and tl.specular_then_refracted > 0
    if name == "olive":        # the olive sits in the sphere in the cube: every medium the tumbler has is on the list when it is reached
        return tl.opaque_in_media[2] > 0 and tl.deepest == 2 and tl.shadow_traced > 0
    if name == "deep-olive":   # opaque hits reached with a list of three, lit through the glass by one light and shadowed from the other
        return tl.opaque_in_media[3] > 0 and tl.shadow_lit > 0 and tl.shadow_occluded > 0 and tl.specular_children > 0
    if name == "lamp":
        return tl.opaque_in_media[1] > 0 and tl.shadow_traced == 0
    if name == "alone":
        return tl.opaque_hits > 0 and tl.shadow_lit > 0 and tl.shadow_occluded > 0 and tl.opaque_back > 0
    raise KeyError(name)


_refs = {}


def fixture_ref(name, max_reflect):
    """(Fixture, rays, ref_shade's result) of a ray fixture at max_refract 8, computed once per process"""
    from materials_helpers import H, W, view
    key = (name, max_reflect)
    if key not in _refs:
        fx = FIXTURES[name]()
        rays = rr.camera_rays(view(*VIEW), W, H)
        _refs[key] = (fx, rays, fx.ref(rays, max_refract=8, max_reflect=max_reflect))
    return _refs[key]


# ------------------------------------------------------------------------------------------------- closed forms
CF_ENV = NH.CF_ENV


def _const_env():
    env = np.zeros((8, 16, 3), np.float32)
    env[:] = CF_ENV
    return env


def cf_floor(specular=(0, 0, 0), albedo=(0.7, 0.6, 0.5)):
    """a floor whose top is the plane y = 0 and a small cube hovering over x = 1 (both mask 1) under a constant environment"""
    key = "cf-floor"
    if key not in NH._scenes:
        inst = rr.make_instances(transforms=[xf(0, -0.1, 0, (3, 0.1, 3)), xf(1.0, 1.0, 0.0, (0.2, 0.2, 0.2))], meshes=[0, 0], materials=[0, 1])
        NH._scenes[key] = Scene(key, [load("cube.obj")], _const_env(), inst)
    sc = NH._scenes[key]
    assert_disjoint(sc, 0, 1)
    return sc, surfaces(rr.opaque(albedo, specular=specular), rr.opaque((0.5, 0.5, 0.5)))


def down_ray(x, z=0.13):
    """straight down onto the floor of cf_floor from y = 3, off the faces' diagonals"""
    return rr.pack_rays(np.array([[x, 3.0, z]], np.float32), np.array([[0.0, -1.0, 0.0]], np.float32), np.float32(1e-4), np.float32(100.0))
