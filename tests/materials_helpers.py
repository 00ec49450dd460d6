"""The reference of per-instance glass (test_materials_cpu.py, test_gpu_materials.py): tests/native/materials_ref.c, compiled when
first asked for with the C compiler and the floating-point flags the oracle is built with, and loaded with ctypes beside
oracle/librr_oracle.so, whose rro_trace and rro_env_lookup it calls.  Scenes are scenes.Scene objects whose instances carry their
material index in the low 24 bits of hitgroup_flags (rr.make_instances(materials=...))."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import oracle as O
import refraction_raytracing_dxr_amd as rr
from scenes import Scene, load, oracle_instances, xf
from shading_helpers import env_map, fold, view_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "materials_ref.c")
W, H = 48, 36
# the mixed table of the issue: a clear crown-like glass, a red one, a blue-absorbing one of low index
MIXED = np.array([(1.3, (0.0, 0.0, 0.0)), (1.5, (0.8, 0.1, 0.1)), (1.1, (0.05, 0.4, 2.0))], rr.MATERIAL_DTYPE)
# The view of the three-instance scene: chosen on the CPU (test_materials_cpu.py asserts it) so that every material absorbs at inside
# hits and the mixed frame's ray counts differ from those of every uniform table
VIEW3 = (0.6, 0.9)


class _Mesh(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("idx", C.c_void_p)]


_lib = None
_dir = None


def lib():
    """materials_ref.c as a shared object in a temporary directory of this process"""
    global _lib, _dir
    if _lib is None:
        O.lib()                                                 # builds oracle/librr_oracle.so if it is missing
        _dir = tempfile.TemporaryDirectory(prefix="materials_ref")
        so = os.path.join(_dir.name, "libmaterials_ref.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.run([cc, "-O2", "-g0", "-std=gnu11", "-fPIC", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
                        "-shared", "-o", so, SRC, "-L" + O.ORACLE_DIR, "-l:librr_oracle.so", "-Wl,-rpath," + O.ORACLE_DIR, "-lm"], check=True)
        L = C.CDLL(so)
        L.mref_expf_neg.restype, L.mref_expf_neg.argtypes = C.c_float, [C.c_float]
        L.mref_shade.restype = C.c_int
        L.mref_shade.argtypes = [C.c_void_p, C.POINTER(_Mesh), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(O.Params), C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def uniform(ior, n=1):
    t = np.zeros(n, rr.MATERIAL_DTYPE)
    t["ior"] = ior
    return t


def scene_instances(sc):
    """a Scene's instances; the reference's one identity instance (material 0) where it has none"""
    return rr.make_instances(meshes=[0]) if sc.instances is None else sc.instances


def ref_shade(sc, rays, table, use_bvh=0, **kw):
    """the ray trees of RAY_DTYPE rays in Scene sc under the material table -> (rgb float32 [n, 3], rgba8 uint8 [n, 4], TraceRay
    calls uint32 [n], inside hits absorbed at per material uint64 [len(table)]); kw: max_refract, max_reflect, tmin_secondary,
    tmax_secondary"""
    L = lib()
    table = np.ascontiguousarray(table, rr.MATERIAL_DTYPE)
    inst = np.ascontiguousarray(oracle_instances(scene_instances(sc)))
    keep = [(np.ascontiguousarray(v), np.ascontiguousarray(i, np.uint32)) for v, i in sc.meshes]
    meshes = (_Mesh * len(keep))(*[_Mesh(v.ctypes.data, i.ctypes.data) for v, i in keep])
    n = len(rays)
    r8 = np.zeros((n, 8), np.float32)
    r8[:, 0:3], r8[:, 3], r8[:, 4:7], r8[:, 7] = rays["origin"], rays["tmin"], rays["dir"], rays["tmax"]
    rgb, u8, cnt = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint32)
    absorbed = np.zeros(len(table), np.uint64)
    p = O.default_params(use_bvh=use_bvh, use_libm=0, accum_mode=1, **kw)
    rc = L.mref_shade(sc.oracle().h, meshes, inst.ctypes.data, len(inst), table.ctypes.data, len(table), C.byref(p), r8.ctypes.data, n,
                      rgb.ctypes.data, u8.ctypes.data, cnt.ctypes.data, absorbed.ctypes.data)
    assert rc == 0, "mref_shade refused the scene"
    return rgb, u8, cnt, absorbed


def ref_frame(sc, camera, w, h, offsets, table, use_bvh=0, **kw):
    """render_materials' contract on the CPU: sample s is ref_shade of rr.camera_rays(camera, w, h, *offsets[s]), resolved by
    shading_helpers.fold -> (rgb [h, w, 3], counts [h, w], absorbed)"""
    p = rr.default_params(**kw)
    cols, total, absorbed = [], np.zeros(w * h, np.uint32), 0
    for ox, oy in np.asarray(offsets, np.float32):
        rgb, _, cnt, ab = ref_shade(sc, rr.camera_rays(camera, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), table, use_bvh, **kw)
        cols.append(rgb)
        total += cnt
        absorbed = absorbed + ab
    return fold(cols).reshape(h, w, 3), total.reshape(h, w), absorbed


_scenes = {}


def monkey_scene(material=0):
    """monkey.obj alone, the reference's one identity instance, made of row `material`"""
    key = "monkey-%d" % material
    if key not in _scenes:
        inst = rr.make_instances(meshes=[0], materials=[material]) if material else None
        _scenes[key] = Scene(key, [load("monkey.obj")], env_map(), inst)
    return _scenes[key]


def three_scene(materials=(0, 1, 2)):
    """two meshes under three instances: the monkey where it is, a cube scaled unevenly, a smaller monkey rotated about y"""
    key = "three-%d-%d-%d" % tuple(materials)
    if key not in _scenes:
        inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(-1.9, 0.2, 0.4, (0.5, 0.8, 0.6)), xf(1.8, -0.2, -0.3, (0.7, 0.7, 0.7), 0.7)],
                                 meshes=[0, 1, 0], materials=list(materials))
        _scenes[key] = Scene(key, [load("monkey.obj"), load("cube.obj")], env_map(), inst)
    return _scenes[key]


def view(angle, fov, w=W, h=H):
    return view_constants(angle, fov, w, h)[0]
