"""The ray-tree kernels' instantiations, each at its deepest tree (test_tree_matrix_cpu.py, test_gpu_tree_matrix.py).  No GPU code.

Fourteen kernel templates are built through for_tree_variant (csrc/rr_choice.h) as the 20 instantiations of codeobj.LAUNCHABLE.  CASES
names, for each of the 20, a chain of test_gpu_stack_rungs.py, a max_reflect and the debug switches with which fused_variant
(csrc/rr_choice.cpp, depth 64 as every ray-tree call passes it) and for_tree_variant arrive at it with the tree at the deepest depth it
takes; BOUNDARIES the trees one level deeper than a rung's last, where the next instantiation takes over.  RR_DEBUG_STACK=n is the
project's way to the 32-bit rungs of one instance with a mesh of a few dozen triangles: the instantiation is the one a mesh of 32 768
triangles or more takes.  Nothing here restates the ladder: expected_variant asks tests/native/kernel_choice_driver.cpp.

The scenes are chain_scene's.  Two-level ones get material rows 1 and 2 of nested_helpers.TABLE and instance masks 1 and 2; for the
surfaces calls the first instance is glass and the second an opaque mirror under a directional light whose shadow rays see only the
glass one (shadow_mask 1) and a point light whose shadow rays see both.  The one identity instance (row 0, mask 1) is, for the
surfaces calls, the opaque mirror of test_gpu_surfaces.py::test_surfaces_on_either_side_of_a_stack_rung under its two lights.  The CPU
references of a case are computed once per process and shared by the cases that use the same chain and max_reflect."""
import collections
import os
import shutil
import subprocess
import tempfile

import numpy as np

import composed_helpers as CH
import materials_helpers as MH
import nested_helpers as NH
import oracle as O
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as KH
import surfaces_helpers as SH
import test_gpu_stack_rungs as RUNGS
from depth_meshes import ploc_model, stack_high_water, to_object_space, tree_depth
from nested_helpers import TABLE
from shading_helpers import OFFP16, PERM16, adaptive_reference
from test_gpu_samples import oracle_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "refraction_raytracing_dxr_amd", "csrc")
U16, U32 = "unsigned short", "unsigned int"
BITS = {16: U16, 32: U32}

# variant: the (STACK, PEND, TLAS, E) of codeobj.LAUNCHABLE; need: rr_stats.bvh_depth of the scene; env: the renderer's debug switches
Case = collections.namedtuple("Case", "variant single need max_reflect env")


def _case(stack, pend, tlas, e, need, **env):
    return Case((stack, pend, tlas, e), not tlas, need, 2 if pend == 2 else 3, env)


CASES = [
    # one identity instance: chain_scene(need)
    _case(19, 2, False, U32, 19),
    _case(26, 2, False, U32, 26, RR_DEBUG_STACK=26),
    _case(31, 2, False, U32, 31, RR_DEBUG_STACK=31),
    _case(39, 2, False, U32, 39, RR_DEBUG_STACK=39),
    _case(64, 2, False, U32, 64),
    _case(31, 8, False, U32, 31, RR_DEBUG_STACK=31),
    _case(39, 8, False, U32, 39, RR_DEBUG_STACK=39),
    _case(64, 8, False, U32, 64),
    _case(39, 2, False, U16, 39),
    _case(39, 8, False, U16, 39),
    # two instances: chain_scene(need, True), a chain TLAS_DEPTH shallower under one top-level node
    _case(30, 2, True, U16, 30),
    _case(39, 2, True, U16, 39),
    _case(19, 2, True, U32, 19, RR_DEBUG_TLAS32=1),
    _case(26, 2, True, U32, 26, RR_DEBUG_TLAS32=1),
    _case(31, 2, True, U32, 31, RR_DEBUG_TLAS32=1),
    _case(39, 2, True, U32, 39, RR_DEBUG_TLAS32=1),
    _case(64, 2, True, U32, 64),
    _case(31, 8, True, U32, 31),
    _case(39, 8, True, U32, 39),
    _case(64, 8, True, U32, 64),
]
# one level deeper than a rung's last tree, max_reflect 2: the instantiation that must have taken over
BOUNDARIES = [
    _case(39, 2, False, U16, 20),
    _case(64, 2, False, U32, 40),
    _case(39, 2, True, U16, 31),
    _case(64, 2, True, U32, 40),
    _case(26, 2, True, U32, 20, RR_DEBUG_TLAS32=1),
    _case(31, 2, True, U32, 27, RR_DEBUG_TLAS32=1),
    _case(39, 2, True, U32, 32, RR_DEBUG_TLAS32=1),
    _case(64, 2, True, U32, 40, RR_DEBUG_TLAS32=1),
]


def case_id(c):
    return "%d-%d-%s-%s-need%d%s" % (c.variant[0], c.variant[1], "two" if c.variant[2] else "one", "u16" if c.variant[3] == U16 else "u32", c.need,
                                      "".join("-%s%s" % (k[9:].lower(), v) for k, v in sorted(c.env.items())))


def shallower(c):
    """the case's scene one level shallower under the same switches: a boundary's neighbour on the rung below"""
    return c._replace(need=c.need - 1)


# ------------------------------------------------------------------------------------------------- the model: rr_choice.cpp itself
_driver = []


def driver():
    """tests/native/kernel_choice_driver.cpp, built as test_kernel_choice.py builds it, once per process"""
    if not _driver:
        gxx = shutil.which("g++")
        assert gxx, "the kernel-choice driver needs g++"
        tmp = tempfile.TemporaryDirectory(prefix="tree_matrix")
        out = os.path.join(tmp.name, "kernel_choice_driver")
        srcs = [os.path.join(ROOT, "tests", "native", "kernel_choice_driver.cpp"), os.path.join(CSRC, "rr_choice.cpp"),
                os.path.join(CSRC, "host", "rr_host_partition.cpp"), os.path.join(CSRC, "host", "rr_host_camera.cpp")]
        subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + srcs + ["-o", out], check=True)
        _driver.extend([out, tmp])
    return _driver[0]


def chain_counts(single, need):
    """(blas_tris, pool_nodes, pool_refs) as scene_facts (csrc/rr_capi_dispatch.cpp) counts them on the chain scene of `need`: one
    triangle per level; the pool of a two-level scene holds the one mesh's nodes, and its references are the triangles and the instances"""
    n = need if single else need - RUNGS.TLAS_DEPTH
    return (n, 0, 0) if single else (0, n - 1, n + 2)


def expected_variants(queries):
    """[(single, need, max_reflect, dbg_stack, tlas32, counts or None)] -> [(STACK, PEND, TLAS, E)]: for_tree_variant of fused_variant
    at depth 64 under RR_DEBUG_KERNEL=fused, as the driver's `variant` command composes them"""
    lines = []
    for single, need, max_reflect, dbg_stack, tlas32, counts in queries:
        tris, nodes, refs = chain_counts(single, need) if counts is None else counts
        lines.append("variant %d %d %d %d %d 0 64 %d 1 %d %d" % (single, need, tris, nodes, refs, max_reflect, dbg_stack, tlas32))
    r = subprocess.run([driver()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(lines) and all(len(v) == 4 for v in out), r.stdout
    return [(s, p, bool(t), BITS[b]) for s, p, t, b in out]


def expected_variant(single, need, max_reflect, dbg_stack, tlas32, counts=None):
    """the instantiation a ray-tree call launches on a scene of these facts; counts: (blas_tris, pool_nodes, pool_refs) of a loaded
    scene, the chain's by default"""
    return expected_variants([(bool(single), int(need), int(max_reflect), int(dbg_stack), int(bool(tlas32)), counts)])[0]


def case_query(c, counts=None):
    return (c.single, c.need, c.max_reflect, int(c.env.get("RR_DEBUG_STACK", 0)), int(c.env.get("RR_DEBUG_TLAS32", 0)), counts)


# ------------------------------------------------------------------------------------------------- scenes, views and sample tables
W, H = 48, 32                                               # the caller rays of the shade_rays calls
FW, FH = RUNGS.SW, RUNGS.SH                                 # the frames
ROWS, MASKS = (1, 2), (1, 2)                                # the two instances' material rows and InstanceMasks
LENS = rr.Lens(0.1, 5.0)                                    # as test_gpu_lens.py's rungs: focused on the chain
LOFF2 = np.array([[0.0, 0.0], [1.0, -0.5]], np.float32)     # lens sample 0 through the lens centre: the deep direction
LOFF4 = np.array([[0.0, 0.0], [1.0, -0.5], [-0.5, 0.75], [0.0, -1.0]], np.float32)
BANDS2 = np.array([(1.25, (1.5, 0.5, 1.0)), (1.4, (0.5, 1.5, 1.0))], rr.BAND_DTYPE)     # as test_gpu_spectral.py's rungs
# render_adaptive's contrast threshold here: 2 base samples of 4.  Under shading_helpers.THRESHOLD (0.1 of the displayed range) the
# oracle refines no pixel of the shallow one-instance chains -- a few sheets of clear glass show little contrast: the largest is 0.074 to
# 0.099 at needs 19, 20, 26 and 31 -- and k_adaptive_refine would trace nothing there.  At a fifth of it the oracle refines 96 to 172 of
# the 384 pixels of every case and leaves the others at their base samples, so both classes stay in every frame
# (test_tree_matrix_cpu.py asserts it)
ADAPTIVE_BASE, ADAPTIVE_MAX, ADAPTIVE_THRESHOLD = 2, 4, 0.02
BAND_ORDER = [0, 1, 1, 0]                                   # two positions, each in both bands, sample 0 in band 0
_scenes = {}
_models = {}


def scene(c):
    """chain_scene of the case; a two-level one with its material rows and masks"""
    if c.single:
        return RUNGS.chain_scene(c.need)
    key = "matrix-%d" % c.need
    if key not in _scenes:
        base = RUNGS.chain_scene(c.need, True)
        inst = base.instances.copy()
        inst["hitgroup_flags"] |= np.array(ROWS, inst["hitgroup_flags"].dtype)
        inst["instance_id_mask"] = (inst["instance_id_mask"] & 0xffffff) | (np.array(MASKS, inst["instance_id_mask"].dtype) << 24)
        _scenes[key] = RUNGS.RungScene(key, base.meshes, RUNGS.ENV, inst)
    return _scenes[key]


def fov(c):
    """test_gpu_stack_rungs.py's field of view, which the 64-level chain (half a side 1.0375) fills from five units away; one identity
    instance of a shallower, and so smaller, chain gets the same share of the frame: under the fixed one the 19- and 26-level chains
    leave fewer than 100 of the 48x32 caller rays a hit (72 and 98).  A two-level scene's instances stand 0.8 to either side of the
    middle whatever their size: it keeps the fixed one."""
    return RUNGS.FOV * (1.0 + 0.05 * (c.need - 1)) / (1.0 + 0.05 * 63) if c.single else RUNGS.FOV


def view(c, w, h):
    """test_gpu_stack_rungs.view from the deep side (the camera on the -z side, its rays travelling towards +z) with the case's fov"""
    return rr.camera_orbit(float(RUNGS.DEEP), fov_y=float(fov(c)), aspect=float(np.float32(w / h)))


def cam_rays(c):
    return view(c, W, H)


def cam_frame(c):
    return view(c, FW, FH)


def caller_rays(c):
    return rr.camera_rays(cam_rays(c), W, H)


def raygen_rays(c):
    """the rays whose walk must fill the rung, one bundle per RayGen the calls use: the pinhole rays of the 48x32 view, sample 0 of
    the 24x16 frames, and lens sample 0 through the lens centre"""
    cam = cam_frame(c)
    return {"pinhole": caller_rays(c), "sample 0": rr.camera_rays(cam, FW, FH, *OFFP16[0]),
            "lens sample 0": rr.lens_rays(cam, FW, FH, *OFFP16[0], *LOFF2[0], LENS)}


def composed_records():
    return CH.records(np.repeat(OFFP16[:2], 2, axis=0), LOFF4, BAND_ORDER)


def shutter_records():
    """composed_records with every sample in scene key 0"""
    return KH.records(np.repeat(OFFP16[:2], 2, axis=0), LOFF4, BAND_ORDER, 0)


def bands():
    """(iors [2, 6], weights [2, 3]): TABLE in two bands, as the composed fixtures take them"""
    return CH.fixture_bands()


# The two-level lights.  The opaque instance (x = +0.8) is the mirrored one with TRIANGLE_FRONT_COUNTERCLOCKWISE, whose shading normals do
# not follow the flag: the face normal the hit group lights points along a ray travelling towards +z, so both lights stand on the +z
# side (on the camera's side every light is skipped).  The sun grazes the sheets towards -x, where the glass instance stands: its
# shadow rays see that instance alone (shadow_mask 1), and would be stopped by the mirror's own larger sheets otherwise.  The lamp's see
# both: the sheet a ray stopped on is lit past the last sheet's rim and shadowed by the larger sheets behind it elsewhere.
SUN2 = (-1.0, 0.05, 0.12)
LAMP2 = (0.1, 0.9, 2.5)


def surfaces_fixture(c):
    """the case's scene with what the surfaces calls read beside it (a surfaces_helpers.Fixture)"""
    sc = scene(c)
    if sc.single:
        surf = SH.surfaces(rr.opaque((0.6, 0.5, 0.4), specular=(0.5, 0.5, 0.5)))
        lts = SH.lights(rr.directional_light((1.0, 0.2, -0.02), (1.0, 0.9, 0.8), 0x01),
                        rr.directional_light((-0.3, 0.2, -1.0), (0.5, 0.6, 0.7), 0xff))
        return SH.Fixture(sc, surf, lts, (0.01, 0.01, 0.01))
    surf = SH.surfaces(rr.glass(), rr.glass(), rr.opaque((0.6, 0.5, 0.4), specular=(0.4, 0.4, 0.4)))
    lts = SH.lights(rr.directional_light(SUN2, (1.0, 0.9, 0.8), 0x01), rr.point_light(LAMP2, (4.0, 4.0, 4.0), 0xff))
    return SH.Fixture(sc, surf, lts, (0.02, 0.03, 0.04))


# ------------------------------------------------------------------------------------------------- the builder's model of a chain
def model_nodes(c):
    """the default builder's hierarchy of the case's one mesh, from depth_meshes.ploc_model: what rr_download_blas gives"""
    n = c.need if c.single else c.need - RUNGS.TLAS_DEPTH
    if n not in _models:
        (v, i), = scene(c).meshes
        nodes, _, depth = ploc_model(v, i)
        assert depth == n == tree_depth(nodes), (depth, n)
        _models[n] = nodes
    return _models[n]


def model_high_water(c, rays):
    """the deepest stack `rays` reach on the model, as assert_rung reads it off the downloaded tree"""
    sc, nodes = scene(c), model_nodes(c)
    if sc.single:
        return int(stack_high_water(nodes, rays).max())
    return max(int(stack_high_water(nodes, to_object_space(rays, t)).max()) for t in sc.instances["transform"])


# ------------------------------------------------------------------------------------------------- the references, once per process
_refs = {}


def params(c):
    return dict(max_refract=5, max_reflect=c.max_reflect)


def _ref(c, what, make):
    key = (scene(c).key, c.max_reflect, what)
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def ref_oracle_counts(c):
    """TraceRay counts [H, W] of the oracle's frame of the caller rays' view: what shading_helpers.check_against_oracle compares"""
    cam = cam_rays(c)
    M, loc = np.array(cam.proj_inv, np.float32), np.array(cam.camera_loc, np.float32)
    return _ref(c, "oracle", lambda: scene(c).oracle().render(M, loc, W, H, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, **params(c)),
                                                               want_rays=True)["rays"].astype(np.uint32))


def ref_samples(c):
    """the oracle's 96x64 frame as the sub-pixel samples of the 24x16 frame (test_gpu_samples.oracle_samples): rgb [4, 4, FH, FW, 3] and
    TraceRay counts [4, 4, FH, FW]: the reference of render_samples and render_adaptive"""
    cam = cam_frame(c)
    M, loc = np.array(cam.proj_inv, np.float32), np.array(cam.camera_loc, np.float32)
    return _ref(c, "samples", lambda: oracle_samples(scene(c).oracle(), M, loc, FW, FH, **params(c)))


def ref_adaptive(c):
    """(colours [4, FH, FW, 3], counts [4, FH, FW]) of the adaptive frame's four samples in PERM16's order, and the mask [FH, FW] of
    the pixels shading_helpers.adaptive_reference refines from the first two"""
    rgb, cnt = ref_samples(c)
    cols = np.stack([rgb[j, i] for i, j in PERM16[:ADAPTIVE_MAX]])
    cnts = np.stack([cnt[j, i] for i, j in PERM16[:ADAPTIVE_MAX]])
    return cols, cnts, adaptive_reference(cols, ADAPTIVE_BASE, ADAPTIVE_THRESHOLD, False)[0]


def refine_rays(c):
    """the primary rays k_adaptive_refine traces: samples 2 and 3 of the pixels the reference refines"""
    sel = np.flatnonzero(ref_adaptive(c)[2].reshape(-1))
    cam = cam_frame(c)
    return np.concatenate([rr.camera_rays(cam, FW, FH, *OFFP16[s])[sel] for s in range(ADAPTIVE_BASE, ADAPTIVE_MAX)])


def ref_materials_rays(c):
    return _ref(c, "materials rays", lambda: MH.ref_shade(scene(c), caller_rays(c), TABLE, **params(c)))


def ref_materials_frame(c):
    return _ref(c, "materials frame", lambda: MH.ref_frame(scene(c), cam_frame(c), FW, FH, OFFP16[:2], TABLE, **params(c)))


def ref_nested_rays(c):
    return _ref(c, "nested rays", lambda: NH.ref_shade(scene(c), caller_rays(c), TABLE, **params(c)))


def ref_nested_frame(c):
    return _ref(c, "nested frame", lambda: NH.ref_frame(scene(c), cam_frame(c), FW, FH, OFFP16[:2], TABLE, **params(c)))


def ref_composed(c):
    iors, weights = bands()
    return _ref(c, "composed", lambda: CH.ref_composed(scene(c), cam_frame(c), FW, FH, composed_records(), LENS, TABLE, iors, weights, **params(c)))


def ref_shutter(c):
    iors, weights = bands()
    return _ref(c, "shutter", lambda: KH.ref_shutter([scene(c)], cam_frame(c), FW, FH, shutter_records(), LENS, TABLE, iors, weights, **params(c)))


def ref_surfaces_rays(c):
    return _ref(c, "surfaces rays", lambda: surfaces_fixture(c).ref(caller_rays(c), **params(c)))


def ref_surfaces_frame(c):
    return _ref(c, "surfaces frame", lambda: surfaces_fixture(c).frame(cam_frame(c), FW, FH, OFFP16[:2], **params(c)))
