"""GPU: every launchable instantiation of k_shade_rays_shadows, k_render_shadows and k_render_lit_shadows, once, at the deepest tree it
takes, with the walks of transparent shadows on the stack.

test_gpu_tree_matrix.py and test_gpu_lit_tree_matrix.py run the other fifteen ray-tree kernels on tree_matrix.CASES + BOUNDARIES; these
are the rows of the three new ones, all under shadow_steps K = 4:

  shade_rays_surfaces (48x32 caller rays)                        shadows_helpers.ref_shade
  render_surfaces (two samples)                          24x16   shadows_helpers.ref_frame
  render_lit (key 0, 4 records, 2 light offsets)         24x16   shadows_helpers.ref_lit

The fixture.  tree_matrix.surfaces_fixture gives no walk a glass hit: the one identity instance is opaque, and the two-level scenes'
glass chain stands beside the opaque one, where no shadow ray of either light reaches it (test_shadows_cpu.py shows both on the
CPU).  A third instance would deepen the top level, and with it rr_stats' depth, by one, and move every case off the rung it is in
the table for; so shadow_fixture keeps the scene's two instances, meshes, rows and masks and moves the glass one to stand between the
opaque chain and the lamp, whose shadow_mask meets it.  Then in every two-level case walks cross both faces of glass sheets and end
lit, others are stopped by the opaque chain's own sheets, and in the deep ones the cap of four ends some -- while sample 0 of every
RayGen still fills the stack of the rung (assert_rung).  Per case: rr_stats' depth is the case's need, the instantiation is the
model's, and float colours, RGBA8 and TraceRay counts equal the reference bit for bit."""
import numpy as np
import pytest

import lit_helpers as LH
import refraction_raytracing_dxr_amd as rr
import shadows_helpers as S
import test_gpu_stack_rungs as RUNGS
import tree_matrix as TM
from kernel_oracle_helpers import make_renderer  # noqa: F401  (a fixture)
from scenes import xf
from shading_helpers import OFFP16
from test_gpu_nested import check_rays
from test_gpu_samples import check
from test_gpu_stack_rungs import assert_rung
from tree_matrix import BOUNDARIES, CASES, FH, FW, LENS, TABLE, case_id

pytestmark = pytest.mark.gpu

K = 4
OUT = dict(rgba8=True, ray_counts=True)
GLASS_AT = xf(0.7, 0.3, 0.8, (0.6, 0.6, 0.6), 0.35)        # between the opaque chain (x 0.8, z 0.2) and tree_matrix.LAMP2
LIGHT_OFFSETS = np.array([[-1.0, 0.5], [-1.0, 0.5], [0.75, -1.0], [0.75, -1.0]], np.float32)
SHAPES = LH.shapes(rr.light_shape((0.0, 0.04, 0.0), (0.0, 0.0, 0.04)), rr.light_shape((0.05, 0.0, 0.0), (0.0, 0.05, 0.0)))
_scenes = {}
_refs = {}


def shadow_scene(c):
    """tree_matrix.scene(c); a two-level one with its glass instance at GLASS_AT"""
    base = TM.scene(c)
    if base.single:
        return base
    key = "shadow-" + base.key
    if key not in _scenes:
        inst = base.instances.copy()
        inst["transform"][0] = np.asarray(GLASS_AT, np.float32).reshape(inst["transform"][0].shape)
        _scenes[key] = RUNGS.RungScene(key, base.meshes, RUNGS.ENV, inst)
    return _scenes[key]


def shadow_fixture(c):
    """tree_matrix.surfaces_fixture(c) on shadow_scene(c), under the cap K"""
    fx = TM.surfaces_fixture(c)
    return S.Fixture(shadow_scene(c), fx.surf, fx.lights, fx.ambient, K, fx.table)


def lit_records():
    s = TM.shutter_records()
    return LH.records(s["offset"], s["lens_offset"], s["band"], s["key"], LIGHT_OFFSETS)


def _ref(c, what, make):
    key = (shadow_scene(c).key, c.max_reflect, what)
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def ref_rays(c):
    return _ref(c, "rays", lambda: shadow_fixture(c).ref(TM.caller_rays(c), **TM.params(c)))


def ref_frame(c):
    return _ref(c, "frame", lambda: shadow_fixture(c).frame(TM.cam_frame(c), FW, FH, OFFP16[:2], **TM.params(c)))


def ref_lit(c):
    fx = shadow_fixture(c)
    iors, weights = TM.bands()
    return _ref(c, "lit", lambda: S.ref_lit([fx.scene], TM.cam_frame(c), FW, FH, lit_records(), LENS, TABLE, fx.surf, fx.lights, SHAPES, fx.ambient, K,
                                            iors, weights, **TM.params(c)))


def walks_through_glass(tl):
    return tl.walk_lit_glass[1] + tl.walk_lit_glass[2] + tl.walk_occluded_after_glass + tl.walk_capped


@pytest.mark.parametrize("c", CASES + BOUNDARIES, ids=case_id)
def test_the_shadow_kernels_on_the_instantiation(make_renderer, c):
    r = make_renderer("fused", **c.env)
    sc = shadow_scene(c)
    sc.load_gpu(r)
    assert r.stats().bvh_depth == c.need
    rays = TM.raygen_rays(c)
    for bundle in ("pinhole", "sample 0", "lens sample 0"):
        assert_rung(r, sc, c.need, rays[bundle])
    n_inst = 1 if sc.single else len(sc.instances)
    counts = (sc.n_tris(), 0, 0) if sc.single else (0, len(sc.nodes), sc.n_tris() + n_inst)
    dbg_stack, tlas32 = int(c.env.get("RR_DEBUG_STACK", 0)), int(c.env.get("RR_DEBUG_TLAS32", 0))
    assert TM.expected_variant(sc.single, r.stats().bvh_depth, c.max_reflect, dbg_stack, tlas32, counts=counts) == c.variant
    fx = shadow_fixture(c)
    r.set_materials(TABLE)
    r.set_surfaces(fx.surf)
    r.set_lights(fx.lights, fx.ambient)
    r.set_shadow_steps(K)
    p = rr.default_params(**TM.params(c))
    # k_shade_rays_shadows
    ref = ref_rays(c)
    tl = ref[3]
    assert tl.walks > 0 and tl.shadow_occluded > 0 and tl.shadow_lit > 0 and tl.specular_children > 0, tl
    assert sc.single or tl.walk_lit_glass[2] > 0, tl
    check_rays(r.shade_rays_surfaces(TM.caller_rays(c), p, **OUT), ref)
    # k_render_shadows
    rgb, cnt, ftl = ref_frame(c)
    assert ftl.walks > 0
    check(r.render_surfaces(FW, FH, TM.cam_frame(c), OFFP16[:2], p, **OUT), rgb, cnt, False)
    # k_render_lit_shadows
    r.set_material_bands(*TM.bands())
    r.set_light_shapes(SHAPES)
    r.capture_scene_key(0)
    assert r.scene_key_info(0).stack_need == c.need
    rgb, cnt, _, extras = ref_lit(c)
    assert sum(e[2].walks for e in extras) > 0 and sum(e[2].opaque_hits for e in extras) > 0
    check(r.render_lit(FW, FH, TM.cam_frame(c), lit_records(), lens=LENS, params=p, **OUT), rgb, cnt, False)


def test_over_the_matrix_the_walks_cross_glass():
    """the reference's tallies of the caller rays, summed over the cases: walks lit through two glass hits, walks an opaque row stops,
    walks of one call and walks the cap ends"""
    total = S.Tallies()
    for c in CASES + BOUNDARIES:
        S.add_tallies(total, ref_rays(c)[3])
    print(total)
    assert total.walk_lit_glass[2] > 0 and total.walk_lit_glass[1] > 0 and total.walk_capped > 0 and total.walk_calls[1] > 0 and total.shadow_occluded > 0
    assert walks_through_glass(total) >= 100
