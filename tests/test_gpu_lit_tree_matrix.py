"""GPU: every launchable instantiation of k_render_lit, once, at the deepest tree it takes, with shadow rays on the stack.

test_gpu_tree_matrix.py runs the other fourteen ray-tree kernels on tree_matrix.CASES + BOUNDARIES; this is its row for the fifteenth:

  render_lit (the scene as key 0, 4 records, 2 light offsets)   24x16   lit_helpers.ref_lit

Per case the chain scene is loaded, tree_matrix.surfaces_fixture(c) set -- the opaque, specular chain under its two lights, which
test_tree_matrix_cpu.py shows to trace shadow rays occluded and lit --, the lights given a small shape each, key 0 captured, and
render_lit called with tree_matrix.shutter_records() under the case's lens and bands, the first two records at one light offset and
the last two at another.  Float colours, RGBA8 and TraceRay counts are compared bit for bit with the CPU fold.  As there: rr_stats'
depth is the case's need, sample 0 of the lens fills the stack (assert_rung), and the instantiation is the model's."""
import numpy as np
import pytest

import lit_helpers as LH
import refraction_raytracing_dxr_amd as rr
import tree_matrix as TM
from kernel_oracle_helpers import make_renderer  # noqa: F401  (a fixture)
from test_gpu_samples import check
from test_gpu_stack_rungs import assert_rung
from tree_matrix import BOUNDARIES, CASES, FH, FW, LENS, TABLE, case_id

pytestmark = pytest.mark.gpu

OUT = dict(rgba8=True, ray_counts=True)
LIGHT_OFFSETS = np.array([[-1.0, 0.5], [-1.0, 0.5], [0.75, -1.0], [0.75, -1.0]], np.float32)
SHAPES = LH.shapes(rr.light_shape((0.0, 0.04, 0.0), (0.0, 0.0, 0.04)), rr.light_shape((0.05, 0.0, 0.0), (0.0, 0.05, 0.0)))
_refs = {}


def lit_records():
    s = TM.shutter_records()
    return LH.records(s["offset"], s["lens_offset"], s["band"], s["key"], LIGHT_OFFSETS)


def ref_lit(c):
    key = (TM.scene(c).key, c.max_reflect)
    if key not in _refs:
        fx = TM.surfaces_fixture(c)
        iors, weights = TM.bands()
        _refs[key] = LH.ref_lit([fx.scene], TM.cam_frame(c), FW, FH, lit_records(), LENS, TABLE, fx.surf, fx.lights, SHAPES, fx.ambient, iors, weights,
                                **TM.params(c))
    return _refs[key]


@pytest.mark.parametrize("c", CASES + BOUNDARIES, ids=case_id)
def test_render_lit_on_the_instantiation(make_renderer, c):
    r = make_renderer("fused", **c.env)
    sc = TM.scene(c)
    sc.load_gpu(r)
    assert r.stats().bvh_depth == c.need
    assert_rung(r, sc, c.need, TM.raygen_rays(c)["lens sample 0"])
    n_inst = 1 if sc.single else len(sc.instances)
    counts = (sc.n_tris(), 0, 0) if sc.single else (0, len(sc.nodes), sc.n_tris() + n_inst)
    dbg_stack, tlas32 = int(c.env.get("RR_DEBUG_STACK", 0)), int(c.env.get("RR_DEBUG_TLAS32", 0))
    assert TM.expected_variant(sc.single, r.stats().bvh_depth, c.max_reflect, dbg_stack, tlas32, counts=counts) == c.variant
    fx = TM.surfaces_fixture(c)
    r.set_materials(TABLE)
    r.set_material_bands(*TM.bands())
    r.set_surfaces(fx.surf)
    r.set_lights(fx.lights, fx.ambient)
    r.set_light_shapes(SHAPES)
    r.capture_scene_key(0)
    assert r.scene_key_info(0).stack_need == c.need
    rgb, cnt, _, extras = ref_lit(c)
    assert sum(e[2].shadow_traced for e in extras) > 0 and sum(e[2].opaque_hits for e in extras) > 0
    check(r.render_lit(FW, FH, TM.cam_frame(c), lit_records(), lens=LENS, params=rr.default_params(**TM.params(c)), **OUT), rgb, cnt, False)
