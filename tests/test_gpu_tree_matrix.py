"""GPU: every launchable instantiation of every ray-tree kernel, once, at the deepest tree it takes.

k_shade_rays, k_render_samples, k_adaptive_base, k_adaptive_refine, k_render_lens, k_render_spectral, k_shade_rays_mat,
k_render_materials, k_shade_rays_nested, k_render_nested, k_render_composed, k_render_shutter, k_shade_rays_surfaces and
k_render_surfaces are each built as the 20 instantiations of codeobj.LAUNCHABLE, 280 device functions with a register allocation,
a scratch and an LDS footprint of their own, and none of them checks its stack.  tree_matrix.CASES reaches each of the 20 with a chain
of test_gpu_stack_rungs.py exactly as deep as the instantiation's stack allows; tree_matrix.BOUNDARIES are the trees one level deeper,
where the next one must have taken over.  Per case the scene is loaded once.  First
  * rr_stats.bvh_depth == need, and assert_rung: the downloaded tree has the depth and sample 0 of each RayGen -- the pinhole rays of
    the 48x32 view, sample 0 of the 24x16 frames, lens sample 0 through the lens centre -- fills its stack to need - 1 entries;
  * tree_matrix.expected_variant (csrc/rr_choice.cpp itself, through the test driver) of the loaded scene's facts is the case's
    instantiation.  The library has no kernel-name slot for ray-tree calls, and the suite asserts that they leave rr_stats
    untouched: the instantiation is known from this model, the test cannot observe it.  test_kernel_choice.py holds the model to
    the written-out ladder, each family's CPU test (test_shade_abi.py, test_samples_abi.py, ...) its 20 symbols to the code object;
then every ray-tree call is made once with max_refract 5 and the case's max_reflect (3: the builds with eight parked rays), and its
float colours, RGBA8 and TraceRay counts are compared bit for bit with the reference its own test file uses:

  call                                              size           reference
  shade_rays                                        48x32 rays     shading_helpers.check_against_oracle (the CPU oracle's frame)
  render_samples (2), render_adaptive (2 of 4)      24x16          the oracle's 96x64 frame, as test_gpu_stack_rungs.check_ray_trees
                                                                   (the threshold is tree_matrix.ADAPTIVE_THRESHOLD, at which the oracle
                                                                   refines pixels in every case: k_adaptive_refine traces only those)
  render_lens (2 samples, lens sample 0 centred)    24x16          test_gpu_lens.check_composition
  render_spectral (2 bands)                         24x16          test_gpu_spectral.check_composition
  shade_rays_materials, render_materials (2)        48x32, 24x16   materials_helpers.ref_shade / ref_frame
  shade_rays_nested, render_nested (2)              48x32, 24x16   nested_helpers.ref_shade / ref_frame
  render_composed (lens, 2 bands, 4 records)        24x16          composed_helpers.ref_composed
  render_shutter (the scene as key 0, 4 records)    24x16          shutter_helpers.ref_shutter
  shade_rays_surfaces, render_surfaces (2)          48x32, 24x16   surfaces_helpers.ref_shade / ref_frame

No case leaves a call out.  What the references must show for the comparison to mean something -- hits, shadow rays occluded and
lit, mirror children, interfaces and passes, pixels the adaptive rule refines and pixels it leaves -- test_tree_matrix_cpu.py asserts
from the references alone.  The references of render_lens and render_spectral are folds of this GPU's own shade_rays, as their test
files have it, so their conditions (more than one ray per sample on at least 10 pixels) can only be asserted here.

What a case can and cannot see is what test_gpu_stack_rungs.py says of a rung: the deepest walk fills all but one entry of the
instantiation's stack, so a stack two entries short, spill code that loses a live value on the deep path, or an LDS size that
does not match the instantiation corrupts a neighbouring wave's stack or the ray's own state and the frames differ; a stack exactly
one entry short still holds the walk.  shade_rays is held to the oracle on the pinhole rays only: an error in the ray_tree code it
shares with k_render_lens and k_render_spectral that shows only on off-centre lens rays or at a band's index of refraction is on both
sides of those two comparisons and cancels (k_render_composed and k_render_shutter trace such rays against the CPU reference).

Run time on an MI355X: 0.04 to 0.12 s per case, the CPU references included (they are shared between the cases of one chain and
max_reflect); the first case of a process also builds the choice driver and the references' C helpers."""
import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
import tree_matrix as TM
from kernel_oracle_helpers import make_renderer  # noqa: F401  (a fixture)
from shading_helpers import OFFP16, PERM16, fold
from shading_helpers import check_against_oracle as check_shade
from test_gpu_adaptive import follows_the_rule
from test_gpu_lens import check_composition as check_lens
from test_gpu_nested import check_rays
from test_gpu_samples import check
from test_gpu_spectral import check_composition as check_spectral
from test_gpu_stack_rungs import assert_rung
from tree_matrix import BOUNDARIES, CASES, FH, FW, H, LENS, TABLE, W, case_id

pytestmark = pytest.mark.gpu

OUT = dict(rgba8=True, ray_counts=True)


@pytest.mark.parametrize("c", CASES + BOUNDARIES, ids=case_id)
def test_every_ray_tree_call_on_the_instantiation(make_renderer, c):
    r = make_renderer("fused", **c.env)
    sc = TM.scene(c)
    sc.load_gpu(r)
    assert r.stats().bvh_depth == c.need
    for rays in TM.raygen_rays(c).values():
        assert_rung(r, sc, c.need, rays)
    n_inst = 1 if sc.single else len(sc.instances)
    counts = (sc.n_tris(), 0, 0) if sc.single else (0, len(sc.nodes), sc.n_tris() + n_inst)
    dbg_stack, tlas32 = int(c.env.get("RR_DEBUG_STACK", 0)), int(c.env.get("RR_DEBUG_TLAS32", 0))
    assert TM.expected_variant(sc.single, r.stats().bvh_depth, c.max_reflect, dbg_stack, tlas32, counts=counts) == c.variant
    kw = TM.params(c)
    p = rr.default_params(**kw)
    s = sc.oracle()
    rays, cam_r, cam = TM.caller_rays(c), TM.cam_rays(c), TM.cam_frame(c)

    # k_shade_rays; k_render_samples, k_adaptive_base and k_adaptive_refine as test_gpu_stack_rungs.check_ray_trees holds them to the oracle
    ref = check_shade(r, s, np.array(cam_r.proj_inv, np.float32), np.array(cam_r.camera_loc, np.float32), W, H, rays, **kw)
    assert ref["stats"].hits > 0
    rgb, cnt = TM.ref_samples(c)
    got = r.render_samples(FW, FH, cam, OFFP16[:2], p, **OUT)
    check(got, fold([rgb[j, i] for i, j in PERM16[:2]]), sum(cnt[j, i] for i, j in PERM16[:2]), False)
    # (k_adaptive_refine traces only the pixels the rule refines: the reference's mask is not empty, and their later samples fill the stack)
    cols, cnts, want_mask = TM.ref_adaptive(c)
    assert want_mask.sum() > 0
    assert_rung(r, sc, c.need, TM.refine_rays(c))
    got = r.render_adaptive(FW, FH, cam, (TM.ADAPTIVE_BASE, OFFP16[:TM.ADAPTIVE_MAX]), TM.ADAPTIVE_THRESHOLD, p, sample_counts=True, **OUT)
    mask = follows_the_rule(got, cols, cnts, TM.ADAPTIVE_BASE, TM.ADAPTIVE_THRESHOLD, False)
    assert mask.sum() > 0 and np.array_equal(mask, want_mask)

    # k_render_lens, k_render_spectral: the folds of shade_rays
    assert (check_lens(r, cam, FW, FH, LENS, OFFP16[:2], TM.LOFF2, **kw) > 2).sum() >= 10
    assert (check_spectral(r, cam, FW, FH, TM.BANDS2, OFFP16[:2], True, **kw) > 2).sum() >= 10

    # k_shade_rays_mat, k_render_materials; k_shade_rays_nested, k_render_nested
    r.set_materials(TABLE)
    check_rays(r.shade_rays_materials(rays, p, **OUT), TM.ref_materials_rays(c))
    want = TM.ref_materials_frame(c)
    check(r.render_materials(FW, FH, cam, OFFP16[:2], p, **OUT), want[0], want[1], False)
    check_rays(r.shade_rays_nested(rays, p, **OUT), TM.ref_nested_rays(c))
    want = TM.ref_nested_frame(c)
    check(r.render_nested(FW, FH, cam, OFFP16[:2], p, **OUT), want[0], want[1], False)

    # k_render_composed; k_render_shutter with the scene captured as key 0
    r.set_material_bands(*TM.bands())
    want = TM.ref_composed(c)
    check(r.render_composed(FW, FH, cam, TM.composed_records(), lens=LENS, params=p, **OUT), want[0], want[1], False)
    r.capture_scene_key(0)
    assert r.scene_key_info(0).stack_need == c.need
    want = TM.ref_shutter(c)
    check(r.render_shutter(FW, FH, cam, TM.shutter_records(), lens=LENS, params=p, **OUT), want[0], want[1], False)
    r.set_material_bands(None)

    # k_shade_rays_surfaces, k_render_surfaces: shadow rays on the same stacks
    fx = TM.surfaces_fixture(c)
    r.set_surfaces(fx.surf)
    r.set_lights(fx.lights, fx.ambient)
    check_rays(r.shade_rays_surfaces(rays, p, **OUT), TM.ref_surfaces_rays(c))
    want = TM.ref_surfaces_frame(c)
    check(r.render_surfaces(FW, FH, cam, OFFP16[:2], p, **OUT), want[0], want[1], False)
