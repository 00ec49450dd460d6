"""tree_matrix.py on the CPU: the case table against csrc/rr_choice.cpp, and what the references alone say about every case, so that
both are known before any GPU run (test_gpu_tree_matrix.py).

Completeness: through tests/native/kernel_choice_driver.cpp every case resolves to the instantiation it names, the 20 of them are
codeobj.LAUNCHABLE exactly, and every boundary resolves to its own, which its neighbour one level shallower does not.

Conditions, with the views, frame sizes, tables and lights the GPU module uses: the rays of every RayGen's sample 0 fill the stack of
depth_meshes.ploc_model's hierarchy of the chain to need - 1 entries (the GPU module asserts the same on the downloaded tree); the
references' TraceRay counts show hits on at least 100 of the 48x32 caller rays of one identity instance and on at least 10 pixels of
every frame of a two-level scene (its chains are scaled to 0.6 and stand to either side of the middle); the surfaces reference occludes
and lights shadow rays and spawns mirror children; the nested reference meets interfaces and passes; under
tree_matrix.ADAPTIVE_THRESHOLD the oracle's frame has at least 10 pixels that the adaptive rule refines and 10 that it leaves, and the
later samples of the refined ones -- the only rays k_adaptive_refine traces -- fill the model's stack too.  The references of render_lens
and render_spectral are folds of the GPU's own shade_rays (test_gpu_lens.py, test_gpu_spectral.py): what they must show, more than one
ray per sample on at least 10 pixels, is asserted in the GPU module and cannot be here."""
import pytest

import tree_matrix as TM
from codeobj import LAUNCHABLE
from tree_matrix import BOUNDARIES, CASES, case_id

ALL = CASES + BOUNDARIES


def test_the_cases_are_the_launchable_instantiations():
    got = TM.expected_variants([TM.case_query(c) for c in CASES])
    assert got == [c.variant for c in CASES], [(case_id(c), g) for c, g in zip(CASES, got) if g != c.variant]
    assert len(CASES) == 20 and len(set(got)) == 20 and set(got) == set(LAUNCHABLE) and len(LAUNCHABLE) == 20


def test_every_boundary_hands_over():
    here = TM.expected_variants([TM.case_query(c) for c in BOUNDARIES])
    below = TM.expected_variants([TM.case_query(TM.shallower(c)) for c in BOUNDARIES])
    assert here == [c.variant for c in BOUNDARIES], [(case_id(c), g) for c, g in zip(BOUNDARIES, here) if g != c.variant]
    for c, h, b in zip(BOUNDARIES, here, below):
        assert h != b and b in LAUNCHABLE and h in LAUNCHABLE, (case_id(c), h, b)
        # the neighbour is a case of the table: the rung below at its deepest tree (one instance at need 19 runs on the 19-entry build)
        assert any(k.variant == b and k.need == c.need - 1 and k.single == c.single for k in CASES), (case_id(c), b)
    assert sorted((c.single, c.need, int(c.env.get("RR_DEBUG_TLAS32", 0))) for c in BOUNDARIES) == sorted(
        [(True, 20, 0), (True, 40, 0), (False, 31, 0), (False, 40, 0)] + [(False, n, 1) for n in (20, 27, 32, 40)])


def test_a_loaded_scenes_counts_change_nothing():
    """expected_variant with counts of its caller's (the GPU module passes those of the loaded scene) and with the chain's own: a few
    dozen triangles, nodes and references are far from where 16-bit stack entries end, one more of each changes nothing"""
    for c in (CASES[0], CASES[10], BOUNDARIES[2]):
        q = TM.case_query(c)[:5]
        tris, nodes, refs = TM.chain_counts(c.single, c.need)
        assert TM.expected_variant(*q, counts=(tris + 1, nodes + 1, refs + 1)) == TM.expected_variant(*q) == c.variant
    # and where they end: the same two-level scene with a pool of 32 768 nodes runs on 32-bit entries
    c = CASES[10]
    assert TM.expected_variant(*TM.case_query(c)[:5], counts=(0, 32768, 30)) == (31, 2, True, TM.U32)


@pytest.mark.parametrize("c", ALL, ids=case_id)
def test_sample_0_of_every_raygen_fills_the_models_stack(c):
    blas = c.need if c.single else c.need - TM.RUNGS.TLAS_DEPTH
    for name, rays in TM.raygen_rays(c).items():
        assert TM.model_high_water(c, rays) == blas - 1, (name, TM.model_high_water(c, rays), blas - 1)


@pytest.mark.parametrize("c", ALL, ids=case_id)
def test_the_adaptive_rule_refines_pixels_whose_later_samples_fill_the_stack(c):
    """without a refined pixel k_adaptive_refine returns before its first ray_tree call"""
    cols, cnts, mask = TM.ref_adaptive(c)
    assert cols.shape == (TM.ADAPTIVE_MAX, TM.FH, TM.FW, 3) and cnts.shape == (TM.ADAPTIVE_MAX, TM.FH, TM.FW)
    assert int(mask.sum()) >= 10 and int((~mask).sum()) >= 10, (int(mask.sum()), mask.size)
    assert int((cnts[TM.ADAPTIVE_BASE:][:, mask] > 1).sum()) >= 10          # the refine samples hit the chain, they are not all Misses
    rays = TM.refine_rays(c)
    assert len(rays) == (TM.ADAPTIVE_MAX - TM.ADAPTIVE_BASE) * int(mask.sum())
    blas = c.need if c.single else c.need - TM.RUNGS.TLAS_DEPTH
    assert TM.model_high_water(c, rays) == blas - 1, (TM.model_high_water(c, rays), blas - 1)


@pytest.mark.parametrize("c", ALL, ids=case_id)
def test_the_references_conditions(c):
    n_rays, n_frame, n_recs = (100, 10, 10) if c.single else (10, 10, 10)
    rgb, cnt = TM.ref_samples(c)
    assert int(((cnt[0, 1] + cnt[1, 3]) > 2).sum()) >= n_frame                 # render_samples' two samples, PERM16[:2]
    rays = {"oracle": TM.ref_oracle_counts(c).reshape(-1), "materials": TM.ref_materials_rays(c)[2], "nested": TM.ref_nested_rays(c)[2],
            "surfaces": TM.ref_surfaces_rays(c)[2]}
    for name, cnt in rays.items():
        assert int((cnt > 1).sum()) >= n_rays, (name, int((cnt > 1).sum()))
    frames = {"materials": TM.ref_materials_frame(c)[1], "nested": TM.ref_nested_frame(c)[1], "surfaces": TM.ref_surfaces_frame(c)[1]}
    for name, cnt in frames.items():
        assert cnt.shape == (TM.FH, TM.FW) and int((cnt > 2).sum()) >= n_frame, (name, int((cnt > 2).sum()))
    for name, ref in (("composed", TM.ref_composed(c)), ("shutter", TM.ref_shutter(c))):
        assert int((ref[1] > 4).sum()) >= n_recs, (name, int((ref[1] > 4).sum()))
        assert ref[2][0].tobytes() != ref[2][1].tobytes()       # the two bands give the first position two colours
    tl = TM.ref_surfaces_rays(c)[3]
    assert tl.shadow_occluded > 0 and tl.shadow_lit > 0 and tl.specular_children > 0, tl
    assert tl.light_used[0] > 0 and tl.light_used[1] > 0, tl
    tl = TM.ref_nested_rays(c)[3]
    assert tl.interfaces > 0 and tl.passes > 0, tl
    for tl in TM.ref_composed(c)[3] + TM.ref_shutter(c)[3]:
        assert tl.interfaces > 0 and tl.passes > 0, tl
