"""CPU: transparent shadows -- the conditions the GPU fixtures are chosen for, read from the tallies of the reference restatement
(tests/native/shadows_ref.c); closed forms in float64 that no reference takes part in; the reference's reductions to
surfaces_ref.c; and the new kernels in the code object, with the figures DESIGN 5.17 records."""
import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
import shadows_helpers as S
import surfaces_helpers as SH
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from test_shutter_cpu import _register_counts

KW = dict(max_refract=8, max_reflect=2)
TOL = 1e-4                                                  # the closed forms, relative


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def same(a, b):
    return bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------- (a) the fixtures' conditions
@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_a_fixture_meets_its_condition(name):
    """tinted: walks lit through two glass hits, walks an opaque row stops after glass, walks of one call; drink and deep-drink:
    walks that start with a list of two and of three media; capped: walks the cap of two calls ends"""
    for ml in (2, 3):
        fx, rays, ref = S.fixture_ref(name, ml)
        print(name, ml, ref[3])
        assert S.fixture_condition(name, ref[3]), ref[3]
        assert (ref[2] > 1).mean() > 0.05


def test_tinted_lights_both_see_the_sphere_and_the_tint_shows():
    """both masks are 0xff and the sphere (instance 1, mask 0x02) is a glass row with sigma_a != 0; the walks change only pixels
    whose first-hit shadow ray the sphere stopped: brighter than under K = 0, never beyond the frame with the sphere's mask taken from
    the lights, and red, which the sphere's glass absorbs least, gains most"""
    fx, rays, ref = S.fixture_ref("tinted", 2)
    assert list(fx.lights["shadow_mask"]) == [0xff, 0xff] and fx.surf["kind"][1] == rr.SURFACE_GLASS and (fx.table["sigma_a"][1] > 0).all()
    black = fx.ref(rays, k=0, **KW)
    blind = fx.lights.copy()
    blind["shadow_mask"] = 0x01                             # the floor and the occluder, not the sphere
    clear = fx.ref(rays, lts=blind, k=0, **KW)
    changed = (ref[0] != black[0]).any(axis=1)
    assert changed.sum() >= 5
    assert np.all(ref[0] >= black[0]) and np.all(ref[0] <= clear[0])
    gain = (ref[0][changed] - black[0][changed]).sum(axis=0)
    assert gain[0] > gain[1] > gain[2] > 0, gain


# ------------------------------------------------------------------------------------------------- (b) closed forms
ALBEDO = np.array((0.7, 0.6, 0.5))
AMB = np.array((0.05, 0.06, 0.08), np.float32)
RAD = np.array((1.2, 1.1, 0.9), np.float32)
CHORD = 0.4                                                 # the hovering cube's side: cube.obj's 2 under a scale of 0.2


def through_the_cube():
    """the weight the ray of down_ray(1.0) reaches the floor with at max_reflect 0: it enters and leaves the hovering cube at normal
    incidence, (1 - R) at either face with R = R0 (1 - R0) 2^5, and is absorbed over the chord between them"""
    R0 = (0.2 / 2.2) ** 2
    R = R0 * (1.0 - R0) * 32.0
    return (1.0 - R) ** 2 * np.exp(-np.array(S.CF_SIGMA, np.float64) * CHORD)


def cf_shade(x, k, lts):
    sc, surf, table = S.cf_glass_cube(ALBEDO)
    return S.ref_shade(sc, SH.down_ray(x), table, surf, lts, AMB, k, max_refract=8, max_reflect=0)


def test_closed_form_shadow_of_a_tinted_cube():
    """straight down onto the floor y = 0 under the cube, the light straight up: the walk meets the cube's bottom at 0.8, its top 0.4
    further on and then nothing -- three calls.  With K >= 3 the floor is albedo * (ambient + radiance * exp(-sigma * 0.4)); no
    absorption, the absorption twice, and swapped channels are all tens of percent away"""
    up = SH.lights(rr.directional_light((0, 1, 0), RAD, 0xff))
    sigma = np.array(S.CF_SIGMA, np.float64)
    want = ALBEDO * (AMB.astype(np.float64) + RAD.astype(np.float64) * np.exp(-sigma * CHORD))
    for k in (3, 4, 16):
        rgb, _, cnt, tl = cf_shade(1.0, k, up)
        floor = rgb[0].astype(np.float64) / through_the_cube()
        print("K = %d: floor %s, closed form %s" % (k, floor.tolist(), want.tolist()))
        assert cnt[0] == 3 + 3 and tl.walk_calls[3] == 1 and tl.walk_lit_glass[2] == 1 and tl.walk_absorbed == 1
        assert np.all(np.abs(floor - want) <= TOL * want)
    for wrong in (ALBEDO * (AMB + RAD.astype(np.float64)), ALBEDO * (AMB + RAD * np.exp(-sigma * 2 * CHORD)), ALBEDO * (AMB + RAD * np.exp(-sigma[::-1] * CHORD))):
        assert np.any(np.abs(wrong - want) > 0.1 * want)


def test_closed_form_the_cap_is_conservative():
    """K = 2 ends the same walk at the cube's top, occluded: the floor is albedo * ambient EXACTLY -- the bits of the frame with no
    light at all, and of K = 0 and K = 1, whose shadow ray the cube stops"""
    up = SH.lights(rr.directional_light((0, 1, 0), RAD, 0xff))
    rgb, _, cnt, tl = cf_shade(1.0, 2, up)
    assert cnt[0] == 3 + 2 and tl.walk_capped == 1 and tl.shadow_occluded == 1
    dark = cf_shade(1.0, 2, None)
    assert dark[2][0] == 3 and bits_equal(rgb, dark[0])
    for k in (0, 1):
        assert bits_equal(cf_shade(1.0, k, up)[0], rgb)
    floor = rgb[0].astype(np.float64) / through_the_cube()
    assert np.all(np.abs(floor - ALBEDO * AMB) <= TOL * ALBEDO * AMB)


def test_closed_form_away_from_the_cube_nothing_changes():
    """down_ray(-1.0): the walk's first call misses, and every K gives the K = 0 colour bit for bit"""
    up = SH.lights(rr.directional_light((0, 1, 0), RAD, 0xff))
    base = cf_shade(-1.0, 0, up)
    assert base[2][0] == 2 and base[3].shadow_lit == 1
    want = ALBEDO * (AMB.astype(np.float64) + RAD)
    assert np.all(np.abs(base[0][0] - want) <= TOL * want)
    for k in (1, 2, 3, 16):
        got = cf_shade(-1.0, k, up)
        assert same(got, base) and got[3].walk_calls[1] == 1


# ------------------------------------------------------------------------------------------------- (c) the reference's reductions
@pytest.mark.parametrize("name", sorted(SH.FIXTURES))
def test_one_call_is_the_first_hit_shadow_ray(name):
    """K = 1 (and K = 0, the same text as surfaces_ref.c) against surfaces_helpers.ref_shade on its six fixtures: colours, RGBA8 and
    TraceRay counts bit for bit"""
    for ml in (2, 3):
        fx, rays, want = SH.fixture_ref(name, ml)
        for k in (0, 1):
            got = S.ref_shade(fx.scene, rays, fx.table, fx.surf, fx.lights, fx.ambient, k, max_refract=8, max_reflect=ml)
            assert same(got, want), (name, ml, k)
            assert (got[3].shadow_occluded, got[3].shadow_lit, got[3].opaque_hits) == (want[3].shadow_occluded, want[3].shadow_lit, want[3].opaque_hits)


@pytest.mark.parametrize("name", ["alone", "lamp", "table-0x01"])
def test_eight_calls_change_nothing_where_no_first_hit_is_glass(name):
    """alone: one opaque instance; lamp: no light; table with the lamp's mask 0x01, like the sun's: no shadow ray sees the sphere"""
    if name == "table-0x01":
        fx = SH.table()
        fx.lights["shadow_mask"][1] = 0x01
        from materials_helpers import H, W, view
        rays = rr.camera_rays(view(*SH.VIEW), W, H)
        want = fx.ref(rays, **KW)
        assert want[3].shadow_occluded > 0 and want[3].shadow_lit > 0
    else:
        fx, rays, want = SH.fixture_ref(name, 2)
    got = S.ref_shade(fx.scene, rays, fx.table, fx.surf, fx.lights, fx.ambient, 8, **KW)
    assert same(got, want)
    assert got[3].walks == want[3].shadow_traced and sum(got[3].walk_calls[2:]) == 0 and got[3].walk_lit_glass[1] == got[3].walk_lit_glass[2] == 0


# ------------------------------------------------------------------------------------------------- (d) the tree matrix's fixture
def _distinct_cases():
    import test_gpu_shadows_tree_matrix as M
    import tree_matrix as TM
    seen = {}
    for c in TM.CASES + TM.BOUNDARIES:
        seen.setdefault((M.shadow_scene(c).key, c.max_reflect), c)
    return M, TM, list(seen.values())


def test_the_tree_matrix_fixture_as_it_is_gives_no_walk_a_glass_hit():
    """tree_matrix.surfaces_fixture under K = 4: every walk is one call -- a miss or an opaque row -- in every case, which is why
    test_gpu_shadows_tree_matrix.py moves the two-level scenes' glass instance into the lamp's light"""
    M, TM, cases = _distinct_cases()
    for c in cases:
        fx = TM.surfaces_fixture(c)
        tl = S.ref_shade(fx.scene, TM.caller_rays(c), fx.table, fx.surf, fx.lights, fx.ambient, M.K, **TM.params(c))[3]
        assert tl.walks > 0 and tl.walk_calls[1] == tl.walks and M.walks_through_glass(tl) == 0, (TM.case_id(c), tl)


def test_the_moved_glass_chain_is_walked_through_and_the_rungs_stay_filled():
    """test_gpu_shadows_tree_matrix.shadow_fixture: in every two-level case walks lit through both faces of a glass sheet, shadow rays
    occluded and lit and mirror children as before; sample 0 of every RayGen still fills the model's stack to the rung's last entry"""
    from depth_meshes import stack_high_water, to_object_space
    M, TM, cases = _distinct_cases()
    for c in cases:
        tl = M.ref_rays(c)[3]
        print(TM.case_id(c), tl)
        assert tl.shadow_occluded > 0 and tl.shadow_lit > 0 and tl.specular_children > 0 and tl.light_used[0] > 0 and tl.light_used[1] > 0, tl
        assert (M.ref_rays(c)[2] > 1).sum() >= 10
        if c.single:
            continue
        assert tl.walk_lit_glass[2] > 0 and tl.walk_absorbed > 0, (TM.case_id(c), tl)
        sc, nodes, blas = M.shadow_scene(c), TM.model_nodes(c), c.need - TM.RUNGS.TLAS_DEPTH
        assert len(sc.instances) == 2 and sc.instances["transform"][1].tobytes() == TM.scene(c).instances["transform"][1].tobytes()
        for name, rays in TM.raygen_rays(c).items():
            high = max(int(stack_high_water(nodes, to_object_space(rays, t)).max()) for t in sc.instances["transform"])
            assert high == blas - 1, (TM.case_id(c), name, high)
    M.test_over_the_matrix_the_walks_cross_glass()


# ------------------------------------------------------------------------------------------------- (e) the code object
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_shadow_kernels_exist(tmp_path):
    """every instantiation of the three walk kernels and of their twins the host can launch is in the gfx950 code object exactly once; lane moves, scratch
    instructions and register counts are printed next to the twin's (no assertion on the counts: DESIGN 5.17 records them)"""
    k = kernels(tmp_path)
    regs = _register_counts(tmp_path / "co")
    for new, twin in (("k_shade_rays_shadows", "k_shade_rays_surfaces"), ("k_render_shadows", "k_render_surfaces"), ("k_render_lit_shadows", "k_render_lit")):
        for name in (new, twin):                                # (the pair shares one source file and one body)
            assert len([n for n in k if name + "<" in n]) == len(LAUNCHABLE), name
        for variant in LAUNCHABLE:
            args = template_args(*variant)
            for name in (new, twin):
                got = [(n, v) for n, v in k.items() if "rr::" + name + args in n]
                assert len(got) == 1, (name, args, got)
                r = [c for m, c in regs.items() if "rr::" + name + args in m]
                print("%s%s: %d lane moves, %d scratch instructions%s" % (name, args, got[0][1]["lane"], got[0][1]["scratch"],
                      ", %d SGPRs, %d VGPRs, %d bytes of scratch per lane" % r[0] if r else ""))
