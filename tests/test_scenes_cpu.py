"""CPU: the shared helpers of tests/scenes.py give the inputs the suite has always used, and their checks still fail when they should.

The digests below were recorded from the helper copies that scenes.py replaced (test_gpu_parity.py, test_gpu_refit.py,
query_helpers.py, kernel_oracle_helpers.py, shading_helpers.py as of the commit before it), for argument sets the suite uses: every
seeded ray set, soup and mesh a GPU test builds on is the one it was built on before."""
import hashlib
import types

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from query_helpers import RAY_MASKS
from scenes import check_closest, check_frame, load, oracle_instances, oracle_scene, procedural_mesh, random_rays, soup, xf

F = np.float32
OLD_CULLS = dict(cull_p=(0.45, 0.45, 0.1))        # what the parity and refit copies of random_rays drew the cull flags with


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def five(rays):
    """all of a ray record but instance_mask, which the parity and refit copies left 0 and rr_trace_rays ignores"""
    return digest(*[rays[f] for f in ("origin", "dir", "tmin", "tmax", "flags")])


# ------------------------------------------------------------------------------------------------- 1. pinned inputs
PINNED = [
    (lambda: five(random_rays(4000, seed=8, **OLD_CULLS)), "f9c6734b6b21e15b77bfd17a484630ae36bfe5417901b33cf1c81184d4987b7a"),
    (lambda: five(random_rays(4000, seed=11, radius=5.0, **OLD_CULLS)), "c41553923d6da500fd571799266d8c1575fac3ec99109836e06be06fe9025aa0"),
    (lambda: five(random_rays(400, seed=41, radius=3.0, **OLD_CULLS)), "a742413b60beb0e0b07e162c7fe8eb9302744786b4a0519e52d06a5f91e3299c"),
    (lambda: five(random_rays(1500, seed=11, radius=2.5, extent=0.75, **OLD_CULLS)), "9de3bd146409c0a40a826a8de44f89a03189ee3468979df34c688a58ef5a7303"),
    (lambda: digest(random_rays(3000, seed=5)), "98e99ff1333c4cc15c832277f9248c401bd2150c19ebf3c9f50172d68f81d5be"),
    (lambda: digest(random_rays(6000, seed=21, radius=5.0, extent=2.5, masks=RAY_MASKS)),
     "09879b74706c2fd882314fcc9d67182ba404c56c92318a6d3ecdfb27fa7f8133"),
    (lambda: digest(random_rays(2000, seed=42, masks=(0xff, 1, 2), any_frac=0.5)), "3523f42b4b773bfb915917faf3111218abd06d4f9c63c1972bf6052fe69606f5"),
    (lambda: digest(*soup("flat", 300, seed=304)), "19ded06a1f05245fea69b03168403f93ee40d3c80a4632b9010c2ed09911c977"),
    (lambda: digest(*soup("far", 400, seed=403)), "972f5d1a211801ad197a16e917d23b69cf2a8f16acae2fe62ffadb92b93acd3e"),
    (lambda: digest(*soup("mixed", 700, seed=705)), "f55626435d24afbcb7d528c98c9f7c9ef1eb9ef10ce70b84fa5069d6350b3751"),
    (lambda: digest(*soup("line", 500, seed=504)), "1b20abbc3c7a6e39c87c30a5c92d28c80a2a85de588fd73a395a2cbc40246835"),
    (lambda: digest(*soup("flat", 300, seed=304, collinear=False)), "19ded06a1f05245fea69b03168403f93ee40d3c80a4632b9010c2ed09911c977"),
    (lambda: digest(*soup("mixed", 700, seed=705, collinear=False)), "481dbb285179cc28661d0621647b549e7ef22e515d603b5f5aa695d670cbfd89"),
    (lambda: digest(*soup("line", 500, seed=504, collinear=False)), "1b20abbc3c7a6e39c87c30a5c92d28c80a2a85de588fd73a395a2cbc40246835"),
    (lambda: digest(*procedural_mesh(6, seed=3)), "958bd924229053dbc957bd4b8f9f68726fe50fc1aada7e74e8c120795ea620a5"),
    (lambda: digest(xf(0.3, 0.2, 2.4, (0.7, 0.8, 0.5), -1.0)), "763bde9b21d12088dd3dafd4ee66df20a828f2aae22ad0f0a3d1a92e7bcfb361"),
    (lambda: digest(*load("cube.obj")), "a20006c5b0d3fe2b9d7c80158f26b1221a09259132b60b7640db1ec7ee31ce03"),
]


@pytest.mark.parametrize("k", range(len(PINNED)))
def test_pinned_inputs(k):
    make, want = PINNED[k]
    assert make() == want


def test_the_old_ray_sets_differ_from_the_new_only_in_the_mask():
    rays = random_rays(4000, seed=8, **OLD_CULLS)
    assert np.all(rays["instance_mask"] == 0xff) and rays.dtype == rr.RAY_DTYPE
    assert five(rays) != five(random_rays(4000, seed=8))                      # cull_p reaches the draw


# ------------------------------------------------------------------------------------------------- 2. the checks still bite
def one_triangle():
    v = np.zeros(3, rr.VERTEX_DTYPE)
    v["position"] = [(0, 0, 0), (0, 1, 0), (0, 0, 1)]
    v["norm"] = (1, 0, 0)
    return v, np.arange(3, dtype=np.uint32)


def exact_hits(s, rays):
    hits = np.zeros(len(rays), rr.HIT_DTYPE)
    for k in range(len(rays)):
        h = s.trace(rays["origin"][k], rays["dir"][k], float(rays["tmin"][k]), float(rays["tmax"][k]), int(rays["flags"][k]), use_bvh=0)
        for f in ("hit", "prim", "inst", "t", "u", "v"):
            hits[f][k] = getattr(h, f)
    return hits


def test_check_closest_passes_on_the_exact_record_and_on_nothing_else():
    s = oracle_scene([one_triangle()])
    rays = rr.pack_rays([(2, 0.25, 0.25), (2, 0.75, 0.75)], [(-1, 0, 0), (-1, 0, 0)], 1e-4, 100.0)      # into the triangle, past its edge
    hits = exact_hits(s, rays)
    assert list(hits["hit"]) == [1, 0] and hits["t"][0] == 2.0 and (hits["prim"][0], hits["inst"][0]) == (0, 0)
    assert check_closest(hits, s, rays) == 1
    for field in ("t", "u", "v"):
        for towards in (0.0, 9.0):
            bad = hits.copy()
            bad[field][0] = np.nextafter(hits[field][0], F(towards))
            with pytest.raises(AssertionError):
                check_closest(bad, s, rays)
    for field, k in (("prim", 0), ("inst", 0), ("hit", 0), ("hit", 1)):
        bad = hits.copy()
        bad[field][k] ^= 1
        with pytest.raises(AssertionError):
            check_closest(bad, s, rays)
    bad = hits.copy()
    bad["t"][1] = 5.0                                   # ... while what a miss leaves in the other fields is nobody's business
    assert check_closest(bad, s, rays, sel=[1]) == 0


COUNTERS = ("rays", "primary", "secondary", "hits", "misses", "terminal_hits", "tir")


def frame():
    """(rgba, f32, st, lit, pw) of a 2 x 3 frame that check_frame accepts: the GPU's side equal to both oracle renders"""
    rgb = np.random.default_rng(1).random((2, 3, 3)).astype(F)
    rgba8 = np.full((2, 3, 4), 255, np.uint8)
    rgba8[..., :3] = np.floor(rgb * F(255) + F(0.5))
    stats = dict(traversal_overflow=0, stats_valid=1, rays=9, primary=6, secondary=3, hits=4, misses=5, terminal_hits=1, tir=2)
    ref = dict(rgb=rgb, rgba8=rgba8, stats=types.SimpleNamespace(**stats))
    return rgba8.copy(), np.concatenate([rgb, np.ones((2, 3, 1), F)], axis=-1), types.SimpleNamespace(**stats), ref, ref


def test_check_frame_passes_on_the_exact_frame_and_on_nothing_else():
    check_frame(*frame())
    rgba, f32, st, lit, pw = frame()
    f32[0, 1, 2] = np.nextafter(f32[0, 1, 2], F(2))    # one ulp: inside FLOAT_TOL of the literal render, not the path-weight render's bits
    with pytest.raises(AssertionError):
        check_frame(rgba, f32, st, lit, pw)
    rgba, f32, st, lit, pw = frame()
    rgba[1, 2, 0] ^= 1                                  # one LSB: allowed against the literal render only
    with pytest.raises(AssertionError):
        check_frame(rgba, f32, st, lit, pw)
    for name in COUNTERS:
        rgba, f32, st, lit, pw = frame()
        setattr(st, name, getattr(st, name) + 1)
        with pytest.raises(AssertionError):
            check_frame(rgba, f32, st, lit, pw)
    rgba, f32, st, lit, pw = frame()
    rgba[0, 0, 3] = 254
    with pytest.raises(AssertionError):
        check_frame(rgba, f32, st, lit, pw)
    rgba, f32, st, lit, pw = frame()
    f32[1, 1, 3] = np.nextafter(F(1), F(0))
    with pytest.raises(AssertionError):
        check_frame(rgba, f32, st, lit, pw)
    rgba, f32, st, lit, pw = frame()
    st.traversal_overflow = 1
    with pytest.raises(AssertionError):
        check_frame(rgba, f32, st, lit, pw)


# ------------------------------------------------------------------------------------------------- 3. scenes in the oracle
def test_oracle_instances_copies_every_field_and_a_scene_without_env_traces():
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, -2.5, (0.5, 0.8, 0.5), 0.4)], meshes=[1, 0], masks=[1, 0x81], flags=[0, 1])
    o = oracle_instances(inst)
    assert o.dtype == O.INSTANCE_DTYPE and set(o.dtype.names) == {"transform", "id_mask", "hitgroup_flags", "blas"}
    for theirs, ours in (("transform", "transform"), ("id_mask", "instance_id_mask"), ("hitgroup_flags", "hitgroup_flags"), ("blas", "blas")):
        assert o[theirs].tobytes() == inst[ours].tobytes() and o[theirs].any(), theirs
    # two instances of the triangle, the second one moved along -z: each ray finds its own
    inst = rr.make_instances(transforms=[xf(0, 0, 0), xf(0, 0, -2.5)], meshes=[0, 0], masks=[1, 1])
    s = oracle_scene([one_triangle()], instances=inst)
    rays = rr.pack_rays([(2, 0.25, 0.25), (2, 0.25, -2.25)], [(-1, 0, 0), (-1, 0, 0)], 1e-4, 100.0)
    hits = exact_hits(s, rays)
    assert list(hits["hit"]) == [1, 1] and list(hits["inst"]) == [0, 1]
    assert check_closest(hits, s, rays) == 2 and check_closest(hits, s, rays, inst_map={0: 0, 1: 1}) == 2
    with pytest.raises(AssertionError):
        check_closest(hits, s, rays, inst_map={0: 0, 1: 2})
