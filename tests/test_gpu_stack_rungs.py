"""GPU: every traversal-stack rung at its boundary, on every kernel, against the CPU oracle.

No traversal kernel checks its stack: the host reads the built tree's depth (rr_stats.bvh_depth, `need`) and launches an
instantiation whose LDS stack is just large enough -- k_render_fused 19 / 22 / 26 / 31 / 39 / 64 entries, the ray-tree kernels
19 / 26 / 31 / 39 / 64 with 2 or 8 parked rays, 16-bit-entry builds 39 (one instance) and 30 / 39 (two-level scenes), k_render_lds a
run-time need + 1 while that fits LDS, k_render_paths and k_stream_* need <= 39 only, the query kernels 31 or 64.  A rung one entry
short writes into the neighbouring wave's stack and nothing reports it.  depth_meshes.chain_mesh builds trees of an exact depth
that a ray travelling towards +z fills to their last entry, so here every rung is run at the deepest tree it takes and the next
rung at the tree one deeper.  Every test first asserts
  * rr_stats.bvh_depth == the depth it was built for (and the downloaded tree's own depth), and
  * stack_high_water of its own rays or pixels on the downloaded tree reaches need - 1 (two-level: the BLAS part, depth - 1),
then compares: frames with the oracle's path-weight mode bit for bit (RGBA8 and float) with equal counters and the asserted
render_kernel (check_launch), hits for t / u / v / prim / inst bits (check_closest, check_slots), ray trees as test_gpu_shade,
test_gpu_samples and test_gpu_adaptive do.  Views: the camera on the -z side (its rays travel towards +z: the deep direction), on
the +z side (one entry), and two oblique ones.  The chain's triangles alternate their winding: sheets of glass that a ray tree
crosses level after level, every level a walk of the whole chain.

What this can and cannot see: a walk pushes at most one entry per internal node of a root-to-leaf path, so a tree of depth `need`
(the leaf level counted) holds need - 1 entries at most, and every rung (>= need entries) has one to spare.  A rung chosen one
tree level too late (need 32 on the 31-entry build) still holds the deepest walk exactly; from two entries short, or a stack
sized from anything but the scene's deepest tree, the deep views here overwrite a neighbour's stack and the frames differ.

Run time on an MI355X: 0.01 to 0.17 s per case, the oracle's frames included (they are 96x64 at most and cached per rung)."""
import collections

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from conftest import procedural_env
from depth_meshes import axis_rays, chain_mesh, stack_high_water, to_object_space, to_world_space, tree_depth
from kernel_oracle_helpers import (check_launch,  # noqa: F401  (make_renderer: a fixture)
                                   dispatch, expected_kernel, FUSED, LDS, make_renderer, PATHS, report, STREAM)
from query_helpers import CULLS
from scenes import check_closest, load, Scene, xf
from shading_helpers import OFFP16, PERM16, THRESHOLD, fold
from shading_helpers import check_against_oracle as check_shade
from test_gpu_adaptive import follows_the_rule
from test_gpu_query_multi import check_slots
from test_gpu_query_multi import expected as multi_expected
from test_gpu_samples import check as check_samples
from test_gpu_samples import oracle_samples

pytestmark = pytest.mark.gpu

W, H = 96, 64
SW, SH = 24, 16                                      # supersampled frames: the oracle renders them 4 times as large per axis
FOV = 0.5                                            # the chain (+-1.05 at most) fills most of the frame from five units away
DEEP, SHALLOW = -np.pi / 2, np.pi / 2                # the camera on the -z side (rays towards +z: the full stack) and on the +z side
ANGLES = (DEEP, SHALLOW, -1.0, 2.2)                  # and two oblique views, one from either side
FLOAT = rr.DISPATCH_FLOAT_OUTPUT
KW = dict(max_refract=5)
SINGLE_NEEDS = (19, 20, 22, 23, 26, 27, 31, 32, 39, 40, 64)
TLAS_DEPTH = 2                                       # two instances: one top-level node above the two BLAS roots
TWO_LEVEL_NEEDS = (30, 31, 39, 40, 64)               # bvh_depth = chain depth + TLAS_DEPTH
MIRROR = np.concatenate([np.diag([-0.6, 0.6, 0.6]), [[0.8], [0.1], [0.2]]], axis=1).astype(np.float32)
ENV = procedural_env(128, 64, seed=3)
_scenes = {}


class RungScene(Scene):
    """a Scene that keeps what it built: the mesh id and the downloaded fp32 hierarchy of its one mesh"""

    def load_gpu(self, r):
        (v, i), = self.meshes
        self.mid = r.upload_mesh(v, i)
        r.build_blas(self.mid)
        inst = rr.make_instances(meshes=[self.mid]) if self.instances is None else self.instances.copy()
        inst["blas"] = self.mid
        r.build_tlas(inst)
        r.upload_envmap(self.env)
        r.set_tile_partition(0, 1)
        self.nodes = r.download_blas(self.mid)[0]


def chain_scene(need, two_level=False):
    """the chain of exactly `need` levels: one identity instance, or two instances of a chain TLAS_DEPTH shallower -- one rotated
    and scaled, one mirrored with TRIANGLE_FRONT_COUNTERCLOCKWISE.  One scene (and oracle twin) per rung for the whole module."""
    key = "chain-%d-%d" % (need, two_level)
    if key not in _scenes:
        inst = None
        if two_level:
            inst = rr.make_instances(transforms=[xf(-0.8, 0, 0, (0.6, 0.6, 0.6), 0.35), MIRROR], meshes=[0, 0], masks=[1, 1],
                                     flags=[0, rr._capi.INSTANCE_FLAG_FRONT_CCW])
        _scenes[key] = RungScene(key, [chain_mesh(need - TLAS_DEPTH * two_level, front_to_plus_z=True, alternate=True)], ENV, inst)
    return _scenes[key]


def view(angle, w=W, h=H):
    return rr.camera_orbit(float(angle), fov_y=FOV, aspect=float(np.float32(w / h)))


def views(angles=ANGLES):
    return [view(a) for a in angles]


def ring(n):
    """n views round the orbit from the deep one: the +z side and the obliques are among them"""
    return [view(DEEP + 2 * np.pi * k / n) for k in range(n)]


def assert_rung(r, scene, need, rays):
    """the scene on r has the depth it was built for and one of `rays` fills the stack that depth needs"""
    blas = need if scene.single else need - TLAS_DEPTH
    assert r.stats().bvh_depth == need, (r.stats().bvh_depth, need)
    assert tree_depth(scene.nodes) == blas, (tree_depth(scene.nodes), blas)
    if scene.single:
        high = int(stack_high_water(scene.nodes, rays).max())
    else:
        high = max(int(stack_high_water(scene.nodes, to_object_space(rays, t)).max()) for t in scene.instances["transform"])
    assert high == blas - 1, "the deepest stack of these rays holds %d entries, the rung is for %d" % (high, blas - 1)


def loaded(make_renderer, kernel, need, two_level=False, cams=None, rays=None, **env):
    """a renderer forced to `kernel` with the chain scene of the rung on it, depth and fill asserted for the first camera's pixels
    (or for `rays`)"""
    r = make_renderer(kernel, **env)
    sc = chain_scene(need, two_level)
    sc.load_gpu(r)
    assert_rung(r, sc, need, rr.camera_rays(cams[0], W, H) if rays is None else rays)
    return r, sc


def rung32(need):
    return next(s for s in (19, 22, 26, 31, 39, 64) if need <= s)


def fused_name(r, sc, cams, kw, stack, pend, stack16):
    """the instantiation k_render_fused rendered this launch with: its stack entries, parked rays and entry type"""
    _, st = dispatch(r, W, H, cams, kw, FLOAT)
    name = st.render_kernel_name.decode()
    assert st.render_kernel == FUSED and name.startswith("k_render_fused<%d, %d, " % (stack, pend)), (name, stack, pend)
    assert ("unsigned short" in name) == stack16, (name, stack16)


def frames(r, kernel, sc, cams, kw, tally, tag, batch=True):
    """every view as a dispatch of its own, then all of them as one launch; -> the kernels that rendered them"""
    got = [check_launch(r, kernel, sc, W, H, [c], kw, FLOAT, tally, tag="%s view %d" % (tag, k)) for k, c in enumerate(cams)]
    if batch:
        got.append(check_launch(r, kernel, sc, W, H, cams, kw, FLOAT, tally, oracle_slices=range(len(cams)), tag="%s batch" % tag))
    return got


# ------------------------------------------------------------------------------------------- 1. one identity instance: frames
@pytest.mark.parametrize("need", SINGLE_NEEDS)
def test_fused_rungs(make_renderer, need):
    """Depth 1: the 32-bit ladder 19 / 22 / 26 / 31 / 39 / 64; Depth 4: 16-bit entries on the 39-entry rung for 20 <= need <= 39"""
    cams = views()
    r, sc = loaded(make_renderer, "fused", need, cams=cams)
    tally = collections.Counter()
    assert set(frames(r, "fused", sc, cams, KW, tally, "fused need %d" % need)) == {FUSED}
    fused_name(r, sc, cams[:1], KW, rung32(need), 2, False)
    s16 = 19 < need <= 39
    fused_name(r, sc, cams, KW, 39 if s16 else rung32(need), 2, s16)
    report("fused need %d" % need, tally)


@pytest.mark.parametrize("need", SINGLE_NEEDS)
def test_lds_rungs(make_renderer, need):
    """k_render_lds sizes its stacks at run time (need + 1 entries): a 24-slice batch round the orbit, every slice also alone"""
    cams = ring(24)
    r, sc = loaded(make_renderer, "lds", need, cams=cams)
    tally = collections.Counter()
    got = check_launch(r, "lds", sc, W, H, cams, KW, FLOAT, tally, oracle_slices=(0, 3, 12, 17), tag="lds need %d" % need)
    assert got == (LDS if need <= lds_fit_limit() else FUSED)
    report("lds need %d" % need, tally)


@pytest.mark.parametrize("need", SINGLE_NEEDS)
def test_paths_rungs(make_renderer, need):
    """k_render_paths takes need <= 39 and hands deeper trees to k_render_fused"""
    cams = views()
    r, sc = loaded(make_renderer, "paths", need, cams=cams)
    tally = collections.Counter()
    got = frames(r, "paths", sc, cams, KW, tally, "paths need %d" % need, batch=False)
    assert set(got) == {PATHS if need <= 39 else FUSED}, (need, got)
    report("paths need %d" % need, tally)


_limit = []


def lds_fit_limit():
    """the deepest chain whose nodes and need + 1 stack entries per lane expected_kernel lets into LDS"""
    if not _limit:
        cams = ring(24)
        fits = [n for n in range(19, 65) if expected_kernel("lds", Scene("fit", [chain_mesh(n)], ENV), W, H, cams, KW, n) == LDS]
        assert fits == list(range(19, fits[-1] + 1)) and 39 < fits[-1] < 64, fits
        _limit.append(fits[-1])
    return _limit[0]


@pytest.mark.parametrize("over", [0, 1])
def test_lds_fit_limit(make_renderer, over):
    """the last depth that fits LDS beside its stacks renders on k_render_lds, the next one on k_render_fused: both as the oracle"""
    need = lds_fit_limit() + over
    cams = ring(24)
    r, sc = loaded(make_renderer, "lds", need, cams=cams)
    tally = collections.Counter()
    got = check_launch(r, "lds", sc, W, H, cams, KW, FLOAT, tally, oracle_slices=(0, 3, 12, 17), tag="lds fit limit %d" % need)
    assert got == (FUSED if over else LDS), (need, got)
    report("lds fit limit, need %d" % need, tally)


# ------------------------------------------------------------------------------------------ 2. one identity instance: queries
def query_bundle(sc, seed, n_aimed):
    """per instance, rays along the chain's axis towards +z and towards -z through its middle (the deep direction and the
    one-entry one, in the instance's space); then seeded oblique rays from a sphere round the scene, each aimed at a point of a
    triangle of an instance, 0.03 beside it (the smallest triangle is 0.3 wide), with the three cull modes and a fifth of them
    too short to arrive: most hit something, some nothing"""
    (v, i), = sc.meshes
    P = v["position"][i].reshape(-1, 3, 3).astype(np.float64)
    T = [np.eye(4)[:3]] if sc.single else [t.reshape(3, 4).astype(np.float64) for t in sc.instances["transform"]]
    rng = np.random.default_rng(seed)
    tgt = np.einsum("nc,ncx->nx", rng.dirichlet((1, 1, 1), n_aimed), P[rng.integers(0, len(P), n_aimed)])
    t = np.stack(T)[rng.integers(0, len(T), n_aimed)]
    tgt = np.einsum("nxy,ny->nx", t[:, :, :3], tgt) + t[:, :, 3] + rng.normal(size=(n_aimed, 3)) * 0.03
    o = rng.normal(size=(n_aimed, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 3.0
    d = tgt - o
    aimed = rr.pack_rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), 1e-4, rng.choice([100.0, 2.0], n_aimed, p=[0.8, 0.2]),
                         flags=rng.choice(CULLS, n_aimed))
    return np.concatenate([to_world_space(axis_rays(), t) for t in T] + [aimed])


def check_queries(r, sc, need):
    """trace_rays on about 1 200 rays and the multi-hit query (K = 4, with counts) on about 120: closest hits and slots as the
    oracle's brute force"""
    rays = query_bundle(sc, need, 1150)
    s = sc.oracle()
    n_hit = check_closest(r.trace_rays(rays), s, rays)
    assert n_hit >= len(rays) // 2, (n_hit, len(rays))         # (four fifths are long enough, and aimed within a tenth of a triangle)
    few = query_bundle(sc, need + 1, 90)
    hits, counts = r.query_rays_multi(few, 4, counts=True)
    inst = None
    if sc.instances is not None:
        inst = sc.instances.copy()
        inst["blas"] = 0
    exp = multi_expected(sc.meshes, inst, few)
    check_slots(hits, counts, exp, few, 4)
    assert max(len(a) for a in exp) > 4                        # a ray along the axis crosses more sheets than there are slots


def sample_view(angle):
    sc = view(angle, SW, SH)
    return sc, np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32)


def check_ray_trees(r, sc, kw, angles=(DEEP, SHALLOW, -1.0), samples=True):
    """shade_rays on the pixels' rays of three 48x32 views; render_samples with S = 2 and render_adaptive (2 of 4 samples) on
    24x16 frames, against the oracle's 96x64 frame of sub-pixels"""
    s = sc.oracle()
    for a in angles:
        cam = view(a, 48, 32)
        ref = check_shade(r, s, np.array(cam.proj_inv, np.float32), np.array(cam.camera_loc, np.float32), 48, 32, rr.camera_rays(cam, 48, 32), **kw)
        assert ref["stats"].hits > 0
    if not samples:
        return
    for a in angles[:2]:
        cam, M, loc = sample_view(a)
        rgb, cnt = oracle_samples(s, M, loc, SW, SH, **kw)
        p = rr.default_params(**kw)
        got = r.render_samples(SW, SH, cam, OFFP16[:2], p, rgba8=True, ray_counts=True)
        check_samples(got, fold([rgb[j, i] for i, j in PERM16[:2]]), sum(cnt[j, i] for i, j in PERM16[:2]), False)
        got = r.render_adaptive(SW, SH, cam, (2, OFFP16[:4]), THRESHOLD, p, rgba8=True, ray_counts=True, sample_counts=True)
        follows_the_rule(got, np.stack([rgb[j, i] for i, j in PERM16[:4]]), np.stack([cnt[j, i] for i, j in PERM16[:4]]), 2, THRESHOLD, False)


@pytest.mark.parametrize("need", SINGLE_NEEDS)
def test_query_rungs(make_renderer, need):
    """rr_trace_rays and the multi-hit query: 31 entries to need 31, 64 from 32"""
    r, sc = loaded(make_renderer, "fused", need, rays=query_bundle(chain_scene(need), need, 1150))
    check_queries(r, sc, need)


@pytest.mark.parametrize("need", SINGLE_NEEDS)
def test_ray_tree_rungs(make_renderer, need):
    """k_shade_rays, k_render_samples, k_adaptive_*: 19 entries to need 19, the 16-bit 39-entry build to 39, 64 from 40"""
    r, sc = loaded(make_renderer, "fused", need, rays=rr.camera_rays(view(DEEP, 48, 32), 48, 32))
    assert_rung(r, sc, need, rr.camera_rays(sample_view(DEEP)[0], SW, SH, *OFFP16[0]))
    check_ray_trees(r, sc, KW)


@pytest.mark.parametrize("need", [31, 39, 64])
def test_eight_parked_rays_rungs(make_renderer, need):
    """max_reflect = 3: the builds with eight parked-ray slots, k_render_fused (Depth 1: 32-bit entries; Depth 4: 16-bit to 39) and
    k_shade_rays"""
    kw = dict(max_refract=6, max_reflect=3)
    cams = views()
    r, sc = loaded(make_renderer, "fused", need, cams=cams)
    tally = collections.Counter()
    assert set(frames(r, "fused", sc, cams, kw, tally, "pend 8 need %d" % need)) == {FUSED}
    fused_name(r, sc, cams[:1], kw, rung32(need), 8, False)
    fused_name(r, sc, cams, kw, 39 if need <= 39 else 64, 8, need <= 39)
    check_ray_trees(r, sc, kw, samples=False)
    report("eight parked rays, need %d" % need, tally)


# ------------------------------------------------------------------------------------------------------ 3. two-level scenes
@pytest.mark.parametrize("need", TWO_LEVEL_NEEDS)
@pytest.mark.parametrize("tlas32", [0, 1])
def test_two_level_fused_rungs(make_renderer, need, tlas32):
    """16-bit entries (the 30-entry build at any Depth, the 39-entry one from Depth 3), and the 32-bit ladder under RR_DEBUG_TLAS32=1"""
    cams = views()
    r, sc = loaded(make_renderer, "fused", need, True, cams=cams, **({"RR_DEBUG_TLAS32": 1} if tlas32 else {}))
    tally = collections.Counter()
    assert set(frames(r, "fused", sc, cams, KW, tally, "two-level fused need %d tlas32 %d" % (need, tlas32))) == {FUSED}
    for launch in (cams[:1], cams):
        s16 = not tlas32 and (need <= 30 or (need <= 39 and len(launch) > 2))
        fused_name(r, sc, launch, KW, (30 if need <= 30 else 39) if s16 else rung32(need), 2, s16)
    report("two-level fused need %d tlas32 %d" % (need, tlas32), tally)


@pytest.mark.parametrize("need", TWO_LEVEL_NEEDS)
def test_two_level_stream_rungs(make_renderer, need):
    """k_stream_* at Depth 16: need 39 is the last it takes"""
    cams = ring(16)
    r, sc = loaded(make_renderer, "stream", need, True, cams=cams)
    tally = collections.Counter()
    got = check_launch(r, "stream", sc, W, H, cams, KW, FLOAT, tally, oracle_slices=(0, 2, 8, 11), tag="stream need %d" % need)
    assert got == (STREAM if need <= 39 else FUSED), (need, got)
    report("two-level stream need %d" % need, tally)


@pytest.mark.parametrize("need", TWO_LEVEL_NEEDS)
@pytest.mark.parametrize("tlas32", [0, 1])
def test_two_level_query_and_ray_tree_rungs(make_renderer, need, tlas32):
    r, sc = loaded(make_renderer, "fused", need, True, rays=query_bundle(chain_scene(need, True), need, 1150), **({"RR_DEBUG_TLAS32": 1} if tlas32 else {}))
    check_queries(r, sc, need)
    assert_rung(r, sc, need, rr.camera_rays(view(DEEP, 48, 32), 48, 32))
    assert_rung(r, sc, need, rr.camera_rays(sample_view(DEEP)[0], SW, SH, *OFFP16[0]))
    check_ray_trees(r, sc, KW)


# ---------------------------------------------------------------------------------------------------------------- 4. one over
def test_one_level_too_many_is_refused_at_the_build(make_renderer):
    """a 64-level BLAS under a two-instance TLAS needs 66 entries: rr_build_tlas says so, and the context goes on to build and
    render an ordinary scene"""
    r = make_renderer("fused")
    deep = chain_scene(64)
    deep.load_gpu(r)
    assert_rung(r, deep, 64, axis_rays())
    two = chain_scene(64, True).instances.copy()
    two["blas"] = deep.mid
    with pytest.raises(rr.RRError, match="RR_ERR_UNSUPPORTED"):
        r.build_tlas(two)
    with pytest.raises(rr.RRError, match="RR_ERR_STATE"):
        r.dispatch_rays(W, H)                                   # nothing is left to render
    monkey = Scene("monkey-after-one-over", [load("monkey.obj")], ENV)
    monkey.load_gpu(r)
    tally = collections.Counter()
    assert check_launch(r, "fused", monkey, W, H, [rr.camera_orbit(0.4)], KW, FLOAT, tally, tag="after the refused build") == FUSED
    report("after a refused build", tally)
