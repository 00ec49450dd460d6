"""The kernel-choice policy (csrc/rr_choice.cpp) on the CPU: which render kernel a dispatch takes before any measurement, the
class and candidates of a measured choice, k_render_fused's stack variant, the measurement's state machine and the owned-pixel
count.  The driver (tests/native/kernel_choice_driver.cpp) is built with g++ with the mesh-partition and camera host code; the
tables below pin today's decisions."""
import os
import shutil
import subprocess

import pytest

from codeobj import LAUNCHABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "refraction_raytracing_dxr_amd", "csrc")

FUSED, LDS, PATHS, STREAM = 0, 1, 2, 7
NONE, TLAS, MANY, FEW = -1, 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("choice") / "kernel_choice_driver")
    srcs = [os.path.join(ROOT, "tests", "native", "kernel_choice_driver.cpp"), os.path.join(CSRC, "rr_choice.cpp"),
            os.path.join(CSRC, "host", "rr_host_partition.cpp"), os.path.join(CSRC, "host", "rr_host_camera.cpp")]
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + srcs + ["-o", out], check=True)
    return out


def run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


# the reference's scene (monkey.obj: 968 triangles, a 22-deep tree that fits LDS) and a two-level scene
SINGLE = dict(single=1, need=22, blas_tris=968, pool_nodes=0, pool_refs=0, lds_fits=1)
TWO = dict(single=0, need=30, blas_tris=0, pool_nodes=2000, pool_refs=3000, lds_fits=0)
# a 1920 x 1080 launch of one slice, unsharded, default bounce limits, the scene on a tenth of the frame
LAUNCH = dict(depth=1, n_tiles=60 * 34, world=1, compact=0, mesh=0, have_rect=1, share=0.1, refract=5, reflect=2, no_cull=0, diag=0)
DEBUG = dict(dbg_kernel=0, dbg_stack=0, tlas32=0)


def scene_args(s):
    return "%d %d %d %d %d %d" % (s["single"], s["need"], s["blas_tris"], s["pool_nodes"], s["pool_refs"], s["lds_fits"])


def debug_args(d):
    return "%d %d %d" % (d["dbg_kernel"], d["dbg_stack"], d["tlas32"])


def pick_cmd(scene, **kw):
    s, l, d = dict(scene), dict(LAUNCH), dict(DEBUG)
    for k, v in kw.items():
        (s if k in s else l if k in l else d)[k] = v
    return "pick %s %d %d %d %d %d %d %r %d %d %d %d %s" % (
        scene_args(s), l["depth"], l["n_tiles"], l["world"], l["compact"], l["mesh"], l["have_rect"], l["share"], l["refract"],
        l["reflect"], l["no_cull"], l["diag"], debug_args(d))


# (scene, launch / debug changes) -> (kernel without a class, class, candidate A, candidate B, kernel before any measurement)
PICKS = [
    # launches of one or two slices: k_render_fused / k_render_paths, paths first where the scene is small on screen
    (SINGLE, dict(depth=1, share=0.1), (FUSED, FEW, FUSED, PATHS, PATHS)),
    (SINGLE, dict(depth=1, share=0.5), (FUSED, FEW, FUSED, PATHS, FUSED)),
    (SINGLE, dict(depth=2, share=0.24), (FUSED, FEW, FUSED, PATHS, PATHS)),
    (SINGLE, dict(depth=2, share=0.25), (FUSED, FEW, FUSED, PATHS, FUSED)),
    (SINGLE, dict(depth=1, have_rect=0, share=0.0), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, reflect=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, need=40), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=2, reflect=3), (FUSED, NONE, FUSED, FUSED, FUSED)),            # no LDS class below three slices
    # launches of many slices on an LDS-fitting scene: k_render_fused / k_render_lds, LDS the default from 24 slices
    (SINGLE, dict(depth=3), (FUSED, MANY, FUSED, LDS, FUSED)),
    (SINGLE, dict(depth=16), (FUSED, MANY, FUSED, LDS, FUSED)),
    (SINGLE, dict(depth=23), (FUSED, MANY, FUSED, LDS, FUSED)),
    (SINGLE, dict(depth=24), (FUSED, MANY, LDS, FUSED, LDS)),
    (SINGLE, dict(depth=64), (FUSED, MANY, LDS, FUSED, LDS)),
    (SINGLE, dict(depth=24, lds_fits=0), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=64, n_tiles=1 << 18), (FUSED, NONE, FUSED, FUSED, FUSED)),          # n_tiles * depth^2 = 2^30
    (SINGLE, dict(depth=64, n_tiles=(1 << 18) - 1), (FUSED, MANY, LDS, FUSED, LDS)),
    # compact, mesh-partition and sharded launches: neither LDS nor paths
    (SINGLE, dict(depth=1, compact=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=24, compact=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=24, compact=1, mesh=1, world=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, compact=1, world=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=64, compact=1, world=8), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=24, mesh=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=24, mesh=1, dbg_kernel=4), (FUSED, NONE, FUSED, FUSED, FUSED)),
    # two-level scenes: k_render_fused / the stream renderer while max_reflect <= 2 and the pool fits 16-bit stack entries
    (TWO, dict(depth=1), (FUSED, TLAS, FUSED, STREAM, FUSED)),
    (TWO, dict(depth=16), (FUSED, TLAS, FUSED, STREAM, FUSED)),
    (TWO, dict(depth=16, compact=1, mesh=1, world=8), (FUSED, TLAS, FUSED, STREAM, FUSED)),
    (TWO, dict(depth=16, reflect=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=1, reflect=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, refract=62), (FUSED, TLAS, FUSED, STREAM, FUSED)),
    (TWO, dict(depth=16, refract=63), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, pool_nodes=32768), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, pool_refs=32768), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, need=40), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, tlas32=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=1, tlas32=1), (FUSED, FEW, FUSED, PATHS, PATHS)),
    (TWO, dict(depth=16, dbg_stack=64), (FUSED, NONE, FUSED, FUSED, FUSED)),
    # RR_DEBUG_KERNEL: the forced kernel where it can render the launch, k_render_fused where it cannot; never a class
    (TWO, dict(depth=16, dbg_kernel=10), (STREAM, NONE, FUSED, FUSED, STREAM)),
    (TWO, dict(depth=16, dbg_kernel=10, reflect=3), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=16, dbg_kernel=10), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, dbg_kernel=5, share=0.9), (PATHS, NONE, FUSED, FUSED, PATHS)),
    (SINGLE, dict(depth=3, dbg_kernel=5), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, dbg_kernel=5, compact=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, dbg_kernel=4), (LDS, NONE, FUSED, FUSED, LDS)),
    (SINGLE, dict(depth=16, dbg_kernel=4), (LDS, NONE, FUSED, FUSED, LDS)),
    (SINGLE, dict(depth=16, dbg_kernel=4, compact=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=16, dbg_kernel=4, lds_fits=0), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, dbg_kernel=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=64, dbg_kernel=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (TWO, dict(depth=16, dbg_kernel=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    # RR_DEBUG_DIAG: no measurement; the path-parallel kernel where the scene is small on screen
    (SINGLE, dict(depth=1, diag=1, share=0.1), (PATHS, NONE, FUSED, FUSED, PATHS)),
    (SINGLE, dict(depth=1, diag=1, share=0.25), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=24, diag=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    (SINGLE, dict(depth=1, diag=1, share=0.1, dbg_kernel=1), (FUSED, NONE, FUSED, FUSED, FUSED)),
    # NO_CULL does not change the pick (it only never measures)
    (SINGLE, dict(depth=24, no_cull=1), (FUSED, MANY, LDS, FUSED, LDS)),
]


def test_pick(driver):
    out = run(driver, [pick_cmd(scene, **kw) for scene, kw, _ in PICKS])
    got = [tuple(int(t) for t in line.split()) for line in out]
    bad = [(scene["single"], kw, want, g) for (scene, kw, want), g in zip(PICKS, got) if g != want]
    assert not bad, bad


# (scene, changes, depth, max_reflect) -> (stack entries, parked-ray slots, 16-bit stack entries)
FUSED_VARIANTS = [(SINGLE, dict(need=n), 16, 2, v) for n, v in [
    (10, (19, 2, 0)), (19, (19, 2, 0)), (20, (22, 2, 1)), (22, (22, 2, 1)), (23, (26, 2, 1)), (26, (26, 2, 1)), (27, (31, 2, 1)),
    (31, (31, 2, 1)), (32, (39, 2, 1)), (39, (39, 2, 1)), (40, (64, 2, 0)), (64, (64, 2, 0))]] + [
    (SINGLE, {}, 2, 2, (22, 2, 0)),                        # one or two slices: 32-bit entries
    (SINGLE, {}, 3, 2, (22, 2, 1)),
    (SINGLE, dict(blas_tris=32768), 16, 2, (22, 2, 0)),
    (SINGLE, {}, 16, 3, (22, 8, 1)),
    (SINGLE, dict(dbg_stack=40), 16, 2, (40, 2, 0)),
    (SINGLE, dict(dbg_stack=10), 16, 2, (22, 2, 0)),       # never below the tree depth
    (TWO, dict(need=20), 16, 2, (20, 2, 1)),               # two-level 16-bit builds are sized by the tree itself
    (TWO, {}, 1, 2, (30, 2, 1)),
    (TWO, dict(need=31), 1, 2, (31, 2, 0)),
    (TWO, dict(need=31), 3, 2, (31, 2, 1)),
    (TWO, dict(need=35), 3, 2, (35, 2, 1)),
    (TWO, dict(need=40), 3, 2, (64, 2, 0)),
    (TWO, dict(tlas32=1), 16, 2, (31, 2, 0)),
    (TWO, {}, 16, 3, (31, 8, 0)),
    (TWO, dict(pool_nodes=32768), 16, 2, (31, 2, 0)),
    (TWO, dict(dbg_stack=33), 16, 2, (33, 2, 0)),
]


def test_fused_variant(driver):
    lines = []
    for scene, kw, depth, reflect, _ in FUSED_VARIANTS:
        s, d = dict(scene), dict(DEBUG)
        for k, v in kw.items():
            (s if k in s else d)[k] = v
        lines.append("fused %s %d %d %s" % (scene_args(s), depth, reflect, debug_args(d)))
    got = [tuple(int(t) for t in line.split()) for line in run(driver, lines)]
    bad = [(kw, depth, reflect, want, g) for (_, kw, depth, reflect, want), g in zip(FUSED_VARIANTS, got) if g != want]
    assert not bad, bad


def tree_rung(single, stack, pend, stack16):
    """the ray-tree kernels' ladder as launch_shade_rays, launch_render_samples and launch_render_adaptive each spelt it before
    for_tree_variant (csrc/rr_choice.h) replaced the three copies, rung for rung -> (STACK, PEND, TLAS, bits per stack entry)"""
    if stack16 and not single and pend <= 2 and stack <= 30:
        return (30, 2, 1, 16)
    if stack16 and not single and pend <= 2 and stack <= 39:
        return (39, 2, 1, 16)
    if stack16 and single and stack <= 39:
        return (39, 2 if pend <= 2 else 8, 0, 16)
    tlas = 0 if single else 1
    if stack <= 19 and pend <= 2:
        return (19, 2, tlas, 32)
    if stack <= 26 and pend <= 2:
        return (26, 2, tlas, 32)
    for rung in (31, 39):
        if stack <= rung:
            return (rung, 2 if pend <= 2 else 8, tlas, 32)
    return (64, 2 if pend <= 2 else 8, tlas, 32)


# (single, stack, pend, stack16) -> (STACK, PEND, TLAS, bits): both sides of every rung's boundary, written out
TREE_VARIANTS = [
    # the 16-bit rungs: two-level scenes up to 30 and up to 39 entries with two parked rays, a single BLAS up to 39 with two or eight
    ((0, 30, 2, 1), (30, 2, 1, 16)), ((0, 31, 2, 1), (39, 2, 1, 16)), ((0, 39, 2, 1), (39, 2, 1, 16)), ((0, 40, 2, 1), (64, 2, 1, 32)),
    ((0, 30, 3, 1), (31, 8, 1, 32)), ((0, 39, 3, 1), (39, 8, 1, 32)), ((0, 1, 0, 1), (30, 2, 1, 16)),
    ((1, 19, 2, 1), (39, 2, 0, 16)), ((1, 39, 2, 1), (39, 2, 0, 16)), ((1, 39, 3, 1), (39, 8, 0, 16)), ((1, 39, 8, 1), (39, 8, 0, 16)),
    ((1, 40, 2, 1), (64, 2, 0, 32)), ((1, 40, 3, 1), (64, 8, 0, 32)),
    # 32-bit entries: 19 and 26 only with two parked rays
    ((1, 19, 2, 0), (19, 2, 0, 32)), ((1, 20, 2, 0), (26, 2, 0, 32)), ((1, 26, 2, 0), (26, 2, 0, 32)), ((1, 27, 2, 0), (31, 2, 0, 32)),
    ((1, 19, 3, 0), (31, 8, 0, 32)), ((1, 26, 3, 0), (31, 8, 0, 32)), ((1, 30, 2, 0), (31, 2, 0, 32)), ((1, 31, 2, 0), (31, 2, 0, 32)),
    ((1, 31, 3, 0), (31, 8, 0, 32)), ((1, 32, 2, 0), (39, 2, 0, 32)), ((1, 32, 3, 0), (39, 8, 0, 32)), ((1, 39, 2, 0), (39, 2, 0, 32)),
    ((1, 39, 3, 0), (39, 8, 0, 32)), ((1, 40, 2, 0), (64, 2, 0, 32)), ((1, 40, 3, 0), (64, 8, 0, 32)), ((1, 64, 2, 0), (64, 2, 0, 32)),
    ((1, 64, 3, 0), (64, 8, 0, 32)), ((1, 64, 8, 0), (64, 8, 0, 32)),
    ((0, 19, 2, 0), (19, 2, 1, 32)), ((0, 20, 2, 0), (26, 2, 1, 32)), ((0, 26, 2, 0), (26, 2, 1, 32)), ((0, 27, 2, 0), (31, 2, 1, 32)),
    ((0, 19, 3, 0), (31, 8, 1, 32)), ((0, 30, 2, 0), (31, 2, 1, 32)), ((0, 31, 2, 0), (31, 2, 1, 32)), ((0, 31, 3, 0), (31, 8, 1, 32)),
    ((0, 32, 2, 0), (39, 2, 1, 32)), ((0, 32, 3, 0), (39, 8, 1, 32)), ((0, 39, 2, 0), (39, 2, 1, 32)), ((0, 39, 3, 0), (39, 8, 1, 32)),
    ((0, 40, 2, 0), (64, 2, 1, 32)), ((0, 40, 3, 0), (64, 8, 1, 32)), ((0, 64, 2, 0), (64, 2, 1, 32)), ((0, 64, 3, 0), (64, 8, 1, 32)),
]
TREE_BOUNDARIES = [(single, stack, pend, stack16) for single in (0, 1) for stack16 in (0, 1) for stack in (19, 20, 26, 27, 30, 31, 32, 39, 40, 64)
                   for pend in (2, 3)]
TREE_DOMAIN = [(single, stack, pend, stack16) for single in (0, 1) for stack16 in (0, 1) for stack in range(1, 65) for pend in range(0, 9)]


def test_tree_variant_ladder(driver):
    """for_tree_variant against the written-out table, against the ladder its three launchers carried (every boundary of every rung
    and the whole domain), and its answers over the whole domain are exactly the launchable instantiations (4 with 16-bit stack entries, 10 with two
    parked rays, 6 with eight)"""
    assert [tree_rung(*q) for q, _ in TREE_VARIANTS] == [want for _, want in TREE_VARIANTS]
    queries = [q for q, _ in TREE_VARIANTS] + TREE_BOUNDARIES + TREE_DOMAIN
    got = [tuple(int(t) for t in line.split()) for line in run(driver, ["tree %d %d %d %d" % q for q in queries])]
    bad = [(q, g, tree_rung(*q)) for q, g in zip(queries, got) if g != tree_rung(*q)]
    assert not bad, bad[:10]
    bits = {"unsigned short": 16, "unsigned int": 32}
    launchable = {(s, p, int(t), bits[e]) for s, p, t, e in LAUNCHABLE}
    assert len(launchable) == 20 and set(got[-len(TREE_DOMAIN):]) == launchable


def key(driver, w, h, refract, reflect, depth):
    return int(run(driver, ["key %d %d %d %d %d" % (w, h, refract, reflect, depth)])[0])


def test_choice_key_depth_buckets(driver):
    lines = ["key 1920 1080 5 2 %d" % d for d in (1, 2, 3, 7, 8, 23, 24, 47, 48, 65535)]
    keys = [int(t) for t in run(driver, lines)]
    assert [k & 0xf for k in keys] == [1, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert keys[0] == (1920 << 48) ^ (1080 << 32) ^ (5 << 8) ^ (2 << 4) ^ 1
    assert key(driver, 1920, 1080, 5, 2, 3) != key(driver, 1920, 1088, 5, 2, 3) != key(driver, 1920, 1088, 6, 2, 3)


def test_slower_first_time_decides_at_once(driver):
    out = run(driver, ["new", "due 7 0.1 0", "due 7 0.1 0", "rec 1.0 1.02 0.1", "due 7 0.1 0", "peek 7"])
    assert out[1:] == ["0 0 1", "1 0 2", "1", "0 1 2", "1"]
    # just under 2 % slower: measured once more on the next dispatch of the shape
    out = run(driver, ["new", "due 7 0.1 0", "due 7 0.1 0", "rec 1.0 1.019 0.1", "due 7 0.1 0"])
    assert out[3:] == ["0", "1 0 3"]


def test_two_rounds_decide_by_the_98_percent_rule(driver):
    base = ["new", "due 7 0.1 0", "due 7 0.1 0", "rec 1.0 0.99 0.1", "due 7 0.1 0"]
    out = run(driver, base + ["rec 1.0 0.97 0.1", "due 7 0.1 0", "peek 7"])
    assert out[3:] == ["0", "1 0 3", "1", "0 1 3", "1"]         # 1.96 is not below 0.98 x 2.0: the default stays
    out = run(driver, base + ["rec 1.0 0.9 0.1", "due 7 0.1 0", "peek 7"])
    assert out[5:] == ["2", "0 2 3", "2"]
    # the second round is decided by the sums, even where that round alone is slower
    out = run(driver, ["new", "due 7 0.1 0", "due 7 0.1 0", "rec 2.0 1.0 0.1", "due 7 0.1 0", "rec 1.0 1.5 0.1"])
    assert out[3:] == ["0", "1 0 3", "2"]


def test_share_that_doubles_or_halves_renews_the_choice(driver):
    decided = ["new", "due 7 0.1 0", "due 7 0.1 0", "rec 1.0 1.5 0.1"]
    assert run(driver, decided + ["due 7 0.2 0", "due 7 0.05 0"])[4:] == ["0 1 2", "0 1 2"]
    assert run(driver, decided + ["due 7 0.2001 0", "due 7 0.2001 0"])[4:] == ["0 0 1", "1 0 2"]
    assert run(driver, decided + ["due 7 0.0499 0"])[4:] == ["0 0 1"]


def test_no_cull_never_measures(driver):
    out = run(driver, ["new"] + ["due 7 0.1 1"] * 4 + ["due 7 0.1 0", "due 7 0.1 0"])
    assert out[1:] == ["0 0 0"] * 4 + ["0 0 1", "1 0 2"]


def test_fifth_shape_evicts_the_least_recently_used(driver):
    out = run(driver, ["new"] + ["due %d 0.1 0" % k for k in (1, 2, 3, 4, 1, 5)] + ["peek %d" % k for k in (1, 2, 3, 4, 5)])
    assert out[7:] == ["0", "-1", "0", "0", "0"]
    # a shape's entry survives the switch to another depth and back: the second dispatch of it measures
    out = run(driver, ["new", "due 1 0.1 0", "due 2 0.1 0", "due 1 0.1 0"])
    assert out[3] == "1 0 2"


@pytest.mark.parametrize("w,h", [(1920, 1080), (100, 70), (33, 33), (32, 32), (31, 1), (1000, 1000)])
@pytest.mark.parametrize("world", [1, 3, 8])
def test_owned_pixels_sum_to_the_frame(driver, w, h, world):
    out = run(driver, ["owned %d %d %d %d" % (w, h, world, mode) for mode in (0, 1, 2)])
    for line in out:
        assert int(line.split()[0]) == w * h, (line, w, h, world)


def test_owned_pixels_of_edge_tiles_and_partitions(driver):
    # 100 x 70: 4 x 3 tiles, the last column 4 and the last row 6 pixels wide; rank 0 of 3 holds tiles 0, 3, 6, 9
    assert run(driver, ["owned 100 70 3 0"])[0].split()[:2] == ["7000", str(1024 + 4 * 32 + 1024 + 32 * 6)]
    px, rank0, mesh, bg = (int(t) for t in run(driver, ["owned 1920 1080 3 1"])[0].split())
    assert mesh > 0 and bg > 0 and mesh + bg == 60 * 34 and rank0 > px // 3      # rank 0 renders the background tiles
    px, rank0, mesh, bg = (int(t) for t in run(driver, ["owned 1920 1080 8 2"])[0].split())
    assert (mesh, bg) == (60 * 34, 0) and px == 1920 * 1080 and rank0 < px // 4      # NO_CULL: every tile a mesh tile
