"""CPU: the builder models that test_gpu_capacity_edges.py compares GPU trees with.

The banded ploc_model is the dense one (every pair's area in a table) on every mesh the dense one was written for and on the three
input families; karras_model's tree is a radix tree over the sorted keys with Karras' numbering; the instance-box model's fused
multiply-add rounds once; pushed_refs reports what a hand-made tree makes a ray push."""
import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from builder_models import (FAMILIES, _fma32, aimed_rays, check_structure, has_negative_zero, inst_world_box_model, karras_model, karras_tree,
                            same_tree)
from depth_meshes import (CHAIN_DEPTHS, DEGENERATE, F, axis_rays, chain_mesh, morton_keys, ploc_model, ploc_model_dense, pushed_refs,
                          stack_high_water, tree_depth, tri_boxes)

SMALL = (2, 3, 17, 33, 300, 600)
MESHES = dict(DEGENERATE)
MESHES.update({"chain-%d" % n: (lambda n=n: chain_mesh(n)) for n in CHAIN_DEPTHS})
MESHES.update({"%s-%d" % (f, n): (lambda f=f, n=n: FAMILIES[f](n)) for f in FAMILIES for n in SMALL})


@pytest.mark.parametrize("name", list(MESHES))
def test_banded_model_is_the_dense_model(name):
    verts, idx = MESHES[name]()
    nodes, order, depth = ploc_model(verts, idx)
    dnodes, dorder, ddepth = ploc_model_dense(verts, idx)
    assert nodes.tobytes() == dnodes.tobytes() and np.array_equal(order, dorder) and depth == ddepth == tree_depth(nodes)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n", (2, 3, 1025, 2049, 32769))
def test_karras_model_is_a_radix_tree(family, n):
    verts, idx = FAMILIES[family](n)
    assert len(idx) == 3 * n and np.all(np.isfinite(verts["position"])) and not has_negative_zero(verts)
    box = tri_boxes(verts, idx)
    keys = morton_keys(box)
    nodes, order, depth, ranges = karras_tree(keys, box)
    assert karras_model(verts, idx)[0].tobytes() == nodes.tobytes()
    assert depth == tree_depth(nodes) and depth <= 64
    # every leaf and every node referenced once, boxes the exact unions (leaf records as k_pack_tris writes them)
    tris = np.zeros(n, rr.TRI_DTYPE)
    P = verts["position"][idx].reshape(n, 3, 3)
    tris["prim"], tris["v0"], tris["e1"], tris["e2"] = order, P[order, 0], P[order, 1] - P[order, 0], P[order, 2] - P[order, 0]
    check_structure(nodes, tris, verts, idx)
    # each node's key range is contiguous, its children split it at the highest differing bit, Karras' numbering
    k = [int(x) for x in keys]
    c = nodes["c"].tolist()
    assert tuple(ranges[0]) == (0, n - 1)
    for node in range(n - 1):
        first, last = (int(x) for x in ranges[node])
        assert first < last and node in (first, last)
        bit = (k[first] ^ k[last]).bit_length() - 1
        l, r = c[node]
        l_rng = (~l, ~l) if l < 0 else tuple(int(x) for x in ranges[l])
        r_rng = (~r, ~r) if r < 0 else tuple(int(x) for x in ranges[r])
        assert l_rng[0] == first and r_rng[1] == last and l_rng[1] + 1 == r_rng[0]
        assert l < 0 or l == l_rng[1]
        assert r < 0 or r == r_rng[0]
        assert (k[l_rng[1]] >> bit) & 1 == 0 and (k[r_rng[0]] >> bit) & 1 == 1 and k[first] >> (bit + 1) == k[last] >> (bit + 1)


def test_the_line_family_has_thousands_of_equal_codes():
    verts, idx = FAMILIES["line"](4097)
    codes = morton_keys(tri_boxes(verts, idx)) >> np.uint64(32)
    assert np.unique(codes, return_counts=True)[1].max() >= 4000


def test_fma_model_rounds_once():
    # a * b + c exactly half way between two fp32 values plus a little: a double rounding (to float64, then to fp32) would tie to even
    a = np.array([1.0 + 2.0 ** -23], F)
    b = F(1.0 + 2.0 ** -23)                       # a * b = 1 + 2^-22 + 2^-46
    c = F(2.0 ** -24)                             # exact sum 1 + 2^-22 + 2^-24 + 2^-46: above the midpoint of 1 + 2^-22 and 1 + 3 * 2^-23
    assert _fma32(a, b, c)[0] == F(1.0 + 3 * 2.0 ** -23)
    assert _fma32(a, b, -c)[0] == F(1.0 + 2.0 ** -22)
    # against exact rational arithmetic on seeded values
    from fractions import Fraction
    rng = np.random.default_rng(5)
    v = np.abs(rng.normal(size=2000) * 10.0 ** rng.uniform(-6, 3, 2000)).astype(F)
    got = _fma32(v, F(1e-5), F(1e-7))
    for x, g in zip(v.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(float(F(1e-5))) + Fraction(float(F(1e-7)))
        lo, hi = np.nextafter(F(g), F(-np.inf)), np.nextafter(F(g), F(np.inf))
        assert abs(exact - Fraction(g)) <= abs(exact - Fraction(float(lo))) and abs(exact - Fraction(g)) <= abs(exact - Fraction(float(hi)))


def test_instance_box_model_on_hand_cases():
    ident = np.eye(3, 4, dtype=F).reshape(12)
    bb = np.array([[-1, -2, -3, 1, 2, 3]], F)
    got = inst_world_box_model(ident[None], bb)[0]
    grow = lambda v: _fma32(np.abs(np.array([v], F)), F(1e-5), F(1e-7))[0]
    assert np.array_equal(got, np.array([F(-1) - grow(1), F(-2) - grow(2), F(-3) - grow(3), F(1) + grow(1), F(2) + grow(2), F(3) + grow(3)], F))
    # a quarter turn about y with a move: x' = z + 10, y' = y, z' = -x
    T = np.array([0, 0, 1, 10, 0, 1, 0, 0, -1, 0, 0, 0], F)
    got = inst_world_box_model(T[None], bb)[0]
    want_lo, want_hi = np.array([7, -2, -1], F), np.array([13, 2, 1], F)
    assert np.array_equal(got[:3], want_lo - _fma32(np.abs(want_lo), F(1e-5), F(1e-7)))
    assert np.array_equal(got[3:], want_hi + _fma32(np.abs(want_hi), F(1e-5), F(1e-7)))
    assert np.all(got[:3] < want_lo) and np.all(got[3:] > want_hi)


def test_pushed_refs_on_a_chain_and_a_hand_made_tree():
    verts, idx = chain_mesh(40)
    nodes = ploc_model(verts, idx)[0]
    rays = axis_rays()
    high, top_node, top_leaf = pushed_refs(nodes, rays)
    assert np.array_equal(high, stack_high_water(nodes, rays)) and high.max() == 39
    assert top_leaf == 39 and top_node == 38        # +z rays push every leaf but leaf 0, -z rays the chain below each node
    # two leaves under one root, a ray through both boxes: the far leaf (~1 -> 1) is pushed, no internal node is
    n = np.zeros(1, rr.NODE_DTYPE)
    n["lox"], n["hix"], n["loy"], n["hiy"] = [[0, 2]], [[1, 3]], [[0, 0]], [[1, 1]]
    n["loz"], n["hiz"], n["c"] = [[0, 0]], [[1, 1]], [[~5, ~7]]
    r = rr.pack_rays([[-1, 0.5, 0.5], [4, 0.5, 0.5], [0.5, 0.5, -1]], [[1, 0, 0], [-1, 0, 0], [0, 0, 1]], 1e-4, 100.0)
    high, top_node, top_leaf = pushed_refs(n, r)
    assert high.tolist() == [1, 1, 0] and top_node == -1 and top_leaf == 7
    assert pushed_refs(n, r[:1])[2] == 7 and pushed_refs(n, r[1:2])[2] == 5 and pushed_refs(n, r[2:])[1:] == (-1, -1)


def test_aimed_rays_mostly_hit_their_triangles():
    verts, idx = FAMILIES["soup"](300)
    rays = aimed_rays(verts, idx, 200, seed=3, prims=np.arange(290, 300))
    assert len(rays) == 200 and np.all(np.isfinite(rays["dir"]))
