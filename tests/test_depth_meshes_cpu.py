"""depth_meshes.py on the CPU: the generator's shapes and windings, stack_high_water on a hand-built chain, and the model of the
default builder on the chain meshes (a pure chain of exactly the asked depth, filled to its last entry by a +z ray) and on the
meshes whose every merged-box area ties (a chain as deep as the mesh is large: what the builder's fall-back is for)."""
import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from depth_meshes import (axis_rays, chain_mesh, CHAIN_DEPTHS, CHAIN_SCALE, DEGENERATE, identical_mesh, is_chain, morton_order, one_point_mesh,
                          ploc_model, same_box_mesh, stack_high_water, to_object_space, to_world_space, tree_depth)

F = np.float32


def hand_chain(n):
    """n unit squares of boxes stacked along z, chained as the builder chains them: node d = (node d + 1 | leaf n - 1 - d)"""
    nodes = np.zeros(n - 1, rr.NODE_DTYPE)
    for d in range(n - 1):
        top = n - 1 - d                                       # child 1: leaf `top`, a slab at z = top
        nodes["lox"][d], nodes["hix"][d] = (-1, -1), (1, 1)
        nodes["loy"][d], nodes["hiy"][d] = (-1, -1), (1, 1)
        nodes["loz"][d], nodes["hiz"][d] = (0, top), (top - 1, top)
        nodes["c"][d] = (d + 1 if d < n - 2 else ~0, ~top)
    return nodes


def test_stack_high_water_on_a_hand_built_chain():
    n = 6
    nodes = hand_chain(n)
    assert tree_depth(nodes) == n and is_chain(nodes)
    o = [(0, 0, -5), (0, 0, 9), (3, 0, -5), (0.5, 0.5, 2.5), (0, 0, -5), (-5, 0, 0.5), (0, 0, -5)]
    d = [(0, 0, 1), (0, 0, -1), (0, 0, 1), (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 0, -1)]
    rays = rr.pack_rays(o, d, 0.0, [100, 100, 100, 100, 7.5, 100, 100])
    hw = stack_high_water(nodes, rays)
    # +z from below: every node pushes its leaf; -z from above: the leaf first, the chain waits: one entry; beside the boxes: none;
    # from inside, between leaves 2 and 3: the chain below is behind the ray, only leaves 3, 4, 5 are ahead: nodes 0, 1 push, node 2
    # sees its leaf only; tmax between leaves 2 and 3 (z = 2.5): the leaves above are not reached, nodes 3 and 4 push; along x at
    # z = 0.5: inside the chain's box at every node, beside every leaf: nothing is ever pushed; pointing away: nothing
    assert hw.tolist() == [n - 1, 1, 0, 2, 2, 0, 0]
    assert stack_high_water(nodes[:0], rays).tolist() == [0] * len(rays)
    # the deep ray again through an instance transform: rotated about y, scaled and moved, and back
    c, s = np.cos(0.7), np.sin(0.7)
    T = np.array([[c * 2, 0, s * 2, 0.3], [0, 2, 0, -1], [-s * 2, 0, c * 2, 4]], np.float64)
    world = to_world_space(rays, T)
    assert np.allclose(np.linalg.norm(world["dir"], axis=1), 1) and np.allclose(world["origin"][0], T[:, 3] - 5 * T[:, 2])
    assert stack_high_water(nodes, to_object_space(world, T))[:3].tolist() == [n - 1, 1, 0]


def test_generator_shapes_and_windings():
    n = 23
    v, i = chain_mesh(n)
    assert v.dtype == rr.VERTEX_DTYPE and len(v) == 3 * n and i.dtype == np.uint32 and i.tolist() == list(range(3 * n))
    P = v["position"].reshape(n, 3, 3)
    k = np.arange(n)
    s = (1 + 0.05 * k).astype(F) * F(CHAIN_SCALE)
    z = (0.0005 * (k - (n - 1) / 2)).astype(F) * F(CHAIN_SCALE)
    assert np.array_equal(P[:, 0], np.stack([-s, -s, z], -1)) and np.array_equal(P[:, 1], np.stack([s, -s, z], -1))
    assert np.array_equal(P[:, 2], np.stack([0 * s, s, z], -1))
    # a power-of-two scale is exact: the scaled mesh is the unscaled one times the scale, bit for bit
    assert np.array_equal(chain_mesh(n, scale=1.0)[0]["position"] * F(CHAIN_SCALE), v["position"])
    with pytest.raises(AssertionError):
        chain_mesh(n, scale=0.3)
    g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert np.all(g[:, 2] > 0) and np.all(g[:, :2] == 0) and np.all(v["norm"] == (0, 0, 1))       # front face towards +z: seen by -z rays
    vf, _ = chain_mesh(n, front_to_plus_z=True)
    Pf = vf["position"].reshape(n, 3, 3)
    gf = np.cross(Pf[:, 1] - Pf[:, 0], Pf[:, 2] - Pf[:, 0])
    assert np.all(gf[:, 2] < 0) and np.all(vf["norm"] == (0, 0, -1))                                # seen by +z rays
    assert np.array_equal(np.sort(Pf.reshape(n, 9), axis=1), np.sort(P.reshape(n, 9), axis=1))      # the same corners
    va, _ = chain_mesh(n, front_to_plus_z=True, alternate=True)
    assert np.array_equal(va["norm"][::3, 2], np.where(k % 2 == 0, -1, 1)) and np.array_equal(va["position"][0::6], vf["position"][0::6])
    assert np.array_equal(va["position"].reshape(n, 3, 3)[1::2], P[1::2]) and np.array_equal(va["position"].reshape(n, 3, 3)[0::2], Pf[0::2])
    for mesh, m in ((identical_mesh(65), 65), (one_point_mesh(100), 100), (same_box_mesh(100), 100)):
        assert len(mesh[0]) == 3 * m and len(mesh[1]) == 3 * m
    Q = same_box_mesh(100)[0]["position"].reshape(100, 3, 3)
    assert np.all(Q.min(1) == 0) and np.all(Q.max(1) == 1) and len(np.unique(Q.reshape(100, 9), axis=0)) >= 8
    assert np.all(np.linalg.norm(np.cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0]), axis=1) > 0)
    assert np.ptp(one_point_mesh(100)[0]["position"], axis=0).max() == 0


@pytest.mark.parametrize("n", CHAIN_DEPTHS)
def test_default_builder_model_chains_the_chain_mesh(n):
    rays = axis_rays()
    for flip, alt in ((False, False), (True, False), (True, True)):
        v, i = chain_mesh(n, front_to_plus_z=flip, alternate=alt)
        order, _ = morton_order(v, i)
        assert order.tolist() == list(range(n))
        nodes, order, depth = ploc_model(v, i)
        assert depth == n and tree_depth(nodes) == n and is_chain(nodes)
        assert (~nodes["c"][:, 1]).tolist() == list(range(n - 1, 0, -1)) and nodes["c"][n - 2, 0] == ~0
        hw = stack_high_water(nodes, rays)
        m = len(rays) // 2
        assert np.all(hw[:m] == n - 1) and np.all(hw[m:] == 1), hw


def test_wider_spacing_breaks_the_chain():
    """the spacing matters: ten times the z step and the chain ends near 20 triangles (cluster [0, k) is then nearer to nothing than
    triangle k is to k + 1)"""
    def spaced(n, dz):
        v, i = chain_mesh(n, scale=1.0)
        k = np.repeat(np.arange(n), 3)
        v["position"][:, 2] = (dz * (k - (n - 1) / 2)).astype(F)
        return v, i
    assert ploc_model(*spaced(19, 0.005))[2] == 19
    assert ploc_model(*spaced(32, 0.005))[2] < 32
    assert ploc_model(*spaced(32, 0.0005))[2] == 32


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_default_builder_model_on_tied_areas_is_as_deep_as_the_mesh(name):
    v, i = DEGENERATE[name]()
    n = len(i) // 3
    nodes, _, depth = ploc_model(v, i)
    print("%s: %d triangles, clustered depth %d" % (name, n, depth))
    assert depth == n and depth > 64 and tree_depth(nodes) == n
