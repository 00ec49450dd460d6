"""CPU models of the radix-tree builder and of the instance boxes, the input families of the builder-size tests and the checks they
share (test_builder_models_cpu.py, test_gpu_capacity_edges.py).  depth_meshes.py has the clustered builder's model (ploc_model) and
the stack walk (pushed_refs).  No GPU code: numpy only.

A model is compared with the GPU's tree exactly (same_tree): child refs, leaf order and depth as integers, box planes by value
(np.array_equal: the sign of a zero that a min or a max returns is not specified, and the families below hold no negative zero)."""
import bisect

import numpy as np

import refraction_raytracing_dxr_amd as rr
from depth_meshes import F, _mesh, morton_keys, pack_nodes, tri_boxes

PLANES = ("lox", "loy", "loz", "hix", "hiy", "hiz")


# ------------------------------------------------------------------------------------------------------------ input families
def soup(T, seed=1):
    """T seeded random small triangles in the unit cube [-1, 0]^3: the end of the Morton order, where the largest node and leaf
    indices are, lies at the origin, which the orbit camera looks at"""
    rng = np.random.default_rng(seed * 100003 + T)
    P = rng.uniform(-1.0, 0.0, (T, 1, 3)) + rng.uniform(-0.02, 0.02, (T, 3, 3))
    return _mesh(P.astype(F) + F(0))


def lattice(T):
    """the first T cells (x fastest) of a cubic grid of equal triangles, one per unit cell: (x, y, z), (x + 1/2, y, z),
    (x, y + 1/2, z), every coordinate exact in fp32, so the merged-box areas of equally placed pairs tie everywhere and the
    candidate order and the mutual-pair rule decide the clustered tree"""
    side = 1
    while side ** 3 < T:
        side += 1
    k = np.arange(T)
    o = np.stack([k % side, (k // side) % side, k // (side * side)], -1).astype(F)[:, None, :]
    P = o + np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]], F)[None]
    return _mesh(P * F(0.125))


def line(T):
    """T equal triangles across the diagonal (1, 1, 1), centroids on it: triangle k starts 1 to 8 steps of 2^-23 (seeded) after
    triangle k - 1, the last one at (8, 8, 8).  The scene box is 8 wide, a Morton cell 2^-7, so thousands of triangles in a row
    share each code and the index bits of the key decide their order.  (The uneven steps keep the clustered builder's rounds few:
    with even ones every cluster's nearest neighbour is the one before it and one pair merges a round.)"""
    t = np.concatenate([[0], np.cumsum(np.random.default_rng(T).integers(1, 9, max(T - 1, 0)))]).astype(np.float64) * 2.0 ** -23
    t[-1] = 8.0
    p = (t[:, None] * np.ones(3))[:, None, :]
    P = p + 0.25 * np.eye(3)[None]
    return _mesh(P.astype(F))


FAMILIES = {"soup": soup, "lattice": lattice, "line": line}


def has_negative_zero(verts):
    x = verts["position"]
    return bool(np.any((x == 0) & np.signbit(x)))


def aimed_rays(verts, idx, n, seed, prims=None):
    """n seeded rays from outside the mesh: three in four aimed at a point inside a triangle (of `prims`, or any), the rest at a
    point of the mesh's box; no culling, whole interval"""
    P = verts["position"][np.asarray(idx, np.int64)].reshape(-1, 3, 3).astype(np.float64)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    ext = max(float((hi - lo).max()), 0.5)
    rng = np.random.default_rng(seed)
    pick = rng.choice(np.arange(len(P)) if prims is None else np.asarray(prims), n)
    w = rng.dirichlet([2.0, 2.0, 2.0], n)
    target = np.einsum("nk,nkc->nc", w, P[pick])
    box = rng.random(n) < 0.25
    target[box] = rng.uniform(lo - 0.05 * ext, hi + 0.05 * ext, (int(box.sum()), 3))
    o = rng.normal(size=(n, 3))
    o = (lo + hi) / 2 + o / np.linalg.norm(o, axis=1, keepdims=True) * ext * 3
    d = target - o
    return rr.pack_rays(o, d / np.linalg.norm(d, axis=1, keepdims=True), 1e-4, 100.0 * ext)


# ------------------------------------------------------------------------------------------------------------ the radix tree
def karras_tree(keys, box, leaf_base=None):
    """The radix tree over sorted unique 64-bit keys (low word: the primitive) and the primitives' fp32 boxes [n, 6], n >= 2, by
    top-down recursion: a range of keys splits where the highest bit in which its first and last key differ changes.  Karras'
    numbering: the root is 0; a left child that is an internal node has the index of the last key of its range, a right child
    the index of the first key of its range.  Boxes by bottom-up union in fp32.  leaf_base=None: leaves are ~position (a BLAS);
    otherwise ~(leaf_base + primitive) (the TLAS).
    -> (NODE_DTYPE nodes, leaf position -> primitive, depth: nodes on the longest path, the leaf included,
        ranges [n - 1, 2]: first and last key position of every internal node)"""
    k = [int(x) for x in keys]
    n = len(k)
    assert n >= 2 and all(a < b for a, b in zip(k, k[1:]))
    prim = (np.asarray(keys, np.uint64) & np.uint64(0xffffffff)).astype(np.int64)
    child = np.zeros((n - 1, 2), np.int64)
    ranges = np.zeros((n - 1, 2), np.int64)
    node_box = np.zeros((2 * n - 1, 6), F)
    node_box[n - 1:] = np.asarray(box, F)[prim]
    depth, visit, todo = 0, [], [(0, 0, n - 1, 1)]
    while todo:
        node, first, last, d = todo.pop()
        visit.append(node)
        ranges[node] = first, last
        bit = (k[first] ^ k[last]).bit_length() - 1
        split = bisect.bisect_left(k, ((k[first] >> bit) | 1) << bit, first, last + 1)     # the first key with that bit set
        assert first < split <= last
        for side, (a, b, me) in enumerate(((first, split - 1, split - 1), (split, last, split))):
            if a == b:
                child[node, side] = ~a
                depth = max(depth, d + 1)
            else:
                child[node, side] = me
                todo.append((me, a, b, d + 1))
    for node in reversed(visit):                                      # children before parents
        l, r = (c if c >= 0 else (n - 1) + ~c for c in child[node].tolist())
        node_box[node, :3] = np.minimum(node_box[l, :3], node_box[r, :3])
        node_box[node, 3:] = np.maximum(node_box[l, 3:], node_box[r, 3:])
    nodes = pack_nodes(n, child, node_box)
    if leaf_base is not None:
        c = nodes["c"]
        nodes["c"] = np.where(c < 0, ~(leaf_base + prim[np.where(c < 0, ~c, 0)]), c)
    return nodes, prim, depth, ranges


def karras_model(verts, idx):
    """the radix-tree build of a mesh (fast_build=True, more than 32 768 triangles, or the fallback of a clustered tree deeper
    than 64) -> (nodes as rr_download_blas gives them, leaf position -> primitive, depth as k_depth counts it)"""
    box = tri_boxes(verts, idx)
    return karras_tree(morton_keys(box), box)[:3]


def karras_tlas_model(boxes, leaf_base):
    """the top level over per-instance world boxes fp32 [n, 6], n >= 2; leaves are ~(leaf_base + instance)"""
    boxes = np.asarray(boxes, F)
    return karras_tree(morton_keys(boxes), boxes, leaf_base)[:3]


# --------------------------------------------------------------------------------------------------------- instance boxes
def _fma32(a, b, c):
    """fmaf on fp32 arrays: a * b is exact in float64; the float64 sum is exact or, where it is not, is moved off a midpoint of
    two fp32 values towards the exact sum, so the rounding to fp32 is the single rounding of the exact a * b + c"""
    p = a.astype(np.float64) * np.float64(b)
    c = np.full_like(p, np.float64(c))
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                    # TwoSum: s + err == p + c exactly
    half = (s.view(np.uint64) & np.uint64(0x1fffffff)) == np.uint64(0x10000000)
    s = np.where(half & (err > 0), np.nextafter(s, np.inf), np.where(half & (err < 0), np.nextafter(s, -np.inf), s))
    return s.astype(F)


def inst_world_box_model(transforms, bounds):
    """inst_world_box in fp32: transforms [n, 12] (object to world, 3x4 row major), bounds [n, 6] (each instance's BLAS bounds)
    -> [n, 6].  Per corner ((m0 x + m1 y) + m2 z) + m3, min and max over the 8 corners, each plane grown by
    fmaf(|v|, 1e-5f, 1e-7f); an instance whose transform is the identity bit for bit keeps its corners"""
    M = np.ascontiguousarray(transforms, F).reshape(-1, 3, 4)
    bb = np.ascontiguousarray(bounds, F).reshape(-1, 6)
    ident = np.all(M.view(np.uint32) == np.eye(3, 4, dtype=F).view(np.uint32)[None], axis=(1, 2))
    lo = np.full((len(M), 3), np.inf, F)
    hi = np.full((len(M), 3), -np.inf, F)
    for c in range(8):
        x, y, z = (bb[:, 3 * ((c >> a) & 1) + a] for a in range(3))
        w = np.stack([((M[:, r, 0] * x + M[:, r, 1] * y) + M[:, r, 2] * z) + M[:, r, 3] for r in range(3)], -1)
        assert w.dtype == F
        w = np.where(ident[:, None], np.stack([x, y, z], -1), w)
        lo, hi = np.minimum(lo, w), np.maximum(hi, w)
    lo = lo - _fma32(np.abs(lo), F(1e-5), F(1e-7))
    hi = hi + _fma32(np.abs(hi), F(1e-5), F(1e-7))
    return np.concatenate([lo, hi], axis=1).astype(F)


# ------------------------------------------------------------------------------------------------------------- shared checks
def same_tree(nodes, model_nodes):
    """the comparison rule: child refs and pads exactly, box planes by value"""
    assert len(nodes) == len(model_nodes)
    assert np.array_equal(nodes["c"], model_nodes["c"])
    for f in PLANES:
        assert np.array_equal(nodes[f], model_nodes[f]), f
    assert not nodes["pad"].any()


def check_structure(nodes, tris, verts, idx):
    """leaf records of every primitive once, every node and leaf referenced once from the root, every child box the exact union
    of what is below it"""
    T = len(idx) // 3
    assert len(tris) == T and len(nodes) == T - 1
    assert sorted(tris["prim"].tolist()) == list(range(T))
    P = verts["position"][idx].reshape(T, 3, 3)
    assert np.array_equal(tris["v0"], P[tris["prim"], 0])
    assert np.array_equal(tris["e1"], P[tris["prim"], 1] - P[tris["prim"], 0])
    assert np.array_equal(tris["e2"], P[tris["prim"], 2] - P[tris["prim"], 0])
    leaf_box = np.concatenate([P[tris["prim"]].min(1), P[tris["prim"]].max(1)], axis=1)
    check_tree(nodes, leaf_box)


def check_tree(nodes, leaf_box, leaf_base=0):
    """every node and every leaf ~(leaf_base + k), k < len(leaf_box), referenced once from the root; every child box the exact
    union of what is below it, a leaf's being leaf_box[k]"""
    n = len(leaf_box)
    assert len(nodes) == n - 1
    seen_nodes, seen_leaves = np.zeros(n - 1, int), np.zeros(n, int)
    seen_nodes[0] = 1
    cc = nodes["c"].tolist()
    order, stack = [], [0]
    while stack:
        x = stack.pop()
        order.append(x)
        for c in cc[x]:
            if c >= 0:
                seen_nodes[c] += 1
                stack.append(c)
            else:
                assert 0 <= ~c - leaf_base < n
                seen_leaves[~c - leaf_base] += 1
    assert np.all(seen_nodes == 1) and np.all(seen_leaves == 1)
    planes = np.stack([nodes[f] for f in PLANES], -1)                  # [node, child, plane]
    box = np.zeros((n - 1, 6), F)
    for x in reversed(order):
        for k in (0, 1):
            c = cc[x][k]
            want = leaf_box[~c - leaf_base] if c < 0 else box[c]
            assert np.array_equal(planes[x, k], want), "node %d child %d" % (x, k)
        box[x, :3] = np.minimum(planes[x, 0, :3], planes[x, 1, :3])
        box[x, 3:] = np.maximum(planes[x, 0, 3:], planes[x, 1, 3:])


def check_quantised(q, org, cell, nodes, lo_bound, hi_bound, node_off=0, leaf_off=0):
    """the quantised nodes as traversal reads them against the fp32 nodes they were made from: every stored child box contains
    its fp32 box (evaluated in float64 from the same float32 grid the kernels use), by no more than the fp16 spacing there
    (<= 16 cells at the faces of the bounds) plus the guard cell; child refs are the same tree with internal refs as byte
    offsets; the grid spans the bounds [lo_bound, hi_bound], origin at their centre"""
    assert len(q) == len(nodes) and np.all(cell > 0)
    org, cell = org.astype(np.float64), cell.astype(np.float64)
    for ax, (lo, hi) in enumerate((("lox", "hix"), ("loy", "hiy"), ("loz", "hiz"))):
        qlo = org[ax] + q[lo].astype(np.float64) * cell[ax]
        qhi = org[ax] + q[hi].astype(np.float64) * cell[ax]
        flo, fhi = nodes[lo].astype(np.float64), nodes[hi].astype(np.float64)
        real = flo <= fhi                                      # (a one-triangle mesh has an empty second child)
        assert np.all(np.abs(q[lo][real].astype(np.float64)) <= 32768) and np.all(np.abs(q[hi][real].astype(np.float64)) <= 32768)
        assert np.all(qlo[real] <= flo[real]) and np.all(qhi[real] >= fhi[real])
        assert np.all(flo[real] - qlo[real] <= 18 * cell[ax]) and np.all(qhi[real] - fhi[real] <= 18 * cell[ax])
    c, qc = nodes["c"], q["c"]
    assert np.array_equal(qc[c < 0], ~(~c[c < 0] + leaf_off)) and np.array_equal(qc[c >= 0], (c[c >= 0] + node_off) * 32)
    lo_bound, hi_bound = np.asarray(lo_bound, np.float64), np.asarray(hi_bound, np.float64)
    assert np.all(org - 32768 * cell <= lo_bound) and np.all(org + 32768 * cell >= hi_bound)
    assert np.all(np.abs(org - (lo_bound + hi_bound) / 2) <= 8 * cell + 1e-6 * np.abs(org))
