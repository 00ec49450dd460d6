"""Indexed twins of un-indexed meshes, and natively indexed grids.

TEST INFRASTRUCTURE ONLY: imported by tests/test_indexed_cpu.py and tests/test_gpu_indexed.py.

Every mesh the rest of the suite uploads has indices = 0..3T-1 (the OBJ loader writes them so, as the reference's Mesh::load
does), so n_verts == n_idx everywhere and an index buffer is never more than the identity.  The generators here turn such a
mesh into the same geometry behind a real index buffer.  All of them are seeded and keep the triangle order, so primitive ids
compare directly.  For any variant (V, I) the flat twin is flat(V, I) = (V[I], arange(len(I))): the same triangles in the form
the rest of the suite already proves correct.
"""
import numpy as np

VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("norm", "<f4", 3), ("uv", "<f4", 2)])
assert VERTEX_DTYPE.itemsize == 32

VARIANTS = ("welded", "shuffled", "holes", "padded", "smooth", "degenerate")
N_HOLES = 7                 # unreferenced vertices at the front, inside and at the end of `holes`
N_PAD_EXTRA = 5             # `padded` has n_idx + N_PAD_EXTRA vertices
GRID_SIDES = (1, 2, 8, 181)  # 181: 65 522 triangles, above the 32 768 of the clustered builder -- the plain LBVH builds it


def _records(verts):
    v = np.ascontiguousarray(verts)
    assert v.dtype.itemsize == 32 and v.ndim == 1
    return v.view(VERTEX_DTYPE)


def flat(verts, indices):
    """the un-indexed twin: one vertex record per corner, identity indices"""
    v = np.ascontiguousarray(_records(verts)[np.asarray(indices, np.int64)])
    return v, np.arange(len(v), dtype=np.uint32)


def _unique_rows(words):
    _, first, inv = np.unique(words, axis=0, return_index=True, return_inverse=True)
    return first, np.asarray(inv).reshape(-1)


def welded(verts):
    """unique 32-byte vertex records (compared as bytes: -0.0 and 0.0 stay apart), indices into them"""
    v = _records(verts)
    first, inv = _unique_rows(v.view(np.uint32).reshape(-1, 8))
    return np.ascontiguousarray(v[first]), inv.astype(np.uint32)


def _permuted(V, I, rng):
    perm = rng.permutation(len(V))
    where = np.empty(len(V), np.int64)
    where[perm] = np.arange(len(V))                     # old vertex j now sits at where[j]
    return np.ascontiguousarray(V[perm]), where[I].astype(np.uint32)


def shuffled(verts, seed=0):
    """`welded` with the vertex order permuted"""
    V, I = welded(verts)
    return _permuted(V, I, np.random.default_rng([seed, 1]))


def junk_vertices(n, rng):
    """unreferenced vertices: finite positions far outside any mesh of the suite (|x| between 5e5 and 2e6 on every axis),
    garbage normals and uvs (huge values, infinities, NaNs -- only positions have to be finite)"""
    v = np.zeros(n, VERTEX_DTYPE)
    v["position"] = (rng.uniform(5e5, 2e6, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    junk = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 30, (n, 3))
    junk[rng.random((n, 3)) < 0.15] = np.nan
    junk[rng.random((n, 3)) < 0.10] = np.inf
    with np.errstate(over="ignore"):
        v["norm"] = junk.astype(np.float32)
    v["uv"] = rng.uniform(-1e9, 1e9, (n, 2)).astype(np.float32)
    return v


def holes(verts, seed=0):
    """`shuffled` plus N_HOLES unreferenced vertices at the front, N_HOLES scattered inside and N_HOLES at the end"""
    V, I = shuffled(verts, seed)
    rng = np.random.default_rng([seed, 2])
    n_in = len(V) + N_HOLES                              # referenced + inside ones, between the front and end blocks
    inside = np.sort(rng.choice(np.arange(1, n_in - 1), N_HOLES, replace=False)) if n_in > 2 + N_HOLES else np.arange(1, 1 + N_HOLES)
    is_hole = np.zeros(n_in, bool)
    is_hole[inside] = True
    slot = np.flatnonzero(~is_hole)                     # referenced vertex k sits at middle slot slot[k]
    mid = np.zeros(n_in, VERTEX_DTYPE)
    mid[slot] = V
    mid[inside] = junk_vertices(N_HOLES, rng)
    out = np.concatenate([junk_vertices(N_HOLES, rng), mid, junk_vertices(N_HOLES, rng)])
    return np.ascontiguousarray(out), (slot[I] + N_HOLES).astype(np.uint32)


def hole_mask(verts, indices):
    """True for every vertex no index refers to"""
    m = np.ones(len(verts), bool)
    m[np.asarray(indices, np.int64)] = False
    return m


def padded(verts, seed=0):
    """`welded` plus unreferenced vertices at the end until n_verts = n_idx + N_PAD_EXTRA: code that read verts[3 * prim + k]
    instead of verts[idx[3 * prim + k]] stays inside the vertex buffer of this variant, and is merely wrong"""
    V, I = welded(verts)
    rng = np.random.default_rng([seed, 3])
    n = len(I) + N_PAD_EXTRA - len(V)
    return np.ascontiguousarray(np.concatenate([V, junk_vertices(n, rng)])), I


def smooth(verts):
    """welded by position only; the normal of a vertex is the re-normalised mean of its corners' normals (computed in float64,
    the first corner's normal where the mean vanishes), its uv the first corner's.  Another shading input than the source's:
    what an indexed asset with smooth normals looks like."""
    v = _records(verts)
    first, inv = _unique_rows(np.ascontiguousarray(v["position"]).view(np.uint32).reshape(-1, 3))
    V = np.ascontiguousarray(v[first])
    acc = np.zeros((len(V), 3), np.float64)
    np.add.at(acc, inv, v["norm"].astype(np.float64))
    ln = np.linalg.norm(acc, axis=1)
    ok = ln > 1e-9
    V["norm"][ok] = (acc[ok] / ln[ok, None]).astype(np.float32)
    return V, inv.astype(np.uint32)


def degenerate_layout(n_src_tris, seed=0):
    """-> (p, [ids of the three index-degenerate triangles], id of the duplicate of triangle p) in `degenerate`"""
    p = int(np.random.default_rng([seed, 4]).integers(0, n_src_tris))
    return p, [n_src_tris, n_src_tris + 1, n_src_tris + 2], n_src_tris + 3


def degenerate(verts, seed=0, of=None):
    """`shuffled` with four triangles appended: with (a, b, c) the indices of triangle p, the index-degenerate (a, a, b),
    (a, b, a), (a, a, a), then the exact duplicate (a, b, c).  p is degenerate_layout's, or `of`."""
    V, I = shuffled(verts, seed)
    p = degenerate_layout(len(I) // 3, seed)[0] if of is None else int(of)
    a, b, c = (int(x) for x in I[3 * p:3 * p + 3])
    extra = np.array([a, a, b, a, b, a, a, a, a, a, b, c], np.uint32)
    return V, np.concatenate([I, extra])


def variant(name, verts, seed=0):
    """the indexed twin `name` (one of VARIANTS) of an un-indexed mesh's vertex records"""
    if name in ("welded", "smooth"):
        return globals()[name](verts)
    if name in ("shuffled", "holes", "padded", "degenerate"):
        return globals()[name](verts, seed)
    raise ValueError(name)


_TILT = np.deg2rad(55.0)       # about the x axis: the orbit camera circles in the plane y = 0 and would see a level grid edge-on
GRID_TILT = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(_TILT), -np.sin(_TILT)], [0.0, np.sin(_TILT), np.cos(_TILT)]])
GRID_UP = GRID_TILT[:, 1]      # the side every triangle of a heightfield faces


def heightfield(n, seed=0):
    """a natively indexed grid over [-1, 1]^2, tilted by GRID_TILT: (n + 1)^2 vertices, 2 n^2 triangles, a bumpy height with its
    analytic normals"""
    rng = np.random.default_rng([seed, 5, n])
    g = np.linspace(-1.0, 1.0, n + 1)
    x, z = np.meshgrid(g, g, indexing="ij")
    y = 0.25 * np.sin(3.0 * x + 0.4) * np.cos(2.5 * z) + 0.002 * rng.standard_normal(x.shape)
    dx = 0.75 * np.cos(3.0 * x + 0.4) * np.cos(2.5 * z)
    dz = -0.625 * np.sin(3.0 * x + 0.4) * np.sin(2.5 * z)
    N = np.stack([-dx, np.ones_like(dx), -dz], -1)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    V = np.zeros((n + 1) * (n + 1), VERTEX_DTYPE)
    V["position"] = (np.stack([x, y, z], -1).reshape(-1, 3) @ GRID_TILT.T).astype(np.float32)
    V["norm"] = (N.reshape(-1, 3) @ GRID_TILT.T).astype(np.float32)
    V["uv"] = np.stack([(x + 1) / 2, (z + 1) / 2], -1).reshape(-1, 2).astype(np.float32)
    k = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = k[:-1, :-1].ravel(), k[1:, :-1].ravel(), k[1:, 1:].ravel(), k[:-1, 1:].ravel()
    I = np.stack([a, d, c, a, c, b], 1).reshape(-1).astype(np.uint32)     # two triangles per cell, facing GRID_UP
    return V, I


def one_triangle():
    """one triangle with indices (2, 0, 1) over four vertices (vertex 3 is unreferenced and far away)"""
    V = np.zeros(4, VERTEX_DTYPE)
    V["position"] = [(0.8, -0.5, 0.1), (-0.1, 0.9, -0.2), (-0.9, -0.6, 0.3), (4.0e5, -7.0e5, 1.0e6)]
    V["norm"] = [(0.1, 0.2, 0.97), (-0.2, 0.1, 0.97), (0.0, -0.1, 0.99), (np.nan, 1e30, -np.inf)]
    V["norm"][:3] /= np.linalg.norm(V["norm"][:3], axis=1, keepdims=True)
    return V, np.array([2, 0, 1], np.uint32)
