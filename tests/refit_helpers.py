"""What other tests take from the refit tests (test_gpu_refit.py): deformed copies of a mesh, a BLAS's downloaded bytes, and the
two-instance scene of the TLAS updates."""
import numpy as np

import refraction_raytracing_dxr_amd as rr


def deform(verts, kind, seed=0, amount=1.0):
    """a copy of the vertex records with moved positions (and, for some kinds, moved normals)"""
    v = verts.copy()
    P = v["position"].astype(np.float64)
    rng = np.random.default_rng(seed)
    if kind == "wave":
        P[:, 1] += 0.15 * amount * np.sin(4.0 * P[:, 0] + 0.7 * seed) * np.cos(3.0 * P[:, 2])
        N = v["norm"].astype(np.float64)
        N[:, 0] += 0.2 * amount * np.cos(4.0 * P[:, 0] + 0.7 * seed)
        v["norm"] = (N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    elif kind == "scale":                          # x3 and translated: bounds and grid move
        P = P * 3.0 + np.array([0.5, -0.25, 1.0])
    elif kind == "jitter":
        P += rng.normal(size=P.shape) * 0.02 * amount
        N = v["norm"].astype(np.float64) + rng.normal(size=P.shape) * 0.1
        v["norm"] = (N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)).astype(np.float32)
    elif kind == "permute":                        # positions shuffled across vertices: the kept tree fits the new mesh badly
        P = P[rng.permutation(len(P))]
    else:
        raise ValueError(kind)
    v["position"] = P.astype(np.float32)
    return v


def blas_bytes(gpu, mid):
    nodes, tris = gpu.download_blas(mid)
    q, org, cell = gpu.download_qnodes(mid)
    return nodes, tris, q, org, cell


def _two_instances(mid, shift):
    t0 = np.eye(4, dtype=np.float32)[:3].copy()
    t0[0, 3] = -0.9
    t1 = np.array([[0.0, 0.0, 0.7, 0.9 + shift], [0.0, 0.7, 0.0, 0.2 * shift], [-0.7, 0.0, 0.0, 0.0]], np.float32)
    return rr.make_instances(transforms=[t0, t1], meshes=[mid, mid], masks=[1, 1 if shift < 0.5 else 3],
                             flags=[0, rr._capi.INSTANCE_FLAG_CULL_DISABLE if shift > 0 else 0])
