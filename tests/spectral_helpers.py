"""The references of the spectral frames (test_spectral_cpu.py, test_gpu_spectral.py): the weighted resolve rule in np.float32, a
few hand-made band tables, and the CPU oracle's frame of four bands with distinct indices of refraction."""
import numpy as np

import refraction_raytracing_dxr_amd as rr
from shading_helpers import oracle_colours

F = np.float32
# four hand-made bands: distinct iors, a negative weight (XYZ-derived tables have them), a zero weight and weights above 1
BANDS4 = np.array([(1.27, (1.5, 0.0, -0.25)), (1.3, (0.75, 1.25, 0.5)), (1.34, (0.5, 2.0, 1.0)), (1.41, (1.25, 0.75, 2.75))], rr.BAND_DTYPE)
ORACLE_VIEW = (1.3, 0.35)
ORACLE_KW = dict(max_refract=8, max_reflect=2)


def uniform_bands(n, ior):
    """the table bands=None stands for"""
    t = np.zeros(n, rr.BAND_DTYPE)
    t["ior"] = ior
    t["weight"] = 1.0
    return t


def weighted_fold(colours, weights):
    """the resolve rule of rr_render_spectral over a list of [..., 3] float32 colours and as many [3] float32 weights, in np.float32:
    p_k = w_k * c_k, the sum starts at p_0 and takes the others in their order, then / S.  Every operation rounds once."""
    assert len(colours) == len(weights) and len(colours) >= 1
    s = np.asarray(colours[0], F) * np.asarray(weights[0], F)
    for c, w in zip(colours[1:], weights[1:]):
        s = s + np.asarray(c, F) * np.asarray(w, F)
    assert s.dtype == F
    return s / F(len(colours))


_cache = {}


def oracle_spectral_frame():
    """monkey.obj at shading_helpers' 52x37 frame: band k of BANDS4 rendered by the CPU oracle at 4x resolution with rro_params.ior =
    ior_k, sub-pixel SUB4[k] of it taken as sample k (oracle_colours lists SUB4 first), folded with the bands' weights
    -> (rgb [H, W, 3], counts [H, W], the four unweighted colours [4, H, W, 3])"""
    if "frame" not in _cache:
        cols, cnts = [], []
        for k in range(4):
            c, n = oracle_colours(*ORACLE_VIEW, ior=float(BANDS4["ior"][k]), **ORACLE_KW)
            cols.append(c[k])
            cnts.append(n[k])
        _cache["frame"] = (weighted_fold(cols, list(BANDS4["weight"])), sum(cnts).astype(np.uint32), np.stack(cols))
    return _cache["frame"]
