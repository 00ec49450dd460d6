"""What the composed-frame tests share (test_composed_cpu.py, test_gpu_composed.py): the sample records of the fixtures, the band
tables T_b of a band set as material tables, and the contract of rr_render_composed on the CPU -- sample k is nested_helpers.ref_shade
of rr.lens_rays under T_band_k, resolved by spectral_helpers.weighted_fold.  Each reference is computed once per process."""
import numpy as np

import materials_helpers as MH
import nested_helpers as NH
import refraction_raytracing_dxr_amd as rr
from nested_helpers import FH, FW, OFF3, TABLE
from spectral_helpers import weighted_fold

LENS = rr.Lens(0.15, 5.0)
ABBE = 25.0
BAND_ORDER = [1, 0, 0, 1, 1, 0]                             # three positions, each in both bands, deliberately not 0, 1, 0, 1, ...
KW = dict(max_refract=8)


def records(positions, lens_offsets, bands):
    """COMPOSED_SAMPLE_DTYPE [S]: sample k has positions[k], lens_offsets[k] (None: zeros) and bands[k]"""
    rec = np.zeros(len(positions), rr.COMPOSED_SAMPLE_DTYPE)
    rec["offset"] = np.asarray(positions, np.float32)
    if lens_offsets is not None:
        rec["lens_offset"] = np.asarray(lens_offsets, np.float32)
    rec["band"] = bands
    return rec


def fixture_records():
    """the six samples of the tumbler, overlap and monkey fixtures: position k // 2 of OFF3, band BAND_ORDER[k], lens point k of
    lens_pattern(6)"""
    return records(np.repeat(OFF3, 2, axis=0), rr.lens_pattern(6), BAND_ORDER)


def fixture_bands():
    """(iors [2, 6], weights [2, 3]): TABLE in two bands of Abbe number 25"""
    return rr.material_bands(TABLE, ABBE, 2)


def band_table(table, iors, b):
    """T_b: the material table with band b's column of indices"""
    t = np.array(table, rr.MATERIAL_DTYPE).reshape(-1).copy()
    t["ior"] = np.asarray(iors, np.float32)[b]
    return t


def sample_rays(camera, w, h, rec, lens, p):
    """the rays of sample `rec` of the contract: rr_host_lens_rays, or rr_host_camera_rays without a lens or with radius 0"""
    ox, oy = (float(v) for v in rec["offset"])
    if lens is None or lens.radius == 0.0:
        return rr.camera_rays(camera, w, h, ox, oy, p.tmin_primary, p.tmax_primary)
    lx, ly = (float(v) for v in rec["lens_offset"])
    return rr.lens_rays(camera, w, h, ox, oy, lx, ly, lens, p.tmin_primary, p.tmax_primary)


def fold_samples(shade, camera, w, h, recs, lens, table, iors, weights, **kw):
    """the contract's fold with shade(rays, T_band) -> (rgb [n, 3], counts [n], extra) giving c_k -> (rgb [h, w, 3], counts [h, w],
    the unweighted colours [S, h, w, 3], the extras)"""
    p = rr.default_params(**kw)
    iors = np.asarray(table["ior"], np.float32)[None, :] if iors is None else iors
    weights = np.ones((len(iors), 3), np.float32) if weights is None else np.asarray(weights, np.float32)
    cols, total, extras = [], np.zeros(w * h, np.uint32), []
    for rec in recs:
        b = int(rec["band"])
        rgb, cnt, extra = shade(sample_rays(camera, w, h, rec, lens, p), band_table(table, iors, b))
        cols.append(np.ascontiguousarray(rgb, np.float32).reshape(h, w, 3))
        total += cnt
        extras.append(extra)
    return weighted_fold(cols, [weights[int(r["band"])] for r in recs]), total.reshape(h, w), np.stack(cols), extras


def ref_composed(sc, camera, w, h, recs, lens, table, iors=None, weights=None, **kw):
    """rr_render_composed's contract on the CPU, c_k from the nested reference; the extras are its tallies per sample"""
    def shade(rays, t):
        rgb, _, cnt, tl = NH.ref_shade(sc, rays, t, **kw)
        return rgb, cnt, tl
    return fold_samples(shade, camera, w, h, recs, lens, table, iors, weights, **kw)


_refs = {}


def tumbler_ref(max_reflect, negative=False):
    """(scene, camera, records, iors, weights, ref_composed's result) of the tumbler fixture at FW x FH through LENS; negative: one
    weight of band 1 made negative"""
    key = (max_reflect, negative)
    if key not in _refs:
        sc = NH.tumbler()
        cam = MH.view(*NH.VIEW, FW, FH)
        iors, weights = fixture_bands()
        if negative:
            weights = weights.copy()
            weights[1, 2] = -0.5
        recs = fixture_records()
        _refs[key] = (sc, cam, recs, iors, weights, ref_composed(sc, cam, FW, FH, recs, LENS, TABLE, iors, weights, max_reflect=max_reflect, **KW))
    return _refs[key]


# ------------------------------------------------------------------------------------------------- the cube reductions
CUBE_IOR = 1.5
CUBE_TABLE = MH.uniform(CUBE_IOR, 3)                        # NH.reduction_scene("cube.obj") is made of row 1; no absorption
CUBE_VIEW = NH.REDUCTION_VIEWS["cube.obj"]
CUBE_KW = dict(max_refract=8, max_reflect=3)


def cube_lens_records():
    """the lens reduction: the built-in pattern of four positions, the built-in lens points, band 0"""
    return records(rr.sample_pattern(4), rr.lens_pattern(4), 0)


def cube_spectral():
    """the spectral reduction: OFF3 crossed with two bands of rr_host_spectral_bands(2, CUBE_IOR, ABBE) -> (records, BAND_DTYPE [2],
    iors [2, 3], weights [2, 3])"""
    bands = rr.spectral_bands(2, CUBE_IOR, ABBE)
    iors = np.repeat(bands["ior"][:, None], len(CUBE_TABLE), axis=1).astype(np.float32)
    return records(np.repeat(OFF3, 2, axis=0), None, np.tile(np.arange(2), len(OFF3))), bands, iors, np.ascontiguousarray(bands["weight"], np.float32)


def cube_tallies(recs, lens, iors):
    """the nested reference's tallies of every sample of a cube reduction frame"""
    sc = NH.reduction_scene("cube.obj")
    return ref_composed(sc, MH.view(*CUBE_VIEW, FW, FH), FW, FH, recs, lens, CUBE_TABLE, iors, None, **CUBE_KW)[3]
