"""What the lit-frame tests share (test_lit_cpu.py, test_gpu_lit.py, test_gpu_lit_tree_matrix.py): the contract of rr_render_lit on
the CPU, with no new C -- sample k is surfaces_helpers.ref_shade of composed_helpers.sample_rays in the Scene of key_k under T_band_k,
with the lights rr.moved_lights(lights, shapes, *light_offset_k), folded by the shutter helpers' weighted fold -- and the fixtures:
the soft-shadow table and the moving tumbler with an opaque olive.  Each reference is computed once per process."""
import numpy as np

import composed_helpers as CH
import materials_helpers as MH
import refraction_raytracing_dxr_amd as rr
import shutter_helpers as KH
import surfaces_helpers as SH
from nested_helpers import TABLE

W, H = MH.W, MH.H                                           # 48 x 36
KW = dict(max_refract=8)


def records(positions, lens_offsets, bands, keys, light_offsets):
    """LIT_SAMPLE_DTYPE [S]: shutter_helpers.records with light_offsets[k] (None: zeros)"""
    src = KH.records(positions, lens_offsets, bands, keys)
    rec = np.zeros(len(src), rr.LIT_SAMPLE_DTYPE)
    for f in ("offset", "lens_offset", "band", "key"):
        rec[f] = src[f]
    if light_offsets is not None:
        rec["light_offset"] = np.asarray(light_offsets, np.float32)
    return rec


def as_shutter(recs):
    """the records without their light offsets, as render_shutter takes them"""
    out = np.zeros(len(recs), rr.SHUTTER_SAMPLE_DTYPE)
    for f in ("offset", "lens_offset", "band", "key"):
        out[f] = recs[f]
    return out


def ref_lit(scenes, camera, w, h, recs, lens, table, surf, lts, shapes, ambient, iors=None, weights=None, **kw):
    """rr_render_lit's contract on the CPU -> (rgb [h, w, 3], counts [h, w], the unweighted colours [S, h, w, 3], per sample
    (colour [h, w, 3], counts [h, w], the surfaces reference's tallies))"""
    k = [0]

    def shade(key, rays, t):
        rec = recs[k[0]]
        k[0] += 1
        moved = rr.moved_lights(lts, shapes, *(float(v) for v in rec["light_offset"]))
        rgb, _, cnt, tl = SH.ref_shade(scenes[key], rays, t, surf, moved, ambient, **kw)
        return rgb, cnt, (rgb.reshape(h, w, 3).copy(), cnt.reshape(h, w).copy(), tl)
    return KH.fold_keys(shade, camera, w, h, recs, lens, table, iors, weights, **kw)


# ------------------------------------------------------------------------------------------------- the soft-shadow fixture
SOFT_SHAPE = ((0.4, 0.0, 0.0), (0.0, 0.0, 0.4))
SOFT_OFFSETS = np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], np.float32)


class Lit(SH.Fixture):
    """a surfaces fixture with the shapes of its lights"""

    def __init__(self, scene, surf, lts, ambient, shapes, table=TABLE):
        super().__init__(scene, surf, lts, ambient, table)
        self.shapes = shapes

    def load(self, r):
        super().load(r)
        r.set_light_shapes(self.shapes)

    def lit(self, camera, w, h, recs, lens=None, iors=None, weights=None, scenes=None, **kw):
        return ref_lit([self.scene] if scenes is None else scenes, camera, w, h, recs, lens, self.table, self.surf, self.lights, self.shapes,
                       self.ambient, iors, weights, **kw)


def shapes(*rows):
    return np.array(list(rows), rr.LIGHT_SHAPE_DTYPE) if rows else None


def soft(sun=False):
    """surfaces_helpers.table() under its lamp alone, a point light at LAMP_AT that sees everything, with no ambient term: a square
    of half-edge 0.4 in the xz-plane.  sun: the table's sun beside it (a directional light with a shape of its own)"""
    t = SH.table()
    lamp = rr.point_light(SH.LAMP_AT, (2.0, 2.2, 2.6), 0xff)
    if not sun:
        return Lit(t.scene, t.surf, SH.lights(lamp), None, shapes(rr.light_shape(*SOFT_SHAPE)))
    return Lit(t.scene, t.surf, SH.lights(t.lights[0], lamp), None, shapes(rr.light_shape((0.1, 0.0, 0.0), (0.0, 0.0, 0.15)), rr.light_shape(*SOFT_SHAPE)))


def soft_records(position=(0.5, 0.5)):
    """the four corners of the lamp at one sub-pixel position, key 0, band 0"""
    return records([position] * 4, None, 0, 0, SOFT_OFFSETS)


def soft_view(w=W, h=H):
    return MH.view(*SH.VIEW, w, h)


_refs = {}


def soft_ref(max_reflect=2):
    """(fixture, camera, records, ref_lit's result) of the soft-shadow fixture at pixel centres, W x H"""
    if max_reflect not in _refs:
        fx, cam, recs = soft(), soft_view(), soft_records()
        _refs[max_reflect] = (fx, cam, recs, fx.lit(cam, W, H, recs, max_reflect=max_reflect, **KW))
    return _refs[max_reflect]


def occluded(sample):
    """bool [h, w]: the pixel's colour is exactly 0 and it traced exactly two rays -- the floor hit and a shadow ray that was blocked"""
    col, cnt, _ = sample
    return (col == 0.0).all(axis=-1) & (cnt == 2)


# ------------------------------------------------------------------------------------------------- the moving olive
OLIVE_SURF = SH.surfaces(rr.glass(), rr.glass(), rr.glass(), rr.opaque((0.4, 0.5, 0.1), emission=(0.1, 0.2, 0.05)))
# every instance of the moving keys has InstanceMask 1: the first light's shadow rays see them all and stop in the glass round the
# olive, the second's (shadow_mask 0x02) see none, are traced and counted all the same, and light it through the glass
OLIVE_LIGHTS = SH.lights(rr.point_light((2.0, 2.5, 1.0), (6.0, 6.0, 6.0), 0xff), rr.point_light((-1.5, 2.0, 2.0), (3.0, 3.0, 3.0), 0x02))
OLIVE_SHAPES = shapes(rr.light_shape((0.5, 0.0, 0.0), (0.0, 0.0, 0.5)), rr.light_shape((0.0, 0.3, 0.0), (0.3, 0.0, 0.0)))
OLIVE_AMBIENT = (0.02, 0.02, 0.02)


def moving_olive():
    """the three keys of shutter_helpers.moving_keys() with the innermost cube (row 3) opaque and emissive, as surfaces_helpers.olive
    has it, under two shaped point lights outside the glass -> (Lit of key 0, the three Scenes)"""
    scs = KH.moving_keys()
    return Lit(scs[0], OLIVE_SURF, OLIVE_LIGHTS, OLIVE_AMBIENT, OLIVE_SHAPES), scs


def olive_records():
    """the three keys crossed with two light offsets, out of order, through lens points of lens_pattern(6)"""
    from nested_helpers import OFF3
    keys = [2, 0, 1, 1, 0, 2]
    lo = np.array([[-1.0, 0.5], [0.75, -1.0]], np.float32)
    return records(np.repeat(OFF3, 2, axis=0), rr.lens_pattern(6), 0, keys, lo[[0, 0, 0, 1, 1, 1]])
