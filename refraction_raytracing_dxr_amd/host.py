"""Host-side mirror of the reference's asset surface and frame driver, over the C ABI.

  Mesh            <-> Mesh.hpp:14-25 (load / verts / indices / upload)
  load_texture    <-> RefractionDemo.cpp:108-140 (stbi_loadf(...,3))
  camera_orbit    <-> RefractionDemo.cpp:559-566
  Renderer        <-> the D3D12 calls of RefractionDemo.cpp:272-361, 566, 580-611
  RefractionDemo  <-> RefractionDemo.hpp:9-10 (initialize / drawFrame)
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (DISPATCH_COLLECT_STATS, DISPATCH_FLOAT_OUTPUT, DISPATCH_KEEP_COUNTERS, DISPATCH_TIME_KERNEL, BAND_DTYPE, HIT_DTYPE, INSTANCE_DTYPE, LIGHT_DTYPE, MATERIAL_DTYPE, NODE_DTYPE, RAY_DTYPE, SURFACE_DTYPE,
                    TRI_DTYPE, VERTEX_DTYPE, DispatchParams, Lens, RRError, SceneConstants, Stats)

FOV_Y = float(np.float32(52.0 / 180.0 * 3.1415))     # RefractionDemo.cpp:559
ASPECT = float(np.float32(1.333))
TILE = 32
# render_adaptive's default threshold, in display units (1 = the whole range of a channel): DESIGN 5.7 has how it was chosen
ADAPTIVE_THRESHOLD = 0.05


def default_params(**kw):
    p = DispatchParams()
    _capi.lib().rr_default_dispatch_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def camera_orbit(angle, fov_y=FOV_Y, aspect=ASPECT, zn=1.0, zf=125.0):
    """-> SceneConstants for the orbit angle (frame k of the reference uses 0.01*(k+1))."""
    sc = SceneConstants()
    rc = _capi.lib().rr_host_camera_orbit(float(np.float32(angle)), fov_y, aspect, zn, zf, C.byref(sc))
    if rc:
        raise RRError(rc, "rr_host_camera_orbit")
    return sc


def scene_constants(proj_inv, camera_loc):
    sc = SceneConstants()
    sc.proj_inv[:] = [float(v) for v in np.asarray(proj_inv, np.float32).reshape(16)]
    sc.camera_loc[:] = [float(v) for v in np.asarray(camera_loc, np.float32).reshape(4)]
    return sc


def load_texture(filename, req_comp=3):
    """stbi_loadf(filename,&x,&y,&n,req_comp) -> (float32 [h,w,req_comp], channels_in_file)."""
    L = _capi.lib()
    x, y, n = C.c_int(), C.c_int(), C.c_int()
    p = L.rr_host_image_loadf(str(filename).encode(), C.byref(x), C.byref(y), C.byref(n), req_comp)
    if not p:
        raise RRError(6, "rr_host_image_loadf(%s)" % filename)
    oc = req_comp if req_comp else n.value
    arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(y.value, x.value, oc)).copy()
    L.rr_host_free(p)
    return arr, n.value


def write_hdr(filename, rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w, c = rgb.shape
    assert c == 3
    rc = _capi.lib().rr_host_image_write_hdr(str(filename).encode(), w, h, rgb.ctypes.data)
    if rc:
        raise RRError(rc, "rr_host_image_write_hdr")


def sample_pattern(n):
    """-> float32 [n, 2]: the built-in sub-pixel positions of render_samples(samples=n), D3D's standard multisample pattern for
    n = 1, 2, 4, 8 or 16, in pixel units ((0.5, 0.5) is the pixel centre)"""
    n = int(n)
    out = np.zeros((max(n, 1), 2), np.float32)
    rc = _capi.lib().rr_host_sample_pattern(n if n >= 0 else 0, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise RRError(rc, "rr_host_sample_pattern(%d)" % n)
    return out


def spectral_bands(n, ior_d=1.3, abbe=30.0):
    """-> BAND_DTYPE [n]: a band table for render_spectral (rr_host_spectral_bands), n = 1..64 bands at the midpoints of n equal
    slices of 400..700 nm.  ior follows Cauchy's law through ior_d at 587.6 nm with the Abbe number abbe (smaller: more dispersion;
    inf: none); the weights are tents of half-width 100 nm round 650 (R), 550 (G) and 450 nm (B), each channel summing to n, so a
    white environment stays white.  n == 1: (ior_d, 1, 1, 1)."""
    n = int(n)
    out = np.zeros(max(n, 1), BAND_DTYPE)
    rc = _capi.lib().rr_host_spectral_bands(n if n >= 0 else 0, float(np.float32(ior_d)), float(abbe), out.ctypes.data)
    if rc:
        raise RRError(rc, "rr_host_spectral_bands(%d, %r, %r)" % (n, ior_d, abbe))
    return out


def material_bands(table, abbe=30.0, n=8):
    """-> (iors float32 [n, rows], weights float32 [n, 3]): a band set for Renderer.set_material_bands -- dispersion per material.
    Column r of iors is spectral_bands(n, table[r].ior, abbe_r)["ior"]: Cauchy's law through the row's own index.  abbe: one Abbe
    number for every row or one per row; inf gives that row no dispersion.  The weights are those of spectral_bands(n): they
    do not depend on the row.  table: a MATERIAL_DTYPE array or rows of (ior, (sigma_r, sigma_g, sigma_b))."""
    t = np.ascontiguousarray(table, MATERIAL_DTYPE).reshape(-1)
    ab = np.broadcast_to(np.asarray(abbe, np.float64), (len(t),))
    n = int(n)
    iors = np.zeros((max(n, 1), len(t)), np.float32)
    for r in range(len(t)):
        iors[:, r] = spectral_bands(n, t["ior"][r], float(ab[r]))["ior"]
    return iors, np.ascontiguousarray(spectral_bands(n)["weight"], np.float32)


def camera_rays(camera, w, h, ox=0.5, oy=0.5, tmin=1e-4, tmax=100.0):
    """-> RAY_DTYPE [w * h], row-major: the primary ray of every pixel of a w x h frame through the sub-pixel position (ox, oy)
    (pixel units, in [0, 1]) -- with the default, the pixel centre, the rays of a dispatch; what render_samples traces for
    that offset.  camera: SceneConstants (camera_orbit, scene_constants)."""
    rays = np.zeros(int(w) * int(h), RAY_DTYPE)
    rc = _capi.lib().rr_host_camera_rays(C.byref(camera), int(w), int(h), float(ox), float(oy), float(np.float32(tmin)),
                                         float(np.float32(tmax)), rays.ctypes.data)
    if rc:
        raise RRError(rc, "rr_host_camera_rays")
    return rays


def lens_pattern(n):
    """-> float32 [n, 2]: the built-in lens offsets of render_lens for n = 1..64 samples, a golden-angle spiral inside the unit disk,
    in units of the lens radius"""
    n = int(n)
    out = np.zeros((max(n, 1), 2), np.float32)
    rc = _capi.lib().rr_host_lens_pattern(n if n >= 0 else 0, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise RRError(rc, "rr_host_lens_pattern(%d)" % n)
    return out


def lens_rays(camera, w, h, ox, oy, lx, ly, lens, tmin=1e-4, tmax=100.0):
    """-> RAY_DTYPE [w * h], row-major: what render_lens traces for the sample with sub-pixel position (ox, oy) (pixel units, in
    [0, 1]) and lens offset (lx, ly) (units of lens.radius, each in [-1, 1]): rays from the lens point through the focal-plane point
    of every pixel.  lens.radius == 0: camera_rays(camera, w, h, ox, oy, tmin, tmax)."""
    rays = np.zeros(int(w) * int(h), RAY_DTYPE)
    rc = _capi.lib().rr_host_lens_rays(C.byref(camera), int(w), int(h), float(ox), float(oy), float(lx), float(ly), C.byref(lens),
                                       float(np.float32(tmin)), float(np.float32(tmax)), rays.ctypes.data)
    if rc:
        raise RRError(rc, "rr_host_lens_rays")
    return rays


def lens_screen_rect(bounds, camera, lens, w, h):
    """-> (x0, y0, x1, y1): the pixels from which any point of the lens can see the box bounds = (lo xyz, hi xyz), aligned outward to
    8 with 8 pixels of margin; the whole frame (rounded up to 8) when the projection cannot be trusted or camera is None.
    render_lens traces the 8x8 blocks that touch it and shades the others as one Miss per sample."""
    b = (C.c_float * 6)(*[float(v) for v in np.asarray(bounds, np.float32).reshape(6)])
    r = (C.c_uint32 * 4)()
    rc = _capi.lib().rr_host_lens_screen_rect(b, C.byref(camera) if camera is not None else None, C.byref(lens), int(w), int(h), r)
    if rc:
        raise RRError(rc, "rr_host_lens_screen_rect")
    return tuple(int(v) for v in r)


def shutter_samples(positions, keys, bands=None, lens_offsets=None):
    """The crossed sample records of render_shutter -> SHUTTER_SAMPLE_DTYPE [A * K * B].  positions: an int (sample_pattern) or an
    [A, 2] array of offsets in [0, 1]; keys: an int K for the scene keys 0 .. K-1, or a sequence of K key indices; bands: None for
    band 0, an int B for bands 0 .. B-1, or a sequence of B band indices.  Sample (a * K + j) * B + b has position a, key j and band
    b.  lens_offsets: None for lens_pattern(S), or an [S, 2] array in [-1, 1], one row per sample after crossing."""
    pos = sample_pattern(positions) if isinstance(positions, (int, np.integer)) else np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError("shutter_samples: positions must be an int or an [A, 2] array")
    ks = np.arange(int(keys)) if isinstance(keys, (int, np.integer)) else np.ascontiguousarray(keys, np.int64).reshape(-1)
    bs = np.zeros(1, np.int64) if bands is None else np.arange(int(bands)) if isinstance(bands, (int, np.integer)) else np.ascontiguousarray(bands, np.int64).reshape(-1)
    if len(ks) == 0 or len(bs) == 0 or (ks < 0).any() or (bs < 0).any():
        raise ValueError("shutter_samples: need at least one key and one band, none negative")
    n = len(pos) * len(ks) * len(bs)
    if n > _capi.MAX_SAMPLES:
        raise ValueError("shutter_samples: positions x keys x bands must not exceed %d samples" % _capi.MAX_SAMPLES)
    rec = np.zeros(n, _capi.SHUTTER_SAMPLE_DTYPE)
    rec["offset"] = np.repeat(pos, len(ks) * len(bs), axis=0)
    rec["key"] = np.tile(np.repeat(ks, len(bs)), len(pos))
    rec["band"] = np.tile(bs, len(pos) * len(ks))
    if lens_offsets is not None:
        loff = np.ascontiguousarray(lens_offsets, np.float32)
        if loff.shape != (n, 2) or n == 0:
            raise ValueError("shutter_samples: lens_offsets must be an [S, 2] array with one row per sample")
        rec["lens_offset"] = loff
    elif n >= 1:
        rec["lens_offset"] = lens_pattern(n)
    return rec


def light_pattern(n):
    """-> float32 [n, 2]: the built-in light offsets of render_lit for n = 1..64 positions, each in [-1, 1], in units of a light's
    edges.  Deterministic, a Hammersley set centred in its cells: point k is (2 * (k + 0.5) / n - 1, 2 * (phi2(k) + 0.5 / m) - 1) with
    phi2 the base-2 radical inverse and m the smallest power of two >= n, computed in float64 and rounded once; n == 1 gives (0, 0)."""
    n = int(n)
    if not 1 <= n <= _capi.MAX_SAMPLES:
        raise ValueError("light_pattern: need 1 <= n <= %d" % _capi.MAX_SAMPLES)
    m = 1
    while m < n:
        m *= 2
    k = np.arange(n)
    phi = np.zeros(n, np.float64)
    f, i = 0.5, k.copy()
    while i.any():
        phi += f * (i & 1)
        i >>= 1
        f *= 0.5
    return np.stack([2.0 * (k + 0.5) / n - 1.0, 2.0 * (phi + 0.5 / m) - 1.0], axis=1).astype(np.float32)


def light_shape(ex, ey):
    """A LIGHT_SHAPE_DTYPE row (Renderer.set_light_shapes): the two edge vectors a light's position (or direction) moves along; a
    sample with light offset (lu, lv) sees the light at v + lu * ex + lv * ey (moved_lights has the arithmetic)."""
    r = np.zeros((), _capi.LIGHT_SHAPE_DTYPE)
    r["ex"], r["ey"] = ex, ey
    return r


def moved_lights(lights, shapes, lu, lv):
    """-> LIGHT_DTYPE [n]: the lights one sample of render_lit is lit by (rr_host_moved_lights): row i with
    v = fmaf(lv, shapes[i].ey, fmaf(lu, shapes[i].ex, v)) per component in fp32, everything else copied.  shapes None: the rows
    unchanged.  Otherwise one LIGHT_SHAPE_DTYPE row per light."""
    t = np.ascontiguousarray(lights, LIGHT_DTYPE).reshape(-1)
    out = np.zeros(len(t), LIGHT_DTYPE)
    sp = None
    if shapes is not None:
        s = np.ascontiguousarray(shapes, _capi.LIGHT_SHAPE_DTYPE).reshape(-1)
        if len(s) != len(t):
            raise ValueError("moved_lights: need one shape per light")
        sp = s.ctypes.data if len(s) else None
    rc = _capi.lib().rr_host_moved_lights(t.ctypes.data if len(t) else None, sp, len(t), float(np.float32(lu)), float(np.float32(lv)),
                                          out.ctypes.data if len(t) else None)
    if rc:
        raise RRError(rc, "rr_host_moved_lights")
    return out


def lit_samples(positions, keys, bands=None, lens_offsets=None, light_offsets=None):
    """The crossed sample records of render_lit -> LIT_SAMPLE_DTYPE [A * K * B]: shutter_samples(positions, keys, bands, lens_offsets)
    with a light offset per POSITION -- every sample of position a, whatever its key and band, has light_offsets[a].  light_offsets:
    None for light_pattern(A), or an [A, 2] array in [-1, 1]."""
    src = shutter_samples(positions, keys, bands, lens_offsets)
    n_pos = int(positions) if isinstance(positions, (int, np.integer)) else len(positions)
    if light_offsets is None:
        lo = light_pattern(n_pos)
    else:
        lo = np.ascontiguousarray(light_offsets, np.float32)
        if lo.shape != (n_pos, 2):
            raise ValueError("lit_samples: light_offsets must be an [A, 2] array with one row per position")
    rec = np.zeros(len(src), _capi.LIT_SAMPLE_DTYPE)
    for f in ("offset", "lens_offset", "band", "key"):
        rec[f] = src[f]
    rec["light_offset"] = np.repeat(lo, len(src) // n_pos, axis=0)
    return rec


def make_instances(transforms=None, meshes=None, masks=None, flags=None, materials=None):
    """64-byte instance records (RefractionDemo.cpp:324-334 fills exactly one: identity, mask 1, flags 0).  materials: per instance
    the row of the material table (Renderer.set_materials) it is made of -- DXR's InstanceContributionToHitGroupIndex, the low 24
    bits of hitgroup_flags; default 0."""
    if transforms is None:
        transforms = [np.eye(4, dtype=np.float32)[:3]]
    n = len(transforms)
    inst = np.zeros(n, INSTANCE_DTYPE)
    for i, t in enumerate(transforms):
        inst["transform"][i] = np.asarray(t, np.float32).reshape(12)
        inst["instance_id_mask"][i] = (i & 0xffffff) | (((masks[i] if masks is not None else 1) & 0xff) << 24)
        inst["hitgroup_flags"][i] = (((flags[i] if flags is not None else 0) & 0xff) << 24) | ((int(materials[i]) if materials is not None else 0) & 0xffffff)
        inst["blas"][i] = meshes[i] if meshes is not None else 0
    return inst


def glass():
    """A row of the surface table (Renderer.set_surfaces) that leaves everything to the material row: SURFACE_GLASS"""
    return np.zeros((), SURFACE_DTYPE)


def opaque(albedo, emission=(0, 0, 0), specular=(0, 0, 0)):
    """A row of the surface table for an opaque surface: albedo times what the lights and the ambient term send, plus emission, plus
    -- where specular is not (0, 0, 0) -- a mirror child weighted by specular.  RGB triples; albedo and specular >= 0."""
    r = np.zeros((), SURFACE_DTYPE)
    r["kind"], r["albedo"], r["emission"], r["specular"] = _capi.SURFACE_OPAQUE, albedo, emission, specular
    return r


def directional_light(towards, radiance, shadow_mask=0xff):
    """A LIGHT_DTYPE row: a light infinitely far away in direction `towards` (normalised here, in float64, then rounded), with an RGB
    radiance.  Its shadow rays see the instances whose mask meets shadow_mask."""
    d = np.asarray(towards, np.float64)
    n = float(np.sqrt((d * d).sum()))
    if not np.isfinite(n) or n == 0.0:
        raise ValueError("directional_light: need a finite direction that is not zero")
    r = np.zeros((), LIGHT_DTYPE)
    r["v"], r["kind"], r["radiance"], r["shadow_mask"] = d / n, _capi.LIGHT_DIRECTIONAL, radiance, shadow_mask
    return r


def point_light(position, radiance, shadow_mask=0xff):
    """A LIGHT_DTYPE row: a point light at `position` whose contribution falls with the square of the distance"""
    r = np.zeros((), LIGHT_DTYPE)
    r["v"], r["kind"], r["radiance"], r["shadow_mask"] = position, _capi.LIGHT_POINT, radiance, shadow_mask
    return r


def pack_rays(origin, dir, tmin, tmax, flags=0, instance_mask=0xff):
    """Ray records for Renderer.query_rays / query_rays_multi / trace_rays.  origin, dir: [n, 3]; tmin, tmax, flags, instance_mask: [n] or
    scalars.  numpy inputs give a RAY_DTYPE array; torch tensors give a contiguous [n, 12] int32 tensor holding the raw
    48-byte records (the float fields as their bits) on the inputs' device.  The default mask, 0xff, passes every instance."""
    if type(origin).__module__.startswith("torch"):
        import torch
        o = origin.to(torch.float32).reshape(-1, 3)
        n, dev = o.shape[0], o.device
        out = torch.zeros((n, 12), dtype=torch.int32, device=dev)
        f = out.view(torch.float32)

        def col(x, dt):
            return torch.as_tensor(x, dtype=dt, device=dev).expand(n) if not torch.is_tensor(x) or x.dim() == 0 \
                else x.to(device=dev, dtype=dt).reshape(n)
        f[:, 0:3] = o
        f[:, 3] = col(tmin, torch.float32)
        f[:, 4:7] = dir.to(device=dev, dtype=torch.float32).reshape(n, 3)
        f[:, 7] = col(tmax, torch.float32)
        out[:, 8] = col(flags, torch.int64).to(torch.int32)
        out[:, 9] = col(instance_mask, torch.int64).to(torch.int32)
        return out
    o = np.asarray(origin, np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["origin"] = o
    rays["dir"] = np.asarray(dir, np.float32).reshape(-1, 3)
    rays["tmin"] = tmin
    rays["tmax"] = tmax
    rays["flags"] = np.asarray(flags, np.int64) & 0xffffffff
    rays["instance_mask"] = np.asarray(instance_mask, np.int64) & 0xffffffff
    return rays


def _outputs(shape, rgba8, counts, device=None):
    """The outputs of shade_rays, render_samples and render_adaptive for `shape` rays or pixels: float32 shape + (4,), the uint8
    store of the same shape if rgba8, and one count array of `shape` per true entry of counts (None where not asked for) -- numpy
    arrays with uint32 counts, or with device new torch tensors there with int32 counts -> (arrays, their pointers as the C ABI
    takes them: null for an output not asked for and for an empty tensor)."""
    if device is None:
        outs = [np.zeros(shape + (4,), np.float32), np.zeros(shape + (4,), np.uint8) if rgba8 else None]
        outs += [np.zeros(shape, np.uint32) if c else None for c in counts]
        return outs, [a.ctypes.data if a is not None else None for a in outs]
    import torch
    outs = [torch.empty(shape + (4,), dtype=torch.float32, device=device),
            torch.empty(shape + (4,), dtype=torch.uint8, device=device) if rgba8 else None]
    outs += [torch.empty(shape, dtype=torch.int32, device=device) if c else None for c in counts]
    return outs, [C.c_void_p(t.data_ptr() if t is not None and t.numel() else None) for t in outs]


def _result(outs):
    out = tuple(a for a in outs if a is not None)
    return out if len(out) > 1 else out[0]


def _sample_offsets(samples, complaint):
    """samples: an int (a built-in pattern) or an [S, 2] array of offsets -> (pointer to the float32 offsets or None, S); the
    pointer keeps its array alive"""
    if isinstance(samples, (int, np.integer)):
        return None, int(samples)
    off = np.ascontiguousarray(samples, np.float32)
    if off.ndim != 2 or off.shape[1] != 2:
        raise ValueError(complaint)
    return (off.ctypes.data_as(C.c_void_p) if off.shape[0] else None), off.shape[0]


def _per_sample(rec, field, given, pattern, what):
    """rec[field] of S sample records: the rows of `given`, an [S, 2] array, or with None pattern(S) where 1 <= S <= MAX_SAMPLES
    (any other S the library refuses, so the field stays zero)"""
    if given is not None:
        rows = np.ascontiguousarray(given, np.float32)
        if rows.shape != (len(rec), 2) or len(rec) == 0:
            raise ValueError("%s must be an [S, 2] array with one row per sample" % what)
        rec[field] = rows
    elif 1 <= len(rec) <= _capi.MAX_SAMPLES:
        rec[field] = pattern(len(rec))


def _paired_indices(n, complaint, *columns, refuse=False):
    """paired=True: every column (indices, or None for zeros) -> int64 [n]; complains of a column of another length or with a negative
    entry, and where the caller has seen a reason of its own (refuse)"""
    idx = [np.zeros(n, np.int64) if c is None else np.ascontiguousarray(c, np.int64).reshape(-1) for c in columns]
    if refuse or any(len(i) != n or (i < 0).any() for i in idx):
        raise ValueError(complaint)
    return idx


class Mesh:
    """Mesh.hpp:14-25.  verts: structured array of 32-byte Vertex; indices: uint32."""

    def __init__(self):
        self.verts = np.zeros(0, VERTEX_DTYPE)
        self.indices = np.zeros(0, np.uint32)
        self.mesh_id = None

    def load(self, filename, hardened=False):
        """Mesh::load (Mesh.cpp:6-37): True on success, False if the file cannot be opened.
        hardened=True additionally accepts polygons, v / v/vt / v//vn corners and negative indices."""
        L = _capi.lib()
        v, i = C.c_void_p(), C.c_void_p()
        nv, ni = C.c_uint32(), C.c_uint32()
        rc = L.rr_host_mesh_load_obj_ex(str(filename).encode(), 1 if hardened else 0, C.byref(v), C.byref(nv), C.byref(i),
                                        C.byref(ni))
        if rc:
            return False
        verts = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_uint8)), shape=(max(nv.value, 1) * 32,))
        verts = verts[:nv.value * 32].copy().view(VERTEX_DTYPE)
        idx = np.ctypeslib.as_array(C.cast(i, C.POINTER(C.c_uint32)), shape=(max(ni.value, 1),))[:ni.value].copy()
        L.rr_host_free(v)
        L.rr_host_free(i)
        base = len(self.verts)            # the reference appends (Mesh.cpp:31-32)
        self.verts = np.concatenate([self.verts, verts])
        self.indices = np.concatenate([self.indices, (idx + base).astype(np.uint32)])
        return True

    def upload(self, device):
        """Mesh::upload (Mesh.cpp:55-94); `device` is a Renderer."""
        self.mesh_id = device.upload_mesh(self.verts, self.indices)
        return self.mesh_id

    def raytracingGeometry(self):
        return dict(mesh_id=self.mesh_id, vertex_count=len(self.verts), index_count=len(self.indices),
                    vertex_stride=32)


class Renderer:
    """One context on one GPU (one process per GPU; see dist.py for the sharded frame)."""

    def __init__(self, device=0):
        self._L = _capi.lib()
        h = C.c_void_p()
        rc = self._L.rr_create(int(device), C.byref(h))
        if rc:
            raise RRError(rc, "rr_create(device=%d): no usable gfx950 device" % device)
        self._h = h
        self.device = int(device)
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.rr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc:
            raise RRError(rc, "%s: %s" % (what, self._L.rr_last_error(self._h).decode()))

    def set_stream(self, hip_stream):
        """run on a caller-owned hipStream_t handle (0 / None = HIP's default stream)"""
        self._ck(self._L.rr_set_stream(self._h, C.c_void_p(hip_stream or None)), "rr_set_stream")
        self._stream_key = int(hip_stream or 0)

    def reset_stream(self):
        self._ck(self._L.rr_reset_stream(self._h), "rr_reset_stream")
        self._stream_key = None

    def wait(self):
        self._ck(self._L.rr_wait(self._h), "rr_wait")

    def upload_mesh(self, verts, indices):
        verts = np.ascontiguousarray(verts)
        assert verts.dtype.itemsize == 32
        indices = np.ascontiguousarray(indices, np.uint32)
        mid = C.c_uint32()
        self._ck(self._L.rr_upload_mesh(self._h, verts.ctypes.data, len(verts), indices.ctypes.data, len(indices),
                                        C.byref(mid)), "rr_upload_mesh")
        return mid.value

    def upload_envmap(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w, c = rgb.shape
        assert c == 3
        self._ck(self._L.rr_upload_envmap(self._h, rgb.ctypes.data, w, h), "rr_upload_envmap")

    def build_blas(self, mesh_id, fast_build=False, allow_update=False, update=False):
        """BuildRaytracingAccelerationStructure (bottom level); fast_build=True forces the plain Morton LBVH.
        allow_update=True keeps what a refit needs (DXR ALLOW_UPDATE); update=True refits the hierarchy of such a build over
        the mesh's current vertices (DXR PERFORM_UPDATE) instead of building a new one."""
        if update:
            flags = _capi.BUILD_PERFORM_UPDATE
        else:
            flags = _capi.BUILD_PREFER_FAST_BUILD if fast_build else _capi.BUILD_PREFER_FAST_TRACE
            if allow_update:
                flags |= _capi.BUILD_ALLOW_UPDATE
        self._ck(self._L.rr_build_blas_ex(self._h, mesh_id, flags), "rr_build_blas")

    def build_tlas(self, instances=None, allow_update=False, update=False):
        """BuildRaytracingAccelerationStructure (top level).  update=True refits a TLAS built with allow_update=True over new
        transforms / masks / flags of the same instances (same count, same BLAS per slot) and re-pools the updated BLASes."""
        inst = make_instances() if instances is None else np.ascontiguousarray(instances, INSTANCE_DTYPE)
        flags = (_capi.BUILD_ALLOW_UPDATE if allow_update else 0) | (_capi.BUILD_PERFORM_UPDATE if update else 0)
        self._ck(self._L.rr_build_tlas_ex(self._h, inst.ctypes.data, len(inst), flags), "rr_build_tlas")

    def update_mesh_vertices(self, mesh_id, verts):
        """Replace a mesh's vertices in place (same count; the indices never change); the mesh id stays.  Then
        build_blas(mesh_id, update=True) (or a full build) and build_tlas(...) before the next dispatch.

        verts: a VERTEX_DTYPE numpy array (or [n, 8] float32), copied from the host before this returns; or a contiguous
        float32 torch tensor of shape [n, 8] on this renderer's GPU, copied on the renderer's stream without passing through
        the host.  The copy is ordered after the work already queued on that stream only: a tensor produced on another stream
        (torch's current stream, say) must be finished or ordered first -- call set_stream(torch.cuda.current_stream()
        .cuda_stream) once, or torch.cuda.current_stream().synchronize() before the call.  A non-finite position in a tensor is
        reported by the next build_blas of the mesh (RR_ERR_INVALID_ARGUMENT), which leaves the mesh as it was."""
        if type(verts).__module__.startswith("torch"):
            t = verts
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError("update_mesh_vertices: the tensor must live on GPU %d" % self.device)
            import torch
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 8 or not t.is_contiguous():
                raise ValueError("update_mesh_vertices: need a contiguous [n, 8] float32 tensor")
            self._ck(self._L.rr_update_mesh_vertices_device(self._h, mesh_id, C.c_void_p(t.data_ptr()), len(t)),
                     "rr_update_mesh_vertices_device")
            return
        verts = np.ascontiguousarray(verts)
        if verts.dtype != VERTEX_DTYPE:
            verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 8)
        assert verts.dtype.itemsize * (verts.size // len(verts)) == 32
        self._ck(self._L.rr_update_mesh_vertices(self._h, mesh_id, verts.ctypes.data, len(verts)), "rr_update_mesh_vertices")

    def set_camera(self, sc):
        self._ck(self._L.rr_set_camera(self._h, C.byref(sc)), "rr_set_camera")

    def set_tile_partition(self, rank, world):
        self._ck(self._L.rr_set_tile_partition(self._h, rank, world), "rr_set_tile_partition")

    def dispatch_rays(self, width, height, params=None):
        p = params if params is not None else default_params()
        self._ck(self._L.rr_dispatch_rays(self._h, width, height, C.byref(p)), "rr_dispatch_rays")
        self.width, self.height = width, height

    def dispatch_rays_batch(self, width, height, constants, params=None):
        """DispatchRays(W, H, Depth=len(constants)): one launch, slice f rendered with constants[f]."""
        p = params if params is not None else default_params()
        arr = (SceneConstants * len(constants))(*constants)
        self._ck(self._L.rr_dispatch_rays_batch(self._h, width, height, len(constants), C.cast(arr, C.c_void_p),
                                                C.byref(p)), "rr_dispatch_rays_batch")
        self.width, self.height = width, height

    def read_frame(self, want_float=False, slice=0):
        """-> rgba8 uint8 [h,w,4] (and float32 [h,w,4] if the dispatch kept it)."""
        rgba = np.empty((self.height, self.width, 4), np.uint8)
        f32 = np.empty((self.height, self.width, 4), np.float32) if want_float else None
        self._ck(self._L.rr_read_frame_slice(self._h, slice, rgba.ctypes.data, f32.ctypes.data if want_float else None),
                 "rr_read_frame")
        return (rgba, f32) if want_float else rgba

    def local_tile_count(self, width, height):
        n, mx = C.c_uint32(), C.c_uint32()
        self._ck(self._L.rr_local_tile_count(self._h, width, height, C.byref(n), C.byref(mx)), "rr_local_tile_count")
        return n.value, mx.value

    def export_tiles(self, device_ptr):
        self._ck(self._L.rr_export_tiles(self._h, C.c_void_p(device_ptr)), "rr_export_tiles")

    def assemble_tiles(self, gathered_ptr, world, frame_ptr=None):
        self._ck(self._L.rr_assemble_tiles(self._h, C.c_void_p(gathered_ptr), world,
                                           C.c_void_p(frame_ptr) if frame_ptr else None), "rr_assemble_tiles")

    def render_orbit(self, width, height, n_frames, angle=0.01, angle_step=0.01, params=None, frames_per_dispatch=1,
                     fov_y=FOV_Y, aspect=ASPECT, zn=1.0, zf=125.0):
        """n_frames of the drawFrame loop (camera -> DispatchRays -> angle += step), asynchronous.
        Returns the angle the next frame would use."""
        p = params if params is not None else default_params()
        a = C.c_float(float(np.float32(angle)))
        self._ck(self._L.rr_render_orbit(self._h, width, height, C.byref(p), C.byref(a), float(np.float32(angle_step)),
                                         n_frames, frames_per_dispatch, fov_y, aspect, zn, zf), "rr_render_orbit")
        self.width, self.height = width, height
        return a.value

    def render_orbit_to_host(self, width, height, n_frames, angle=0.01, angle_step=0.01, params=None, frames_per_dispatch=16,
                             fov_y=FOV_Y, aspect=ASPECT, zn=1.0, zf=125.0, pin=True):
        """The drawFrame loop with every frame delivered to host memory (copies overlap rendering).
        -> uint8 [n_frames, h, w, 4]; blocks until all frames have arrived."""
        p = params if params is not None else default_params()
        a = C.c_float(float(np.float32(angle)))
        out = np.empty((n_frames, height, width, 4), np.uint8)
        pinned = pin and self._L.rr_host_register(self._h, out.ctypes.data, out.nbytes) == 0
        try:
            self._ck(self._L.rr_render_orbit_to_host(self._h, width, height, C.byref(p), C.byref(a), float(np.float32(angle_step)),
                                                     n_frames, frames_per_dispatch, fov_y, aspect, zn, zf, out.ctypes.data),
                     "rr_render_orbit_to_host")
        finally:
            if pinned:
                self._L.rr_host_unregister(self._h, out.ctypes.data)
        self.width, self.height = width, height
        return out

    def render_orbit_sharded(self, width, height, n_frames, tiles_ptr, frame_stride_bytes, angle=0.01,
                             angle_step=0.01, params=None, frames_per_dispatch=1, fov_y=FOV_Y, aspect=ASPECT, zn=1.0,
                             zf=125.0, lane=None):
        """lane=None: on the context's stream.  lane=0..3: on that internal stream, not joined until lane_join(lane)."""
        p = params if params is not None else default_params()
        a = C.c_float(float(np.float32(angle)))
        if lane is None:
            self._ck(self._L.rr_render_orbit_sharded(self._h, width, height, C.byref(p), C.byref(a),
                                                     float(np.float32(angle_step)), n_frames, frames_per_dispatch, fov_y,
                                                     aspect, zn, zf, C.c_void_p(tiles_ptr), frame_stride_bytes),
                     "rr_render_orbit_sharded")
        else:
            self._ck(self._L.rr_render_orbit_sharded_lane(self._h, width, height, C.byref(p), C.byref(a),
                                                          float(np.float32(angle_step)), n_frames, frames_per_dispatch,
                                                          fov_y, aspect, zn, zf, C.c_void_p(tiles_ptr), frame_stride_bytes,
                                                          lane), "rr_render_orbit_sharded_lane")
        self.width, self.height = width, height
        return a.value

    def mesh_partition_for_orbit(self, width, height, n_frames, angle=0.01, angle_step=0.01, fov_y=FOV_Y, aspect=ASPECT, zn=1.0, zf=125.0):
        """rr_mesh_partition of the n_frames frames starting at `angle` for this context's (rank, world)."""
        part = _capi.MeshPartition()
        self._ck(self._L.rr_mesh_partition_for_orbit(self._h, width, height, float(np.float32(angle)), float(np.float32(angle_step)), n_frames,
                                                     fov_y, aspect, zn, zf, C.byref(part)), "rr_mesh_partition_for_orbit")
        return part

    def render_orbit_mesh_sharded(self, width, height, n_frames, mesh_ptr, mesh_stride_bytes, bg_ptr, bg_stride_bytes, angle=0.01,
                                  angle_step=0.01, params=None, lane=0, fov_y=FOV_Y, aspect=ASPECT, zn=1.0, zf=125.0):
        """One DispatchRays(W, H, n_frames) of a sharded context under the mesh-tile partition, on render lane `lane`:
        this rank's mesh tiles (RGB8) to mesh_ptr, rank 0's background tiles to bg_ptr.  -> the angle after the last frame."""
        a = C.c_float(np.float32(angle))
        p = params if params is not None else default_params()
        self._ck(self._L.rr_render_orbit_mesh_sharded_lane(self._h, width, height, C.byref(p), C.byref(a), float(np.float32(angle_step)), n_frames,
                                                           fov_y, aspect, zn, zf, mesh_ptr, mesh_stride_bytes, bg_ptr, bg_stride_bytes, lane),
                 "rr_render_orbit_mesh_sharded_lane")
        self.width, self.height = width, height
        return float(a.value)

    def assemble_frames_mesh(self, gathered_ptr, rank_stride_bytes, frame_stride_bytes, bg_ptr, bg_stride_bytes, part, n_frames, width, height,
                             frames_ptr, out_stride_bytes):
        self._ck(self._L.rr_assemble_frames_mesh_rgb8(self._h, gathered_ptr, rank_stride_bytes, frame_stride_bytes, bg_ptr, bg_stride_bytes,
                                                      C.byref(part), n_frames, width, height, frames_ptr, out_stride_bytes),
                 "rr_assemble_frames_mesh_rgb8")

    def set_frames_in_flight(self, n):
        """launches of render_orbit that may overlap (1 = the reference's one-at-a-time frame loop)"""
        self._ck(self._L.rr_set_frames_in_flight(self._h, n), "rr_set_frames_in_flight")

    def lane_join(self, lane):
        self._ck(self._L.rr_lane_join(self._h, lane), "rr_lane_join")

    def assemble_frames(self, gathered_ptr, world, rank_stride_bytes, frame_stride_bytes, n_frames, width, height,
                        frames_ptr, out_stride_bytes, rgb8=False):
        fn = self._L.rr_assemble_frames_rgb8 if rgb8 else self._L.rr_assemble_frames
        self._ck(fn(self._h, C.c_void_p(gathered_ptr), world, rank_stride_bytes,
                                            frame_stride_bytes, n_frames, width, height, C.c_void_p(frames_ptr),
                                            out_stride_bytes), "rr_assemble_frames")

    def timing_begin(self):
        self._ck(self._L.rr_timing_begin(self._h), "rr_timing_begin")

    def timing_end(self):
        ms = C.c_float()
        self._ck(self._L.rr_timing_end(self._h, C.byref(ms)), "rr_timing_end")
        return ms.value

    def kernel_time(self):
        """-> (sum of render-kernel milliseconds, launches) of the dispatches flagged DISPATCH_TIME_KERNEL"""
        ms, n = C.c_float(), C.c_uint32()
        self._ck(self._L.rr_kernel_time(self._h, C.byref(ms), C.byref(n)), "rr_kernel_time")
        return ms.value, n.value

    def stats(self):
        st = Stats()
        self._ck(self._L.rr_get_stats(self._h, C.byref(st)), "rr_get_stats")
        return st

    def trace_rays(self, rays):
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._ck(self._L.rr_trace_rays(self._h, rays.ctypes.data, len(rays), hits.ctypes.data), "rr_trace_rays")
        return hits

    def query_rays(self, rays):
        """TraceRay(Scene, flags, instance_mask, ...) on caller rays: the ray's InstanceInclusionMask (RAY_DTYPE's instance_mask)
        and RAY_FLAG_ACCEPT_FIRST_HIT are honoured (trace_rays ignores both).  Build rays with pack_rays.

        rays: a RAY_DTYPE numpy array -> a HIT_DTYPE array (host arrays, blocking); or a contiguous [n, 12] int32 or float32
        torch tensor of raw ray records on this renderer's GPU -> a new [n, 6] tensor of the same dtype and device holding the
        raw hit records (t, u, v as float bits, then prim, inst, hit), computed on the renderer's stream without passing
        through the host and without waiting for it.  The query is ordered after the work already queued on that stream only:
        rays produced on another stream (torch's current stream, say) must be finished or ordered first -- call
        set_stream(torch.cuda.current_stream().cuda_stream) once, or torch.cuda.current_stream().synchronize() before the call
        -- and the hits are ready once that stream has run the query."""
        if type(rays).__module__.startswith("torch"):
            import torch
            t = rays
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError("query_rays: the tensor must live on GPU %d" % self.device)
            if t.dtype not in (torch.int32, torch.float32) or t.dim() != 2 or t.shape[1] != 12 or not t.is_contiguous():
                raise ValueError("query_rays: need a contiguous [n, 12] int32 or float32 tensor")
            hits = torch.empty((t.shape[0], 6), dtype=t.dtype, device=t.device)
            self._ck(self._L.rr_query_rays_device(self._h, C.c_void_p(t.data_ptr()), t.shape[0], C.c_void_p(hits.data_ptr())),
                     "rr_query_rays_device")
            return hits
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._ck(self._L.rr_query_rays(self._h, rays.ctypes.data, len(rays), hits.ctypes.data), "rr_query_rays")
        return hits

    def query_rays_multi(self, rays, k, counts=False):
        """Multi-hit query (rr_query_rays_multi): for each ray the first k of the triangles a closest-hit query would accept, in
        ascending (t, inst, prim) order, each with the closest-hit query's t, u, v, prim, inst and its DXR HitKind in the hit word
        (HIT_KIND_FRONT_FACE / HIT_KIND_BACK_FACE); unused slots are miss records.  counts=True also returns the number of accepted
        triangles per ray (k may then be 0).  Ray flags ACCEPT_FIRST_HIT and 0x8 are ignored.

        rays: a RAY_DTYPE numpy array -> a HIT_DTYPE array of shape [n, k] (and uint32 [n] counts), blocking; or a contiguous
        [n, 12] int32 or float32 torch tensor on this renderer's GPU -> a [n, k, 6] tensor of the same dtype and device (and int32
        [n] counts), computed on the renderer's stream without waiting for it (stream order as query_rays)."""
        k = int(k)
        if k < 0 or k > _capi.QUERY_MAX_HITS or (k == 0 and not counts):
            raise ValueError("query_rays_multi: need 1 <= k <= %d, or k == 0 with counts=True" % _capi.QUERY_MAX_HITS)
        if type(rays).__module__.startswith("torch"):
            import torch
            t = rays
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError("query_rays_multi: the tensor must live on GPU %d" % self.device)
            if t.dtype not in (torch.int32, torch.float32) or t.dim() != 2 or t.shape[1] != 12 or not t.is_contiguous():
                raise ValueError("query_rays_multi: need a contiguous [n, 12] int32 or float32 tensor")
            n = t.shape[0]
            hits = torch.empty((n, k, 6), dtype=t.dtype, device=t.device)
            cnt = torch.empty((n,), dtype=torch.int32, device=t.device) if counts else None
            self._ck(self._L.rr_query_rays_multi_device(self._h, C.c_void_p(t.data_ptr()), n, k,
                                                        C.c_void_p(hits.data_ptr() if k and n else None),
                                                        C.c_void_p(cnt.data_ptr() if cnt is not None and n else None)),
                     "rr_query_rays_multi_device")
            return (hits, cnt) if counts else hits
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        n = len(rays)
        hits = np.zeros((n, k), HIT_DTYPE)
        cnt = np.zeros(n, np.uint32) if counts else None
        self._ck(self._L.rr_query_rays_multi(self._h, rays.ctypes.data, n, k, hits.ctypes.data if k else None,
                                             cnt.ctypes.data if counts else None), "rr_query_rays_multi")
        return (hits, cnt) if counts else hits

    def shade_rays(self, rays, params=None, rgba8=False, ray_counts=False):
        """Radiance query (rr_shade_rays): the shader's whole ray tree -- RayGen's payload, ClosestHit's refraction / reflection tree,
        Miss's env-map lookup -- on caller rays instead of the pinhole camera's, i.e. a RayGen shader of your own.  Ray i starts
        with origin, dir (not normalised), tmin and tmax of its record (pack_rays; flags and instance_mask are ignored), outside the
        glass with weight 1; params (default_params()) gives the bounce limits, ior, the secondary rays' interval and, for the RGBA8
        output, DISPATCH_TONEMAP_REINHARD.  The colour of a ray has the bits dispatch_rays gives a pixel with that primary ray.
        Not a dispatch: read_frame and stats() stay as the last dispatch left them.

        rays: a RAY_DTYPE numpy array -> float32 [n, 4] (r, g, b, 1), blocking; or a contiguous [n, 12] int32 or float32 torch
        tensor on this renderer's GPU -> a new float32 [n, 4] tensor on that device, computed on the renderer's stream without
        waiting for it (stream order as query_rays).  rgba8=True adds the R8G8B8A8_UNORM store (uint8 [n, 4]), ray_counts=True the
        TraceRay calls of each ray's tree, the primary included (uint32 [n]; torch: int32 [n]); the result is then a tuple in
        that order."""
        return self._shade("shade_rays", rays, params, rgba8, ray_counts)

    def _shade(self, name, rays, params, rgba8, ray_counts):
        """the four shade_rays* methods: rr_<name>_device on a tensor of rays, rr_<name> on an array"""
        p = params if params is not None else default_params()
        if type(rays).__module__.startswith("torch"):
            import torch
            t = rays
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError("%s: the tensor must live on GPU %d" % (name, self.device))
            if t.dtype not in (torch.int32, torch.float32) or t.dim() != 2 or t.shape[1] != 12 or not t.is_contiguous():
                raise ValueError("%s: need a contiguous [n, 12] int32 or float32 tensor" % name)
            n, fn = t.shape[0], "rr_%s_device" % name
            rayp = C.c_void_p(t.data_ptr() if n else None)
            outs, ptrs = _outputs((n,), rgba8, (ray_counts,), t.device)
        else:
            rays = np.ascontiguousarray(rays, RAY_DTYPE)
            n, fn, rayp = len(rays), "rr_%s" % name, rays.ctypes.data
            outs, ptrs = _outputs((n,), rgba8, (ray_counts,))
        self._ck(getattr(self._L, fn)(self._h, rayp, n, C.byref(p), *ptrs), fn)
        return _result(outs)

    def _frame(self, name, w, h, rgba8, counts, device, *args, tail=()):
        """what every frame method ends in: the outputs of an h x w frame, rr_<name>_device or rr_<name> with args before their
        pointers and tail behind them, the result"""
        outs, ptrs = _outputs((h, w), rgba8, counts, "cuda:%d" % self.device if device else None)
        fn = "rr_%s_device" % name if device else "rr_%s" % name
        self._ck(getattr(self._L, fn)(self._h, w, h, *args, *ptrs, *tail), fn)
        return _result(outs)

    def _supersampled(self, name, width, height, camera, samples, params, rgba8, ray_counts, device):
        """render_samples and the three methods that differ from it in the ray tree alone"""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        offp, n = _sample_offsets(samples, "%s: samples must be an int or an [S, 2] array" % name)
        if n < 0 or w < 0 or h < 0:
            raise ValueError("%s: negative size" % name)
        return self._frame(name, w, h, rgba8, (ray_counts,), device, C.byref(camera), C.byref(p), offp, n)

    def render_samples(self, width, height, camera, samples=4, params=None, rgba8=False, ray_counts=False, device=False):
        """Supersampled frame (rr_render_samples): every pixel of a width x height frame takes S primary rays through S sub-pixel
        positions, each with the shader's whole ray tree, averaged on the GPU in sample order: ((c_0 + c_1) + ...) / S in fp32, c_s
        being what shade_rays gives the ray camera_rays(camera, width, height, *offset_s) has for the pixel.  samples: an int
        (1, 2, 4, 8, 16) for the built-in pattern sample_pattern(samples), or an [S, 2] float32 array of offsets in [0, 1],
        S <= 64.  camera: SceneConstants.  params (default_params()): bounce limits, ior, the ray intervals, and of the flags
        DISPATCH_TONEMAP_REINHARD (RGBA8 output only) and DISPATCH_DEBUG_NO_CULL.  Not a dispatch: read_frame, stats() and the
        tile partition are neither used nor changed.

        -> float32 [height, width, 4] (r, g, b, 1); rgba8=True adds the R8G8B8A8_UNORM store (uint8 [height, width, 4]),
        ray_counts=True the TraceRay calls of the pixel's S trees (uint32 [height, width]); the result is then a tuple in that
        order.  device=False: numpy arrays, blocking.  device=True: new torch tensors on this renderer's GPU (the counts as
        int32), computed on the renderer's stream without waiting for it (stream order as query_rays)."""
        return self._supersampled("render_samples", width, height, camera, samples, params, rgba8, ray_counts, device)

    def set_materials(self, table):
        """The material table (rr_set_materials): a MATERIAL_DTYPE array, or rows of (ior, (sigma_r, sigma_g, sigma_b)) -- index of
        refraction and absorption per unit length and channel.  Instance i is made of row make_instances(materials=...)[i].  Copied;
        an empty table or None clears it.  May come before or after build_tlas and takes effect on the next shade_rays_materials /
        render_materials without a rebuild."""
        t = np.zeros(0, MATERIAL_DTYPE) if table is None else np.ascontiguousarray(table, MATERIAL_DTYPE).reshape(-1)
        self._ck(self._L.rr_set_materials(self._h, t.ctypes.data if len(t) else None, len(t)), "rr_set_materials")
        self._n_materials = len(t)

    def shade_rays_materials(self, rays, params=None, rgba8=False, ray_counts=False):
        """shade_rays with the material table (rr_shade_rays_materials): the same rays, outputs and stream order, shaded by the ray
        tree with an RGB path weight -- ClosestHit refracts with the index of refraction of the hit instance's material, and a ray
        that crossed the glass of an instance is absorbed per channel by exp(-sigma_a * distance) before it is shaded.  params.ior is
        ignored.  A table whose rows are all (ior, (0, 0, 0)) gives shade_rays under default_params(ior=ior) byte for byte."""
        return self._shade("shade_rays_materials", rays, params, rgba8, ray_counts)

    def render_materials(self, width, height, camera, samples=4, params=None, rgba8=False, ray_counts=False, device=False):
        """render_samples with the material table (rr_render_materials): the same arguments, samples, resolve and outputs, every
        sample shaded as shade_rays_materials shades camera_rays(camera, width, height, *offset_s).  params.ior is ignored."""
        return self._supersampled("render_materials", width, height, camera, samples, params, rgba8, ray_counts, device)

    def shade_rays_nested(self, rays, params=None, rgba8=False, ray_counts=False):
        """shade_rays_materials for instances inside, or overlapping, other instances (rr_shade_rays_nested): the same rays, table,
        outputs and stream order, but every ray carries the list of the media it is in (NESTED_MAX_MEDIA at most, empty = air) and
        sees both faces of every triangle.  A front face enters the hit instance's material, a back face leaves it; a surface between
        two different media refracts with ior_from / ior_to, a surface inside one medium is passed straight on; absorption is that of
        the medium crossed.  On closed, consistently wound, pairwise disjoint instances this is shade_rays_materials byte for byte.
        Every instance's row must be <= NESTED_MAX_MATERIAL.  params.ior is ignored."""
        return self._shade("shade_rays_nested", rays, params, rgba8, ray_counts)

    def render_nested(self, width, height, camera, samples=4, params=None, rgba8=False, ray_counts=False, device=False):
        """render_materials with the ray tree of shade_rays_nested (rr_render_nested): the same arguments, samples, resolve and
        outputs, every sample shaded as shade_rays_nested shades camera_rays(camera, width, height, *offset_s)."""
        return self._supersampled("render_nested", width, height, camera, samples, params, rgba8, ray_counts, device)

    def set_surfaces(self, table):
        """The surface table (rr_set_surfaces): a SURFACE_DTYPE array or a list of glass() / opaque(...) rows.  Row r says what an
        instance of material row r is; rows at or beyond the table's length are glass, and None or an empty table makes every row
        glass.  Copied; takes effect on the next shade_rays_surfaces / render_surfaces / render_lit without a rebuild.  set_materials
        leaves it alone, and only those three calls read it."""
        t = np.zeros(0, SURFACE_DTYPE) if table is None else np.ascontiguousarray(table, SURFACE_DTYPE).reshape(-1)
        self._ck(self._L.rr_set_surfaces(self._h, t.ctypes.data if len(t) else None, len(t)), "rr_set_surfaces")

    def set_lights(self, lights=None, ambient=None):
        """The lights of the opaque surfaces (rr_set_lights): a LIGHT_DTYPE array or a list of directional_light(...) /
        point_light(...) rows, MAX_LIGHTS at most, and an RGB ambient term (None: 0).  Copied.  Clears the shape table of
        set_light_shapes, whose rows belong with the lights they were set for."""
        t = np.zeros(0, LIGHT_DTYPE) if lights is None else np.ascontiguousarray(lights, LIGHT_DTYPE).reshape(-1)
        amb = None if ambient is None else np.ascontiguousarray(ambient, np.float32).reshape(3)
        self._ck(self._L.rr_set_lights(self._h, t.ctypes.data if len(t) else None, len(t), None if amb is None else amb.ctypes.data), "rr_set_lights")

    def set_shadow_steps(self, k):
        """Transparent shadows (rr_set_shadow_steps): 0, the default, leaves every shadow ray a first-hit ray that any instance stops,
        glass included.  With 1 <= k <= SHADOW_MAX_STEPS the shadow ray of an opaque hit walks straight through the glass between
        the hit and the light, k closest-hit calls at most (each counted in the ray counts): every stretch inside a medium dims it
        by that medium's sigma_a, only an opaque row stops it, and a walk the cap ends counts as occluded.  Read by
        shade_rays_surfaces, render_surfaces and render_lit; set_lights, set_surfaces and set_materials leave it alone."""
        self._ck(self._L.rr_set_shadow_steps(self._h, int(k)), "rr_set_shadow_steps")

    def shadow_steps(self):
        """the setting of set_shadow_steps in force"""
        k = C.c_uint32(0)
        self._ck(self._L.rr_get_shadow_steps(self._h, C.byref(k)), "rr_get_shadow_steps")
        return int(k.value)

    def shade_rays_surfaces(self, rays, params=None, rgba8=False, ray_counts=False):
        """shade_rays_nested with opaque hit groups (rr_shade_rays_surfaces): the same rays, material table, outputs and stream
        order.  A hit on an instance whose row of the surface table is opaque is, after the absorption of the medium crossed, lit by
        every light it faces and whose shadow ray -- first hit, instances selected by the light's shadow_mask, counted in the ray
        counts -- finds nothing, adds albedo * (ambient + sum) + emission, and continues as a mirror where specular is not zero.
        Without a surface table, or with every row glass, this is shade_rays_nested byte for byte."""
        return self._shade("shade_rays_surfaces", rays, params, rgba8, ray_counts)

    def render_surfaces(self, width, height, camera, samples=4, params=None, rgba8=False, ray_counts=False, device=False):
        """render_nested with the ray tree of shade_rays_surfaces (rr_render_surfaces): the same arguments, samples, resolve and
        outputs, every sample shaded as shade_rays_surfaces shades camera_rays(camera, width, height, *offset_s)."""
        return self._supersampled("render_surfaces", width, height, camera, samples, params, rgba8, ray_counts, device)

    def set_material_bands(self, iors, weights=None):
        """The band set of render_composed (rr_set_material_bands): iors is a float32 [B, rows] array, row b the indices of
        refraction that the rows of the material table in force take in band b (material_bands makes one); weights a float32 [B, 3]
        array, the weight of band b's colour per channel (None: all 1; negative weights allowed).  Copied.  None or an empty array
        clears the set; so does set_materials.  Without a set there is one band, band 0: the table itself, weights 1."""
        if iors is None or np.size(iors) == 0:
            self._ck(self._L.rr_set_material_bands(self._h, None, None, 0), "rr_set_material_bands")
            return
        t = np.ascontiguousarray(iors, np.float32)
        if t.ndim != 2:
            raise ValueError("set_material_bands: iors must be a [B, rows] array")
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float32)
            if w.shape != (t.shape[0], 3):
                raise ValueError("set_material_bands: weights must be a [B, 3] array with one row per band")
            wp = w.ctypes.data_as(C.c_void_p)
        rows = getattr(self, "_n_materials", 0)                 # (no table: the library says so)
        if rows and t.shape[1] != rows:
            raise ValueError("set_material_bands: iors needs one column per row of the material table (%d)" % rows)
        self._ck(self._L.rr_set_material_bands(self._h, t.ctypes.data_as(C.c_void_p), wp, t.shape[0]), "rr_set_material_bands")

    def render_composed(self, width, height, camera, samples=4, lens=None, lens_samples=None, bands=None, paired=False, params=None, rgba8=False,
                        ray_counts=False, device=False):
        """Composed frame (rr_render_composed): render_nested with render_lens' primary rays and render_spectral's resolve over the
        band set of set_material_bands.  Sample k starts at lens offset k of the lens (None or radius 0: a pinhole), is shaded as
        shade_rays_nested shades lens_rays(camera, width, height, *offset_k, *lens_offset_k, lens) under band band_k of the set, and
        channel ch of the pixel is ((w[band_0] * c_0 + w[band_1] * c_1) + ...) / S in fp32, each product and sum rounded once.
        samples: an int (1, 2, 4, 8, 16: sample_pattern), an [A, 2] array of offsets in [0, 1], or a COMPOSED_SAMPLE_DTYPE record
        array, which is passed straight through (lens_samples, bands and paired must then be left alone).  bands: None for band 0
        throughout; an int B crosses the A positions with bands 0 .. B-1, S = A * B <= 64, sample a * B + b being position a in
        band b; with paired=True an [S] array of band indices, one per position.  lens_samples: None for lens_pattern(S), or an
        [S, 2] array in [-1, 1], one row per sample after crossing.  Without a band set only band 0 exists.  A lens disk must lie
        outside every instance.  The other arguments, the outputs and device=True as render_nested; not a dispatch either."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        if w < 0 or h < 0:
            raise ValueError("render_composed: negative size")
        if isinstance(samples, np.ndarray) and samples.dtype == _capi.COMPOSED_SAMPLE_DTYPE:
            if lens_samples is not None or bands is not None or paired:
                raise ValueError("render_composed: a record array of samples carries its own lens offsets and bands")
            rec = np.ascontiguousarray(samples).reshape(-1)
        else:
            offp, n = _sample_offsets(samples, "render_composed: samples must be an int, an [S, 2] array or a COMPOSED_SAMPLE_DTYPE array")
            pos = sample_pattern(n) if offp is None else np.ascontiguousarray(samples, np.float32)
            if bands is None:
                if paired:
                    raise ValueError("render_composed: paired=True needs an array of band indices")
                idx = np.zeros(len(pos), np.uint32)
            elif paired:
                idx, = _paired_indices(len(pos), "render_composed: paired=True needs one band index >= 0 per sample", bands)
            else:
                if not isinstance(bands, (int, np.integer)) or bands < 1:
                    raise ValueError("render_composed: bands must be None, an int >= 1 or, with paired=True, an array of indices")
                if len(pos) * int(bands) > _capi.MAX_SAMPLES:
                    raise ValueError("render_composed: positions x bands must not exceed %d samples" % _capi.MAX_SAMPLES)
                idx = np.tile(np.arange(int(bands)), len(pos))                      # sample a * B + b: position a, band b
                pos = np.repeat(pos, int(bands), axis=0)
            rec = np.zeros(len(pos), _capi.COMPOSED_SAMPLE_DTYPE)
            rec["offset"], rec["band"] = pos, idx
            _per_sample(rec, "lens_offset", lens_samples, lens_pattern, "render_composed: lens_samples")
        return self._record_frame("render_composed", w, h, camera, p, rec, lens, rgba8, ray_counts, device)

    def _record_frame(self, name, w, h, camera, p, rec, lens, rgba8, ray_counts, device):
        """the call of render_composed, render_shutter and render_lit: a frame over sample records and an optional lens"""
        recp = rec.ctypes.data_as(C.c_void_p) if len(rec) else None
        lp = C.byref(lens) if lens is not None else None
        return self._frame(name, w, h, rgba8, (ray_counts,), device, C.byref(camera), C.byref(p), recp, len(rec), lp)

    def capture_scene_key(self, key):
        """Freezes the scene a render call issued now would trace as scene key `key` (rr_capture_scene_key), 0 <= key <
        MAX_SCENE_KEYS: its instances, hierarchy, triangles and normals are copied, device to device on the renderer's stream, into
        buffers the key owns.  Needs a built TLAS.  Capturing into a used key replaces it.  Later builds, refits, vertex updates
        and load_scene change no key; the environment map, the material table and the band set are not part of one."""
        self._ck(self._L.rr_capture_scene_key(self._h, int(key)), "rr_capture_scene_key")

    def release_scene_key(self, key=None):
        """Frees scene key `key`, or every key with None (rr_release_scene_key); an empty key is fine."""
        self._ck(self._L.rr_release_scene_key(self._h, _capi.ALL_SCENE_KEYS if key is None else int(key)), "rr_release_scene_key")

    def scene_key_info(self, key):
        """-> SceneKeyInfo of scene key `key` (rr_scene_key_info): captured, top_level, n_instances, n_triangles, bounds (lo xyz, hi
        xyz), stack_need, max_material, bytes; all zero for an empty key."""
        info = _capi.SceneKeyInfo()
        self._ck(self._L.rr_scene_key_info(self._h, int(key), C.byref(info)), "rr_scene_key_info")
        return info

    def render_shutter(self, width, height, camera, samples=4, keys=None, lens=None, lens_samples=None, bands=None, paired=False, params=None,
                       rgba8=False, ray_counts=False, device=False):
        """Shutter frame (rr_render_shutter): render_composed with every sample traced in a captured scene key -- motion blur over
        the instants capture_scene_key froze.  Sample k is shaded as shade_rays_nested shades lens_rays(...) (no lens: camera_rays)
        in the scene of key key_k under band band_k, and the pixel resolves as render_composed's.  The live scene is not used and
        need not be built.
        samples: an int (sample_pattern), an [A, 2] array of offsets, or a SHUTTER_SAMPLE_DTYPE record array, which is passed
        straight through (keys, lens_samples, bands and paired must then be left alone; shutter_samples makes one).  keys: an int K
        crosses the positions with keys 0 .. K-1; with paired=True an [S] array, one key per position.  None is refused: there is
        no implicit key.  bands: None for band 0; an int B crosses with bands 0 .. B-1; with paired=True an [S] array.  With ints,
        sample (a * K + j) * B + b is position a, key j, band b, and A * K * B <= 64.  The other arguments, the outputs and
        device=True as render_composed; not a dispatch either.  The camera and the lens disk must lie outside every instance of
        every key used."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        if w < 0 or h < 0:
            raise ValueError("render_shutter: negative size")
        if isinstance(samples, np.ndarray) and samples.dtype == _capi.SHUTTER_SAMPLE_DTYPE:
            if keys is not None or lens_samples is not None or bands is not None or paired:
                raise ValueError("render_shutter: a record array of samples carries its own keys, lens offsets and bands")
            rec = np.ascontiguousarray(samples).reshape(-1)
        else:
            if keys is None:
                raise ValueError("render_shutter: keys is required (an int K, or with paired=True one key per sample): there is no implicit key")
            offp, n = _sample_offsets(samples, "render_shutter: samples must be an int, an [S, 2] array or a SHUTTER_SAMPLE_DTYPE array")
            pos = sample_pattern(n) if offp is None else np.ascontiguousarray(samples, np.float32)
            if paired:
                rec = np.zeros(len(pos), _capi.SHUTTER_SAMPLE_DTYPE)
                rec["offset"] = pos
                rec["key"], rec["band"] = _paired_indices(
                    len(pos), "render_shutter: paired=True needs one key index >= 0 (and, if given, one band index >= 0) per sample", keys, bands,
                    refuse=isinstance(keys, (int, np.integer)))
                _per_sample(rec, "lens_offset", lens_samples, lens_pattern, "render_shutter: lens_samples")
            else:
                if not isinstance(keys, (int, np.integer)) or keys < 1 or not (bands is None or (isinstance(bands, (int, np.integer)) and bands >= 1)):
                    raise ValueError("render_shutter: keys must be an int >= 1 and bands None or an int >= 1, or both arrays with paired=True")
                rec = shutter_samples(pos, int(keys), bands, lens_samples)
        return self._record_frame("render_shutter", w, h, camera, p, rec, lens, rgba8, ray_counts, device)

    def set_light_shapes(self, shapes=None):
        """The shapes of the lights (rr_set_light_shapes): a LIGHT_SHAPE_DTYPE array or a list of light_shape(ex, ey) rows, one per
        light in force, row i with light i; None or an empty table clears it.  Copied; takes effect on the next render_lit without a
        rebuild.  set_lights clears it, and only render_lit reads it."""
        t = np.zeros(0, _capi.LIGHT_SHAPE_DTYPE) if shapes is None else np.ascontiguousarray(shapes, _capi.LIGHT_SHAPE_DTYPE).reshape(-1)
        self._ck(self._L.rr_set_light_shapes(self._h, t.ctypes.data if len(t) else None, len(t)), "rr_set_light_shapes")

    def render_lit(self, width, height, camera, samples=4, keys=None, lens=None, lens_samples=None, bands=None, light_samples=None, paired=False,
                   params=None, rgba8=False, ray_counts=False, device=False):
        """Lit shutter frame (rr_render_lit): render_shutter over the ray tree of shade_rays_surfaces, with a point on every light per
        sample -- the lit scene through the lens, with motion blur, dispersion and soft shadows.  Sample k is shaded as
        shade_rays_surfaces shades lens_rays(...) (no lens: camera_rays) in the scene of key key_k under band band_k, the surface table
        and ambient term in force and the lights moved_lights(lights, shapes, *light_offset_k); the pixel resolves as render_shutter's.
        samples, keys, lens, lens_samples, bands and paired as render_shutter; a LIT_SAMPLE_DTYPE record array is passed straight
        through (lit_samples makes one).  light_samples: None for light_pattern(A), one offset per position, or an [A, 2] array in
        [-1, 1] (with paired=True a position is a sample).  A shaped light is a rectangle of point emitters: no cosine at the light and
        no normalisation by its area.  The outputs and device=True as render_shutter; not a dispatch either."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        if w < 0 or h < 0:
            raise ValueError("render_lit: negative size")
        if isinstance(samples, np.ndarray) and samples.dtype == _capi.LIT_SAMPLE_DTYPE:
            if keys is not None or lens_samples is not None or bands is not None or light_samples is not None or paired:
                raise ValueError("render_lit: a record array of samples carries its own keys, lens offsets, bands and light offsets")
            rec = np.ascontiguousarray(samples).reshape(-1)
        else:
            if keys is None:
                raise ValueError("render_lit: keys is required (an int K, or with paired=True one key per sample): there is no implicit key")
            offp, n = _sample_offsets(samples, "render_lit: samples must be an int, an [S, 2] array or a LIT_SAMPLE_DTYPE array")
            pos = sample_pattern(n) if offp is None else np.ascontiguousarray(samples, np.float32)
            if paired:
                rec = np.zeros(len(pos), _capi.LIT_SAMPLE_DTYPE)
                rec["offset"] = pos
                rec["key"], rec["band"] = _paired_indices(
                    len(pos), "render_lit: paired=True needs one key index >= 0 (and, if given, one band index >= 0) per sample", keys, bands,
                    refuse=isinstance(keys, (int, np.integer)))
                _per_sample(rec, "lens_offset", lens_samples, lens_pattern, "render_lit: lens_samples")
                _per_sample(rec, "light_offset", light_samples, light_pattern, "render_lit: light_samples")
            else:
                if not isinstance(keys, (int, np.integer)) or keys < 1 or not (bands is None or (isinstance(bands, (int, np.integer)) and bands >= 1)):
                    raise ValueError("render_lit: keys must be an int >= 1 and bands None or an int >= 1, or both arrays with paired=True")
                rec = lit_samples(pos, int(keys), bands, lens_samples, light_samples)
        return self._record_frame("render_lit", w, h, camera, p, rec, lens, rgba8, ray_counts, device)

    def render_lens(self, width, height, camera, lens, samples=16, lens_samples=None, params=None, rgba8=False, ray_counts=False, device=False):
        """Thin-lens frame (rr_render_lens): render_samples with a lens of finite aperture -- sample s of a pixel starts at lens
        offset s on a disk of lens.radius round the camera and passes through the point its sub-pixel position sees at
        lens.focus_distance, so what lies in that plane is sharp and the rest is averaged over the aperture.  Bit for bit the fold of
        shade_rays on lens_rays(camera, width, height, *offset_s, *lens_offset_s, lens) by render_samples' resolve rule; with
        lens.radius == 0, render_samples itself.  lens: Lens(radius, focus_distance).  samples: as for render_samples.  lens_samples:
        None for the built-in lens_pattern(S), or an [S, 2] float32 array of offsets in [-1, 1] (units of the radius), S being the
        number of samples.  The other arguments, the outputs and device=True as render_samples; not a dispatch either."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        offp, n = _sample_offsets(samples, "render_lens: samples must be an int or an [S, 2] array")
        if n < 0 or w < 0 or h < 0:
            raise ValueError("render_lens: negative size")
        loffp = None
        if lens_samples is not None:
            loff = np.ascontiguousarray(lens_samples, np.float32)
            if loff.shape != (n, 2) or n == 0:
                raise ValueError("render_lens: lens_samples must be an [S, 2] array with one row per sample")
            loffp = loff.ctypes.data_as(C.c_void_p)
        lp = C.byref(lens) if lens is not None else None
        return self._frame("render_lens", w, h, rgba8, (ray_counts,), device, C.byref(camera), C.byref(p), offp, loffp, n, lp)

    def render_spectral(self, width, height, camera, bands=8, samples=4, params=None, abbe=30.0, paired=False, rgba8=False, ray_counts=False,
                        device=False):
        """Spectral frame (rr_render_spectral): render_samples with dispersion -- sample k of a pixel is shaded with the index of
        refraction of band k instead of params.ior, and its colour is weighted per channel: channel ch of the pixel is
        ((w_0 * c_0 + w_1 * c_1) + ...) / S in fp32, each product and sum rounded once, c_k being what shade_rays gives the ray of
        camera_rays(camera, width, height, *offset_k) under default_params(ior=ior_k, ...).  Refracting glass gets colour fringes.
        bands: an int B for spectral_bands(B, params.ior, abbe) (abbe is used for nothing else), a BAND_DTYPE array of your own
        (negative weights allowed), or None for (params.ior, 1, 1, 1) throughout, which is render_samples byte for byte.
        samples: as for render_samples, A positions.  By default the positions are crossed with the bands: S = A * B <= 64 samples,
        sample a * B + b is position a in band b.  paired=True: both tables have S rows and sample k takes row k of each
        (bands=None is always paired).  The other arguments, the outputs and device=True as render_samples; not a dispatch either."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        offp, n = _sample_offsets(samples, "render_spectral: samples must be an int or an [S, 2] array")
        if n < 0 or w < 0 or h < 0:
            raise ValueError("render_spectral: negative size")
        bandp = None
        if bands is not None:
            tab = spectral_bands(bands, p.ior, abbe) if isinstance(bands, (int, np.integer)) else np.ascontiguousarray(bands, BAND_DTYPE)
            if tab.ndim != 1 or len(tab) == 0:
                raise ValueError("render_spectral: bands must be an int, None or a non-empty one-dimensional BAND_DTYPE array")
            if paired:
                if len(tab) != n:
                    raise ValueError("render_spectral: paired=True needs one band per sample")
            else:
                if n * len(tab) > _capi.MAX_SAMPLES:
                    raise ValueError("render_spectral: positions x bands must not exceed %d samples" % _capi.MAX_SAMPLES)
                pos = sample_pattern(n) if offp is None else np.ascontiguousarray(samples, np.float32)
                off = np.ascontiguousarray(np.repeat(pos, len(tab), axis=0))        # sample a * B + b: position a, band b
                tab = np.ascontiguousarray(np.tile(tab, n))
                offp, n = off.ctypes.data_as(C.c_void_p), len(off)
            bandp = tab.ctypes.data_as(C.c_void_p)
        return self._frame("render_spectral", w, h, rgba8, (ray_counts,), device, C.byref(camera), C.byref(p), offp, bandp, n)

    def render_adaptive(self, width, height, camera, samples=(4, 16), threshold=ADAPTIVE_THRESHOLD, params=None, rgba8=False, ray_counts=False,
                        sample_counts=False, device=False):
        """Adaptively supersampled frame (rr_render_adaptive): every pixel takes the first n_base samples of the pattern, and the
        rest up to n_max only where its base samples show contrast -- the displayed values (clamped to [0, 1], after Reinhard if
        params asks for it) of its own base samples spread by more than threshold in some channel, or its base colour differs by
        more than threshold from a 4-neighbour's.  Each pixel is bit for bit that pixel of render_samples with n_base or with n_max
        samples (include/rrdxr.h has the rule).  samples: (n_base, n_max) ints for the built-in pattern sample_pattern(n_max), or
        (n_base, offsets [S, 2]) with n_max = S.  The other arguments as render_samples; not a dispatch either.

        -> float32 [height, width, 4]; rgba8=True adds the uint8 [height, width, 4] store, ray_counts=True the TraceRay calls of the
        trees each pixel ran, sample_counts=True n_base or n_max per pixel (uint32 [height, width]); a tuple in that order, with the
        number of refined pixels last when device=False.  device=True: torch tensors (counts as int32) on the renderer's stream,
        the workspace (a tensor the renderer keeps per stream it is put on) included, nothing synchronised -- and no refined-pixel count, which only a read-back could give."""
        p = params if params is not None else default_params()
        w, h = int(width), int(height)
        n_base, top = samples
        n_base = int(n_base)
        offp, n_max = _sample_offsets(top, "render_adaptive: samples must be (n_base, n_max) or (n_base, [S, 2] array)")
        if n_base < 0 or n_max < 0 or w < 0 or h < 0:
            raise ValueError("render_adaptive: negative size")
        args = (C.byref(camera), C.byref(p), offp, n_base, n_max, float(threshold))
        if device:
            import torch
            nbytes = int(self._L.rr_host_adaptive_workspace_bytes(w, h))
            # one workspace per stream the renderer has been put on, reused call after call: the calls on a stream are ordered,
            # calls on different streams are not and never share one.  Before a larger one replaces it that stream is waited
            # for, since the stages in flight still read the old one
            key = getattr(self, "_stream_key", None)
            pool = self.__dict__.setdefault("_adaptive_ws", {})
            ws = pool.get(key)
            if ws is None or ws.numel() * 4 < nbytes:
                if ws is not None:
                    self.wait()
                ws = pool[key] = torch.empty((max(nbytes, 16) // 16, 4), dtype=torch.float32, device="cuda:%d" % self.device)
            return self._frame("render_adaptive", w, h, rgba8, (ray_counts, sample_counts), True, *args, tail=(C.c_void_p(ws.data_ptr()), ws.numel() * 4))
        n_ref = C.c_uint64(0)
        out = self._frame("render_adaptive", w, h, rgba8, (ray_counts, sample_counts), False, *args, tail=(C.byref(n_ref),))
        return (out if isinstance(out, tuple) else (out,)) + (int(n_ref.value),)

    def env_lookup(self, dirs):
        """Miss (RayTracing.hlsl:127-137) on an [n,3] array of directions -> [n,3] texels."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros_like(dirs)
        self._ck(self._L.rr_env_lookup(self._h, dirs.ctypes.data, len(dirs), out.ctypes.data), "rr_env_lookup")
        return out

    def download_blas(self, mesh_id):
        nn, nt = C.c_uint32(), C.c_uint32()
        self._ck(self._L.rr_download_blas(self._h, mesh_id, None, C.byref(nn), None, C.byref(nt)), "rr_download_blas")
        nodes = np.zeros(nn.value, NODE_DTYPE)
        tris = np.zeros(nt.value, TRI_DTYPE)
        self._ck(self._L.rr_download_blas(self._h, mesh_id, nodes.ctypes.data, C.byref(nn), tris.ctypes.data,
                                          C.byref(nt)), "rr_download_blas")
        return nodes, tris

    def download_qnodes(self, mesh_id):
        """-> (QNODE_DTYPE array, grid origin float32[3], grid cell float32[3]): the nodes as traversal reads them"""
        from ._capi import QNODE_DTYPE
        nn = C.c_uint32()
        g = (C.c_float * 6)()
        self._ck(self._L.rr_download_qnodes(self._h, mesh_id, None, C.byref(nn), g), "rr_download_qnodes")
        q = np.zeros(nn.value, QNODE_DTYPE)
        self._ck(self._L.rr_download_qnodes(self._h, mesh_id, q.ctypes.data, C.byref(nn), g), "rr_download_qnodes")
        ga = np.array(list(g), np.float32)
        return q, ga[:3], ga[3:]

    def download_tlas(self):
        """-> (NODE_DTYPE array, QNODE_DTYPE array, grid origin float32[3], grid cell float32[3]): the top level in fp32 and as
        traversal reads it on the scene grid; a leaf ref is ~(triangles of the scene's distinct meshes + instance)"""
        from ._capi import QNODE_DTYPE
        nn = C.c_uint32()
        g = (C.c_float * 6)()
        self._ck(self._L.rr_download_tlas(self._h, None, None, C.byref(nn), g), "rr_download_tlas")
        nodes = np.zeros(nn.value, NODE_DTYPE)
        q = np.zeros(nn.value, QNODE_DTYPE)
        self._ck(self._L.rr_download_tlas(self._h, nodes.ctypes.data, q.ctypes.data, C.byref(nn), g), "rr_download_tlas")
        ga = np.array(list(g), np.float32)
        return nodes, q, ga[:3], ga[3:]

    # convenience: the reference's whole init sequence for one mesh + env map
    def load_scene(self, verts, indices, env_rgb, instances=None):
        mid = self.upload_mesh(verts, indices)
        self.build_blas(mid)
        if instances is None:
            instances = make_instances(meshes=[mid])
        self.build_tlas(instances)
        if env_rgb is not None:
            self.upload_envmap(env_rgb)
        return mid


class RefractionDemo:
    """RefractionDemo.hpp:9-10: initialize(hWnd, w, h) / drawFrame(), headless."""

    def __init__(self):
        self.renderer = None
        self.cubeMesh = Mesh()
        self.angle = 0.01               # static float angle (RefractionDemo.cpp:555)

    def initialize(self, width=1024, height=768, mesh_path="../shell.obj", env_path="../envMap.hdr", device=0,
                   params=None):
        self.width, self.height = width, height
        self.params = params
        self.renderer = Renderer(device)
        env, _ = load_texture(env_path, 3)                       # :527
        self.renderer.upload_envmap(env)
        if not self.cubeMesh.load(mesh_path):                    # :537 (the reference ignores the result)
            raise RRError(6, "Mesh::load(%s)" % mesh_path)
        mid = self.cubeMesh.upload(self.renderer)                # :538
        self.renderer.build_blas(mid)                            # :541
        self.renderer.build_tlas(make_instances(meshes=[mid]))

    def drawFrame(self):
        self.renderer.set_camera(camera_orbit(self.angle))       # :559-566
        self.angle = float(np.float32(self.angle) + np.float32(0.01))   # :567
        self.renderer.dispatch_rays(self.width, self.height, self.params)   # :580-594
        return self.renderer.read_frame()                        # :596-611
