"""Host side of the product (no GPU): OBJ loader, camera math, image decode, C-ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from refraction_raytracing_dxr_amd import _capi
from host_goldens import CAMERA_KATS, LOADER_GOLD, M_GOLD, _adam7_cases, _write_adam7_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------- C ABI surface
def declared_functions():
    """every function prototype in include/rrdxr.h"""
    src = open(os.path.join(ROOT, "include", "rrdxr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rr_[a-z0-9_]+)\s*\(", src)) - {"rr_context"})


def test_library_exports_every_declared_symbol():
    lib = C.CDLL(rr.lib_path())
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "librrdxr.so lacks %s declared in include/rrdxr.h" % n
    # and the binding table covers the header exactly
    assert sorted(_capi.SYMBOLS) == names
    assert rr.lib().rr_abi_version() == 3


def test_header_compiles_as_c_and_structs_have_the_documented_sizes(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rrdxr.h"\n'
                   '_Static_assert(sizeof(rr_vertex) == 32, "vertex");\n'
                   '_Static_assert(sizeof(rr_instance_desc) == 64, "instance");\n'
                   '_Static_assert(sizeof(rr_scene_constants) == 80, "constants");\n'
                   '_Static_assert(sizeof(rr_ray) == 48 && sizeof(rr_hit) == 24, "ray/hit");\n'
                   'int main(void) { return 0; }\n')
    import subprocess
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "t.o")], check=True)


def test_no_device_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(rr.RRError) as e:
        rr.Renderer(0)
    assert e.value.status == 2          # RR_ERR_NO_DEVICE
    h = C.c_void_p()
    assert rr.lib().rr_create(0, C.byref(h)) == 2 and not h.value


def test_default_params_are_the_shader_literals():
    p = rr.default_params()
    assert (p.max_refract, p.max_reflect) == (5, 2)                       # RayTracing.hlsl:82,110
    assert p.ior == np.float32(1.3)                                       # :95
    assert (p.tmin_primary, p.tmax_primary) == (np.float32(1e-4), 100.0)  # :52-53
    assert (p.tmin_secondary, p.tmax_secondary) == (np.float32(1e-3), 1000.0)   # :99-100
    assert p.flags == 0


# ---------------------------------------------------------------------------------- Mesh::load
@pytest.mark.parametrize("name", sorted(LOADER_GOLD))
def test_mesh_load_matches_reference_hashes(name):
    tris, h, lo, hi = LOADER_GOLD[name]
    m = rr.Mesh()
    assert m.load(O.asset(name)) is True
    assert len(m.verts) == 3 * tris and np.array_equal(m.indices, np.arange(3 * tris, dtype=np.uint32))
    assert "%016x" % O.fnv1a64(m.verts) == h
    ov, oi = O.mesh_load(O.asset(name))
    assert m.verts.tobytes() == ov.tobytes() and np.array_equal(m.indices, oi)


def test_mesh_load_edge_cases(tmp_path):
    m = rr.Mesh()
    assert m.load(str(tmp_path / "missing.obj")) is False                 # Mesh.cpp:9-10
    p = tmp_path / "e.obj"
    p.write_text("")                                                      # empty file: loads, no triangles
    assert m.load(str(p)) is True and len(m.verts) == 0
    # sscanf semantics: leading blanks disqualify a line, comments and unknown records are ignored,
    # a 4th corner is dropped, 'v' wins over 'vt'/'vn' only if three floats follow
    p.write_text("# c\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\n v 9 9 9\nvt 0 0\nvt 1 1\nvn 0 0 1\n"
                 "l 1 2\nf 1/1/1 2/2/1 3/1/1 4/2/1\nf 1//1 2//1 3//1\nf 4/2/1 3/1/1 2/2/1\n")
    m = rr.Mesh()
    assert m.load(str(p)) and len(m.verts) == 6
    assert np.array_equal(m.verts["position"][3], (0, 0, 1)) and np.array_equal(m.verts["uv"][1], (1, 1))
    ov, _ = O.mesh_load(str(p))
    assert m.verts.tobytes() == ov.tobytes()
    # loading twice appends, indices keep counting (Mesh.cpp:31-32)
    assert m.load(str(p)) and len(m.verts) == 12 and m.indices[-1] == 11
    # out-of-range references: the reference reads wild memory; this loader refuses
    p.write_text("v 0 0 0\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 1/1/1\n")
    assert rr.Mesh().load(str(p)) is False


# ---------------------------------------------------------------------------------- camera
def test_position_validation(tmp_path):
    """what rr_upload_mesh demands of positions (finite, |coordinate| <= 1e18), checked on the CPU; Mesh::load itself keeps
    accepting such a file, as the reference's loader does (strtof("1e39") is +inf)"""
    L = rr.lib()
    bad = C.c_uint32(99)
    v = np.zeros(5, rr.VERTEX_DTYPE)
    v["position"] = np.arange(15, dtype=np.float32).reshape(5, 3)
    assert L.rr_host_validate_positions(v.ctypes.data, 5, C.byref(bad)) == 0 and bad.value == 99
    for val in (np.inf, -np.inf, np.nan, 1.1e18, -3e38):
        w = v.copy()
        w["position"][3, 1] = val
        assert L.rr_host_validate_positions(w.ctypes.data, 5, C.byref(bad)) == 1 and bad.value == 3, val
    w = v.copy()
    w["position"][0] = (1e18, -1e18, 0)
    assert L.rr_host_validate_positions(w.ctypes.data, 5, None) == 0
    w["norm"][2] = np.nan                                        # normals and uvs are not positions
    assert L.rr_host_validate_positions(w.ctypes.data, 5, None) == 0
    assert L.rr_host_validate_positions(None, 0, None) == 0
    p = tmp_path / "huge.obj"
    p.write_text("v 1e39 0 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")
    m = rr.Mesh()
    assert m.load(p) and np.isinf(np.asarray(m.verts)["position"][0, 0])
    assert L.rr_host_validate_positions(np.asarray(m.verts).ctypes.data, 3, C.byref(bad)) == 1 and bad.value == 0


def test_camera_matches_oracle_and_kats():
    for a in (0.01, 0.02, 1.0, 3.14, 6.28, -0.5):
        sc = rr.camera_orbit(a)
        M, cam = O.camera(a)
        assert np.allclose(np.array(sc.proj_inv), M, rtol=0, atol=2e-6)
        assert np.allclose(np.array(sc.camera_loc), cam, rtol=0, atol=1e-6)
    sc = rr.camera_orbit(0.01)
    assert np.allclose(np.array(sc.proj_inv).reshape(4, 4), M_GOLD, atol=2e-6)
    for W, H, x, y, d in CAMERA_KATS:
        _, dd = O.camera_ray(np.array(sc.proj_inv), np.array(sc.camera_loc), x, y, W, H)
        assert np.allclose(dd, d, atol=1e-5)
    bad = _capi.SceneConstants()
    assert rr.lib().rr_host_camera_orbit(0.01, 0.0, 1.333, 1.0, 125.0, C.byref(bad)) == 1


# ---------------------------------------------------------------------------------- stbi_loadf stand-in
# What the reference's own stb_image.h (v2.28, built by oracle/Makefile where the reference tree is present) returns for every
# file the three *_vs_reference_stb tests below write, stored by tests/golden/make_stb_goldens.py: the tests compare against
# it bit for bit without needing the reference.  Arrays are stored whole; envmap.png's decodes (1.2 M floats each) by FNV-1a 64.
STB_GOLD = os.path.join(ROOT, "tests", "golden", "stb_decode.npz")
_stb_gold = None


def stb_gold():
    global _stb_gold
    if _stb_gold is None:
        _stb_gold = dict(np.load(STB_GOLD))
    return _stb_gold


def assert_matches_reference_stb(key, mine, n):
    """mine / n: rr.load_texture's result for the file stored under `key`; equal bit for bit to stbi_loadf's"""
    g = stb_gold()
    assert n == int(g[key + "/n"]), key
    if key in g:
        ref = g[key]
        assert mine.shape == ref.shape, key
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), key
    else:
        assert mine.shape == tuple(g[key + "/shape"]), key
        assert O.fnv1a64(mine) == int(g[key + "/fnv1a64"]), key


def test_envmap_png_golden():
    env, n = rr.load_texture(O.asset("envmap.png"), 3)
    assert env.shape == (480, 640, 3) and n == 4
    assert "%016x" % O.fnv1a64(env) == "38c5be075155201f"
    assert abs(env.mean() - 0.528603) < 1e-6 and env.max() == 1.0
    assert abs(env[0, 0, 0] - 0.344026) < 1e-6 and abs(env[240, 320, 0] - 0.529523) < 1e-6


def _write_png(path, arr, mode):
    from PIL import Image
    Image.fromarray(arr, mode).save(path)


def png_decode_cases(tmp_path, req):
    """the PNG files test_png_decode_bit_exact_vs_reference_stb decodes -> [(name, path)]"""
    from PIL import Image
    rng = np.random.default_rng(req)
    cases = {
        "rgb.png": (rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), "RGB"),
        "rgba.png": (rng.integers(0, 256, (19, 64, 4), dtype=np.uint8), "RGBA"),
        "gray.png": (rng.integers(0, 256, (40, 31), dtype=np.uint8), "L"),
        "la.png": (rng.integers(0, 256, (16, 16, 2), dtype=np.uint8), "LA"),
        "smooth.png": (np.tile(np.arange(256, dtype=np.uint8), (64, 1)), "L"),     # exercises the PNG filters
    }
    out = []
    for name, (arr, mode) in cases.items():
        _write_png(tmp_path / name, arr, mode)
        out.append((name, tmp_path / name))
    # palette and 16-bit
    Image.fromarray(cases["rgb.png"][0], "RGB").quantize(17).save(tmp_path / "pal.png")
    Image.fromarray(rng.integers(0, 65536, (9, 11), dtype=np.uint16)).save(tmp_path / "g16.png")
    out += [("pal.png", tmp_path / "pal.png"), ("g16.png", tmp_path / "g16.png")]
    return out + [("envmap.png", O.asset("envmap.png"))]


@pytest.mark.parametrize("req", [0, 1, 2, 3, 4])
def test_png_decode_bit_exact_vs_reference_stb(tmp_path, req):
    for name, p in png_decode_cases(tmp_path, req):
        mine, n = rr.load_texture(p, req)
        assert_matches_reference_stb("png/%d/%s" % (req, name), mine, n)


def test_hdr_write_read_roundtrip(tmp_path):
    from conftest import procedural_env
    env = procedural_env(96, 48, seed=2)
    env[0, :9] = 0.0                                   # a run of black pixels (RLE runs, zero exponent)
    env[1, 0] = (1e-40, 0, 0)                          # underflows to the all-zero RGBE pixel
    p = tmp_path / "e.hdr"
    rr.write_hdr(p, env)
    back, n = rr.load_texture(p, 3)
    assert back.shape == env.shape and n == 3
    mx = env.max(axis=2, keepdims=True)
    assert np.all(np.abs(back - env) <= mx / 128.0 + 1e-30)     # 8-bit mantissa shared exponent
    assert np.all(back[0, :9] == 0) and np.all(back[1, 0] == 0)
    # narrow images are stored flat (width < 8): same pixel values
    rr.write_hdr(tmp_path / "n.hdr", env[:, :5].copy())
    nb, _ = rr.load_texture(tmp_path / "n.hdr", 3)
    assert np.array_equal(nb, back[:, :5])
    # idempotent once quantised
    rr.write_hdr(tmp_path / "e2.hdr", back)
    again, _ = rr.load_texture(tmp_path / "e2.hdr", 3)
    assert np.array_equal(again, back)


def hdr_decode_cases(tmp_path):
    """the Radiance files test_hdr_decode_bit_exact_vs_reference_stb decodes -> [(name, path)]"""
    from conftest import procedural_env
    out = []
    for w, h in ((96, 48), (5, 7), (8, 3)):
        p = tmp_path / ("e%dx%d.hdr" % (w, h))
        rr.write_hdr(p, procedural_env(w, h, seed=w))
        out.append((p.name, p))
    return out


@pytest.mark.parametrize("req", [0, 1, 3, 4])
def test_hdr_decode_bit_exact_vs_reference_stb(tmp_path, req):
    for name, p in hdr_decode_cases(tmp_path):
        mine, n = rr.load_texture(p, req)
        assert n == 3
        assert_matches_reference_stb("hdr/%d/%s" % (req, name), mine, n)


def test_adam7_png_decodes_to_the_image_it_was_made_from(tmp_path):
    """Interlaced PNGs (stb_image reads them, RefractionDemo.cpp:111 goes through stbi_loadf): the seven passes are put back
    where they belong -- checked against the pixels the file was built from, through the decoder's own LDR -> float rule."""
    rng = np.random.default_rng(7)
    for name, (arr, depth, pal) in _adam7_cases(rng).items():
        _write_adam7_png(tmp_path / name, arr, depth, pal)
        mine, n = rr.load_texture(tmp_path / name, 0)
        if pal is not None:
            want8 = np.asarray(pal)[arr]
        elif depth == 16:
            want8 = (arr >> 8).astype(np.uint8)
        elif depth < 8:
            want8 = (arr * {1: 255, 2: 85, 4: 17}[depth]).astype(np.uint8)
        else:
            want8 = arr
        want8 = want8.reshape(arr.shape[0], arr.shape[1], -1)
        assert mine.shape == want8.shape and n == want8.shape[2], name
        col = want8.shape[2] - (1 if want8.shape[2] in (2, 4) else 0)               # alpha stays linear
        want = np.empty(want8.shape, np.float32)
        want[..., :col] = np.power(want8[..., :col].astype(np.float32) / np.float32(255.0), np.float32(2.2)).astype(np.float32)
        if col < want8.shape[2]:
            want[..., col:] = want8[..., col:].astype(np.float32) / np.float32(255.0)
        assert np.allclose(mine, want, rtol=2e-6, atol=1e-7), name


def adam7_decode_cases(tmp_path):
    """the interlaced PNGs test_adam7_png_bit_exact_vs_reference_stb decodes -> [(name, path)]"""
    rng = np.random.default_rng(8)
    out = []
    for name, (arr, depth, pal) in _adam7_cases(rng).items():
        _write_adam7_png(tmp_path / name, arr, depth, pal)
        out.append((name, tmp_path / name))
    return out


@pytest.mark.parametrize("req", [0, 3])
def test_adam7_png_bit_exact_vs_reference_stb(tmp_path, req):
    for name, p in adam7_decode_cases(tmp_path):
        mine, n = rr.load_texture(p, req)
        assert_matches_reference_stb("adam7/%d/%s" % (req, name), mine, n)


def test_formats_outside_the_asset_surface_are_refused(tmp_path):
    """rr_host_image_loadf decodes Radiance .hdr and PNG only (include/rrdxr.h); the other formats stbi_loadf accepts
    (stb_image.h:1491) come back as a clean failure, never as a crash or a wrong image."""
    from PIL import Image
    img = Image.fromarray(np.arange(48, dtype=np.uint8).reshape(4, 4, 3), "RGB")
    for name, fmt in (("a.jpg", "JPEG"), ("a.bmp", "BMP"), ("a.tga", "TGA"), ("a.gif", "GIF"), ("a.ppm", "PPM")):
        img.save(tmp_path / name, fmt)
        with pytest.raises(rr.RRError):
            rr.load_texture(tmp_path / name)
    (tmp_path / "interlace2.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\0\0\0\x0dIHDR" + b"\0\0\0\x02\0\0\0\x02\x08\x02\0\0\x02" + b"\0" * 20)
    with pytest.raises(rr.RRError):
        rr.load_texture(tmp_path / "interlace2.png")      # interlace method 2 does not exist


def test_image_load_failures(tmp_path):
    with pytest.raises(rr.RRError):
        rr.load_texture(tmp_path / "nope.hdr")
    (tmp_path / "junk.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\0" * 40)
    with pytest.raises(rr.RRError):
        rr.load_texture(tmp_path / "junk.png")
    (tmp_path / "bad.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 2 +X 2\n" + b"\0" * 16)
    with pytest.raises(rr.RRError):
        rr.load_texture(tmp_path / "bad.hdr")


def test_hardened_obj_loader(tmp_path):
    """quads, v//vn and bare-v corners, negative indices -- additive, default unchanged."""
    for name in LOADER_GOLD:                                   # hardened mode reads the reference's files identically
        a, b = rr.Mesh(), rr.Mesh()
        assert a.load(O.asset(name)) and b.load(O.asset(name), hardened=True)
        assert a.verts.tobytes() == b.verts.tobytes() and np.array_equal(a.indices, b.indices)
    p = tmp_path / "q.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0.5 0.25\n"
                 "f 1//1 2//1 3//1 4//1\n"          # quad, no uv
                 "f -4 -3 -2\n"                      # negative indices, no uv, no normal
                 "f 1/1 2/1 3/1\n")                  # uv but no normal
    strict = rr.Mesh()
    assert strict.load(str(p)) and len(strict.verts) == 0      # the reference's sscanf pattern matches none of these
    m = rr.Mesh()
    assert m.load(str(p), hardened=True)
    assert len(m.verts) == 12 and np.array_equal(m.indices, np.arange(12, dtype=np.uint32))
    P = m.verts["position"]
    assert np.array_equal(P[:6], [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 0), (1, 1, 0), (0, 1, 0)])   # fan
    assert np.array_equal(P[6:9], [(0, 0, 0), (1, 0, 0), (1, 1, 0)])
    assert np.all(m.verts["norm"][:6] == (0, 0, 1)) and np.all(m.verts["uv"][:6] == 0)
    assert np.allclose(m.verts["norm"][6:12], (0, 0, 1))       # flat winding normal where vn is absent
    assert np.all(m.verts["uv"][9:12] == (0.5, 0.25))
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n")
    assert rr.Mesh().load(str(p), hardened=True) is False      # out of range


# ---------------------------------------------------------------------------------- mesh-tile partition without a camera
@pytest.mark.parametrize("w,h", [(1920, 1080), (211, 149), (97, 61), (33, 1), (1, 1), (5, 600)])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_mesh_partition_without_constants_is_the_whole_frame(w, h, world):
    """rr_host_mesh_partition(bounds, NULL, ...) -- what a RR_DISPATCH_DEBUG_NO_CULL launch on the mesh path renders and sizes
    its buffers by: no rectangle, no background tiles, every tile a mesh tile dealt round robin over all ranks."""
    m = rr.Mesh()
    assert m.load(O.asset("monkey.obj"))
    pos = m.verts["position"]
    b = (C.c_float * 6)(*[float(v) for v in pos.min(axis=0)], *[float(v) for v in pos.max(axis=0)])
    part = _capi.MeshPartition()
    assert rr.lib().rr_host_mesh_partition(b, None, 1, w, h, world, C.byref(part)) == 0
    tx = (w + 31) // 32
    n_tiles = tx * ((h + 31) // 32)
    assert (part.tiles_x, part.n_tiles, part.world) == (tx, n_tiles, world)
    assert part.rect_w == 0 and part.rect_h == 0 and part.n_bg_tiles == 0 and part.n_mesh_tiles == n_tiles
    assert part.rank0_rounds == 0
    assert part.max_mesh_tiles_per_rank == -(-n_tiles // world)
    counts = [rr.lib().rr_host_mesh_tiles_of_rank(C.byref(part), r) for r in range(world)]
    assert sum(counts) == n_tiles and max(counts) == part.max_mesh_tiles_per_rank
    # the culled partition of a view where the scene is small on screen holds fewer tiles per rank: a buffer sized from it
    # cannot hold the whole-frame partition (the sharded launch refuses that pairing)
    if (w, h) == (1920, 1080) and world > 1:
        culled = _capi.MeshPartition()
        sc = rr.camera_orbit(0.01)
        assert rr.lib().rr_host_mesh_partition(b, C.byref(sc), 1, w, h, world, C.byref(culled)) == 0
        assert culled.rect_w > 0 and culled.n_bg_tiles > 0
        assert culled.max_mesh_tiles_per_rank < part.max_mesh_tiles_per_rank
