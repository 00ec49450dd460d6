"""GPU: thin-lens frames (Renderer.render_lens, rr_render_lens[_device]) -- render_samples with every sample's primary ray starting
on a lens of finite aperture and aimed at its pixel's point of the focal plane.

The reference is the composition contract: a lens frame is the fold, by render_samples' resolve rule, of S shade_rays calls on the
host-generated rays rr.lens_rays -- entry points that test_gpu_shade.py and test_samples_abi.py pin to the CPU oracle.  Float bits,
RGBA8 (with and without Reinhard) and TraceRay counts of every pixel are compared.  With radius 0 the frame is render_samples byte
for byte."""
import ctypes as C

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from kernel_oracle_helpers import make_renderer  # noqa: F401  (a fixture)
from scenes import gpu, gpu_scene, load  # noqa: F401  (gpu: a fixture)
from shading_helpers import OFFP16, STAT_FIELDS, config4_scene, env_map, fold, instanced_scene, view_constants
from test_gpu_samples import check
from test_gpu_stack_rungs import DEEP, assert_rung, chain_scene
from test_gpu_stack_rungs import view as chain_view

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE, RR_ERR_UNSUPPORTED = 1, 5, 7
W, H = 50, 38
GRID64 = np.array([[((i % 8) + 0.5) / 8, ((i // 8) + 0.5) / 8] for i in range(64)], np.float32)
# 64 lens offsets that are not the built-in spiral: a grid over the square round the disk, its corners included
LENS64 = np.array([[(i % 8) / 3.5 - 1.0, (i // 8) / 3.5 - 1.0] for i in range(64)], np.float32)
LENS4 = np.array([[1.0, 0.0], [-0.5, 0.75], [0.0, -1.0], [-1.0, 1.0]], np.float32)


def lens_fold(gpu, sc, w, h, offsets, lens_offsets, lens, p):
    """fold of len(offsets) shade_rays calls on rr.lens_rays -> (rgb [h, w, 3], counts [h, w])"""
    cols, total = [], np.zeros(w * h, np.uint32)
    for (ox, oy), (lx, ly) in zip(offsets, lens_offsets):
        rays = rr.lens_rays(sc, w, h, float(ox), float(oy), float(lx), float(ly), lens, p.tmin_primary, p.tmax_primary)
        f, n = gpu.shade_rays(rays, p, ray_counts=True)
        cols.append(f[:, :3])
        total += n
    return fold(cols).reshape(h, w, 3), total.reshape(h, w)


def check_composition(gpu, sc, w, h, lens, samples, lens_samples, **kw):
    """render_lens == the fold over rr.lens_rays, with and without Reinhard; samples / lens_samples as render_lens takes them.
    -> the counts"""
    offs = rr.sample_pattern(samples) if isinstance(samples, int) else samples
    loffs = rr.lens_pattern(len(offs)) if lens_samples is None else lens_samples
    cnt = None
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        p = rr.default_params(flags=flags, **kw)
        rgb, cnt = lens_fold(gpu, sc, w, h, offs, loffs, lens, p)
        got = gpu.render_lens(w, h, sc, lens, samples, lens_samples, p, rgba8=True, ray_counts=True)
        assert got[0].shape == (h, w, 4) and got[1].shape == (h, w, 4) and got[2].shape == (h, w)
        check(got, rgb, cnt, flags != 0)
    return cnt


def monkey_scene(gpu):
    gpu.load_scene(*load("monkey.obj"), env_map())


# ------------------------------------------------------------------------------------------------- 1. radius 0 is render_samples
@pytest.mark.parametrize("scene", ["monkey", "instanced"])
def test_radius_zero_is_render_samples(gpu, scene):
    if scene == "monkey":
        monkey_scene(gpu)
    else:
        gpu_scene(gpu, *instanced_scene())
    sc, _, _ = view_constants(0.6, 0.5, W, H)
    for samples, lens_samples in ((4, None), (16, None), (OFFP16[:5], LENS64[:5])):
        for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
            p = rr.default_params(flags=flags, max_refract=8, max_reflect=3)
            want = gpu.render_samples(W, H, sc, samples, p, rgba8=True, ray_counts=True)
            assert (want[2] > len(rr.sample_pattern(samples) if isinstance(samples, int) else samples)).mean() > 0.02
            for focus in (0.5, 5.0):
                got = gpu.render_lens(W, H, sc, rr.Lens(0.0, focus), samples, lens_samples, p, rgba8=True, ray_counts=True)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------- 2. composition
def test_composition_monkey_with_caller_offsets(gpu):
    monkey_scene(gpu)
    w, h = 203, 117                                             # not multiples of 8: partial blocks on two edges
    sc, _, _ = view_constants(0.8, 0.3, w, h)
    cnt = check_composition(gpu, sc, w, h, rr.Lens(0.35, 4.2), OFFP16[:4], LENS4, max_refract=8)
    assert (cnt > 4).mean() > 0.1


@pytest.mark.parametrize("name", ["cube.obj", "shell.obj"])
def test_composition_builtin_sixteen(gpu, name):
    gpu.load_scene(*load(name), env_map())
    sc, _, _ = view_constants(1.3, 0.35, W, H)
    cnt = check_composition(gpu, sc, W, H, rr.Lens(0.25, 5.0), 16, None, max_refract=5, max_reflect=2)
    assert (cnt > 16).mean() > 0.02


@pytest.mark.parametrize("scene", [instanced_scene, config4_scene])
def test_composition_two_level(gpu, scene):
    gpu_scene(gpu, *scene())
    sc = rr.camera_orbit(0.6)
    for (mr, ml), lens in (((8, 2), rr.Lens(0.3, 5.0)), ((5, 3), rr.Lens(0.8, 3.0))):
        cnt = check_composition(gpu, sc, W, H, lens, 4, None, max_refract=mr, max_reflect=ml)
        assert (cnt > 4).mean() > 0.02


def test_composition_sixty_four_samples_both_tables(gpu):
    """both kernel-argument tables full: sample 63's offsets are the last words of each"""
    monkey_scene(gpu)
    w, h = 24, 17
    sc, _, _ = view_constants(1.3, 0.35, w, h)
    cnt = check_composition(gpu, sc, w, h, rr.Lens(0.3, 5.0), GRID64, LENS64, max_refract=8, max_reflect=3)
    assert (cnt > 64).mean() > 0.1
    # the last sample counts: another last row in either table, another frame
    p = rr.default_params(max_refract=8, max_reflect=3)
    base = gpu.render_lens(w, h, sc, rr.Lens(0.3, 5.0), GRID64, LENS64, p)
    for which in (0, 1):
        o, lo = GRID64.copy(), LENS64.copy()
        (o, lo)[which][63] = (0.03, 0.97) if which == 0 else (-1.0, 0.1)
        assert gpu.render_lens(w, h, sc, rr.Lens(0.3, 5.0), o, lo, p).tobytes() != base.tobytes()


@pytest.mark.parametrize("need,two_level,env", [(39, False, {}), (30, True, {}), (31, True, {"RR_DEBUG_TLAS32": 1}), (64, False, {})])
def test_composition_on_the_ladders_rungs(make_renderer, need, two_level, env):
    """the chains of test_gpu_stack_rungs.py at the depth a rung is built for: 16-bit entries (39 for one instance, 30 for a two-level
    scene), the 31-entry and the 64-entry 32-bit stacks, the deep view's lens rays filling the stack to its last entry"""
    r = make_renderer("fused", **env)
    sc = chain_scene(need, two_level)
    sc.load_gpu(r)
    w, h = 24, 16
    cam = chain_view(DEEP, w, h)
    lens = rr.Lens(0.1, 5.0)
    loffs = np.array([[0.0, 0.0], [1.0, -0.5]], np.float32)            # sample 0 through the lens centre: the deep direction
    assert_rung(r, sc, need, rr.lens_rays(cam, w, h, *OFFP16[0], *loffs[0], lens))
    cnt = check_composition(r, cam, w, h, lens, OFFP16[:2], loffs, max_refract=5)
    assert (cnt > 2).sum() >= 10                                # (the two-level chains are scaled to 0.6: a sixteenth of this frame)


# ------------------------------------------------------------------------------------------------- 3. culling
CULL_VIEW, CULL_LENS, CULL_S = (0.01, rr.FOV_Y), (1.2, 2.5), 16


def test_the_lens_rectangle_is_wider_than_the_pinholes_and_needed(gpu):
    """the reference's wide view through a lens of 1.2 units focused halfway to the mesh: the lens' edge sees the mesh a good twenty
    pixels beside where the pinhole does, in blocks the pinhole's rectangle leaves out -- asserted on the counts -- and culling by the
    lens rectangle changes no byte"""
    v, i = load("monkey.obj")
    gpu.load_scene(v, i, env_map())
    w, h = 203, 117
    sc, _, _ = view_constants(*CULL_VIEW, w, h)
    lens = rr.Lens(*CULL_LENS)
    S = CULL_S
    P = v["position"][i]
    bounds = np.concatenate([P.min(axis=0), P.max(axis=0)])
    pin = rr.lens_screen_rect(bounds, sc, rr.Lens(0.0, lens.focus_distance), w, h)
    wide = rr.lens_screen_rect(bounds, sc, lens, w, h)
    assert wide != pin and wide[0] <= pin[0] and wide[2] >= pin[2] and wide != (0, 0, 208, 120), (pin, wide)
    p = rr.default_params(max_refract=8)
    culled = gpu.render_lens(w, h, sc, lens, S, None, p, rgba8=True, ray_counts=True)
    traced = gpu.render_lens(w, h, sc, lens, S, None, rr.default_params(max_refract=8, flags=rr.DISPATCH_DEBUG_NO_CULL), rgba8=True, ray_counts=True)
    for a, b in zip(culled, traced):
        assert a.tobytes() == b.tobytes()
    x0, y0 = (np.arange(w) // 8) * 8, (np.arange(h) // 8) * 8
    in_pin = ((y0 + 8 > pin[1]) & (y0 < pin[3]))[:, None] & ((x0 + 8 > pin[0]) & (x0 < pin[2]))[None, :]
    in_wide = ((y0 + 8 > wide[1]) & (y0 < wide[3]))[:, None] & ((x0 + 8 > wide[0]) & (x0 < wide[2]))[None, :]
    cnt = culled[2]
    beside = int(((cnt > S) & ~in_pin).sum())
    print("pinhole rectangle %s, lens rectangle %s: %d pixels outside the pinhole's blocks hit the mesh" % (pin, wide, beside))
    assert beside > 0                                           # the pinhole's rectangle would have shaded them as Misses
    assert np.all(cnt[~in_wide] == S) and (~in_wide).any()      # and some blocks are still culled
    rgb, want_n = lens_fold(gpu, sc, w, h, rr.sample_pattern(S), rr.lens_pattern(S), lens, p)
    check(culled, rgb, want_n, False)


# ------------------------------------------------------------------------------------------------- 4. not vacuous
def test_an_open_aperture_changes_the_frame(gpu):
    monkey_scene(gpu)
    sc, _, _ = view_constants(0.8, 0.3, W, H)
    p = rr.default_params(max_refract=8)
    sharp = gpu.render_lens(W, H, sc, rr.Lens(0.0, 5.0), 16, None, p)
    soft = gpu.render_lens(W, H, sc, rr.Lens(0.3, 5.0), 16, None, p)
    differ = int((sharp[..., :3].view(np.uint32) != soft[..., :3].view(np.uint32)).any(axis=-1).sum())
    print("%d of %d pixels differ between radius 0 and radius 0.3" % (differ, W * H))
    assert differ >= 100
    # and so does the focus distance and the lens pattern
    assert gpu.render_lens(W, H, sc, rr.Lens(0.3, 3.0), 16, None, p).tobytes() != soft.tobytes()
    assert gpu.render_lens(W, H, sc, rr.Lens(0.3, 5.0), 16, -rr.lens_pattern(16), p).tobytes() != soft.tobytes()


# ------------------------------------------------------------------------------------------------- 5. device variant, context
def test_device_variant_equals_host_variant_on_the_renderers_stream(gpu):
    import torch
    monkey_scene(gpu)
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    lens = rr.Lens(0.25, 4.5)
    p = rr.default_params(max_refract=8, flags=rr.DISPATCH_TONEMAP_REINHARD)
    host = gpu.render_lens(w, h, sc, lens, OFFP16[:4], LENS4, p, rgba8=True, ray_counts=True)
    assert (host[2] > 4).mean() > 0.1
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_lens(w, h, sc, lens, OFFP16[:4], LENS4, p, rgba8=True, ray_counts=True, device=True)
        only = gpu.render_lens(w, h, sc, lens, OFFP16[:4], LENS4, p, device=True)
        total = df.sum()                                        # queued behind the frame on the same stream
        torch.cuda.current_stream().synchronize()
        assert df.dtype == torch.float32 and du.dtype == torch.uint8 and dc.dtype == torch.int32
        assert tuple(df.shape) == (h, w, 4) and tuple(du.shape) == (h, w, 4) and tuple(dc.shape) == (h, w) and df.device.index == gpu.device
        assert df.cpu().numpy().tobytes() == host[0].tobytes() and du.cpu().numpy().tobytes() == host[1].tobytes()
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), host[2])
        assert only.cpu().numpy().tobytes() == host[0].tobytes()
        assert np.isfinite(float(total))
    finally:
        gpu.reset_stream()


def test_a_lens_frame_leaves_the_context_alone(gpu):
    import torch
    monkey_scene(gpu)
    w, h = 160, 120
    sc, _, _ = view_constants(0.3, 0.4, w, h)
    gpu.set_tile_partition(0, 1)
    gpu.set_camera(sc)
    gpu.dispatch_rays(w, h, rr.default_params(flags=rr.DISPATCH_FLOAT_OUTPUT | rr.DISPATCH_COLLECT_STATS, max_refract=8))
    rgba, f32 = (a.copy() for a in gpu.read_frame(want_float=True))
    st = gpu.stats()
    before = {k: getattr(st, k) for k in STAT_FIELDS}
    assert before["rays"] > w * h
    sc2, _, _ = view_constants(2.0, 0.2, 90, 50)
    gpu.render_lens(90, 50, sc2, rr.Lens(0.2, 5.0), 4, None, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.render_lens(90, 50, sc2, rr.Lens(0.2, 5.0), 2, None, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True,
                    device=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_bad_arguments_are_refused(gpu):
    import torch
    monkey_scene(gpu)
    sc, _, _ = view_constants(1.3, 0.35, 8, 8)
    L = rr.lib()
    P = C.c_void_p
    f = np.zeros((8, 8, 4), np.float32)
    n8 = np.zeros((8, 8), np.uint32)
    ok = rr.Lens(0.2, 5.0)
    nan, inf = float("nan"), float("inf")

    def host(lens=ok, n=4, offsets=None, lens_offsets=None, constants=sc, params=None, f32=f, cnt=None):
        o = np.ascontiguousarray(offsets, np.float32) if offsets is not None else None
        lo = np.ascontiguousarray(lens_offsets, np.float32) if lens_offsets is not None else None
        return L.rr_render_lens(gpu._h, 8, 8, C.byref(constants), C.byref(params) if params is not None else None,
                                o.ctypes.data if o is not None else None, lo.ctypes.data if lo is not None else None, n,
                                C.byref(lens) if lens is not None else None, f32.ctypes.data if f32 is not None else None, None,
                                cnt.ctypes.data if cnt is not None else None)
    assert host() == 0
    assert f.tobytes() == gpu.render_lens(8, 8, sc, ok, 4).tobytes()                    # NULL params: the defaults
    assert host(lens=None) == RR_ERR_INVALID_ARGUMENT
    for radius, focus in ((-0.1, 5.0), (nan, 5.0), (inf, 5.0), (-inf, 5.0), (0.2, 0.0), (0.2, -2.0), (0.2, nan), (0.2, inf), (0.0, 0.0), (0.0, nan)):
        assert host(lens=rr.Lens(radius, focus)) == RR_ERR_INVALID_ARGUMENT, (radius, focus)
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                gpu.render_lens(8, 8, sc, rr.Lens(radius, focus), 4, device=device)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, (radius, focus)
    for bad in (1.5, -1.5, nan, inf):
        for axis in (0, 1):
            lo = np.zeros((4, 2), np.float32)
            lo[3, axis] = bad
            assert host(lens_offsets=lo) == RR_ERR_INVALID_ARGUMENT, bad
            with pytest.raises(rr.RRError) as e:
                gpu.render_lens(8, 8, sc, ok, 4, lo)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, bad
    assert host(lens_offsets=np.array([[1.0, -1.0]] * 4, np.float32)) == 0              # the closed interval
    for n in (0, 65):
        assert host(n=n) == RR_ERR_INVALID_ARGUMENT, n
        assert host(n=n, offsets=np.full((65, 2), 0.5, np.float32), lens_offsets=np.zeros((65, 2), np.float32)) == RR_ERR_INVALID_ARGUMENT, n
    assert host(n=3) == RR_ERR_INVALID_ARGUMENT                                         # NULL offsets: a built-in pattern
    assert host(n=3, offsets=np.full((3, 2), 0.5, np.float32)) == 0                     # (NULL lens offsets take any n)
    for col, with_pinhole in ((3, True), (0, False), (1, False)):
        bad = rr.scene_constants(np.array(sc.proj_inv, np.float32), np.array(sc.camera_loc, np.float32))
        for row in range(3):
            bad.proj_inv[4 * row + col] = 0.0
        assert host(constants=bad) == RR_ERR_INVALID_ARGUMENT, col
        assert host(constants=bad, lens=rr.Lens(0.0, 5.0)) == (RR_ERR_INVALID_ARGUMENT if with_pinhole else 0), col
    assert host(f32=None) == RR_ERR_INVALID_ARGUMENT                                    # no outputs
    assert host(f32=None, cnt=n8) == RR_ERR_INVALID_ARGUMENT                            # counts alone are no colour
    assert host(params=rr.default_params(max_reflect=9)) == RR_ERR_UNSUPPORTED
    assert host(params=rr.default_params(ior=0.0)) == RR_ERR_INVALID_ARGUMENT
    # the device variant's pointers
    dev = "cuda:%d" % gpu.device
    out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
    aux = torch.zeros(64 + 4, dtype=torch.int32, device=dev)
    a = (gpu._h, 8, 8, C.byref(sc), None, None, None, 4, C.byref(ok))
    assert out.data_ptr() % 16 == 0 and aux.data_ptr() % 4 == 0
    assert L.rr_render_lens_device(*a, P(out.data_ptr()), P(aux.data_ptr()), P(aux.data_ptr())) == 0
    assert L.rr_render_lens_device(*a, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lens_device(*a, P(out.data_ptr()), P(aux.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lens_device(*a, P(out.data_ptr()), None, P(aux.data_ptr() + 1)) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_lens_device(*a, None, None, P(aux.data_ptr())) == RR_ERR_INVALID_ARGUMENT
    gpu.wait()


def test_lens_frames_need_a_built_scene(gpu):
    fresh = rr.Renderer(gpu.device)
    try:
        sc, _, _ = view_constants(0.4, 0.3, 8, 8)
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                fresh.render_lens(8, 8, sc, rr.Lens(0.2, 5.0), 4, device=device)
            assert e.value.status == RR_ERR_STATE
        m = load("cube.obj")
        mid = fresh.upload_mesh(*m)
        fresh.build_blas(mid)
        with pytest.raises(rr.RRError) as e:
            fresh.render_lens(8, 8, sc, rr.Lens(0.2, 5.0), 4)                          # BLAS built, no TLAS yet
        assert e.value.status == RR_ERR_STATE
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 7. the demo
def test_rrdemo_lens_writes_render_lens_frames(gpu, tmp_path):
    """rrdemo --spp 4 --lens 0.2:5: the C++ host's drawFrameLens end to end, its PPM against render_lens' RGBA8 store"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("cube.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "l_%03d.ppm")]
    out = subprocess.run(args + ["--spp", "4", "--lens", "0.2:5"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "through a lens of radius 0.2 focused at 5" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "l_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    gpu.load_scene(*load("cube.obj"), env_rt)
    _, u8 = gpu.render_lens(64, 48, rr.camera_orbit(0.01), rr.Lens(0.2, 5.0), 4, None, rgba8=True)
    assert np.array_equal(img, u8[..., :3])
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50
    for bad in (["--lens", "0.2:5"], ["--spp", "4", "--lens", "0.2"], ["--spp", "4", "--lens", "-1:5"], ["--spp", "4", "--lens", "0.2:0"],
                ["--spp", "4", "--adaptive", "2:0.1", "--lens", "0.2:5"]):
        assert subprocess.run(args + bad, capture_output=True, text=True, timeout=120).returncode == 2, bad
