"""GPU: spectral frames (Renderer.render_spectral, rr_render_spectral[_device]) -- render_samples with an index of refraction and
three channel weights per sample.

The reference is the composition contract: a spectral frame is the weighted fold, p_k = w_k * c_k summed from p_0 in sample order
and divided by S in np.float32, of S shade_rays calls on rr.camera_rays with default_params(ior=ior_k) -- entry points that
test_gpu_shade.py and test_samples_abi.py pin to the CPU oracle.  Float bits, RGBA8 (with and without Reinhard) and TraceRay counts
of every pixel are compared.  With uniform bands the frame is render_samples byte for byte, and one frame is held to the CPU
oracle's own renders at four indices of refraction (spectral_helpers.py)."""
import ctypes as C

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from kernel_oracle_helpers import make_renderer  # noqa: F401  (a fixture)
from scenes import gpu, gpu_scene, load  # noqa: F401  (gpu: a fixture)
from shading_helpers import H as OH
from shading_helpers import OFFP16, STAT_FIELDS, SUB4, config4_scene, env_map, instanced_scene, view_constants
from shading_helpers import W as OW
from spectral_helpers import BANDS4, ORACLE_KW, ORACLE_VIEW, oracle_spectral_frame, uniform_bands, weighted_fold
from test_gpu_samples import check
from test_gpu_stack_rungs import DEEP, assert_rung, chain_scene
from test_gpu_stack_rungs import view as chain_view

pytestmark = pytest.mark.gpu

RR_ERR_INVALID_ARGUMENT, RR_ERR_STATE, RR_ERR_UNSUPPORTED = 1, 5, 7
W, H = 50, 38
GRID64 = np.array([[((i % 8) + 0.5) / 8, ((i // 8) + 0.5) / 8] for i in range(64)], np.float32)


def bands64():
    """64 caller bands that are not the built-in table: iors from 1.2 to 1.515, weights of both signs"""
    t = np.zeros(64, rr.BAND_DTYPE)
    t["ior"] = 1.2 + 0.005 * np.arange(64)
    t["weight"] = np.array([[1.0 + 0.5 * np.sin(0.7 * i + c) for c in range(3)] for i in range(64)], np.float32)
    t["weight"][5] = (-0.5, 0.0, 2.0)
    return t


def spectral_fold(gpu, sc, w, h, offsets, bands, flags=0, **kw):
    """weighted fold of len(offsets) shade_rays calls on rr.camera_rays, call k with ior = bands[k].ior -> (rgb [h, w, 3], counts [h, w])"""
    assert len(offsets) == len(bands)
    cols, total = [], np.zeros(w * h, np.uint32)
    for (ox, oy), b in zip(offsets, bands):
        p = rr.default_params(flags=flags, ior=float(b["ior"]), **kw)
        f, n = gpu.shade_rays(rr.camera_rays(sc, w, h, float(ox), float(oy), p.tmin_primary, p.tmax_primary), p, ray_counts=True)
        cols.append(f[:, :3])
        total += n
    return weighted_fold(cols, [b["weight"] for b in bands]).reshape(h, w, 3), total.reshape(h, w)


def crossed(positions, bands):
    """the tables render_spectral builds by default: sample a * B + b is position a in band b"""
    return np.repeat(np.asarray(positions, np.float32), len(bands), axis=0), np.tile(bands, len(positions))


def check_composition(gpu, sc, w, h, bands, samples, paired, ior=1.3, **kw):
    """render_spectral == the weighted fold over shade_rays, with and without Reinhard; bands / samples / paired as render_spectral takes
    them (bands: an int or a table).  -> the counts"""
    pos = rr.sample_pattern(samples) if isinstance(samples, int) else samples
    tab = rr.spectral_bands(bands, ior, 30.0) if isinstance(bands, int) else bands
    offs, table = (pos, tab) if paired else crossed(pos, tab)
    cnt = None
    for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
        rgb, cnt = spectral_fold(gpu, sc, w, h, offs, table, flags, **kw)
        got = gpu.render_spectral(w, h, sc, bands, samples, rr.default_params(flags=flags, ior=ior, **kw), paired=paired, rgba8=True, ray_counts=True)
        assert got[0].shape == (h, w, 4) and got[1].shape == (h, w, 4) and got[2].shape == (h, w)
        check(got, rgb, cnt, flags != 0)
    return cnt


def monkey_scene(gpu):
    gpu.load_scene(*load("monkey.obj"), env_map())


# ------------------------------------------------------------------------------------------------- 1. uniform bands are render_samples
@pytest.mark.parametrize("scene", ["monkey", "instanced"])
def test_uniform_bands_are_render_samples(gpu, scene):
    if scene == "monkey":
        monkey_scene(gpu)
    else:
        gpu_scene(gpu, *instanced_scene())
    sc, _, _ = view_constants(0.6, 0.5, W, H)
    for samples in (4, 16, OFFP16[:5]):
        n = samples if isinstance(samples, int) else len(samples)
        for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
            for ior in (1.3, 1.45):
                p = rr.default_params(flags=flags, max_refract=8, max_reflect=3, ior=ior)
                want = gpu.render_samples(W, H, sc, samples, p, rgba8=True, ray_counts=True)
                assert (want[2] > n).mean() > 0.02
                for bands in (None, uniform_bands(n, ior)):
                    got = gpu.render_spectral(W, H, sc, bands, samples, p, paired=True, rgba8=True, ray_counts=True)
                    for a, b in zip(got, want):
                        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # one band crossed with the positions is a uniform table too
    p = rr.default_params(max_refract=8)
    assert gpu.render_spectral(W, H, sc, 1, 4, p).tobytes() == gpu.render_samples(W, H, sc, 4, p).tobytes()


# ------------------------------------------------------------------------------------------------- 2. composition
def test_composition_monkey_with_caller_tables(gpu):
    monkey_scene(gpu)
    w, h = 203, 117                                             # not multiples of 8: partial blocks on two edges
    sc, _, _ = view_constants(0.8, 0.3, w, h)
    assert (BANDS4["weight"] < 0).any() and (BANDS4["weight"] == 0).any() and len(set(BANDS4["ior"])) == 4
    cnt = check_composition(gpu, sc, w, h, BANDS4, OFFP16[:4], True, max_refract=8)
    assert (cnt > 4).mean() > 0.1


@pytest.mark.parametrize("name", ["cube.obj", "shell.obj"])
def test_composition_builtin_sixteen(gpu, name):
    gpu.load_scene(*load(name), env_map())
    sc, _, _ = view_constants(1.3, 0.35, W, H)
    cnt = check_composition(gpu, sc, W, H, 16, 16, True, max_refract=5, max_reflect=2)
    assert (cnt > 16).mean() > 0.02


@pytest.mark.parametrize("scene", [instanced_scene, config4_scene])
def test_composition_two_level_crossed(gpu, scene):
    gpu_scene(gpu, *scene())
    sc = rr.camera_orbit(0.6)
    for (mr, ml), ior, samples in (((8, 2), 1.3, 4), ((5, 3), 1.5, OFFP16[:3])):        # the built-in four positions; three of the caller's
        cnt = check_composition(gpu, sc, W, H, 4, samples, False, ior=ior, max_refract=mr, max_reflect=ml)
        assert (cnt > 4 * len(rr.sample_pattern(samples) if isinstance(samples, int) else samples)).mean() > 0.02


def test_composition_sixty_four_samples_both_tables(gpu):
    """both kernel-argument tables full: sample 63's offset and band are the last words of each"""
    monkey_scene(gpu)
    w, h = 24, 17
    sc, _, _ = view_constants(1.3, 0.35, w, h)
    tab = bands64()
    cnt = check_composition(gpu, sc, w, h, tab, GRID64, True, max_refract=8, max_reflect=3)
    assert (cnt > 64).mean() > 0.1
    # the last band counts: another ior or another blue weight in row 63, another frame
    p = rr.default_params(max_refract=8, max_reflect=3)
    base = gpu.render_spectral(w, h, sc, tab, GRID64, p, paired=True)
    other = tab.copy()
    other["ior"][63] = 1.7
    moved = gpu.render_spectral(w, h, sc, other, GRID64, p, paired=True)
    assert moved.tobytes() != base.tobytes()
    other = tab.copy()
    other["weight"][63, 2] += 0.5
    blue = gpu.render_spectral(w, h, sc, other, GRID64, p, paired=True)
    assert blue[..., 2].tobytes() != base[..., 2].tobytes() and blue[..., :2].tobytes() == base[..., :2].tobytes()


@pytest.mark.parametrize("need,two_level,env", [(39, False, {}), (30, True, {}), (31, True, {"RR_DEBUG_TLAS32": 1}), (64, False, {})])
def test_composition_on_the_ladders_rungs(make_renderer, need, two_level, env):
    """the chains of test_gpu_stack_rungs.py at the depth a rung is built for: 16-bit entries (39 for one instance, 30 for a two-level
    scene), the 31-entry and the 64-entry 32-bit stacks, with two bands"""
    r = make_renderer("fused", **env)
    sc = chain_scene(need, two_level)
    sc.load_gpu(r)
    w, h = 24, 16
    cam = chain_view(DEEP, w, h)
    assert_rung(r, sc, need, rr.camera_rays(cam, w, h, *OFFP16[0]))
    two = np.array([(1.25, (1.5, 0.5, 1.0)), (1.4, (0.5, 1.5, 1.0))], rr.BAND_DTYPE)
    cnt = check_composition(r, cam, w, h, two, OFFP16[:2], True, max_refract=5)
    assert (cnt > 2).sum() >= 10                                # (the two-level chains are scaled to 0.6: a sixteenth of this frame)


# ------------------------------------------------------------------------------------------------- 3. the oracle frame
def test_the_oracle_frame(gpu):
    """the CPU oracle's four renders at four indices of refraction, folded with BANDS4's weights (test_spectral_cpu.py), bit for bit"""
    monkey_scene(gpu)
    rgb, cnt, _ = oracle_spectral_frame()
    sc, _, _ = view_constants(*ORACLE_VIEW)
    offs = np.array([[(2 * i + 1) / 8.0, (2 * j + 1) / 8.0] for i, j in SUB4], np.float32)
    assert rr.sample_pattern(4).tobytes() == offs.tobytes()
    for samples in (4, offs):
        for flags in (0, rr.DISPATCH_TONEMAP_REINHARD):
            got = gpu.render_spectral(OW, OH, sc, BANDS4, samples, rr.default_params(flags=flags, **ORACLE_KW), paired=True, rgba8=True, ray_counts=True)
            check(got, rgb, cnt, flags != 0)


# ------------------------------------------------------------------------------------------------- 4. culling
def test_culling_changes_no_byte(gpu):
    """the reference's wide view: the blocks beside the mesh are one Miss per sample, weighted and resolved like any other"""
    monkey_scene(gpu)
    w, h = 203, 117
    sc, _, _ = view_constants(0.01, rr.FOV_Y, w, h)
    S = 8
    tab = rr.spectral_bands(S, 1.3, 30.0)
    tab["weight"][2] = (-0.75, 0.0, 1.5)
    culled = gpu.render_spectral(w, h, sc, tab, S, rr.default_params(max_refract=8), paired=True, rgba8=True, ray_counts=True)
    traced = gpu.render_spectral(w, h, sc, tab, S, rr.default_params(max_refract=8, flags=rr.DISPATCH_DEBUG_NO_CULL), paired=True, rgba8=True,
                                 ray_counts=True)
    for a, b in zip(culled, traced):
        assert a.tobytes() == b.tobytes()
    v, i = load("monkey.obj")
    P = v["position"][i]
    b = (C.c_float * 6)(*np.concatenate([P.min(axis=0), P.max(axis=0)]).astype(np.float32))
    r = (C.c_uint32 * 4)()
    assert rr.lib().rr_host_screen_rect(b, C.byref(sc), 1, w, h, r) == 0
    x0, y0 = (np.arange(w) // 8) * 8, (np.arange(h) // 8) * 8
    inside = ((y0 + 8 > r[1]) & (y0 < r[3]))[:, None] & ((x0 + 8 > r[0]) & (x0 < r[2]))[None, :]
    cnt = culled[2]
    print("rectangle %s: %d of %d pixels lie in culled blocks" % (tuple(r), int((~inside).sum()), w * h))
    assert (~inside).sum() > 1000 and np.all(cnt[~inside] == S) and (cnt[inside] > S).any()
    rgb, want_n = spectral_fold(gpu, sc, w, h, rr.sample_pattern(S), tab, max_refract=8)
    check(culled, rgb, want_n, False)


# ------------------------------------------------------------------------------------------------- 5. not vacuous
def test_dispersion_changes_the_frame_and_fringes_a_grey_world(gpu):
    v, i = load("monkey.obj")
    gpu.load_scene(v, i, env_map())
    sc, _, _ = view_constants(0.8, 0.3, W, H)
    p = rr.default_params(max_refract=8)
    tab = rr.spectral_bands(8, 1.3, 30.0)
    plain, plain_n = gpu.render_spectral(W, H, sc, None, 8, p, ray_counts=True)
    disp, disp_n = gpu.render_spectral(W, H, sc, tab, 8, p, paired=True, ray_counts=True)
    differ = int((plain[..., :3].view(np.uint32) != disp[..., :3].view(np.uint32)).any(axis=-1).sum())
    recount = int((plain_n != disp_n).sum())
    print("%d of %d pixels differ between 8 bands of Abbe number 30 and none; %d have another ray count; %d hit the mesh" %
          (differ, W * H, recount, int((plain_n > 8).sum())))
    assert differ >= 300
    assert recount >= 20
    # A grey environment, every sample through the pixel centre: without dispersion the eight samples of a pixel are one colour c
    # with R = G = B, and a channel is (sum of w_k * c) / 8 with weights that sum to 8 -- the channels differ by the roundings of
    # eight products and seven sums in either channel, under 32 * 2^-24 of the largest value.  Whatever colour beyond that the frame shows,
    # dispersion put it there.
    env = env_map()
    grey = np.repeat(env.mean(axis=-1, keepdims=True), env.shape[-1], axis=-1).astype(np.float32)
    assert np.all(grey[..., 0] == grey[..., 1]) and np.all(grey[..., 1] == grey[..., 2]) and len(np.unique(grey[..., 0])) > 100
    gpu.load_scene(v, i, grey)
    centre = np.array([[0.5, 0.5]], np.float32)

    def spread(frame):
        return frame[..., :3].max(axis=-1) - frame[..., :3].min(axis=-1)
    flat = gpu.render_spectral(W, H, sc, None, 8, p)
    assert np.all(flat[..., 0] == flat[..., 1]) and np.all(flat[..., 1] == flat[..., 2])
    still = gpu.render_spectral(W, H, sc, rr.spectral_bands(8, 1.3, float("inf")), centre, p)
    fringed = gpu.render_spectral(W, H, sc, tab, centre, p)
    coloured = (fringed[..., 0] != fringed[..., 1]) | (fringed[..., 1] != fringed[..., 2])
    rounding = 32 * 2.0 ** -24 * float(still[..., :3].max())
    print("grey environment: channel spread %.3g without dispersion (rounding allows %.3g), %.4f with it on %d pixels above the rounding" %
          (float(spread(still).max()), rounding, float(spread(fringed).max()), int((spread(fringed) > rounding).sum())))
    assert coloured.any()
    assert float(spread(still).max()) <= rounding and float(spread(fringed).max()) > 100 * rounding


# ------------------------------------------------------------------------------------------------- 6. device variant, context
def test_device_variant_equals_host_variant_on_the_renderers_stream(gpu):
    import torch
    monkey_scene(gpu)
    w, h = 75, 41
    sc, _, _ = view_constants(0.4, 0.3, w, h)
    p = rr.default_params(max_refract=8, flags=rr.DISPATCH_TONEMAP_REINHARD)
    kw = dict(bands=BANDS4, samples=OFFP16[:4], params=p, paired=True)
    host = gpu.render_spectral(w, h, sc, rgba8=True, ray_counts=True, **kw)
    assert (host[2] > 4).mean() > 0.1
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        df, du, dc = gpu.render_spectral(w, h, sc, rgba8=True, ray_counts=True, device=True, **kw)
        only = gpu.render_spectral(w, h, sc, device=True, **kw)
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


def test_a_spectral_frame_leaves_the_context_alone(gpu):
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
    gpu.render_spectral(90, 50, sc2, 4, 2, rr.default_params(max_refract=3, max_reflect=3), rgba8=True, ray_counts=True)
    gpu.render_spectral(90, 50, sc2, 2, 2, rr.default_params(flags=rr.DISPATCH_TONEMAP_REINHARD), rgba8=True, ray_counts=True, device=True)
    gpu.wait()
    torch.cuda.synchronize()
    rgba2, f32_2 = gpu.read_frame(want_float=True)
    assert rgba2.tobytes() == rgba.tobytes() and f32_2.tobytes() == f32.tobytes()
    st2 = gpu.stats()
    assert {k: getattr(st2, k) for k in STAT_FIELDS} == before


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_bad_arguments_are_refused(gpu):
    import torch
    monkey_scene(gpu)
    sc, _, _ = view_constants(1.3, 0.35, 8, 8)
    L = rr.lib()
    P = C.c_void_p
    f = np.zeros((8, 8, 4), np.float32)
    n8 = np.zeros((8, 8), np.uint32)
    ok = rr.spectral_bands(4)
    nan, inf = float("nan"), float("inf")

    def host(bands=ok, n=4, offsets=None, constants=sc, params=None, f32=f, cnt=None):
        o = np.ascontiguousarray(offsets, np.float32) if offsets is not None else None
        b = np.ascontiguousarray(bands, rr.BAND_DTYPE) if bands is not None else None
        return L.rr_render_spectral(gpu._h, 8, 8, C.byref(constants) if constants is not None else None, C.byref(params) if params is not None else None,
                                    o.ctypes.data if o is not None else None, b.ctypes.data if b is not None else None, n,
                                    f32.ctypes.data if f32 is not None else None, None, cnt.ctypes.data if cnt is not None else None)
    assert host() == 0
    assert f.tobytes() == gpu.render_spectral(8, 8, sc, ok, 4, paired=True).tobytes()   # NULL params: the defaults
    assert host(bands=None) == 0
    assert f.tobytes() == gpu.render_samples(8, 8, sc, 4).tobytes()
    assert host(constants=None) == RR_ERR_INVALID_ARGUMENT
    big = rr.spectral_bands(64)
    for n in (0, 65):
        assert host(n=n) == RR_ERR_INVALID_ARGUMENT, n
        assert host(n=n, bands=None) == RR_ERR_INVALID_ARGUMENT, n
        assert host(n=n, offsets=np.full((65, 2), 0.5, np.float32), bands=np.concatenate([big, big[:1]])) == RR_ERR_INVALID_ARGUMENT, n
    assert host(n=3, bands=ok[:3]) == RR_ERR_INVALID_ARGUMENT                           # NULL offsets: a built-in pattern
    assert host(n=3, bands=ok[:3], offsets=np.full((3, 2), 0.5, np.float32)) == 0
    for bad in (0.0, -1.3, nan, inf, -inf):
        t = ok.copy()
        t["ior"][3] = bad
        assert host(bands=t) == RR_ERR_INVALID_ARGUMENT, bad
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                gpu.render_spectral(8, 8, sc, t, 4, paired=True, device=device)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, bad
    for bad in (nan, inf, -inf):
        for ch in range(3):
            t = ok.copy()
            t["weight"][3, ch] = bad
            assert host(bands=t) == RR_ERR_INVALID_ARGUMENT, (bad, ch)
            with pytest.raises(rr.RRError) as e:
                gpu.render_spectral(8, 8, sc, t, 4, paired=True)
            assert e.value.status == RR_ERR_INVALID_ARGUMENT, (bad, ch)
    t = ok.copy()
    t["weight"][3] = (-2.0, 0.0, -0.0)                                                  # negative weights are allowed
    assert host(bands=t) == 0
    assert host(bands=ok, offsets=np.array([[0.5, 0.5]] * 3 + [[0.5, 1.5]], np.float32)) == RR_ERR_INVALID_ARGUMENT
    assert host(f32=None) == RR_ERR_INVALID_ARGUMENT                                    # no outputs
    assert host(f32=None, cnt=n8) == RR_ERR_INVALID_ARGUMENT                            # counts alone are no colour
    assert host(params=rr.default_params(max_reflect=9)) == RR_ERR_UNSUPPORTED
    assert host(params=rr.default_params(ior=0.0)) == RR_ERR_INVALID_ARGUMENT           # validated although the bands replace it
    # the Python wrapper's own refusals
    with pytest.raises(ValueError):
        gpu.render_spectral(8, 8, sc, 8, 16)                                            # 128 samples
    with pytest.raises(ValueError):
        gpu.render_spectral(8, 8, sc, ok, 8, paired=True)                               # 4 bands, 8 positions
    # the device variant's pointers
    dev = "cuda:%d" % gpu.device
    out = torch.zeros(64 * 4 + 4, dtype=torch.float32, device=dev)
    aux = torch.zeros(64 + 4, dtype=torch.int32, device=dev)
    a = (gpu._h, 8, 8, C.byref(sc), None, None, ok.ctypes.data, 4)
    assert out.data_ptr() % 16 == 0 and aux.data_ptr() % 4 == 0
    assert L.rr_render_spectral_device(*a, P(out.data_ptr()), P(aux.data_ptr()), P(aux.data_ptr())) == 0
    assert L.rr_render_spectral_device(*a, P(out.data_ptr() + 4), None, None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_spectral_device(*a, P(out.data_ptr()), P(aux.data_ptr() + 2), None) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_spectral_device(*a, P(out.data_ptr()), None, P(aux.data_ptr() + 1)) == RR_ERR_INVALID_ARGUMENT
    assert L.rr_render_spectral_device(*a, None, None, P(aux.data_ptr())) == RR_ERR_INVALID_ARGUMENT
    gpu.wait()


def test_spectral_frames_need_a_built_scene(gpu):
    fresh = rr.Renderer(gpu.device)
    try:
        sc, _, _ = view_constants(0.4, 0.3, 8, 8)
        for device in (False, True):
            with pytest.raises(rr.RRError) as e:
                fresh.render_spectral(8, 8, sc, 4, 1, device=device)
            assert e.value.status == RR_ERR_STATE
        m = load("cube.obj")
        mid = fresh.upload_mesh(*m)
        fresh.build_blas(mid)
        with pytest.raises(rr.RRError) as e:
            fresh.render_spectral(8, 8, sc, 4, 1)                                      # BLAS built, no TLAS yet
        assert e.value.status == RR_ERR_STATE
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------- 8. the demo
def test_rrdemo_dispersion_writes_render_spectral_frames(gpu, tmp_path):
    """rrdemo --spp 2 --dispersion 4:30: the C++ host's drawFrameSpectral end to end, its PPM against render_spectral's RGBA8 store"""
    import os
    import subprocess

    import oracle as O
    exe = os.path.join(os.path.dirname(rr.lib_path()), "rrdemo")
    assert os.path.exists(exe), "rrdemo was not built"
    hdr = str(tmp_path / "env.hdr")
    rr.write_hdr(hdr, env_map())
    args = [exe, "--mesh", O.asset("cube.obj"), "--env", hdr, "--size", "64x48", "--frames", "1", "--out", str(tmp_path / "s_%03d.ppm")]
    out = subprocess.run(args + ["--spp", "2", "--dispersion", "4:30"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "2 samples per pixel x 4 bands of Abbe number 30" in out.stdout, out.stderr + out.stdout
    raw = open(tmp_path / "s_000.ppm", "rb").read()
    head = b"P6\n64 48\n255\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.uint8).reshape(48, 64, 3)
    env_rt, _ = rr.load_texture(hdr, 3)
    gpu.load_scene(*load("cube.obj"), env_rt)
    _, u8 = gpu.render_spectral(64, 48, rr.camera_orbit(0.01), 4, 2, abbe=30.0, rgba8=True)
    assert np.array_equal(img, u8[..., :3])
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50
    for bad in (["--dispersion", "0"], ["--dispersion", "65"], ["--dispersion", "4:0"], ["--dispersion", "4:-3"], ["--dispersion", "4:"],
                ["--dispersion", "x"], ["--spp", "16", "--dispersion", "8"], ["--spp", "4", "--adaptive", "2:0.1", "--dispersion", "4"],
                ["--spp", "4", "--lens", "0.2:5", "--dispersion", "4"]):
        assert subprocess.run(args + bad, capture_output=True, text=True, timeout=120).returncode == 2, bad
