"""CPU: the rule of rr_render_adaptive (include/rrdxr.h, steps 1 to 6) restated in numpy, and the conditions the GPU test
(test_gpu_adaptive.py) relies on, computed from the CPU oracle alone.

adaptive_reference is what the GPU test compares against, so it is itself tested here: on the oracle's colours of monkey.obj -- a
frame 4 times as large per axis whose pixels are the 16 sub-pixel samples of a 52 x 37 base frame (test_gpu_samples.py) -- and on
hand-made colour arrays with NaN, inf, negative and -0 samples, one-pixel-wide frames and a constant image."""
import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from test_gpu_samples import CELL16, ENV, SUB4, H, W, fold, view_constants

F = np.float32
# the 16 sub-pixels of a 4x4 cell, the built-in 4x pattern first: a pattern whose prefix of 4 is a pattern of its own
PERM16 = list(SUB4) + [c for c in CELL16 if c not in SUB4]
OFFP16 = np.array([[(2 * i + 1) / 8.0, (2 * j + 1) / 8.0] for i, j in PERM16], np.float32)
# The views and the threshold of the GPU test.  The threshold is a tenth of a channel's displayed range: the oracle's frames below
# then have both classes and both causes well above the floors the tests assert (the figures are printed).
VIEWS = [(0.01, rr.FOV_Y), (1.3, 0.35)]
THRESHOLD = 0.1


def display(c, tonemap):
    """step 2: what store_pixel shows of a channel value, in [0, 1] (np.fmax / np.fmin return the operand that is a number)"""
    m = np.fmax(np.asarray(c, F), F(0))
    if tonemap:
        with np.errstate(invalid="ignore"):
            m = m / (F(1) + m)                                  # inf / inf = NaN, which fmin turns into 1
    v = np.fmin(m, F(1))
    assert v.dtype == F
    return v


def adaptive_reference(colours, n_base, threshold, tonemap):
    """colours [S, h, w, 3] float32, sample s of every pixel -> (mask [h, w] bool, resolved [h, w, 3], r_own [h, w], r_nb [h, w])"""
    colours = np.asarray(colours)
    assert colours.dtype == F and colours.ndim == 4 and colours.shape[3] == 3
    S, h, w, _ = colours.shape
    assert 1 <= n_base <= S
    t = F(threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        sum_b = colours[0].copy()                               # 1. the fold starts AT c_0
        for s in range(1, n_base):
            sum_b = sum_b + colours[s]
        v = display(colours[:n_base], tonemap)                  # 3. own contrast
        r_own = (np.fmax.reduce(v, axis=0) - np.fmin.reduce(v, axis=0)).max(axis=-1)
        base = sum_b / F(n_base)
        b = display(base, tonemap)                              # 4. neighbour contrast
        r_nb = np.zeros((h, w), F)
        dx = np.abs(b[:, 1:] - b[:, :-1]).max(axis=-1)
        dy = np.abs(b[1:] - b[:-1]).max(axis=-1)
        r_nb[:, 1:] = np.maximum(r_nb[:, 1:], dx)
        r_nb[:, :-1] = np.maximum(r_nb[:, :-1], dx)
        r_nb[1:] = np.maximum(r_nb[1:], dy)
        r_nb[:-1] = np.maximum(r_nb[:-1], dy)
        mask = (r_own > t) | (r_nb > t)                         # 5.
        full = sum_b
        for s in range(n_base, S):                              # 6. a refined pixel continues the same fold
            full = full + colours[s]
        out = np.where(mask[..., None], full / F(S), base)
    assert out.dtype == F and r_own.dtype == F and r_nb.dtype == F
    return mask, out, r_own, r_nb


# ------------------------------------------------------------------------------------------------- the oracle's colours
_cache = {}


def oracle_colours(angle, fov, **kw):
    """(colours [16, H, W, 3] in PERM16's order, counts [16, H, W]) of monkey.obj from the CPU oracle's 4W x 4H frame"""
    key = (angle, fov, tuple(sorted(kw.items())))
    if key not in _cache:
        if "scene" not in _cache:
            from conftest import procedural_env
            m = rr.Mesh()
            assert m.load(O.asset("monkey.obj"))
            s = O.Scene()
            s.add_mesh(m.verts, m.indices)
            s.set_envmap(procedural_env(ENV["w"], ENV["h"], seed=ENV["seed"]))
            _cache["scene"] = s
        _, M, cam = view_constants(angle, fov)
        ref = _cache["scene"].render(M, cam, 4 * W, 4 * H, O.default_params(use_bvh=1, accum_mode=1, use_libm=0, **kw), want_rays=True)
        rgb = ref["rgb"].reshape(H, 4, W, 4, 3).transpose(1, 3, 0, 2, 4)
        cnt = ref["rays"].astype(np.uint32).reshape(H, 4, W, 4).transpose(1, 3, 0, 2)
        _cache[key] = (np.stack([rgb[j, i] for i, j in PERM16]), np.stack([cnt[j, i] for i, j in PERM16]))
    return _cache[key]


def scene_rect(angle, fov):
    import ctypes as C
    sc, _, _ = view_constants(angle, fov)
    m = rr.Mesh()
    assert m.load(O.asset("monkey.obj"))
    p = m.verts.view(np.float32).reshape(-1, 8)[:, :3]
    bounds = (C.c_float * 6)(*[float(x) for x in np.concatenate([p.min(axis=0), p.max(axis=0)])])
    rect = (C.c_uint32 * 4)()
    assert rr.lib().rr_host_screen_rect(bounds, C.byref(sc), 1, W, H, rect) == 0
    return [int(v) for v in rect]


def test_pattern_prefix_is_the_builtin_4x_pattern():
    assert len(PERM16) == 16 and len(set(PERM16)) == 16
    assert OFFP16[:4].tobytes() == rr.sample_pattern(4).tobytes()
    assert sorted(map(tuple, OFFP16.tolist())) == sorted(((2 * i + 1) / 8.0, (2 * j + 1) / 8.0) for i, j in CELL16)


@pytest.mark.parametrize("tonemap", [False, True])
def test_conditions_the_gpu_test_relies_on(tonemap):
    """with THRESHOLD and VIEWS the oracle's frames hold both classes inside the scene's screen rectangle, both causes of a
    refinement on their own, and a refined pixel on the frame's edge"""
    on_edge = 0
    for angle, fov in VIEWS:
        cols, _ = oracle_colours(angle, fov)
        mask, out, r_own, r_nb = adaptive_reference(cols, 4, THRESHOLD, tonemap)
        x0, y0, x1, y1 = scene_rect(angle, fov)
        inside = np.zeros((H, W), bool)
        inside[y0:min(y1, H), x0:min(x1, W)] = True
        n_ref, n_unref = int((mask & inside).sum()), int((~mask & inside).sum())
        t = F(THRESHOLD)
        own_only = int(((r_own > t) & ~(r_nb > t)).sum())
        nb_only = int((~(r_own > t) & (r_nb > t)).sum())
        edge = np.zeros((H, W), bool)
        edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = True
        on_edge += int((mask & edge).sum())
        # each pixel is the fold of 4 or of 16
        f4, f16 = fold(list(cols[:4])), fold(list(cols))
        assert np.array_equal(out.view(np.uint32), np.where(mask[..., None], f16, f4).view(np.uint32))
        print("view %s tonemap %d: refined %d, unrefined %d inside the rectangle (%d of %d pixels); own only %d, neighbours only %d"
              % ((angle, fov), tonemap, n_ref, n_unref, int(inside.sum()), W * H, own_only, nb_only))
        # the floors hold in every view on its own: the GPU test asserts its two classes per view
        assert n_ref >= 64 and n_unref >= 64
        assert own_only >= 8 and nb_only >= 8
    print("refined on the edge: %d" % on_edge)
    assert on_edge >= 1


def test_degenerate_settings_on_the_oracle():
    cols, _ = oracle_colours(*VIEWS[1])
    mask, out, _, _ = adaptive_reference(cols, 4, 1.0, False)   # display values lie in [0, 1]: no difference exceeds 1
    assert not mask.any() and np.array_equal(out.view(np.uint32), fold(list(cols[:4])).view(np.uint32))
    mask, out, _, _ = adaptive_reference(cols, 16, 0.0, False)  # n_base == n_max: refined or not, the fold of all
    assert mask.any() and np.array_equal(out.view(np.uint32), fold(list(cols)).view(np.uint32))
    mask0, _, _, _ = adaptive_reference(cols, 4, 0.0, False)
    mask1, _, _, _ = adaptive_reference(cols, 4, THRESHOLD, False)
    assert (mask0 | ~mask1).all() and mask0.sum() > mask1.sum()     # the refined set shrinks as the threshold grows


# ------------------------------------------------------------------------------------------------- hand-made colours
def frame(values):
    """[S][h][w] scalars -> grey colours [S, h, w, 3]"""
    a = np.asarray(values, F)
    return np.repeat(a[..., None], 3, axis=-1).copy()


def test_display_values():
    c = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 0.25, 1.0, 7.0, 3.4028234663852886e38], F)
    assert np.array_equal(display(c, False), np.array([0, 1, 0, 0, 0, 0, 0.25, 1, 1, 1], F))
    want = np.array([0, 1, 0, 0, 0, 0, F(0.25) / F(1.25), 0.5, F(7) / F(8), 1], F)
    assert np.array_equal(display(c, True), want)


@pytest.mark.parametrize("tonemap", [False, True])
def test_odd_sample_values(tonemap):
    # one row of 6 pixels, 2 base samples + 1 more; pixel 0: NaN against 0 (no contrast: NaN shows as 0), 1: +inf against 0 (shows
    # as 1), 2: a negative against 0 (shows as 0), 3: -0 against +0, 4 and 5: plain 0
    s0 = [np.nan, np.inf, -5.0, -0.0, 0.0, 0.0]
    s1 = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    s2 = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    cols = frame([[s0], [s1], [s2]])
    mask, out, r_own, r_nb = adaptive_reference(cols, 2, 0.5, tonemap)
    assert np.array_equal(r_own[0], np.array([0, 1, 0, 0, 0, 0], F))
    # base colours: NaN, inf, -2.5, 0, 0, 0 -> shown as 0, 1, 0, 0, 0, 0
    assert np.array_equal(r_nb[0], np.array([1, 1, 1, 0, 0, 0], F))
    assert mask[0].tolist() == [True, True, True, False, False, False]
    with np.errstate(invalid="ignore"):
        want = np.array([np.nan, np.inf, F(-4) / F(3), 0, 0, 0], F)
    assert np.array_equal(out[0, :, 0].view(np.uint32)[1:], want.view(np.uint32)[1:]) and np.isnan(out[0, 0, 0])
    # -0 + 0 = +0 in the fold, and a fold of one sample keeps its -0
    m1, o1, _, _ = adaptive_reference(cols, 1, 1.0, tonemap)
    assert not m1.any() and np.signbit(o1[0, 3, 0]) and not np.signbit(out[0, 3, 0])


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (1, 1)])
def test_frames_one_pixel_wide(shape):
    h, w = shape
    n = h * w
    a = np.zeros(n, F)
    if n > 2:
        a[2] = 0.6                                              # one bright pixel: its neighbours along the line see it, nothing else
    cols = frame([a.reshape(h, w), a.reshape(h, w)])
    mask, out, r_own, r_nb = adaptive_reference(cols, 1, 0.5, False)
    assert not r_own.any()
    want = np.zeros(n, bool)
    if n > 2:
        want[1:4] = True
    assert mask.reshape(-1).tolist() == want.tolist()
    assert np.array_equal(out[..., 0].reshape(-1), a)


def test_threshold_zero_leaves_a_constant_image_alone():
    cols = np.full((4, 5, 6, 3), 0.37, F)
    cols[..., 1] = 2.5                                          # (a channel beyond the display range, the same everywhere)
    for tonemap in (False, True):
        mask, out, r_own, r_nb = adaptive_reference(cols, 2, 0.0, tonemap)
        assert not mask.any() and not r_own.any() and not r_nb.any()
        assert np.array_equal(out, fold(list(cols[:2])))
    cols[3, 2, 2, 0] = 0.9                                      # a sample the base does not see changes nothing
    assert not adaptive_reference(cols, 2, 0.0, False)[0].any()
    cols[1, 2, 2, 0] = 0.38                                     # one the base sees refines the pixel and its four neighbours
    mask = adaptive_reference(cols, 2, 0.0, False)[0]
    assert int(mask.sum()) == 5 and mask[2, 2] and mask[1, 2] and mask[3, 2] and mask[2, 1] and mask[2, 3]
