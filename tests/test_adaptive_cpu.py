"""CPU: the rule of rr_render_adaptive (include/rrdxr.h, steps 1 to 6) restated in numpy, and the conditions the GPU test
(test_gpu_adaptive.py) relies on, computed from the CPU oracle alone.

adaptive_reference is what the GPU test compares against, so it is itself tested here: on the oracle's colours of monkey.obj -- a
frame 4 times as large per axis whose pixels are the 16 sub-pixel samples of a 52 x 37 base frame (test_gpu_samples.py) -- and on
hand-made colour arrays with NaN, inf, negative and -0 samples, one-pixel-wide frames and a constant image."""
import numpy as np
import pytest

import oracle as O
import refraction_raytracing_dxr_amd as rr
from shading_helpers import ADAPTIVE_VIEWS as VIEWS
from shading_helpers import CELL16, OFFP16, PERM16, THRESHOLD, H, W, adaptive_reference, display, fold, oracle_colours, view_constants

F = np.float32


# ------------------------------------------------------------------------------------------------- the oracle's colours


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
