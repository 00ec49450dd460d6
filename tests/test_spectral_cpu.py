"""CPU: the host side of the spectral frames -- the band table of rr_host_spectral_bands (Cauchy's law, the tent weights), the
weighted resolve rule on the CPU oracle's frames as a second opinion on the semantics, and the code generation of
k_render_spectral."""
import ctypes as C

import numpy as np
import pytest

import refraction_raytracing_dxr_amd as rr
from codeobj import HAVE_OBJDUMP, LAUNCHABLE, kernels, template_args
from shading_helpers import H, W, fold, oracle_colours
from spectral_helpers import BANDS4, ORACLE_KW, ORACLE_VIEW, oracle_spectral_frame, weighted_fold

RR_ERR_INVALID_ARGUMENT = 1
F = np.float32
SIZES = (2, 3, 8, 16, 64)


def wavelengths(n):
    return 400.0 + (np.arange(n) + 0.5) / n * 300.0


def cauchy(ior_d, abbe):
    B = (float(F(ior_d)) - 1.0) / (abbe * (1.0 / 486.1 ** 2 - 1.0 / 656.3 ** 2))
    return float(F(ior_d)) - B / 587.6 ** 2, B


# ------------------------------------------------------------------------------------------------- 1. the band table
def test_one_band_is_the_d_line():
    for ior_d, abbe in ((1.3, 30.0), (1.5, 64.0), (2.4, float("inf"))):
        b = rr.spectral_bands(1, ior_d, abbe)
        assert b.shape == (1,) and b.dtype == rr.BAND_DTYPE
        assert b["ior"][0] == F(ior_d) and b["weight"].tobytes() == np.ones(3, F).tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ior_d,abbe", [(1.3, 30.0), (1.5, 64.2), (1.7, 20.0)])
def test_cauchys_law(n, ior_d, abbe):
    b = rr.spectral_bands(n, ior_d, abbe)
    assert b.shape == (n,)
    ior = b["ior"].astype(np.float64)
    lam = wavelengths(n)
    assert np.all(np.diff(ior) < 0)                             # strictly falling with the wavelength
    A, B = cauchy(ior_d, abbe)
    assert np.array_equal(b["ior"], (A + B / lam ** 2).astype(F))       # double, rounded once
    # the d line lies between two bands: so does ior_d, and the chord between them passes it by no more than a chord's error on a
    # convex curve, h^2 / 8 * max f'' with f'' = 6 B / l^4 at the shorter wavelength, plus the two roundings to float
    i = int(np.searchsorted(lam, 587.6)) - 1
    assert 0 <= i < n - 1 and lam[i] < 587.6 < lam[i + 1]
    assert ior[i] > float(F(ior_d)) > ior[i + 1]
    t = (587.6 - lam[i]) / (lam[i + 1] - lam[i])
    at_d = ior[i] + t * (ior[i + 1] - ior[i])
    bound = (lam[i + 1] - lam[i]) ** 2 / 8.0 * 6.0 * B / lam[i] ** 4 + 2.0 ** -23 * ior[i]
    print("n = %d: ior %.6f at the d line by interpolation, ior_d %.6f, bound %.2g" % (n, at_d, ior_d, bound))
    assert ior[i + 1] <= at_d <= ior[i] and 0.0 <= at_d - float(F(ior_d)) + 2.0 ** -23 * ior[i] and abs(at_d - float(F(ior_d))) <= bound
    # an Abbe number over the F and C lines: (n_d - 1) / (n_F - n_C) of the law the table follows
    law = lambda l: A + B / l ** 2                              # noqa: E731
    assert abs((law(587.6) - 1.0) / (law(486.1) - law(656.3)) - abbe) < 1e-9 * abbe


@pytest.mark.parametrize("n", SIZES)
def test_no_dispersion_at_an_infinite_abbe_number(n):
    b = rr.spectral_bands(n, 1.45, float("inf"))
    assert np.all(b["ior"] == F(1.45))
    assert b["weight"].tobytes() == rr.spectral_bands(n, 1.3, 30.0)["weight"].tobytes()       # the weights do not depend on the glass


@pytest.mark.parametrize("n", SIZES)
def test_tent_weights(n):
    w = rr.spectral_bands(n, 1.3, 30.0)["weight"]
    assert w.shape == (n, 3) and w.dtype == F
    assert np.all(w >= 0)
    lam = wavelengths(n)
    for c, centre in enumerate((650.0, 550.0, 450.0)):
        tent = np.maximum(0.0, 1.0 - np.abs(lam - centre) / 100.0)
        assert np.array_equal(w[:, c], (tent * n / tent.sum()).astype(F))
        assert (w[:, c] > 0).any()
        # each weight is rounded once: the n of them sum to n within n * 2^-24 relative, asserted at four times that
        assert abs(w[:, c].astype(np.float64).sum() - n) <= n * 2.0 ** -22
    assert np.argmax(w[:, 0]) > np.argmax(w[:, 2])              # red peaks at the long end, blue at the short one


def test_bad_band_requests_are_refused():
    L = rr.lib()
    buf = np.zeros(65, rr.BAND_DTYPE)
    p = buf.ctypes.data
    nan, inf = float("nan"), float("inf")
    assert L.rr_host_spectral_bands(64, 1.3, 30.0, p) == 0 and L.rr_host_spectral_bands(8, 1.3, inf, p) == 0
    for n, ior_d, abbe, out in ((0, 1.3, 30.0, p), (65, 1.3, 30.0, p), (8, 0.0, 30.0, p), (8, -1.3, 30.0, p), (8, nan, 30.0, p), (8, inf, 30.0, p),
                                (8, 1.3, 0.0, p), (8, 1.3, -30.0, p), (8, 1.3, nan, p), (8, 1.3, -inf, p), (8, 1.3, 30.0, None), (1, nan, 30.0, p),
                                (1, 1.3, 0.0, p), (8, 1.3, 1e-3, p), (8, 1.3, 1e-38, p)):     # (the last two: a law that leaves ior > 0 or the floats)
        assert L.rr_host_spectral_bands(n, ior_d, abbe, out) == RR_ERR_INVALID_ARGUMENT, (n, ior_d, abbe)
    for n in (0, 65, -1):
        with pytest.raises(rr.RRError) as e:
            rr.spectral_bands(n)
        assert e.value.status == RR_ERR_INVALID_ARGUMENT
    assert rr.spectral_bands(8).tobytes() == rr.spectral_bands(8, 1.3, 30.0).tobytes()


# ------------------------------------------------------------------------------------------------- 2. the oracle's opinion
def test_weighted_fold_with_unit_weights_is_the_fold():
    rng = np.random.default_rng(5)
    cols = [rng.standard_normal((7, 5, 3)).astype(F) for _ in range(6)]
    cols[0][0, 0] = -0.0
    got = weighted_fold(cols, [np.ones(3, F)] * 6)
    assert got.tobytes() == fold(cols).tobytes()
    one = weighted_fold(cols[:1], [np.ones(3, F)])
    assert one.tobytes() == cols[0].tobytes()                   # a sum that starts AT p_0 keeps a -0


def test_the_oracle_disperses():
    """Four oracle frames of monkey.obj at four times the size, rro_params.ior = ior_k, sample k at sub-pixel SUB4[k]: the bands see
    different colours where the mesh refracts, different numbers of rays where one band is totally reflected and another is not,
    and the weighted fold of them -- what test_gpu_spectral.py holds render_spectral to -- differs from the fold at one ior"""
    rgb, cnt, cols = oracle_spectral_frame()
    assert rgb.shape == (H, W, 3) and rgb.dtype == F and cnt.shape == (H, W) and cols.shape == (4, H, W, 3)
    assert np.all(np.isfinite(rgb))
    c13, n13 = oracle_colours(*ORACLE_VIEW, ior=float(BANDS4["ior"][1]), **ORACLE_KW)
    assert cols[1].tobytes() == c13[1].tobytes()
    on_mesh = n13[:4].sum(axis=0) > 4
    # the same sample position (sub-pixel 0) under ior 1.27 and under 1.3
    c127, n127 = oracle_colours(*ORACLE_VIEW, ior=float(BANDS4["ior"][0]), **ORACLE_KW)
    moved = (c127[0].view(np.uint32) != c13[0].view(np.uint32)).any(axis=-1)
    recount = n127[0] != n13[0]
    print("%d pixels on the mesh; %d change colour and %d their ray count between ior %.2f and %.2f" %
          (int(on_mesh.sum()), int(moved.sum()), int(recount.sum()), BANDS4["ior"][0], BANDS4["ior"][1]))
    assert on_mesh.sum() > 200 and moved.sum() > 100 and not moved[~(n13[0] > 1) & ~(n127[0] > 1)].any()
    plain = fold([c13[k] for k in range(4)])
    differ = (rgb.view(np.uint32) != plain.view(np.uint32)).any(axis=-1)
    assert differ.sum() > 100
    assert cnt.dtype == np.uint32 and (cnt >= 4).all() and (cnt[on_mesh] > 4).all()


# ------------------------------------------------------------------------------------------------- 3. codegen
@pytest.mark.skipif(not HAVE_OBJDUMP, reason="llvm-objdump of the ROCm toolchain not found")
def test_spectral_kernels_exist(tmp_path):
    """every k_render_spectral<STACK, PEND, TLAS, E> the host can launch is in the gfx950 code object, and k_render_samples still has
    all of its own; the scratch_ instructions of both are printed side by side (no assertion on the counts: DESIGN 5.9 records them)"""
    k = {n: v["scratch"] for n, v in kernels(tmp_path).items()}
    mine = {n: v for n, v in k.items() if "k_render_spectral<" in n}
    assert len(mine) == len(LAUNCHABLE), sorted(mine)
    for variant in LAUNCHABLE:
        args = template_args(*variant)
        got = [v for n, v in mine.items() if "k_render_spectral" + args in n]
        ref = [v for n, v in k.items() if "k_render_samples" + args in n]
        assert len(got) == 1 and len(ref) == 1, (args, got, ref)
        print("k_render_spectral%s: %d scratch instructions, k_render_samples: %d" % (args, got[0], ref[0]))
