"""The float64 model of the multi-scale SSIM (tests/helpers/msssim_model.py) against an independent statement written here, the
properties of its window table, and the cases whose result is known exactly.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import msssim_model as M  # noqa: E402

SIZES_TABLE = {32: ([11, 11, 8, 4, 2], [22, 6, 1, 1, 1]), 64: ([11, 11, 11, 8, 4], [54, 22, 6, 1, 1]),
               128: ([11, 11, 11, 11, 8], [118, 54, 22, 6, 1]), 256: ([11, 11, 11, 11, 11], [246, 118, 54, 22, 6])}


# ---- an independent statement: the 2-D window by explicit sliding windows, no separability ---------------------------------------------
def window_2d(n):
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    sigma = 1.5 * n / 11
    w = np.exp(-(t[:, None] ** 2 + t[None, :] ** 2) / (2.0 * sigma ** 2))
    return w / w.sum()


def independent_levels(x, y, filt):
    S = x.shape[-1]
    out = np.zeros((2, 5))
    for l in range(5):
        s = S >> l
        n = min(11, s)
        w = window_2d(n)
        mx, my, exx, eyy, exy = (filt(p, w) for p in (x, y, x * x, y * y, x * y))
        sxx, syy, sxy = exx - mx ** 2, eyy - my ** 2, exy - mx * my
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        ssim = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
        out[0, l], out[1, l] = ssim.mean(), cs.mean()
        x = x.reshape(3, s // 2, 2, s // 2, 2).mean(axis=(2, 4))
        y = y.reshape(3, s // 2, 2, s // 2, 2).mean(axis=(2, 4))
    return out


def sliding(p, w):
    n = w.shape[0]
    o = p.shape[-1] - n + 1
    out = np.empty((3, o, o))
    for r in range(o):
        for c in range(o):
            out[:, r, c] = (p[:, r:r + n, c:c + n] * w).sum(axis=(1, 2))
    return out


def pairs_for(S):
    a = np.concatenate([M.uniform_bytes(1, S, S), M.low_pass(1, S, S + 1), M.bright_texture(1, S, S + 2)])
    b = np.concatenate([M.uniform_bytes(1, S, S + 3), M.low_pass(1, S, S + 4), M.bright_texture(1, S, S + 5)])
    return list(zip(a, b)) + [M.anticorrelated(S)]


@pytest.mark.parametrize("S", [32, 64])
def test_the_model_agrees_with_an_independent_statement(S):
    """the two differ in summation order over at most 121 non-negative terms, about 1e-14; a wrong sigma, offset or window size is
    off by 1e-3 or more"""
    worst = 0.0
    for x, y in pairs_for(S):
        got, want = M.levels(x, y), independent_levels(x, y, sliding)
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    print("S = %d: worst relative difference %.2e" % (S, worst))


def test_the_model_agrees_with_fftconvolve():
    signal = pytest.importorskip("scipy.signal")

    def filt(p, w):
        return np.stack([signal.fftconvolve(q, w[::-1, ::-1], "valid") for q in p])
    # an FFT's error is relative to the plane's largest moment (65025), not to the output: 1e-9 absolute on a level number leaves a
    # wrong window (1e-3) nowhere to hide
    for x, y in pairs_for(32):
        assert np.abs(M.levels(x, y) - independent_levels(x, y, filt)).max() < 1e-9


# ---- the taps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_properties_of_the_taps(S):
    from locate_amd.msssim import window_taps
    taps = M.window_taps(S)
    assert taps.shape == (5, 11) and taps.dtype == np.float64 and np.array_equal(taps, window_taps(S))
    assert M.window_sizes(S) == SIZES_TABLE[S][0] and M.output_sizes(S) == SIZES_TABLE[S][1]
    for l, n in enumerate(SIZES_TABLE[S][0]):
        g = taps[l]
        assert (g[:n] > 0).all() and (g[n:] == 0).all()
        assert abs(g.sum() - 1.0) <= 2.0 ** -52
        assert np.array_equal(g[:n], g[:n][::-1])
        assert np.argmax(g[:n]) == (n - 1) // 2
    if S == 32:
        assert taps[4][:2].tolist() == [0.5, 0.5]          # an even window is centred between pixels
    for bad in (0, 16, 48, 512):
        with pytest.raises(ValueError):
            window_taps(bad)


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128])
def test_an_image_against_itself_is_exactly_one(S):
    for x in (M.uniform_bytes(1, S, 5)[0], M.low_pass(1, S, 6)[0], M.bright_texture(1, S, 7)[0], np.zeros((3, S, S)), np.full((3, S, S), 255.0)):
        assert (M.levels(x, x) == 1.0).all()
    v, clamped = M.value(M.levels(x, x))
    assert v == 1.0 and not clamped


@pytest.mark.parametrize("S", [32, 64])
def test_white_against_black(S):
    """y = 0: my, eyy, exy are exact zeros, so v1 == C2 exactly; sxx = exx - mx^2 of a constant 255 is rounding noise of a few ulp of
    65025 (1e-11): cs = C2 / (C2 + noise) is 1 and ssim C1 / (255^2 + C1) within 1e-12"""
    lv = M.levels(np.full((3, S, S), 255.0), np.zeros((3, S, S)))
    print("cs - 1: %s; ssim / (C1 / (255^2 + C1)) - 1: %s" % (lv[1] - 1, lv[0] / (M.C1 / (255.0 ** 2 + M.C1)) - 1))
    assert (np.abs(lv[1] - 1.0) <= 1e-12).all()
    assert (np.abs(lv[0] - M.C1 / (255.0 ** 2 + M.C1)) <= 1e-12 * M.C1 / (255.0 ** 2 + M.C1)).all()


@pytest.mark.parametrize("S", [32, 64])
def test_symmetry_in_bits(S):
    for x, y in pairs_for(S):
        assert np.array_equal(M.levels(x, y), M.levels(y, x))


@pytest.mark.parametrize("S", [32, 64, 128])
def test_the_anticorrelated_pair_clamps(S):
    a, b = M.anticorrelated(S)
    lv = M.levels(a, b)
    assert (lv[1, :4] < -0.85).all()
    v, clamped = M.value(lv)
    assert v == 0.0 and clamped


def test_white_noise_goes_negative():
    """unrelated images do go negative at the fine levels: the record must carry the count and the per-level means"""
    lvs = np.stack([M.levels(x, y) for x, y in zip(M.uniform_bytes(8, 32, 1), M.uniform_bytes(8, 32, 2))])
    v, clamped = M.value(lvs)
    print("cs means per level: %s; clamped %d of 8" % (lvs[:, 1].mean(axis=0), clamped.sum()))
    assert clamped.any() and (v[clamped] == 0).all() and (v[~clamped] > 0).all()


def test_value_keeps_nan():
    lv = np.stack([M.levels(*M.anticorrelated(32)), np.full((2, 5), np.nan), np.ones((2, 5))])
    v, clamped = M.value(lv)
    assert v[0] == 0 and np.isnan(v[1]) and v[2] == 1.0 and clamped.tolist() == [True, False, False]


def test_the_bound_is_what_its_derivation_says():
    u = 2.0 ** -53
    assert 5e-10 < M.LEVEL_BOUND < 6e-10
    assert abs(M.C1 - 6.5025) < 1e-14 and abs(M.C2 - 58.5225) < 1e-13 and sum(M.WEIGHTS) == pytest.approx(1.0001)
    assert M.LEVEL_BOUND > 2 * (2 * (4 * 255 * 24 * u * 255) / M.C1)          # the luminance term alone
