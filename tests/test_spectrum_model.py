"""The radial power spectrum's float64 model (tests/helpers/spectrum_model.py) against numpy's FFT and against its own definition,
the derived error bound against numpy's fp32 matmul standing in for the kernel, and the package's host-made tables
(locate_amd/spectrum.py) against the model's.  No GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectrum_model as M  # noqa: E402

SIZES = (32, 64, 128, 256)
BINS = {32: 24, 64: 46, 128: 92, 256: 182}


def planes(S, n=4, seed=0, shift=0.0):
    return (np.tanh(np.random.default_rng(seed + S).standard_normal((n, S, S))) + shift).astype(np.float32)


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("name", ["none", "hann"])
def test_the_model_is_the_real_input_fft(S, name):
    """Against rfft2 of the windowed plane.  The model reads fp32 tables: each entry carries one rounding (relative 2^-24), a
    product of two (1 + 2^-24)^2 - 1, on factors of at most w[y] w[x]: the gap per element is at most that times
    sum |x| w w - plus both sides' float64 evaluation, allowed for with 8 S 2^-53 of the same sum."""
    x = planes(S)
    w = M.window(S, name)
    xw = x.astype(np.float64) * w[:, None] * w[None, :]
    Yr, Yi = M.dft(x, M.tables(S, name))
    F = np.fft.rfft2(xw)
    allowed = (((1 + M.U) ** 2 - 1) + 8 * S * 2.0 ** -53) * np.abs(xw).sum(axis=(1, 2))
    gap = np.maximum(np.abs(Yr - F.real), np.abs(Yi - F.imag)).max(axis=(1, 2))
    print("S = %d %s: gap %.2e of max|F|, allowed %.2e" % (S, name, (gap / np.abs(F).max(axis=(1, 2))).max(), (allowed / np.abs(F).max(axis=(1, 2))).max()))
    assert (gap <= allowed).all()


@pytest.mark.parametrize("S", SIZES)
def test_bin_table_properties(S):
    r, m = M.bins(S)
    H = S // 2
    assert r.shape == (S, H + 1) and r.min() == 0 and int(r.max()) + 1 == BINS[S]          # every frequency lies in exactly one bin
    mult = M.multiplicity(S)
    assert mult.sum() == S * S and (mult > 0).all()
    # the last bin holds (H, H) - alone at 32, 128 and 256; at 64, (H, H - 1) and (H - 1, H) (radius 44.55) round into it as well
    assert r[H, H] == BINS[S] - 1 and mult[-1] == (5 if S == 64 else 1) and (r == BINS[S] - 1).sum() == (4 if S == 64 else 1)
    assert r[0, 0] == 0 and mult[0] == 1
    # the half spectrum with its weights is the full S x S spectrum, bin by bin
    f = np.where(np.arange(S) <= H, np.arange(S), np.arange(S) - S)
    d = 4 * (f[:, None] ** 2 + f[None, :] ** 2)
    full = np.zeros_like(d)
    while (d >= (2 * full + 1) ** 2).any():
        full = full + (d >= (2 * full + 1) ** 2)
    assert np.array_equal(np.bincount(full.ravel()), mult)
    # the rounded radius: |r - sqrt(fy^2 + k^2)| <= 1/2
    assert (np.abs(r - np.sqrt(d[:, :H + 1] / 4.0)) <= 0.5 + 1e-12).all()


@pytest.mark.parametrize("S", SIZES)
def test_the_package_makes_the_models_tables(S):
    from locate_amd.spectrum import bin_slots, dft_tables, radial_bins, window_weights
    r, _ = M.bins(S)
    bins, mult = radial_bins(S)
    assert bins.dtype == np.int32 and np.array_equal(bins, r) and np.array_equal(mult, M.multiplicity(S))
    for name in ("none", "hann"):
        for got, want in zip(dft_tables(S, name), M.tables(S, name)):
            assert got.dtype == np.float32 and got.shape == (S, S) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(window_weights(S, name), M.window(S, name))
    slot, start = bin_slots(bins)
    cells = S * (S // 2 + 1)
    assert slot.dtype == np.int32 and start.dtype == np.int32 and sorted(slot.ravel().tolist()) == list(range(cells))
    assert start[0] == 0 and start[-1] == cells and len(start) == BINS[S] + 1
    flat = np.empty(cells, dtype=np.int64)
    flat[slot.ravel()] = bins.ravel()
    assert (np.diff(flat) >= 0).all() and all((flat[start[b]:start[b + 1]] == b).all() for b in range(BINS[S]))
    where = np.empty(cells, dtype=np.int64)
    where[slot.ravel()] = np.arange(cells)
    assert all((np.diff(where[start[b]:start[b + 1]]) > 0).all() for b in range(BINS[S]))          # ascending (a, k) inside a bin


@pytest.mark.parametrize("S", [32, 64])
def test_table_entries(S):
    C, Sn = M.tables(S)
    q = S // 4
    j = np.arange(S)
    kj = np.outer(j, j) % S
    at = kj % q == 0
    assert set(np.unique(C[at])) <= {-1.0, 0.0, 1.0} and set(np.unique(Sn[at])) <= {-1.0, 0.0, 1.0}
    assert (Sn[0] == 0).all() and (Sn[S // 2] == 0).all() and (np.abs(C[S // 2]) == 1).all() and (C[0] == 1).all()
    assert np.abs(C.astype(np.float64) ** 2 + Sn.astype(np.float64) ** 2 - 1).max() <= 4 * M.U
    w = M.window(S, "hann")
    assert abs((w * w).sum() - S) <= 1e-12 * S and w[0] == 0.0 and abs(w[S // 2] - w.max()) == 0.0
    Ch, _ = M.tables(S, "hann")
    assert abs((Ch[0].astype(np.float64) ** 2).sum() - S) <= 4 * M.U * S


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("name", ["none", "hann"])
def test_parseval(S, name):
    """sum_r spectrum[r] = mean of the windowed squares.  With e = the table-rounding gap of test_the_model_is_the_real_input_fft
    per component, the powers differ by at most sum m (2 (|Fr| + |Fi|) e + 2 e^2) / S^4."""
    x = planes(S, seed=3)
    w = M.window(S, name)
    xw = x.astype(np.float64) * w[:, None] * w[None, :]
    got = M.spectrum(x, M.tables(S, name)).sum(axis=1)
    want = (xw * xw).mean(axis=(1, 2))
    F = np.fft.rfft2(xw)
    e = ((((1 + M.U) ** 2 - 1) + 8 * S * 2.0 ** -53) * np.abs(xw).sum(axis=(1, 2)))[:, None, None]
    _, m = M.bins(S)
    allowed = ((2 * (np.abs(F.real) + np.abs(F.imag)) * e + 2 * e * e) * m).sum(axis=(1, 2)) / float(S) ** 4
    print("S = %d %s: %.2e relative, allowed %.2e" % (S, name, (np.abs(got - want) / want).max(), (allowed / want).max()))
    assert (np.abs(got - want) <= allowed).all() and (allowed <= 1e-4 * want).all()          # the second: the allowance is not vacuous


@pytest.mark.parametrize("S,shift", [(16, 0.0), (64, 0.0), (32, 50.0)])
def test_fp32_matmul_stays_inside_the_derived_bound(S, shift):
    x = planes(S, n=6, seed=1, shift=shift)
    tabs = M.tables(S)
    want, bound = M.spectrum(x, tabs), M.spectrum_bound(x, tabs)
    Yr, Yi = M.dft(x, tabs, dtype=np.float32)
    got = M.spectrum_of(Yr, Yi, S)
    ratio = np.abs(got - want) / bound
    print("S = %d shift %g: worst error / bound %.4f; bound / value: median %.1e, max %.1e" % (S, shift, ratio.max(), np.median(bound / want), (bound / want).max()))
    assert (bound > 0).all() and ratio.max() <= 1.0
    if shift == 0.0:
        assert (bound <= 0.05 * want).all(), "a bound that large would hide a structural mistake"


@pytest.mark.parametrize("S", [32, 64])
def test_exact_cases_of_the_model(S):
    H = S // 2
    yy, xx = np.mgrid[:S, :S]
    tabs = M.tables(S)
    checker = (0.5 * (-1.0) ** (yy + xx)).astype(np.float32)
    const = np.full((S, S), 0.25, dtype=np.float32)
    wave = np.cos(2 * np.pi * (3 * xx + 4 * yy) / S).astype(np.float32)
    sp = M.spectrum(np.stack([checker, const, wave]), tabs)
    bound = M.spectrum_bound(np.stack([checker, const, wave]), tabs)
    assert sp[0, -1] == 0.25 and (sp[0, :-1] <= bound[0, :-1]).all()
    assert sp[1, 0] == 0.0625 and (sp[1, 1:] <= bound[1, 1:]).all()
    r, _ = M.bins(S)
    assert r[4, 3] == 5 and r[S - 4, 3] == 5
    # (the fp32 samples of the cosine are rounded: 1e-15 of its power lies elsewhere, far below the bound)
    assert abs(sp[2, 5] - 0.5) <= bound[2, 5] and (np.delete(sp[2], 5) <= np.delete(bound[2], 5)).all()
    assert bound[2, 5] <= 0.01 and r[H, H] == sp.shape[1] - 1


def test_summary_model():
    S = 32
    rng = np.random.default_rng(5)
    sp = rng.random((5, 3, 24))
    sp[2, 1, 7] = np.nan
    sp[4, 0, 0] = np.inf
    s, q, bad = M.summary(sp, S)
    mult = M.multiplicity(S)
    assert bad.tolist() == [1, 1, 0]
    assert np.allclose(s[2], (sp[:, 2] / mult).sum(0)) and np.allclose(s[1], (np.delete(sp[:, 1], 2, axis=0) / mult).sum(0))
    assert np.allclose(q[0], ((sp[:4, 0] / mult) ** 2).sum(0)) and np.isfinite(s).all() and np.isfinite(q).all()
