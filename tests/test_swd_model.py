"""The float64 model of the sliced Wasserstein metric (tests/helpers/swd_model.py) held to facts outside itself: scipy's mirrored
convolution, the exact invariances of the definition, and the closed-form value for two shifted normal clouds."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import swd_model as M  # noqa: E402


def unit_dirs(rng, D):
    d = rng.standard_normal((M.K, D))
    return d / np.sqrt((d * d).sum(0, keepdims=True))


@pytest.mark.parametrize("S", [8, 16, 32])
def test_down_and_up_are_scipy_mirror_convolutions(S):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(S)
    x = rng.standard_normal((S, S))
    g = np.outer(M.W5, M.W5) / 256.0
    assert np.array_equal(M.mirror(np.array([-1, -2, S, S + 1]), S), [1, 2, S - 2, S - 3])
    want = ndimage.convolve(x, g, mode="mirror")[::2, ::2]
    assert np.abs(M.down(x) - want).max() <= 1e-15 * np.abs(x).max()
    y = rng.standard_normal((S // 2, S // 2))
    z = np.zeros((S, S))
    z[::2, ::2] = y
    want = ndimage.convolve(z, 4.0 * g, mode="mirror")
    assert np.abs(M.up(y) - want).max() <= 1e-15 * np.abs(y).max()
    # the polyphase form the kernel evaluates: even outputs (1, 6, 1) / 8, odd outputs (4, 4) / 8 per axis, the mirror on the doubled grid
    Sc = S // 2
    lo = np.where(np.arange(Sc) == 0, 1, np.arange(Sc) - 1)
    hi = np.where(np.arange(Sc) == Sc - 1, Sc - 1, np.arange(Sc) + 1)
    rows = np.zeros((S, Sc))
    rows[::2], rows[1::2] = (y[lo] + 6 * y + y[hi]) / 8, (y + y[hi]) / 2
    poly = np.zeros((S, S))
    poly[:, ::2], poly[:, 1::2] = (rows[:, lo] + 6 * rows + rows[:, hi]) / 8, (rows + rows[:, hi]) / 2
    assert np.abs(poly - want).max() <= 1e-15 * np.abs(y).max()


def test_constant_image():
    x = np.full((2, 3, 64, 64), 0.37)
    levels = M.laplacian_pyramid(x)
    assert [l.shape[-1] for l in levels] == [64, 32, 16]
    for l in levels[:-1]:
        assert np.abs(l).max() <= 1e-15
    assert np.abs(levels[-1] - 0.37).max() <= 1e-15


def sets(seed, N=6, S=32, P=8):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((N, 3, S, S)).astype(np.float32)
    b = M.blur(rng.standard_normal((N, 3, S, S))).astype(np.float32)
    sizes = M.pyramid_levels(S)
    pos = [[rng.integers(0, s - 6, size=(N * P, 2)) for s in sizes] for _ in range(2)]
    return a, b, pos, P, unit_dirs(rng, 12).astype(np.float32)


def test_a_set_against_itself_is_zero():
    a, _, pos, P, dirs = sets(1)
    out = M.swd(a, a, pos[0], pos[0], P, dirs, 3)
    assert out["levels"] == [0.0, 0.0] and out["mean"] == 0.0
    assert all(v > 0 for v in M.swd(a, a, pos[0], pos[1], P, dirs, 3)["levels"])          # other positions: other descriptors


def test_affine_maps_of_a_set_change_nothing():
    """the float64 statistics are used here, not their fp32 roundings, which the map 2 B + 3 does not commute with"""
    a, b, pos, P, dirs = sets(2)
    la, lb, lc = M.laplacian_pyramid(a), M.laplacian_pyramid(b), M.laplacian_pyramid(2.0 * b.astype(np.float64) + 3.0)
    for l in range(len(la)):
        da = M.descriptors(la[l], pos[0][l], P)
        vals = []
        for lev in (lb, lc):
            db = M.descriptors(lev[l], pos[1][l], P)
            mu_a, sg_a = M.stats64(da)
            mu_b, sg_b = M.stats64(db)
            pa = M.project(da, dirs, np.concatenate([mu_a, 1 / sg_a]))
            pb = M.project(db, dirs, np.concatenate([mu_b, 1 / sg_b]))
            vals.append(M.sliced_distance(pa, pb))
        assert abs(vals[0] - vals[1]) <= 1e-12, (l, vals)
        assert vals[0] > 0.05


def test_shifted_normal_clouds():
    """Descriptors drawn i.i.d. N(0, 1) and N(0, 1) + delta e: a projection of the second cloud is the first one's law shifted by
    delta (e . dir), so the value tends to |delta| mean_d |e . dir_d| (the per-channel normalisation moves each cloud by
    O(n^-1/2), the sorted differences' own noise; e is spread over all 147 elements, so a channel's deviation grows by about
    delta^2 / 2 = 2 %).  seed 7, n = 50000, delta = 0.2 per element, 10 % allowed."""
    rng = np.random.default_rng(7)
    n, delta = 50000, 0.2
    dirs = unit_dirs(rng, 16)
    e = rng.standard_normal(M.K)
    e /= np.sqrt((e * e).sum())
    da = rng.standard_normal((n, M.K))
    db = rng.standard_normal((n, M.K)) + delta * np.sqrt(M.K) * e          # every element shifted by about delta
    got = M.swd_descriptors(da, db, dirs, 2)
    # the shift survives the normalisation only as far as it is not the channel's mean: take that part out
    shift = delta * np.sqrt(M.K) * e
    shift = shift - np.repeat(shift.reshape(3, 49).mean(1), 49)
    want = np.abs(shift @ dirs).mean()
    print("shifted clouds: %.5f against %.5f" % (got, want))
    assert abs(got - want) <= 0.10 * want
