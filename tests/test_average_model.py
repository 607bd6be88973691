"""The averaged generator's arithmetic and host logic without a GPU: the numpy float32 model of the update kernel
(tests/helpers/average_model.py) against a float64 average within the rounding bound of its three operations, the exact copy at a
weight of 1, and beta / one_minus_beta from the constructor's arguments."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import average_model as M  # noqa: E402

WEIGHTS = {"half-life 10000, batch 64": dict(half_life_images=10000, batch=64), "half-life 64, batch 8": dict(half_life_images=64, batch=8),
           "beta 0.5": dict(beta=0.5)}


def trajectory(T, n=4096, seed=0):
    """weights of mixed magnitudes that move a little every iteration, as a training run's do"""
    rng = np.random.default_rng(seed)
    scale = (10.0 ** rng.uniform(-3, 1, size=n)).astype(np.float32)
    s = (rng.standard_normal(n).astype(np.float32) * scale)
    out = [s]
    for _ in range(T):
        s = (s + np.float32(2e-3) * scale * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
        out.append(s)
    return out


@pytest.mark.parametrize("T", [8, 64])
@pytest.mark.parametrize("which", sorted(WEIGHTS))
def test_float32_model_against_float64(which, T):
    from locate_amd import average_weight
    _, w = average_weight(**WEIGHTS[which])
    steps = trajectory(T, seed=T)
    a32, a64 = steps[0].copy(), steps[0].astype(np.float64)
    top = float(np.abs(steps[0]).max())
    for s in steps[1:]:
        a32, a64 = M.update32(a32, s, w), M.update64(a64, s, w)
        assert a32.dtype == np.float32
        top = max(top, float(np.abs(s).max()), float(np.abs(a32).max()))
    err, unit = float(np.abs(a32 - a64).max()), M.U * top
    limit = M.bound(T, w, top)
    print("%s, T = %d: error %.2f units of 2^-24 max|value|, bound %.2f" % (which, T, err / unit, limit / unit))
    assert limit == (1 + 4 * w) * min(T, 1 / w) * 2.0 ** -24 * top
    assert err <= limit
    assert not np.array_equal(a32, steps[-1]) and np.abs(a64 - steps[-1]).max() > 0          # it is an average, not the last value


def test_weight_one_is_an_exact_copy():
    rng = np.random.default_rng(1)
    bits = rng.integers(-2 ** 31, 2 ** 31, size=512, dtype=np.int64).astype(np.int32)          # every kind of value, NaNs included
    src, avg = bits.view(np.float32), rng.standard_normal(512).astype(np.float32)
    got = M.update32(avg, src, 1.0)
    assert np.array_equal(got.view(np.int32), bits) and got is not src
    a, s = np.float32(1.0), np.float32(1e-8)
    assert np.float32(a + (s - a)) != s          # why the copy is a branch of its own


def test_one_update_is_three_roundings():
    a, s, w = np.array([0.1], np.float32), np.array([0.7], np.float32), np.float32(0.3)
    d = np.float32(np.float64(s[0]) - np.float64(a[0]))
    d = np.float32(np.float64(w) * np.float64(d))
    want = np.float32(np.float64(a[0]) + np.float64(d))
    assert M.update32(a, s, w)[0] == want
    tiny = np.array([1e-40], np.float32)          # subnormals are kept, not flushed
    assert M.update32(np.zeros(1, np.float32), tiny, np.float32(0.5))[0] == np.float32(0.5) * tiny[0] != 0


def test_beta_and_one_minus_beta():
    from locate_amd import average_weight
    beta, w = average_weight(half_life_images=10000, batch=64)
    assert beta == 0.5 ** (64 / 10000) and w == float(np.float32(1.0 - beta)) and abs(w - 0.0044263) < 1e-6
    assert np.float32(w) == w          # an fp32 value
    assert average_weight(half_life_images=64, batch=8) == (0.5 ** 0.125, float(np.float32(1.0 - 0.5 ** 0.125)))
    assert average_weight(beta=0.5) == (0.5, 0.5)
    assert average_weight(half_life_images=64, batch=64) == (0.5, 0.5)          # one half-life per iteration
    assert average_weight(beta=0.999) == (0.999, float(np.float32(1.0 - 0.999)))
    assert average_weight(beta=0) == (0.0, 1.0)
    # the half-life is in images: the same per-image decay whatever the batch
    b8, _ = average_weight(half_life_images=1000, batch=8)
    b64, _ = average_weight(half_life_images=1000, batch=64)
    assert abs(b8 ** 8 - b64) < 1e-15


@pytest.mark.parametrize("kw", [dict(), dict(beta=0.9, half_life_images=100, batch=8), dict(beta=0.9, batch=8), dict(half_life_images=100),
                                dict(batch=8), dict(beta=1.0), dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan")),
                                dict(beta=1.0 - 1e-20), dict(half_life_images=0, batch=8), dict(half_life_images=100, batch=0),
                                dict(half_life_images=-5, batch=8), dict(half_life_images=float("inf"), batch=8)])
def test_argument_errors(kw):
    from locate_amd import average_weight
    with pytest.raises(ValueError):
        average_weight(**kw)
