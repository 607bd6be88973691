"""The models the run-dynamics tests rest on (tests/helpers/dynamics_model.py), on hand-made cases, and the condition the sigma
fixtures have to meet before a kernel is held to them."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dynamics_model as M  # noqa: E402


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_delta_record_on_hand_made_cases():
    # plain numbers: d = [0, -0.5, 2, 0], squares 0.25 + 4
    assert M.delta_record([1.0, 2.0, 3.0, -4.0], [1.0, 2.5, 1.0, -4.0]) == (4.25, 1.0 + 6.25 + 1.0 + 16.0, np.float32(2.0), 2, 0)
    # zeros of both signs are equal; their delta is zero
    assert M.delta_record(f32([0x00000000, 0x80000000, 0x00000000]), f32([0x80000000, 0x00000000, 0x00000000])) == (0.0, 0.0, np.float32(0.0), 3, 0)
    # the subtraction is fp32: 1 - 2^-30 rounds to 1, so the delta's square is 1 and not (1 - 2^-30)^2
    assert M.delta_record([1.0], [2.0 ** -30]) == (1.0, 2.0 ** -60, np.float32(1.0), 0, 0)
    # a denormal delta is kept: two neighbours at the bottom of the normal range differ by 2^-149
    w, b = f32([0x00800001]), f32([0x00800000])
    dsq, bsq, amax, same, bad = M.delta_record(w, b)
    assert (bits(amax), same, bad) == (1, 0, 0) and dsq == (2.0 ** -149) ** 2 and bsq == (2.0 ** -126) ** 2 and dsq > 0.0
    # finite operands, infinite delta: counted, left out of the delta fields, the base still summed
    dsq, bsq, amax, same, bad = M.delta_record([3e38, 1.0], [-3e38, 0.5])
    assert (dsq, amax, same, bad) == (0.25, np.float32(0.5), 0, 1) and bsq == float(np.float32(3e38)) ** 2 + 0.25
    # Inf - Inf is NaN, yet Inf == Inf: unchanged AND non-finite; an infinite base is left out of base_sumsq
    assert M.delta_record([np.inf, -np.inf, 2.0], [np.inf, -np.inf, 2.0]) == (0.0, 4.0, np.float32(0.0), 3, 2)
    # NaN on either side: never equal, always non-finite; a NaN in w leaves base_sumsq alone
    nan = f32([0x7FC12345])[0]
    assert M.delta_record([nan, 1.0, 5.0], [1.0, nan, 2.0]) == (9.0, 1.0 + 4.0, np.float32(3.0), 0, 2)
    assert M.delta_record([nan], [nan]) == (0.0, 0.0, np.float32(0.0), 0, 1)
    # the largest delta goes by magnitude, and the result carries no sign
    assert M.delta_record([1.0, 1.0], [8.0, -2.0])[2] == np.float32(7.0)
    # empty
    assert M.delta_record([], []) == (0.0, 0.0, np.float32(0.0), 0, 0)


def test_sums_close():
    assert M.sums_close(0.0, 0.0, 5) and not M.sums_close(1e-300, 0.0, 5)
    assert M.sums_close(1.0 + 2.0 ** -51, 1.0, 4) and not M.sums_close(1.0 + 2.0 ** -49, 1.0, 4)


def test_power_iteration_model():
    W = np.diag([3.0, 1.0, 0.5])[:, :3]
    sigma, u, v = M.power_iteration(W, np.ones(3) / np.sqrt(3.0), rounds=40)
    assert abs(sigma - 3.0) < 1e-11 and abs(abs(u[0]) - 1.0) < 1e-11 and abs(abs(v[0]) - 1.0) < 1e-11          # the 1e-12 terms shorten u and v
    # one round from a singular vector stays there and returns its singular value; sigma is never above the top one
    sigma, u, v = M.power_iteration(W, np.array([0.0, 1.0, 0.0]))
    assert abs(sigma - 1.0) < 1e-11 and abs(u[1] - 1.0) < 1e-11
    rng = np.random.default_rng(5)
    A = rng.standard_normal((7, 11))
    top = M.top_singular_value(A)
    previous = 0.0
    for rounds in (1, 2, 4, 8):
        sigma, _, _ = M.power_iteration(A, np.ones(7) / np.sqrt(7.0), rounds)
        assert previous <= sigma * (1 + 1e-12) and sigma <= top * (1 + 1e-12)
        previous = sigma
    # the reference's 1e-12 terms: a zero matrix gives sigma 0, not NaN
    sigma, u, v = M.power_iteration(np.zeros((3, 4)), np.ones(3))
    assert sigma == 0.0 and not np.isnan(u).any() and not np.isnan(v).any()


def test_the_sigma_fixtures_meet_their_condition():
    """What tests/test_gpu_dynamics.py holds the kernels to is only as good as the fixtures: the float64 model alone, started from
    a random unit u, has to be within 1e-7 relative of numpy's SVD after 8 rounds and within 1e-9 after 12."""
    assert M.FIXTURE_SEEDS == (0, 1, 2, 3)
    for seed in M.FIXTURE_SEEDS:
        W, u = M.sigma_fixture(seed)
        assert W.dtype == np.float32 and W.shape == (24, 40) and abs(float(u @ u) - 1.0) < 1e-12
        s = np.linalg.svd(W.astype(np.float64), compute_uv=False)
        assert abs(s[0] - 2.0) < 1e-5 and abs(s[1] - 1.0) < 1e-5 and s[2] < 0.91 and s[-1] > 0.04          # rounded to fp32, not moved
        top = M.top_singular_value(W)
        after8, _, _ = M.power_iteration(W, u, 8)
        after12, _, _ = M.power_iteration(W, u, 12)
        print("seed %d  sigma_1 %.15g  after 8 rounds %.3g  after 12 rounds %.3g" % (seed, top, abs(after8 - top) / top, abs(after12 - top) / top))
        assert abs(after8 - top) <= 1e-7 * top and abs(after12 - top) <= 1e-9 * top
        assert after8 <= top * (1 + 1e-12) and after12 <= top * (1 + 1e-12)          # a lower bound
