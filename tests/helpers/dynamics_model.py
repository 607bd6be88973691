"""The model of csrc/dynamics.hip - per tensor, with d = w - base as ONE float32 subtraction: the correctly rounded sums of the exact
squares of the finite d and of the finite base elements, the largest finite |d| by its bit pattern, the count of w == base and the
count of non-finite d - and a float64 model of the spectral norm's power iteration (libs/spectral_norm.py:26-32, with the
reference's 1e-12 terms) with the fixtures the sigma tests share."""
import math

import numpy as np

from stats_model import finite_mask, magnitude_bits, sumsq_tolerance


def delta_record(w, base):
    """(delta_sumsq: Python float, base_sumsq: Python float, delta_absmax: np.float32, unchanged: int, nonfinite: int).  The square
    of an fp32 value is exact in float64 and math.fsum returns the correctly rounded sum of exact terms; numpy's float32
    subtraction is the IEEE one, denormals kept."""
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    base = np.ascontiguousarray(base, dtype=np.float32).reshape(-1)
    assert w.shape == base.shape
    with np.errstate(over="ignore", invalid="ignore"):
        d = w - base          # float32
        unchanged = int((w == base).sum())          # +0 == -0, Inf == Inf; a NaN equals nothing
    dfin, bfin = finite_mask(d), finite_mask(base)
    dd, bb = d[dfin].astype(np.float64), base[bfin].astype(np.float64)
    mag = magnitude_bits(d)
    absmax = np.array([mag[dfin].max() if dfin.any() else 0], dtype=np.uint32).view(np.float32)[0]
    return math.fsum((dd * dd).tolist()), math.fsum((bb * bb).tolist()), absmax, unchanged, int((~dfin).sum())


def sums_close(got, want, n):
    """stats_model.sumsq_tolerance(n) bounds a float64 sum of n exact non-negative terms in any order: derived, not measured"""
    if want == 0.0:
        return got == 0.0
    return abs(got - want) <= sumsq_tolerance(n) * want


def power_iteration(W, u, rounds=1):
    """`rounds` rounds of  t = W^T u; v = t / (|t| + 1e-12); s = W v; u = s / (|s| + 1e-12); sigma = u . (W v)  in float64;
    returns (sigma of the last round, u, v)"""
    W = np.asarray(W, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    v = sigma = None
    for _ in range(rounds):
        t = W.T @ u
        v = t / (np.sqrt((t * t).sum()) + 1e-12)
        s = W @ v
        u = s / (np.sqrt((s * s).sum()) + 1e-12)
        sigma = float(u @ (W @ v))
    return sigma, u, v


FIXTURE_SEEDS = (0, 1, 2, 3)
FIXTURE_SHAPE = (24, 40)


def sigma_fixture(seed):
    """(W float32 [24, 40] = U diag(s) V^T with s = [2, 1, uniform(0.05, 0.9) ...] rounded to fp32, a random unit u float64 [24]):
    a ratio of 2 between the first two singular values, so every round of the power iteration gains a factor 4 on the vectors'
    error and 16 on sigma's"""
    rng = np.random.default_rng(seed)
    h, wd = FIXTURE_SHAPE
    U, _ = np.linalg.qr(rng.standard_normal((h, h)))
    V, _ = np.linalg.qr(rng.standard_normal((wd, h)))
    s = np.concatenate([[2.0, 1.0], rng.uniform(0.05, 0.9, size=h - 2)])
    W = ((U * s) @ V.T).astype(np.float32)
    u = rng.standard_normal(h)
    return W, u / np.sqrt((u * u).sum())


def top_singular_value(W):
    return float(np.linalg.svd(np.asarray(W, dtype=np.float64), compute_uv=False)[0])
