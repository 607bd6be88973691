"""The model of csrc/stats.hip: per tensor the correctly rounded sum of the exact squares of the finite elements, the largest
finite magnitude by its bit pattern, and the count of elements whose exponent field is all ones - and the bound the kernel's
`sumsq` is held to."""
import math

import numpy as np


def magnitude_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)


def finite_mask(x):
    """exponent field not all ones: neither NaN (either sign, any payload) nor +-Inf"""
    return magnitude_bits(x) < np.uint32(0x7F800000)


def statistics(x):
    """(sumsq: Python float, absmax: np.float32, nonfinite: int) of a float32 array.  The square of an fp32 value has at most 48
    significant bits and an exponent of at least -298, so it is exact in float64; math.fsum returns the correctly rounded sum of
    those exact terms."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    mag, fin = magnitude_bits(x), finite_mask(x)
    d = x[fin].astype(np.float64)
    sumsq = math.fsum((d * d).tolist())
    absmax = np.array([mag[fin].max() if fin.any() else 0], dtype=np.uint32).view(np.float32)[0]
    return sumsq, absmax, int((~fin).sum())


def sumsq_tolerance(n):
    """Relative bound on a float64 sum of n exactly known non-negative terms added in ANY order: every partial sum carries a
    relative error of at most gamma_(n-1) = (n - 1) u / (1 - (n - 1) u) with u = 2^-53 (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2; the terms are non-negative, so the condition number of the sum is 1).  n * 2^-52 is twice
    that, which also covers the model's own final rounding.  Derived, not measured."""
    return n * 2.0 ** -52


def sumsq_close(got, want, n):
    if want == 0.0:
        return got == 0.0
    return abs(got - want) <= sumsq_tolerance(n) * want
