"""The statistics model (tests/helpers/stats_model.py) against exact rational arithmetic."""
import math
import os
import struct
import sys
from fractions import Fraction

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stats_model as M  # noqa: E402

# denormals (smallest, largest, one of either sign), +-0, +-Inf, NaNs of both signs with payloads (quiet and signalling), 3e38
BITS = [0x00000001, 0x807FFFFF, 0x00400000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001, 0x7F800001,
        0xFF8ABCDE, 0x3F800000, 0xC0490FDB, 0x7F61B1E6, 0xFF61B1E6, 0x00800000, 0x3EAAAAAB]


def values():
    x = np.array(BITS, dtype=np.uint32).view(np.float32)
    assert x[13] == np.float32(3e38) and x[14] == -np.float32(3e38)
    return x


def exact(x):
    """the same three numbers from Python's own view of every value"""
    total, largest, bad = Fraction(0), Fraction(0), 0
    for b in np.ascontiguousarray(x).view(np.uint32).tolist():
        v = struct.unpack("<f", struct.pack("<I", b))[0]
        if math.isnan(v) or math.isinf(v):
            bad += 1
            continue
        f = Fraction(v)          # exact
        total += f * f
        largest = max(largest, abs(f))
    return total, largest, bad


def test_model_against_fractions():
    x = values()
    total, largest, bad = exact(x)
    sumsq, absmax, nonfinite = M.statistics(x)
    assert bad == 6 and nonfinite == 6
    assert sumsq == float(total)          # int / int division is correctly rounded: so is fsum
    assert Fraction(float(absmax)) == largest and float(absmax) == float(np.float32(3e38))
    assert absmax.dtype == np.float32


def test_subsets_and_edge_cases():
    x = values()
    for sel in ([0, 1, 2], [3, 4], [5, 6], [7, 8, 9, 10], [0, 3, 7], [13, 14, 11], [15, 0], list(range(len(BITS)))[::-1]):
        part = x[sel]
        total, largest, bad = exact(part)
        sumsq, absmax, nonfinite = M.statistics(part)
        assert (sumsq, Fraction(float(absmax)), nonfinite) == (float(total), largest, bad), sel
    # denormals are not flushed: their squares are tiny but not zero
    s, a, c = M.statistics(x[[0, 1, 2]])
    assert s > 0.0 and a == x[1] * -1 and c == 0
    assert float(Fraction(float(x[0])) ** 2) == 2.0 ** -298
    # +-0, all non-finite, empty
    assert M.statistics(x[[3, 4]]) == (0.0, np.float32(0), 0)
    assert M.statistics(x[[5, 6, 7, 8]]) == (0.0, np.float32(0), 4)
    assert M.statistics(np.zeros(0, np.float32)) == (0.0, np.float32(0), 0)
    # squares that overflow fp32 are exact in float64
    assert M.statistics(x[[13]])[0] == float(Fraction(float(x[13])) ** 2) > 3.4e38 ** 2 / 2
    # small integers: exact
    k = np.arange(-8, 9, dtype=np.float32)
    assert M.statistics(np.tile(k, 1000))[0] == 1000.0 * float((k.astype(np.float64) ** 2).sum())


def test_masks_and_tolerance():
    x = values()
    fin = M.finite_mask(x)
    assert fin.tolist() == [b & 0x7F800000 != 0x7F800000 for b in BITS]
    assert M.magnitude_bits(x).tolist() == [b & 0x7FFFFFFF for b in BITS]
    assert M.sumsq_tolerance(4096) == 4096 * 2.0 ** -52
    assert M.sumsq_close(0.0, 0.0, 5) and not M.sumsq_close(1e-300, 0.0, 5)
    assert M.sumsq_close(1.0 + 2.0 ** -52, 1.0, 1) and not M.sumsq_close(1.0 + 2.0 ** -50, 1.0, 2)
