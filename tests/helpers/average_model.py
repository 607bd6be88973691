"""Host models of the averaged generator's update (csrc/average.hip): the numpy float32 model that reproduces the kernel bit for bit -
three operations, each rounded once, and an exact copy where the weight is 1 - and the float64 average it is measured against."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def update32(avg, src, one_minus_beta):
    """one update of a float32 array towards a float32 array; the arrays' own dtype keeps every operation in fp32"""
    assert avg.dtype == np.float32 and src.dtype == np.float32
    w = np.float32(one_minus_beta)
    if w == np.float32(1.0):
        return src.copy()
    d = src - avg
    d = w * d
    return avg + d


def update64(avg, src, one_minus_beta):
    """the same step in float64, with the weight the kernel uses (1 - beta as rounded to fp32)"""
    return avg + float(np.float32(one_minus_beta)) * (src.astype(np.float64) - avg)


def bound(T, one_minus_beta, max_abs):
    """|float32 model - float64| after T updates.  One update rounds three times: the difference (|src - avg| <= 2 max, passed on
    times w), the product (<= 2 w max) and the sum (<= max) - at most (1 + 4 w) u max in all; every later update multiplies an
    error by beta = 1 - w, so T updates collect at most min(T, 1 / w) of them."""
    w = float(np.float32(one_minus_beta))
    return (1.0 + 4.0 * w) * min(float(T), 1.0 / w) * U * float(max_abs)
