"""The model of csrc/guard.hip's verdict, in float64 numpy: from the gradients' exact sum of squares and their count of non-finite
elements to {norm, nonfinite, skip, scale} and the running counters - and the global statistics of a list of gradients by
tests/helpers/stats_model.py (the correctly rounded sum of the exact squares of the finite elements)."""
import math

import numpy as np

import stats_model

ZERO = {"steps": 0, "skipped": 0, "clipped": 0, "consecutive_skips": 0, "last_norm": 0.0, "last_scale": 0.0, "last_nonfinite": 0}


def global_statistics(grads):
    """(sumsq: Python float, nonfinite: int, n: int) over a list of float32 arrays"""
    per = [stats_model.statistics(g) for g in grads]
    return math.fsum(s for s, _, _ in per), sum(c for _, _, c in per), sum(int(np.asarray(g).size) for g in grads)


def verdict(sumsq, nonfinite, max_norm=0.0, skip_nonfinite=True, counters=None):
    """One step of the verdict.  Returns (skip: bool, scale: np.float32, counters after the step)."""
    c = dict(counters or ZERO)
    norm = np.sqrt(np.float64(sumsq))
    skip = bool(skip_nonfinite) and nonfinite > 0
    clip = max_norm > 0.0 and norm > max_norm and not skip
    scale = np.float32(np.float64(max_norm) / norm) if clip else np.float32(1.0)
    c["steps"] += 1
    c["skipped"] += int(skip)
    c["clipped"] += int(clip)
    c["consecutive_skips"] = c["consecutive_skips"] + 1 if skip else 0
    c["last_norm"], c["last_scale"], c["last_nonfinite"] = float(norm), float(scale), int(nonfinite)
    return skip, scale, c


def scale_within_one_ulp(got, want):
    """adjacent fp32 values or the same one (both positive and finite)"""
    a, b = (int(np.array([v], dtype=np.float32).view(np.uint32)[0]) for v in (got, want))
    return abs(a - b) <= 1
