"""Numpy int64 model of locate_amd/modes.py and csrc/modes.hip: group sums by a loop over the groups, the rounded mean by Python's
floor division, Lloyd's algorithm over neighbours_model's nearest (lower-index ties, flags), and the proportion test of NDB with
math and fractions of Python integers.  Integers throughout: the GPU tests compare with ==."""
import math
from statistics import NormalDist

import numpy as np

import neighbours_model as NM


def clamp(v, M):
    return min(max(int(v), 0), int(M))


def group_sums(codes, order, starts, K):
    """int64 [K, row_bytes]: group k is order[clamp(starts[k]) : clamp(starts[k + 1])], clamped to 0 .. M = len(order); an index
    outside 0 .. N - 1 adds nothing"""
    codes, order = np.asarray(codes), np.asarray(order, dtype=np.int64)
    N, M = codes.shape[0], order.shape[0]
    wide = codes.astype(np.int64)
    out = np.zeros((K, codes.shape[1]), dtype=np.int64)
    for k in range(K):
        lo, hi = clamp(starts[k], M), clamp(starts[k + 1], M)
        if hi > lo:
            idx = order[lo:hi]
            out[k] = wide[idx[(idx >= 0) & (idx < N)]].sum(0)
    return out


def group_sizes(starts, K, M):
    return [max(clamp(starts[k + 1], M) - clamp(starts[k], M), 0) for k in range(K)]


def centroids(sums, starts, M, previous):
    """(codes int8 [K, row_bytes], norms int64 [K], moved int64 [K]): floor((2 s + n) / (2 n)) per byte - numpy's // floors - and
    previous[k] for an empty group"""
    sums, previous = np.asarray(sums, dtype=np.int64), np.asarray(previous, dtype=np.int8)
    K = sums.shape[0]
    codes = previous.copy()
    for k, n in enumerate(group_sizes(starts, K, M)):
        if n > 0:
            q = (2 * sums[k] + n) // (2 * n)
            assert q.min() >= -128 and q.max() <= 127
            codes[k] = q
    return codes, NM.norms(codes), (codes != previous).sum(1).astype(np.int64)


def grouping(labels, K):
    """(order, starts) of a stable sort of the labels: starts[k] = the labels below k"""
    labels = np.asarray(labels, dtype=np.int64)
    order = np.argsort(labels, kind="stable")
    return order, np.searchsorted(labels[order], np.arange(K + 1), side="left")


def lloyd(x, initial, iterations):
    """x: a (codes, norms, flags) numpy triple; initial: the rows the centres start from.  Returns (centres int8 [K, row_bytes],
    labels int64 [N] (-1: flagged), counts int64 [K], inertia [iterations + 1] of Python ints, moved int64 [iterations, K])"""
    codes, _, flags = x
    K, N = len(initial), codes.shape[0]
    centres = codes[np.asarray(initial)].copy()
    inertia, moved = [], np.zeros((iterations, K), dtype=np.int64)
    for i in range(iterations + 1):
        d2, index = NM.nearest(x, (centres, NM.norms(centres), np.zeros(K, np.int32)), 1)
        labels = index[:, 0].astype(np.int64)
        inertia.append(int(d2[labels >= 0, 0].sum()))
        if i == iterations:
            break
        order, starts = grouping(labels, K)
        centres, _, moved[i] = centroids(group_sums(codes, order, starts, K), starts, N, centres)
    counts = np.array([(labels == k).sum() for k in range(K)], dtype=np.int64)
    return centres, labels, counts, inertia, moved


def ndb_statistics(real_counts, fake_counts, alpha=0.05):
    r, f = [int(v) for v in real_counts], [int(v) for v in fake_counts]
    K, n, m = len(r), sum(r), sum(f)
    if n == 0 or m == 0:
        return {"ndb": None, "ndb_over_k": None, "js": None, "missing": None, "z": None, "different": None, "order": list(range(K))}
    critical = NormalDist().inv_cdf(1 - alpha / 2)
    z = []
    for k in range(K):
        p, q, pooled = r[k] / n, f[k] / m, (r[k] + f[k]) / (n + m)
        se = math.sqrt(pooled * (1 - pooled) * (1 / n + 1 / m))
        z.append(0.0 if se == 0 else (q - p) / se)
    different = [abs(v) > critical for v in z]

    def kl(a, total_a, b, total_b):          # KL(a / total_a || mean of the two histograms)
        return sum(a[k] / total_a * math.log((a[k] / total_a) / ((a[k] / total_a + b[k] / total_b) / 2)) for k in range(K) if a[k] > 0)
    return {"ndb": sum(different), "ndb_over_k": sum(different) / K, "js": (kl(r, n, f, m) + kl(f, m, r, n)) / 2,
            "missing": sum(1 for k in range(K) if different[k] and f[k] == 0), "z": z, "different": different,
            "order": [k for _, k in sorted((z[k], k) for k in range(K))]}


def converged_at(moved):
    """the first round, counted from 1, that moved no centre, else None"""
    still = [i + 1 for i in range(len(moved)) if not np.asarray(moved[i]).any()]
    return still[0] if still else None


def bin_counts(q, centres):
    """(fake_counts [K], nonfinite) of the numpy triple q against the centre rows"""
    K = centres.shape[0]
    _, index = NM.nearest(q, (centres, NM.norms(centres), np.zeros(K, np.int32)), 1)
    return [int((index[:, 0] == k).sum()) for k in range(K)], int((index[:, 0] < 0).sum())


def record(q, centres, real_counts, alpha, kmeans, baseline):
    """what BinnedModes.between returns for the encoded samples q"""
    fake_counts, nonfinite = bin_counts(q, centres)
    stats = ndb_statistics(real_counts, fake_counts, alpha)
    value = {"bins": centres.shape[0], "images": int(sum(real_counts)), "samples": int(q[0].shape[0]), "alpha": alpha,
             "real_counts": [int(v) for v in real_counts], "fake_counts": fake_counts, "nonfinite": nonfinite, "kmeans": kmeans,
             "baseline": baseline}
    value.update(stats)
    return value
