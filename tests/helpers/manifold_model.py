"""Numpy model of locate_amd/manifold.py and the within kernels of csrc/neighbours.hip: brute-force int64 distances and top-k from
neighbours_model, the counts of pairs inside a radius, the k-th-neighbour radii, the four metrics from their definitions and the
record that `ManifoldMetrics.between` returns.  Integers throughout: the GPU tests compare with ==."""
import numpy as np

import neighbours_model as N

distances = N.distances


def within(d2, radius2, qflags=None, rflags=None, skip=None):
    """(hits int32 [Q], covered int32 [N]): the pair (i, j) counts iff query i and reference j are not flagged, radius2[j] >= 0,
    j != skip[i] and d2[i, j] <= radius2[j]; hits are the row sums, covered the column sums"""
    Q, n = d2.shape
    radius2 = np.asarray(radius2, dtype=np.int64)
    ok = (d2 <= radius2[None, :]) & (radius2 >= 0)[None, :]
    if qflags is not None:
        ok &= (np.asarray(qflags) == 0)[:, None]
    if rflags is not None:
        ok &= (np.asarray(rflags) == 0)[None, :]
    if skip is not None:
        ok &= np.arange(n)[None, :] != np.asarray(skip)[:, None]
    return ok.sum(1).astype(np.int32), ok.sum(0).astype(np.int32)


def kth_radius(x, k):
    """int64 [n]: each row's squared distance to its k-th nearest OTHER row of the triple x; -1 for a flagged row or when fewer than
    k others exist"""
    d2, _ = N.nearest(x, x, k, skip=np.arange(len(x[1])))
    return d2[:, k - 1].copy()


def counts(g, r, k):
    """{"precise", "recalled", "hit_sum", "covered"} of the fake triple g against the real triple r"""
    rad_r, rad_g = kth_radius(r, k), kth_radius(g, k)
    hits_g, cov_r = within(distances(g[0], r[0]), rad_r, g[2], r[2])
    hits_r, _ = within(distances(r[0], g[0]), rad_g, r[2], g[2])
    return {"precise": int((hits_g > 0).sum()), "recalled": int((hits_r > 0).sum()), "hit_sum": int(hits_g.sum()),
            "covered": int((cov_r > 0).sum())}


def metrics(c, m, n, k):
    return {"precision": c["precise"] / m, "recall": c["recalled"] / n, "density": c["hit_sum"] / (k * m), "coverage": c["covered"] / n}


def triple(codes):
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    return codes, N.norms(codes), np.zeros(codes.shape[0], np.int32)


def between(g, r, k, baseline=None):
    """the record of the fake triple g against the real triple r"""
    m, n = len(g[1]), len(r[1])
    c = counts(g, r, k)
    value = {"images": m, "real_images": n, "k": k, "counts": c}
    value.update(metrics(c, m, n, k))
    value["nonfinite"] = int((g[2] != 0).sum())
    value["baseline"] = baseline
    return value


def baseline(second, r, k):
    """the four metrics and the counts of a second real triple against the first"""
    value = between(second, r, k)
    return {key: value[key] for key in ("precision", "recall", "density", "coverage", "counts")}


def record(fake, real, k, baseline=None):
    """what ManifoldMetrics.between returns for float32 images fake [m, 3, S, S] against real [n, 3, S, S]"""
    return between(N.encode(fake), N.encode(real), k, baseline)
