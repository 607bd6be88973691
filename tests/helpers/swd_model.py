"""A float64 numpy restatement of the sliced Wasserstein metric (locate_amd/metric.py, csrc/swd.hip): the yardstick of
tests/test_gpu_swd.py, itself held to facts outside it by tests/test_swd_model.py (scipy's mirrored convolution, exact
invariances, a closed-form limit).  fp32 inputs are taken as exact and converted to float64.

  pyramid     g = outer([1,4,6,4,1], [1,4,6,4,1]) / 256; borders mirrored without repeating the edge sample;
              down(x)[i, j] = sum_ab g[a, b] x[m(2i + a - 2), m(2j + b - 2)]; up(y) = y written into the even positions of a zero
              map of twice the size, convolved with 4 g; level l < L - 1 is G_l - up(G_{l+1}), level L - 1 is G_{L-1}
  descriptors element k = c 49 + dy 7 + dx of descriptor j is level[j // P, c, y_j + dy, x_j + dx]
  stats       per channel the mean and the population deviation over all n 49 gathered values; returned as the fp32 roundings of
              the float64 mu and 1 / sigma, which is what everything downstream uses
  projection  proj[d, j] = sum_k dirs[k, d] (v_jk - mu_c) r_c
  distance    per repeat: every direction's projections of both sets sorted, the mean of |sortA - sortB|; a level's value is the
              mean over the repeats"""
import numpy as np

PATCH = 7
K = 3 * PATCH * PATCH
W5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
U24 = 2.0 ** -24
# a Laplacian level in fp32: two chained stencils of <= 25 products with exact weights (25 2^-24 each) and a subtraction
LEVEL_ERR = 3.2e-6


def mirror(i, n):
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(x, scale=1.0):
    """the 5 x 5 filter g * scale at every position of [..., H, W], mirrored"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    rows = sum(W5[a] * x[..., mirror(np.arange(H) + a - 2, H), :] for a in range(5))
    return sum(W5[b] * rows[..., :, mirror(np.arange(W) + b - 2, W)] for b in range(5)) * (scale / 256.0)


def down(x):
    return blur(x)[..., ::2, ::2]


def up(y):
    y = np.asarray(y, np.float64)
    z = np.zeros(y.shape[:-2] + (2 * y.shape[-2], 2 * y.shape[-1]))
    z[..., ::2, ::2] = y
    return blur(z, 4.0)


def pyramid_levels(S, min_size=16):
    sizes = [S]
    while sizes[-1] > min_size:
        sizes.append(sizes[-1] // 2)
    return sizes


def laplacian_pyramid(x, levels=None):
    x = np.asarray(x, np.float64)
    count = len(pyramid_levels(x.shape[-1])) if levels is None else levels
    out, g = [], x
    for _ in range(count - 1):
        coarse = down(g)
        out.append(g - up(coarse))
        g = coarse
    out.append(g)
    return out


def pyr_bound(x):
    """absolute bound on every level of the fp32 pyramid of x: 25 2^-24 max|x| = 1.5e-6 per stencil, 3.2e-6 for a level, margin 3"""
    return 1e-5 * float(np.abs(np.asarray(x, np.float64)).max())


def descriptors(level, pos, P):
    """[n, 147] float64: the gathered values"""
    level = np.asarray(level, np.float64)
    pos = np.asarray(pos).astype(np.int64)
    n = pos.shape[0]
    assert n == level.shape[0] * P
    img = np.arange(n) // P
    dy, dx = np.meshgrid(np.arange(PATCH), np.arange(PATCH), indexing="ij")
    yy = pos[:, 0, None, None] + dy          # [n, 7, 7]
    xx = pos[:, 1, None, None] + dx
    v = level[img[:, None, None, None], np.arange(3)[None, :, None, None], yy[:, None], xx[:, None]]          # [n, 3, 7, 7]
    return v.reshape(n, K)


def stats64(desc):
    """(mu [3], sigma [3]) in float64 over all n 49 values of each channel"""
    v = desc.reshape(desc.shape[0], 3, PATCH * PATCH)
    return v.mean(axis=(0, 2)), v.std(axis=(0, 2))


def stats(desc):
    """fp32 [6]: the roundings of mu and 1 / sigma"""
    mu, sigma = stats64(desc)
    return np.concatenate([mu, 1.0 / sigma]).astype(np.float32)


def normalised(desc, st):
    st = np.asarray(st, np.float64)
    mu, r = np.repeat(st[:3], PATCH * PATCH), np.repeat(st[3:], PATCH * PATCH)
    return (desc - mu) * r


def project(desc, dirs, st):
    """[D, n] float64"""
    return np.asarray(dirs, np.float64).T @ normalised(desc, st).T


def proj_bound(desc, dirs, st):
    """[D, n]: (147 + 4) 2^-24 sum_k |dirs_kd| |v_jk - mu_c| r_c - the dot product of 147 fp32 terms, the subtraction, the scaling"""
    return (K + 4) * U24 * (np.abs(np.asarray(dirs, np.float64)).T @ np.abs(normalised(desc, st)).T)


def stats_slack(desc, dirs, st):
    """[D, n]: 2^-23 sum_k |dirs_kd| (|mu_c| + |v_jk - mu_c|) r_c - what a one-ulp disagreement on mu and r explains"""
    st = np.asarray(st, np.float64)
    mu, r = np.repeat(st[:3], PATCH * PATCH), np.repeat(st[3:], PATCH * PATCH)
    return 2.0 ** -23 * (np.abs(np.asarray(dirs, np.float64)).T @ ((np.abs(mu) + np.abs(desc - mu)) * r).T)


def level_slack(dirs, st, max_abs):
    """[D]: sum_k |dirs_kd| r_c 3.2e-6 max|x| - what the fp32 pyramid's error on a level explains in a projection"""
    r = np.repeat(np.asarray(st, np.float64)[3:], PATCH * PATCH)
    return (np.abs(np.asarray(dirs, np.float64)) * r[:, None]).sum(0) * LEVEL_ERR * max_abs


def sliced_distance(pa, pb):
    """mean |sort(pa) - sort(pb)| for two [D, n] projection sets"""
    return float(np.abs(np.sort(pa, axis=1) - np.sort(pb, axis=1)).mean())


def swd_descriptors(da, db, dirs, repeats):
    """one level's value from descriptors given directly ([n, 147] each): normalise each set, project, sort, compare per repeat"""
    dirs = np.asarray(dirs, np.float64)
    Dr = dirs.shape[1] // repeats
    sa, sb = stats(da), stats(db)
    vals = [sliced_distance(project(da, dirs[:, r * Dr:(r + 1) * Dr], sa), project(db, dirs[:, r * Dr:(r + 1) * Dr], sb)) for r in range(repeats)]
    return sum(vals) / repeats


def swd(a, b, pos_a, pos_b, P, dirs, repeats, with_bound=False):
    """{"levels", "mean"} for image sets a, b [N, 3, S, S]; pos_a / pos_b: per level int [N P, 2].  with_bound: also "bound", per
    level 2 max_dj(proj_bound + stats_slack + level_slack) over both sets - the 1-Wasserstein distance of sorted samples moves by
    at most the sup-norm perturbation of each set."""
    la, lb = laplacian_pyramid(a), laplacian_pyramid(b)
    levels, bounds = [], []
    for l in range(len(la)):
        da, db = descriptors(la[l], pos_a[l], P), descriptors(lb[l], pos_b[l], P)
        levels.append(swd_descriptors(da, db, dirs, repeats))
        if with_bound:
            worst = 0.0
            for d, x in ((da, a), (db, b)):
                st = stats(d)
                per = proj_bound(d, dirs, st) + stats_slack(d, dirs, st) + level_slack(dirs, st, float(np.abs(x).max()))[:, None]
                worst = max(worst, float(per.max()))
            bounds.append(2.0 * worst)
    out = {"levels": levels, "mean": sum(levels) / len(levels)}
    if with_bound:
        out["bound"] = bounds
    return out
