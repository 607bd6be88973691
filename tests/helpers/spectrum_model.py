"""float64 model of the radial power spectrum (locate_amd/spectrum.py, csrc/spectrum.hip).  The definition, stated once:

  tables   C[k][j] = cos(2 pi ((k j) mod S) / S) w[j], Sn likewise with sin: float64, rounded once to fp32; the exact 0 and +-1 where
           (k j) mod S is a multiple of S / 4.  w = 1 ("none") or the periodic Hann window scaled to sum w^2 = S ("hann").
  stage 1  Ar[y][k] = sum_x x[y][x] C[k][x], Ai[y][k] = - sum_x x[y][x] Sn[k][x], k = 0 .. H = S / 2
  stage 2  Yr[a][k] = sum_y C[a][y] Ar[y][k] + Sn[a][y] Ai[y][k], Yi[a][k] = sum_y C[a][y] Ai[y][k] - Sn[a][y] Ar[y][k], a = 0 .. S - 1
  power    (Yr^2 + Yi^2) m[k] / S^4, m = 1 for k in {0, H}, 2 otherwise
  bins     fy = a for a <= H else a - S; d = 4 (fy^2 + k^2); r = the smallest integer with d < (2 r + 1)^2; R = max r + 1
  spectrum[r] = the sum of the powers of bin r

The model computes with the fp32 TABLES (cast to float64), as the kernel does: table rounding is outside the error budget.
Any S that is a multiple of 4 is accepted here (the package takes 32, 64, 128, 256)."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    """the standard dot-product constant n u / (1 - n u) for fp32"""
    return n * U / (1.0 - n * U)


def window(S, name="none"):
    if name == "none":
        return np.ones(S)
    if name != "hann":
        raise ValueError(name)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(S) / S)
    return w * np.sqrt(S / (w * w).sum())


def tables(S, name="none"):
    j = np.arange(S, dtype=np.int64)
    kj = np.outer(j, j) % S
    q = S // 4
    ang = 2 * np.pi * kj / S
    c, s = np.cos(ang), np.sin(ang)
    m = kj % q == 0
    c[m] = np.array([1.0, 0.0, -1.0, 0.0])[(kj[m] // q) % 4]
    s[m] = np.array([0.0, 1.0, 0.0, -1.0])[(kj[m] // q) % 4]
    w = window(S, name)
    return (c * w[None]).astype(np.float32), (s * w[None]).astype(np.float32)


def bins(S):
    """(bin int64 [S, H + 1], m int64 [S, H + 1]) by the definition itself: a search over r, no square root"""
    H = S // 2
    a = np.arange(S)
    fy = np.where(a <= H, a, a - S)
    d = 4 * (fy[:, None] ** 2 + np.arange(H + 1)[None] ** 2)
    r = np.zeros_like(d)
    while True:
        short = d >= (2 * r + 1) ** 2
        if not short.any():
            break
        r = r + short
    m = np.where((np.arange(H + 1) == 0) | (np.arange(H + 1) == H), 1, 2)[None].repeat(S, 0)
    return r, m


def multiplicity(S):
    r, m = bins(S)
    return np.bincount(r.ravel(), weights=m.ravel()).astype(np.int64)


def dft(x, tabs, dtype=np.float64):
    """(Yr, Yi) [p, S, H + 1]; dtype = np.float32 makes numpy's fp32 matmul stand in for the kernel"""
    C, Sn = (t.astype(dtype) for t in tabs)
    x = np.asarray(x).astype(dtype)
    H = x.shape[-1] // 2
    Ar = x @ C[:H + 1].T
    Ai = -(x @ Sn[:H + 1].T)
    Ai[..., 0] = 0          # rows 0 and H of Sn are exact zeros (multiples of S / 4): these two columns are zero already for
    Ai[..., H] = 0          # finite x, and the kernel never forms them
    Yr = np.einsum("ay,pyk->pak", C, Ar) + np.einsum("ay,pyk->pak", Sn, Ai)
    Yi = np.einsum("ay,pyk->pak", C, Ai) - np.einsum("ay,pyk->pak", Sn, Ar)
    return Yr, Yi


def per_bin(P, S):
    """[p, S, H + 1] -> [p, R]: sums per bin"""
    r, _ = bins(S)
    R = int(r.max()) + 1
    return np.stack([np.bincount(r.ravel(), weights=p.ravel(), minlength=R) for p in P])


def spectrum_of(Yr, Yi, S):
    _, m = bins(S)
    return per_bin((Yr.astype(np.float64) ** 2 + Yi.astype(np.float64) ** 2) * m / float(S) ** 4, S)


def spectrum(x, tabs):
    """float64 [p, R] for x [p, S, S]"""
    x = np.asarray(x)
    Yr, Yi = dft(x, tabs)
    return spectrum_of(Yr, Yi, x.shape[-1])


def spectrum_bound(x, tabs):
    """[p, R]: what |fp32 result - model| may be, bin by bin, for ANY summation order - derived, not measured.  With the standard
    bound |fl(sum_n a_i b_i) - sum a_i b_i| <= gamma_n sum |a_i b_i|, u = 2^-24:
      stage 1: e1r = gamma_S sum_x |x| |C|, e1i = gamma_S sum_x |x| |Sn|;
      stage 2, a dot product of 2 S terms on operands that carry e1 (the + 2: the terms the kernel may add at the end when it
      keeps partial sums): e = sum_y |T1| e1a + |T2| e1b + gamma_{2S+2} sum_y |T1| (|A1| + e1a) + |T2| (|A2| + e1b);
      power: |(Y + d)^2 - Y^2| <= (2 |Y| + e) e per component, times m / S^4; summed per bin."""
    x = np.asarray(x).astype(np.float64)
    S = x.shape[-1]
    H = S // 2
    C, Sn = (t.astype(np.float64) for t in tabs)
    aC, aS, ax = np.abs(C), np.abs(Sn), np.abs(x)
    e1r, e1i = gamma(S) * (ax @ aC[:H + 1].T), gamma(S) * (ax @ aS[:H + 1].T)
    Ar, Ai = np.abs(x @ C[:H + 1].T), np.abs(x @ Sn[:H + 1].T)
    for t in (e1i, Ai):          # columns 0 and H of Ai are never formed
        t[..., 0] = 0
        t[..., H] = 0

    def stage2(A1, e1a, A2, e1b):
        carried = np.einsum("ay,pyk->pak", aC, e1a) + np.einsum("ay,pyk->pak", aS, e1b)
        return carried + gamma(2 * S + 2) * (np.einsum("ay,pyk->pak", aC, A1 + e1a) + np.einsum("ay,pyk->pak", aS, A2 + e1b))

    er, ei = stage2(Ar, e1r, Ai, e1i), stage2(Ai, e1i, Ar, e1r)
    Yr, Yi = dft(x, tabs)
    _, m = bins(S)
    return per_bin(((2 * np.abs(Yr) + er) * er + (2 * np.abs(Yi) + ei) * ei) * m / float(S) ** 4, S)


def summary(spectra, S):
    """spectra float64 [n, C, R] -> (sum [C, R], sumsq [C, R], nonfinite [C]) of spectra / multiplicity over the finite planes"""
    v = np.asarray(spectra, dtype=np.float64) / multiplicity(S)[None, None]
    finite = np.isfinite(spectra).all(axis=2)          # [n, C]
    v = np.where(finite[:, :, None], v, 0.0)
    return v.sum(axis=0), (v * v).sum(axis=0), (~finite).sum(axis=0)
