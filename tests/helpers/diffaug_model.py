"""Differentiable augmentation (csrc/diffaug.hip, locate_amd/augment.py), stated ONCE, in float64 numpy.

Per image x [3, S, S] and its parameter row (12 fp32 words: b, s, c, ty, tx, y0, y1, x0, x1, 0, 0, 0; the integers exact):
  colour       z[c, p] = c (s (x[c, p] - mu[p]) + mu[p] - M) + M + b,   mu[p] = mean_c x[c, p],   M = mean(x)
  translation  w[c, i, j] = z[c, i - ty, j - tx] inside the frame, exactly 0.0 elsewhere (a gather: nothing is multiplied)
  cutout       y = keep * w,   keep = 0.0 on [y0, y1) x [x0, x1), 1.0 elsewhere (a multiplication: NaN and Inf survive the cut)
  backward     gz[c, p] = keep[p + t] gy[c, p + t] inside the frame, else 0
               gx[c, p] = c s gz[c, p] + c (1 - s) mean_c gz[:, p] + (1 - c) mean(gz)
The colour line is the closed form of the paper's sequence (brightness x + b, saturation about the channel mean, contrast about the
image mean; `colour_sequential`): the saturation step leaves the image mean alone and the offset rides through both.

The policy (bit 0 colour, 1 translation, 2 cutout) is static.  An op that is off is NOT evaluated with identity values: its line is
skipped, so without colour the result is the input's values moved and masked, and the functions below keep the input's dtype
(float32 in, float32 out, bit for bit).

FORWARD_BOUND / BACKWARD_BOUND: per element, a running error bound of the kernels' fp32 evaluation (the operation sequence is
written out in `forward_bound` / `backward_bound`) under the standard model fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-24."""
import numpy as np

PARAM_FLOATS = 12
COLOR, TRANSLATION, CUTOUT = 1, 2, 4
FULL = COLOR | TRANSLATION | CUTOUT
U32 = 2.0 ** -24          # unit roundoff of fp32, round to nearest
U64 = 2.0 ** -53
TINY = 2.0 ** -126          # an fp32 result below the normal range (kept as a subnormal or flushed): an absolute error <= this


def identity_row():
    r = np.zeros(PARAM_FLOATS, np.float32)
    r[1] = r[2] = 1.0
    return r


def make_row(b=0.0, s=1.0, c=1.0, ty=0, tx=0, y0=0, y1=0, x0=0, x1=0):
    return np.array([b, s, c, ty, tx, y0, y1, x0, x1, 0, 0, 0], np.float32)


def shift_bound(S):
    return int(np.floor(S / 8 + 0.5))


def cut_size(S):
    return int(np.floor(S / 2 + 0.5))


def rows_from_uniform(r, S, policy=FULL):
    """the paper's distributions from uniform numbers r float64 [rows, 7] (locate_amd.augment.draw_parameters)"""
    r = np.asarray(r, np.float64)
    out = np.zeros((r.shape[0], PARAM_FLOATS), np.float64)
    out[:, 1] = out[:, 2] = 1.0
    if policy & COLOR:
        out[:, 0], out[:, 1], out[:, 2] = r[:, 0] - 0.5, 2.0 * r[:, 1], r[:, 2] + 0.5
    if policy & TRANSLATION:
        D = shift_bound(S)
        out[:, 3] = np.floor(r[:, 3] * (2 * D + 1)) - D
        out[:, 4] = np.floor(r[:, 4] * (2 * D + 1)) - D
    if policy & CUTOUT:
        cut = cut_size(S)
        for col, k in ((5, 5), (7, 6)):
            o = np.floor(r[:, k] * (S + 1 - cut % 2))
            out[:, col] = np.clip(o - cut // 2, 0, S)
            out[:, col + 1] = np.clip(o - cut // 2 + cut, 0, S)
    return out.astype(np.float32)


def _ints(row):
    return tuple(int(v) for v in np.asarray(row)[3:9])


# ---- the three ops, one image -----------------------------------------------------------------------------------------------------------
def colour(x, row):
    """closed form, float64"""
    x = np.asarray(x, np.float64)
    b, s, c = (float(v) for v in np.asarray(row)[:3])
    mu = x.mean(axis=0, keepdims=True)
    M = x.mean()
    return c * (s * (x - mu) + mu - M) + M + b


def colour_sequential(x, row):
    """the paper's three steps, one after the other, float64"""
    x = np.asarray(x, np.float64)
    b, s, c = (float(v) for v in np.asarray(row)[:3])
    x = x + b                                                  # rand_brightness
    mu = x.mean(axis=0, keepdims=True)
    x = (x - mu) * s + mu                                      # rand_saturation
    M = x.mean()
    return (x - M) * c + M                                     # rand_contrast


def translate(z, ty, tx, adjoint=False):
    """w[c, i, j] = z[c, i - ty, j - tx] inside the frame, 0 elsewhere (adjoint: i + ty, j + tx); the values are MOVED, dtype kept"""
    if adjoint:
        ty, tx = -ty, -tx
    S = z.shape[-1]
    w = np.zeros_like(z)
    i0, i1 = max(0, ty), min(S, S + ty)
    j0, j1 = max(0, tx), min(S, S + tx)
    if i0 < i1 and j0 < j1:
        w[:, i0:i1, j0:j1] = z[:, i0 - ty:i1 - ty, j0 - tx:j1 - tx]
    return w


def keep_mask(S, y0, y1, x0, x1, dtype=np.float64):
    keep = np.ones((S, S), dtype)
    keep[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 0.0
    return keep


def forward_image(x, row, policy=FULL):
    ty, tx, y0, y1, x0, x1 = _ints(row)
    z = colour(x, row) if policy & COLOR else np.asarray(x)
    w = translate(z, ty, tx) if policy & TRANSLATION else z.copy()
    if policy & CUTOUT:
        with np.errstate(invalid="ignore"):
            w = keep_mask(x.shape[-1], y0, y1, x0, x1, w.dtype)[None] * w
    return w


def gz_image(gy, row, policy=FULL):
    ty, tx, y0, y1, x0, x1 = _ints(row)
    g = np.asarray(gy)
    if policy & CUTOUT:
        with np.errstate(invalid="ignore"):
            g = keep_mask(g.shape[-1], y0, y1, x0, x1, g.dtype)[None] * g
    return translate(g, ty, tx, adjoint=True) if policy & TRANSLATION else g.copy()


def backward_image(gy, row, policy=FULL):
    gz = gz_image(gy, row, policy)
    if not policy & COLOR:
        return gz
    gz = gz.astype(np.float64)
    b, s, c = (float(v) for v in np.asarray(row)[:3])
    return c * s * gz + c * (1.0 - s) * gz.mean(axis=0, keepdims=True) + (1.0 - c) * gz.mean()


def forward(x, rows, policy=FULL):
    return np.stack([forward_image(xi, r, policy) for xi, r in zip(x, rows)])


def backward(gy, rows, policy=FULL):
    return np.stack([backward_image(gi, r, policy) for gi, r in zip(gy, rows)])


# ---- error bounds of the kernels' fp32 evaluation ---------------------------------------------------------------------------------------
def _rnd(exact, e_in):
    """error of one fp32 rounding of a quantity whose exact value is `exact` and whose computed operand-side error is e_in: the
    rounded value is within u |computed| + TINY of the computed one, and |computed| <= |exact| + e_in"""
    return e_in + U32 * (np.abs(exact) + e_in) + TINY


def _mean_error(values, mean_exact):
    """M as the kernels form it: a float64 sum of the n fp32 values in some fixed order (n - 1 roundings: |error| <= gamma_(n-1)
    sum|v|, whatever the order), one float64 division by n, one rounding to fp32"""
    n = values.size
    gamma = (n - 1) * U64 / (1.0 - (n - 1) * U64)
    e_sum = gamma * np.abs(values).sum()
    e_div = e_sum / n + U64 * (abs(mean_exact) + e_sum / n)
    return e_div + U32 * (abs(mean_exact) + e_div) + TINY


def _third_error(a):
    """mu = ((a0 + a1) + a2) / 3 in fp32: two additions and a correctly rounded division; a float64 [3, ...], the inputs exact"""
    e1 = _rnd(a[0] + a[1], 0.0)
    e2 = _rnd(a[0] + a[1] + a[2], e1)
    mu = (a[0] + a[1] + a[2]) / 3.0
    return mu, _rnd(mu, e2 / 3.0)


def forward_bound(x, rows, policy=FULL):
    """FORWARD_BOUND: per element of y, a bound of |kernel - forward(x, rows)| for the sequence (csrc/diffaug.hip, da_pixel_fwd)
         mu = ((x0 + x1) + x2) / 3;  d = x - mu;  t = fma(s, d, mu);  t2 = t - M;  Mb = M + b;  z = fma(c, t2, Mb)
    - one rounding each, M as in _mean_error - followed by the gather and the mask, which are exact.  Without colour: 0."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    if not policy & COLOR:
        return out
    for n, (xi, row) in enumerate(zip(x, rows)):
        b, s, c = (float(v) for v in np.asarray(row)[:3])
        ty, tx, y0, y1, x0, x1 = _ints(row)
        M = xi.mean()
        e_M = _mean_error(xi, M)
        mu, e_mu = _third_error(xi)
        d = xi - mu[None]
        e_d = _rnd(d, e_mu[None])
        t = s * d + mu[None]
        e_t = _rnd(t, abs(s) * e_d + e_mu[None])
        t2 = t - M
        e_t2 = _rnd(t2, e_t + e_M)
        e_Mb = _rnd(M + b, e_M)
        z = c * t2 + (M + b)
        e_z = _rnd(z, abs(c) * e_t2 + e_Mb)
        e = translate(e_z, ty, tx) if policy & TRANSLATION else e_z
        if policy & CUTOUT:
            e = keep_mask(x.shape[-1], y0, y1, x0, x1)[None] * e
        out[n] = e
    return out * (1.0 + 2.0 ** -20)          # the float64 evaluation of the bound itself


def backward_bound(gy, rows, policy=FULL):
    """BACKWARD_BOUND: per element of gx, for the sequence (da_colour_bwd, da_pixel_bwd)
         cs = c * s;  oms = 1 - s;  c1s = c * oms;  omc = 1 - c;  k = omc * G          (per image; G = mean(gz) as in _mean_error)
         m = ((gz0 + gz1) + gz2) / 3;  r = fma(c1s, m, k);  gx = fma(cs, gz, r)          (per pixel)
    with gz exact (a mask by 0.0f / 1.0f and a gather).  Without colour: 0."""
    gy = np.asarray(gy, np.float64)
    out = np.zeros_like(gy)
    if not policy & COLOR:
        return out
    for n, (gi, row) in enumerate(zip(gy, rows)):
        b, s, c = (float(v) for v in np.asarray(row)[:3])
        gz = gz_image(gi, row, policy)
        G = gz.mean()
        e_G = _mean_error(gz, G)
        cs, e_cs = c * s, _rnd(c * s, 0.0)
        e_oms = _rnd(1.0 - s, 0.0)
        c1s = c * (1.0 - s)
        e_c1s = _rnd(c1s, abs(c) * e_oms)
        e_omc = _rnd(1.0 - c, 0.0)
        k = (1.0 - c) * G
        e_k = _rnd(k, abs(1.0 - c) * e_G + e_omc * (abs(G) + e_G))
        m, e_m = _third_error(gz)
        r = c1s * m + k
        e_r = _rnd(r, abs(c1s) * e_m + e_c1s * (np.abs(m) + e_m) + e_k)
        gx = cs * gz + r[None]
        out[n] = _rnd(gx, e_cs * np.abs(gz) + e_r[None])
    return out * (1.0 + 2.0 ** -20)
