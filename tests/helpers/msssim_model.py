"""The definition of the multi-scale SSIM of locate_amd/msssim.py (csrc/msssim.hip), in float64 numpy.  Wang, Simoncelli, Bovik
2003, "Multi-scale structural similarity for image quality assessment"; used between pairs of generated images by Odena et al. 2017
and Karras et al. 2018 (table 1).

Domain.  Images are in the 8-bit domain of `locate_amd.neighbours.encode_images`: value u = code + 128, 0 .. 255, dynamic range
L = 255; a code row is in c, y, x order.  S in {32, 64, 128, 256}; five levels l = 0 .. 4 of side S_l = S >> l.

Downsampling.  Level l + 1 is the plain 2 x 2 mean of level l (the published implementations' box filter gives the same at even
sizes).  Level-l values are multiples of 4^-l below 256: at most 16 significant bits, exact in fp32; their pairwise products have at
most 32: exact in float64.

Window.  n_l = min(11, S_l) taps, sigma_l = 1.5 n_l / 11, g[j] = exp(-t_j^2 / (2 sigma_l^2)) at t_j = j - (n_l - 1) / 2, divided by
their sum - an even window is centred between pixels.  `window_taps(S)`: float64 [5, 11], zero padded.  The 2-D window is the outer
product; filtering is "valid": o_l = S_l - n_l + 1 outputs per side, rows first, then columns.

Per level, channel and output pixel: mx, my, exx, eyy, exy are the filtered x, y, x^2, y^2, x y; sxx = exx - mx^2, syy = eyy - my^2,
sxy = exy - mx my; C1 = (0.01 L)^2, C2 = (0.03 L)^2; v1 = 2 sxy + C2, v2 = sxx + syy + C2; cs = v1 / v2,
ssim = ((2 mx my + C1) v1) / ((mx^2 + my^2 + C1) v2).  The level's two numbers are the means of ssim and cs over all 3 o_l^2 values:
the channels are pooled inside the level.

Per pair, with w = WEIGHTS: value = prod_{l < 4} max(cs_l, 0)^w_l max(ssim_4, 0)^w_4 (the clamp is `tf.image.ssim_multiscale`'s;
without it a negative mean gives NaN); a pair where one of those five numbers is negative is `clamped`.

LEVEL_BOUND: how far two correct float64 evaluations of a level number may lie apart - absolute, on a number in [-1, 1].  With
u = 2^-53:
  * a filtered moment is a sum of at most 11 non-negative terms (tap times an EXACT value or product) of sums of at most 11 such
    terms: whatever the order and whether a product and its addition round once (fma) or twice, the computed sum is within a
    relative gamma = 24 u of the true one (22 additions and multiplications in a chain, two to spare).  The second moments are at
    most 255^2 = 65025, the first at most 255: e2 = 24 u 65025 = 1.74e-10, e1 = 24 u 255 = 6.8e-13 absolute, per evaluation;
  * a variance or covariance, exx - mx^2: e2 from exx, 2 255 e1 from the square of mx, and 3 u 65025 for the product's and the
    difference's own roundings: ev = e2 + 510 e1 + 3 u 65025 = 5.4e-10;
  * v1 = 2 sxy + C2 and v2 = sxx + syy + C2 each carry 2 ev + 2 u 2 65025 = 1.1e-9 (= evv), against v2 >= C2 - evv and |v1| <= v2 + evv
    (Cauchy-Schwarz on the true values): cs = v1 / v2 is off by at most (evv + |cs| evv) / v2 + u <= 2 evv / C2 = 3.8e-11 (= ecs);
  * the luminance term (2 mx my + C1) / (mx^2 + my^2 + C1) <= 1: numerator and denominator each carry 4 255 e1 + 4 u 65025 =
    7.2e-10 (= el) against a denominator >= C1: off by at most 2 el / C1 = 2.2e-10 (= elum);
  * ssim = luminance times cs, both at most 1 in magnitude (to first order): elum + ecs + 2 u; a mean of N such values adds a
    relative N u at most, 2e-11 for the 181548 values of the largest level, whatever the order.
One evaluation is therefore within elum + ecs + 2.1e-11 = 2.8e-10 of the true number, two evaluations within twice that of each
other: LEVEL_BOUND = 5.6e-10, computed below from these terms.  It holds for cs as well (whose own bound is smaller).  For scale:
fp32 accumulation of the moments of a bright near-flat texture is wrong by 3e-5."""
import numpy as np

SIZES = (32, 64, 128, 256)
LEVELS = 5
TAPS = 11
L_RANGE = 255.0
C1 = (0.01 * L_RANGE) * (0.01 * L_RANGE)
C2 = (0.03 * L_RANGE) * (0.03 * L_RANGE)
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _level_bound():
    u = 2.0 ** -53
    top = L_RANGE * L_RANGE
    e2, e1 = 24 * u * top, 24 * u * L_RANGE
    ev = e2 + 2 * L_RANGE * e1 + 3 * u * top
    evv = 2 * ev + 4 * u * top
    ecs = 2 * evv / C2
    el = 4 * L_RANGE * e1 + 4 * u * top
    elum = 2 * el / C1
    one = elum + ecs + 2 * u + 181548 * u
    return 2 * one


LEVEL_BOUND = _level_bound()


def window_sizes(S):
    return [min(TAPS, S >> l) for l in range(LEVELS)]


def output_sizes(S):
    return [(S >> l) - n + 1 for l, n in enumerate(window_sizes(S))]


def window_taps(S):
    """float64 [5, 11], zero padded"""
    if S not in SIZES:
        raise ValueError("S in %s, got %r" % (SIZES, S))
    taps = np.zeros((LEVELS, TAPS))
    for l, n in enumerate(window_sizes(S)):
        t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        sigma = 1.5 * n / TAPS
        g = np.exp(-(t * t) / (2.0 * sigma * sigma))
        taps[l, :n] = g / g.sum()
    return taps


def planes_of_codes(codes, S):
    """an int8 code row (at least 3 S^2 long) -> float64 [3, S, S] of u = code + 128"""
    return np.asarray(codes).reshape(-1)[:3 * S * S].astype(np.float64).reshape(3, S, S) + 128.0


def encode(x):
    """fp32 [..., 3, S, S] in [-1, 1] -> the bytes `encode_images` quantises to, as float64: rint((x + 1) 127.5) clamped to 0 .. 255"""
    x32 = np.asarray(x, dtype=np.float32)
    return np.clip(np.rint((x32 + np.float32(1.0)) * np.float32(127.5)), 0, 255).astype(np.float64)


def decode(u):
    """bytes 0 .. 255 -> fp32 in [-1, 1] that `encode_images` quantises back to the same bytes"""
    return (np.asarray(u, dtype=np.float64) / 127.5 - 1.0).astype(np.float32)


def _valid(p, g, axis):
    """the n-tap "valid" filter along `axis`, taps in ascending order"""
    n = g.size
    o = p.shape[axis] - n + 1
    out = np.zeros(p.shape[:axis] + (o,) + p.shape[axis + 1:])
    for j in range(n):
        out = out + g[j] * np.take(p, np.arange(j, j + o), axis=axis)
    return out


def down(p):
    return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) * 0.25


def level_maps(x, y, g):
    """x, y: float64 [3, s, s]; g: the level's n taps -> (ssim, cs) maps [3, o, o]"""
    f = lambda p: _valid(_valid(p, g, 2), g, 1)          # noqa: E731  rows (along x) first, then columns
    mx, my, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    v1, v2 = 2.0 * sxy + C2, (sxx + syy) + C2
    return ((2.0 * mx * my + C1) * v1) / (((mx * mx + my * my) + C1) * v2), v1 / v2


def levels(x, y):
    """x, y: [3, S, S] of values 0 .. 255 -> float64 [2, 5]: row 0 the levels' ssim means, row 1 their cs means"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    S = x.shape[-1]
    if x.shape != (3, S, S) or y.shape != x.shape or S not in SIZES:
        raise ValueError("two [3, S, S] images, S in %s; got %s and %s" % (SIZES, x.shape, y.shape))
    taps = window_taps(S)
    out = np.zeros((2, LEVELS))
    for l, n in enumerate(window_sizes(S)):
        ssim, cs = level_maps(x, y, taps[l, :n])
        out[0, l], out[1, l] = ssim.mean(), cs.mean()
        if l + 1 < LEVELS:
            x, y = down(x), down(y)
    return out


def value(lv):
    """[..., 2, 5] level numbers -> (value [...], clamped bool [...]); NaN stays NaN (and is not clamped)"""
    lv = np.asarray(lv, dtype=np.float64)
    terms = np.concatenate([lv[..., 1, :LEVELS - 1], lv[..., 0, LEVELS - 1:]], axis=-1)
    clamped = (terms < 0).any(axis=-1)
    with np.errstate(invalid="ignore"):
        clipped = np.where(np.isnan(terms), terms, np.maximum(terms, 0.0))
        return np.prod(clipped ** np.asarray(WEIGHTS), axis=-1), clamped


# ---- the inputs the tests share -------------------------------------------------------------------------------------------------------
def uniform_bytes(n, S, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3, S, S)).astype(np.float64)


def low_pass(n, S, seed, passes=4):
    """smooth random images: white noise box-filtered `passes` times (periodically), stretched to 0 .. 255, rounded"""
    a = np.random.default_rng(seed).standard_normal((n, 3, S, S))
    for _ in range(passes):
        a = (a + np.roll(a, 1, -1) + np.roll(a, -1, -1)) / 3
        a = (a + np.roll(a, 1, -2) + np.roll(a, -1, -2)) / 3
    lo, hi = a.min(axis=(1, 2, 3), keepdims=True), a.max(axis=(1, 2, 3), keepdims=True)
    return np.rint((a - lo) / (hi - lo) * 255.0)


def bright_texture(n, S, seed):
    """bytes 250 .. 255: the moments are near 255^2 and their differences a few units - what fp32 accumulation loses"""
    return np.random.default_rng(seed).integers(250, 256, size=(n, 3, S, S)).astype(np.float64)


def anticorrelated(S):
    """(a, 255 - a) with a = rint(128 + 100 sin(x / 3) cos(y / 5)), the same in all three channels"""
    yy, xx = np.mgrid[:S, :S]
    a = np.rint(128.0 + 100.0 * np.sin(xx / 3.0) * np.cos(yy / 5.0))
    a = np.broadcast_to(a, (3, S, S)).copy()
    return a, 255.0 - a
