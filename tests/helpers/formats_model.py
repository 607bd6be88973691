"""The model of csrc/formats.hip: a generic round-to-nearest-even quantiser onto a small floating-point grid in float64, the two
scale rules (one power of two per tensor; one per 32-element block, OCP MX v1.0), and per view the base record and the five format
records - counts as Python ints, sums by math.fsum of exactly known terms.  Nothing here looks at the kernel: the grids come from
the formats' definitions, the scale rules from the text of include/locate_hip.h."""
import math

import numpy as np

from stats_model import finite_mask, magnitude_bits

BLOCK = 32
HIST = 32
# name, mantissa bits, exponent of the smallest normal, largest finite value, scale ("tensor", top binade) / ("block", emax) / None
FORMATS = (
    ("e4m3_tensor", 3, -6, 448.0, ("tensor", 7)),
    ("e5m2_tensor", 2, -14, 57344.0, ("tensor", 14)),
    ("mxfp8_e4m3", 3, -6, 448.0, ("block", 8)),
    ("mxfp4_e2m1", 1, 0, 6.0, ("block", 2)),
    ("bf16", 7, -126, float(np.array([0x7F7F0000], dtype=np.uint32).view(np.float32)[0]), None),
)
NAMES = tuple(f[0] for f in FORMATS)


def quantise(a, mbits, emin, top):
    """(q, clamped) of float64 values `a` (finite): the nearest point of the grid {m * 2^(e - mbits)}, e >= emin, m < 2^(mbits + 1),
    ties to the even m, subnormals (e = emin, m < 2^mbits) included; a rounded magnitude above `top` is flagged and replaced by
    `top`.  Exact: a power-of-two division, np.rint (ties to even) on a value that float64 holds exactly, a power-of-two product."""
    a = np.asarray(a, dtype=np.float64)
    mag = np.abs(a)
    _, e = np.frexp(mag)          # mag = f * 2^e, f in [0.5, 1): the binade is e - 1
    binade = np.maximum(e.astype(np.int64) - 1, emin)
    step = np.ldexp(1.0, (binade - mbits).astype(np.int64))
    q = np.rint(mag / step) * step
    clamped = q > top
    q = np.where(clamped, top, q)
    return np.copysign(q, a), clamped


def field(mag_bits):
    return (np.asarray(mag_bits, dtype=np.uint32) >> np.uint32(23)).astype(np.int64)


def tensor_scale_exp(top, absmax_bits):
    """k with absmax * 2^k in [2^top, 2^(top + 1)), clamped to +-126; 0 for a zero, denormal or non-finite absmax"""
    f = int(absmax_bits) >> 23 & 0xFF
    if f < 1 or f > 254:
        return 0
    return max(-126, min(126, top - (f - 127)))


def block_scale_exp(block_absmax_bits, emax):
    """X of OCP MX v1.0 per block: the block's largest binade (a denormal counts as the smallest normal) less the grid's largest"""
    return np.clip(np.maximum(field(block_absmax_bits), 1) - 127 - emax, -127, 127)


def blocked(x, axis):
    """x [B, C, P] -> [lines, blocks, 32] along `axis` (1: c, 2: p) and the mask of members that exist"""
    B, C, P = x.shape
    lines = x.transpose(0, 2, 1).reshape(B * P, C) if axis == 1 else x.reshape(B * C, P)
    n = lines.shape[1]
    nb = -(-n // BLOCK)
    pad = np.zeros((lines.shape[0], nb * BLOCK), dtype=lines.dtype)
    pad[:, :n] = lines
    exists = np.zeros((lines.shape[0], nb * BLOCK), dtype=bool)
    exists[:, :n] = True
    return pad.reshape(-1, nb, BLOCK), exists.reshape(-1, nb, BLOCK)


def audit(x, axis):
    """The record of one call on a float32 array x [B, C, P]: {"n", "zeros", "nonfinite", "calls", "sumsq", "absmax" (uint32 bits),
    "hist" [32 ints], "formats": [{"err_sumsq", "flushed", "subnormal", "clamped"}] in FORMATS' order}."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.ndim == 3 and axis in (1, 2)
    v, exists = blocked(x, axis)
    mag = magnitude_bits(v).reshape(v.shape)
    finite = finite_mask(v).reshape(v.shape) & exists
    counted = finite & (mag != 0)
    d = np.where(finite, v, np.float32(0)).astype(np.float64)
    absmax = int(mag[finite].max()) if finite.any() else 0
    rec = {"n": int(x.size), "zeros": int((finite & (mag == 0)).sum()), "nonfinite": int((exists & ~finite).sum()), "calls": 1,
           "sumsq": math.fsum((d[finite] ** 2).tolist()), "absmax": absmax}
    top = max(absmax >> 23, 1)
    below = np.minimum(top - np.maximum(field(mag[counted]), 1), HIST - 1)
    rec["hist"] = [int(c) for c in np.bincount(below, minlength=HIST)]
    block_absmax = np.where(finite, mag, 0).max(axis=2, keepdims=True).astype(np.uint32)
    rec["formats"] = []
    for name, mbits, emin, top_value, scale in FORMATS:
        if scale is None:
            k = np.zeros((1, 1, 1), dtype=np.int64)
        elif scale[0] == "tensor":
            k = np.full((1, 1, 1), tensor_scale_exp(scale[1], absmax), dtype=np.int64)
        else:
            k = -block_scale_exp(block_absmax, scale[1])
        k = np.broadcast_to(k, d.shape)
        q, clamped = quantise(np.ldexp(d, k), mbits, emin, top_value)          # scaled in float64: exact
        e = d - np.ldexp(q, -k)
        aq = np.abs(q)
        rec["formats"].append({"err_sumsq": math.fsum((e[finite] ** 2).tolist()), "flushed": int((counted & (aq == 0)).sum()),
                               "subnormal": int((finite & (aq != 0) & (aq < math.ldexp(1.0, emin))).sum()),
                               "clamped": int((finite & clamped).sum())})
    return rec


def accumulate(a, b):
    """two calls into one slot: every count and sum added, absmax the maximum"""
    out = {key: a[key] + b[key] for key in ("n", "zeros", "nonfinite", "calls")}
    out["sumsq"] = math.fsum((a["sumsq"], b["sumsq"]))
    out["absmax"] = max(a["absmax"], b["absmax"])
    out["hist"] = [p + q for p, q in zip(a["hist"], b["hist"])]
    out["formats"] = [{"err_sumsq": math.fsum((fa["err_sumsq"], fb["err_sumsq"])),
                       **{key: fa[key] + fb[key] for key in ("flushed", "subnormal", "clamped")}} for fa, fb in zip(a["formats"], b["formats"])]
    return out


# ---- the fixture family both test files use ------------------------------------------------------------------------------------------
SHAPES = ((2, 33, 5), (1, 1, 1), (3, 32, 1), (1, 64, 67), (2, 40, 150))          # the last spans several tiles on either axis
FLT_MAX_NEAR = float(np.array([0x7F7FFF00], dtype=np.uint32).view(np.float32)[0])
# one scale block's worth of planted values: its largest magnitude is 1.25 (field 127), so X = -8 (e4m3: scaled = 256 x) and
# X = -2 (e2m1: scaled = 4 x).  e4m3 ties of both parities at scaled 17 and 19, and in its subnormals at 0.5 and 1.5 units of
# 2^-9; bf16 ties at 1 + 2^-8 and 1 + 3 * 2^-8; e2m1 ties at scaled 0.25, 0.75, 1.25, 1.75, 2.5, 3.5 and (the largest) 5
BLOCK_LINE = np.array([1.25, 17 / 256, -19 / 256, 1 + 2.0 ** -8, -(1 + 3 * 2.0 ** -8), 0.0625, 0.1875, 0.3125, 0.4375, 0.625, 0.875,
                       0.5 * 2.0 ** -17, 1.5 * 2.0 ** -17, -0.0, 0.0, 2.0 ** -140, -2.0 ** -149, np.nan, np.inf, -np.inf, 2.0 ** -8,
                       3 * 2.0 ** -9, 2.0 ** -20, 1.0, 2.0 ** -130, -3 * 2.0 ** -134], dtype=np.float32)          # the last two: bf16's subnormals
# with the tensor's largest magnitude at 1.5 * 2^20: k = -13 (e4m3: ties at scaled 17, 19) and k = -6 (e5m2: ties at scaled 18, 22)
TENSOR_POINTS = np.array([1.5 * 2.0 ** 20, 17 * 2.0 ** 13, -19 * 2.0 ** 13, 18 * 64.0, 22 * 64.0, 2.0 ** -6 * 2.0 ** 13 * 0.75], dtype=np.float32)


def fixture(shape, family, seed):
    """float32 [B, C, P].  Magnitudes log-uniform over 36 binades with mixed signs; an all-zero block, the planted block, and a
    block whose largest magnitude 1.9 scales to 486.4 - inside (448, 512) - along each axis; the tensor-scale points; NaN, +-Inf,
    +-0 and denormals.  family "max" adds an element near FLT_MAX, beside which the per-tensor formats flush everything else;
    family "plain" leaves 1.5 * 2^20 the largest, and they reach their subnormals."""
    rng = np.random.default_rng(seed)
    B, C, P = shape
    x = (rng.choice([-1.0, 1.0], size=shape) * 2.0 ** rng.uniform(-18, 18, size=shape)).astype(np.float32)
    n = x.size
    if n == 1:
        return x if family == "plain" else np.full(shape, FLT_MAX_NEAR, dtype=np.float32)
    x[-1, :, P - 1] = 0.0
    x[-1, C - 1, :] = 0.0
    m = min(C, BLOCK_LINE.size)
    x[0, :m, 0] = BLOCK_LINE[:m]
    x[0, m:min(C, 32), 0] = 2.0 ** -4
    m = min(P, BLOCK_LINE.size)
    x[0, 0, :m] = BLOCK_LINE[:m]
    x[0, 0, m:min(P, 32)] = 2.0 ** -4
    if P > 1:
        x[0, :min(C, 32), 1] = 2.0 ** -5
        x[0, min(C, 32) // 2, 1] = -1.9
    if C > 1:
        x[0, 1, :min(P, 32)] = 2.0 ** -5
        x[0, 1, min(P, 32) // 2] = 1.9
    flat = x.reshape(-1)
    at = n // 3
    k = min(TENSOR_POINTS.size, n - at)
    flat[at:at + k] = TENSOR_POINTS[:k]
    if family == "max":
        flat[n // 2] = -FLT_MAX_NEAR
    return x


def fixtures():
    """[(what, x)] over SHAPES and both families"""
    return [("%s %s" % (list(shape), family), fixture(shape, family, 100 + 2 * i + j))
            for i, shape in enumerate(SHAPES) for j, family in enumerate(("plain", "max"))]
