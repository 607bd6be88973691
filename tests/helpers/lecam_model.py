"""The definition of the LeCam regulariser (Tseng et al. 2021, "Regularizing Generative Adversarial Networks under Limited Data") as
this project runs it, in numpy: the D loss with the regulariser, the observer with its state record and ring.  csrc/lecam.hip and
locate_amd/lecam.py (LeCam) are held to it with ==, bytes included.

Raw logits: t = D(real), f = D(G(z).detach()), a = D(augmented real); the hinge is relu(1 - t) + relu(1 + f).

The state record: 16 32-bit words, FIELDS names words 0 .. 7 (the anchors and the last means are fp32 bit patterns, the rest
unsigned counters mod 2^32), words 8 .. 15 are zero.  A ring row: 8 words {iteration, alpha_R, alpha_F, m_R, m_F, 1 if the
observation was accepted else 0, 0, 0}.

Every fp32 operation below is one numpy float32 operation (rounded once); the float64 sums run in the order of the kernels' block
reduction, block_sum(): see block_sum."""
from fractions import Fraction

import numpy as np

STATE_WORDS = 16
RING_WORDS = 8
THREADS = 256
FIELDS = ("alpha_r", "alpha_f", "accepted", "observations", "nonfinite", "rows", "mean_r", "mean_f")
_FLOAT_WORDS = (0, 1, 6, 7)

f32 = np.float32
f64 = np.float64


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


def _float(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def new_state():
    return np.zeros(STATE_WORDS, np.uint32)


def new_ring(capacity):
    return np.zeros((int(capacity), RING_WORDS), np.uint32)


def fields(state):
    out = {name: int(state[k]) for k, name in enumerate(FIELDS)}
    for k in _FLOAT_WORDS:
        out[FIELDS[k]] = _float(state[k])
    return out


def rate_constant(decay):
    """1 - decay in float64, rounded once to fp32"""
    return f32(1.0 - float(decay))


# ---- the two pieces of arithmetic numpy does not have ------------------------------------------------------------------------------------
def block_sum(values):
    """The float64 sum of `values` in the order of a 256-thread block: thread k adds its elements k, k + 256, ... in index order
    starting from 0.0; within each wave of 64 lanes the xor butterfly runs over the distances 32, 16, .. 1 (every lane adds its
    partner's value to its own); the four wave results are added in order, starting from 0.0."""
    v = np.asarray(values, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        lanes = np.zeros(THREADS, np.float64)
        for start in range(0, len(v), THREADS):
            part = v[start:start + THREADS]
            lanes[:len(part)] = lanes[:len(part)] + part
        lane = np.arange(THREADS)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[lane ^ o]          # lane ^ o stays inside the lane's wave of 64
        total = f64(0.0)
        for w in range(THREADS // 64):
            total = total + lanes[64 * w]
    return f64(total)


def fma32(a, b, c):
    """fp32 fused multiply-add, rounded once: exact rational arithmetic, then the nearest fp32 (ties to even)"""
    a, b, c = f32(a), f32(b), f32(c)
    with np.errstate(all="ignore"):
        guess = f32(f64(a) * f64(b) + f64(c))          # the product is exact in float64; the sum is rounded twice
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c) and np.isfinite(guess)):
        return guess
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    best = None
    for cand in (np.nextafter(guess, f32(-np.inf)), guess, np.nextafter(guess, f32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - exact)
        even = int(_bits(cand)) & 1 == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, cand)
    if exact == 0:
        return guess          # keeps the sign IEEE gives an exact zero
    return f32(best[2])


def clamp0(v):
    """clamp(v, min=0) as ATen computes it: v < 0 ? 0 : v - a NaN stays a NaN"""
    v = np.asarray(v, np.float32)
    return np.where(v < 0, f32(0), v).astype(np.float32)


# ---- the D loss --------------------------------------------------------------------------------------------------------------------------
def _plain_parts(t, f, a, gamma):
    t, f, a = (np.asarray(x, np.float32).reshape(-1) for x in (t, f, a))
    B, gamma = len(t), f32(gamma)
    with np.errstate(all="ignore"):
        hs = block_sum(clamp0(f32(1) - t).astype(np.float64) + clamp0(f32(1) + f).astype(np.float64))
        ts, as_ = block_sum(t), block_sum(a)
        invB = f32(1) / f32(B)
        delta = f32(ts / B) - f32(as_ / B)
        pen_g = f32(f32(f32(2) * gamma) * delta) * invB
        d_error = f32(hs / B)
        pen = f32(gamma * delta) * delta
        total = fma32(delta, f32(gamma * delta), d_error)          # the plain total is ONE fused multiply-add (csrc/dloss.h)
        gt = (np.where((f32(1) - t) >= 0, -invB, f32(0)).astype(np.float32) + pen_g).astype(np.float32)
        gf = np.where((f32(1) + f) >= 0, invB, f32(0)).astype(np.float32)
        ga = np.full(B, -pen_g, np.float32)
    return dict(t=t, f=f, B=B, invB=invB, d_error=f32(d_error), pen=f32(pen), total=f32(total), gt=gt, gf=gf, ga=ga)


def plain_d_loss(t, f, a, gamma):
    """locate_d_loss: (losses[3], g_true, g_fake, g_aug)"""
    p = _plain_parts(t, f, a, gamma)
    return np.array([p["d_error"], p["pen"], p["total"]], np.float32), p["gt"], p["gf"], p["ga"]


def is_active(state, weight, warmup):
    return bool(f32(weight) != 0 and int(state[2]) >= max(int(warmup), 1))


def d_loss(t, f, a, gamma, state, weight, one_sided=True, warmup=0):
    """locate_d_loss_lecam: (losses[4] = {d_error, penalty, total, R}, g_true, g_fake, g_aug)"""
    p = _plain_parts(t, f, a, gamma)
    if not is_active(state, weight, warmup):
        return np.array([p["d_error"], p["pen"], p["total"], 0.0], np.float32), p["gt"], p["gf"], p["ga"]
    t, f, B, weight = p["t"], p["f"], p["B"], f32(weight)
    alpha_r, alpha_f = _float(state[0]), _float(state[1])
    with np.errstate(all="ignore"):
        d_raw, e_raw = (t - alpha_f).astype(np.float32), (alpha_r - f).astype(np.float32)
        if one_sided:
            d, e = clamp0(d_raw), clamp0(e_raw)
            d_pass, e_pass = d_raw >= 0, e_raw >= 0          # clamp's gradient mask: false for a NaN
        else:
            d, e = d_raw, e_raw
            d_pass = e_pass = np.ones(B, bool)
        d64, e64 = d.astype(np.float64), e.astype(np.float64)
        R = f32(f32(block_sum(d64 * d64) / B) + f32(block_sum(e64 * e64) / B))
        total = f32(f32(p["d_error"] + p["pen"]) + f32(weight * R))
        c = f32(f32(f32(2) * weight) * p["invB"])
        gt = (p["gt"] + np.where(d_pass, (c * d).astype(np.float32), f32(0)).astype(np.float32)).astype(np.float32)
        gf = (p["gf"] + np.where(e_pass, -(c * e).astype(np.float32), f32(0)).astype(np.float32)).astype(np.float32)
    return np.array([p["d_error"], p["pen"], total, R], np.float32), gt, gf, p["ga"]


# ---- the observer ------------------------------------------------------------------------------------------------------------------------
def _ema(alpha, m, rate):
    with np.errstate(all="ignore"):
        return f32(alpha + f32(rate * f32(m - alpha)))


def observe(d_true, d_gen, iteration, state, ring, rate):
    """One observation, in place on `state` (uint32 [16]) and `ring` (uint32 [capacity, 8]); d_gen = -f, the step's out["d_gen"]."""
    t = np.asarray(d_true, np.float32).reshape(-1)
    f = (-np.asarray(d_gen, np.float32).reshape(-1)).astype(np.float32)
    B, rate = len(t), f32(rate)
    with np.errstate(all="ignore"):
        m_r, m_f = f32(block_sum(t) / B), f32(block_sum(f) / B)
    alpha_r, alpha_f, accepted = _float(state[0]), _float(state[1]), int(state[2])
    took = 0
    if np.isfinite(m_r) and np.isfinite(m_f):
        new_r = m_r if accepted == 0 else _ema(alpha_r, m_r, rate)
        new_f = m_f if accepted == 0 else _ema(alpha_f, m_f, rate)
        if np.isfinite(new_r) and np.isfinite(new_f):
            alpha_r, alpha_f, took = new_r, new_f, 1
    rows = int(state[5])
    ring[rows % len(ring)] = (np.uint32(int(iteration) & 0xFFFFFFFF), _bits(alpha_r), _bits(alpha_f), _bits(m_r), _bits(m_f), took, 0, 0)
    state[0], state[1] = _bits(alpha_r), _bits(alpha_f)
    state[2] = (accepted + took) & 0xFFFFFFFF
    state[3] = (int(state[3]) + 1) & 0xFFFFFFFF
    state[4] = (int(state[4]) + 1 - took) & 0xFFFFFFFF
    state[5] = (rows + 1) & 0xFFFFFFFF
    state[6], state[7] = _bits(m_r), _bits(m_f)
    return state


def curve(ring, first, last):
    """ring rows first .. last - 1 (counted over the whole run) as LeCam.curve() returns them"""
    out = []
    for k in range(first, last):
        row = ring[k % len(ring)]
        out.append({"iteration": int(np.array([row[0]], np.uint32).view(np.int32)[0]), "anchor_real": float(_float(row[1])),
                    "anchor_fake": float(_float(row[2])), "mean_real": float(_float(row[3])), "mean_fake": float(_float(row[4])),
                    "accepted": int(row[5])})
    return out


# ---- the bound of the autograd comparison (tests/test_lecam_model.py) ----------------------------------------------------------------------
def gradient_bound(t, f, a, gamma, state, weight):
    """How far an fp32 gradient of d_loss may lie from the float64 gradient of the same loss, per element, from the operation
    sequence (u = 2^-24, the unit roundoff of fp32; every fp32 operation errs by at most u times its result):

      plain g_true  = s + pen_g, s = -1/B or 0 (1/B: one rounding) and pen_g = ((2 gamma) delta) / B with delta = m_t - m_a: the two
                      means are each rounded once from float64 (u |m|), the subtraction once more, then two multiplications (2 gamma is
                      exact) and the addition:  |err| <= u/B + (2 gamma / B) (u (|m_t| + |m_a|) + 3 u |delta|) + u |g|;
      regulariser   q = c * d_i, c = (2 w) / B (2 w exact, one rounding for 1/B, one for the product), d_i one rounding, the product one
                      and the addition one:  |err| <= 4 u |c d_i| + u |g|.

    Rounding errors of the float64 sums (2^-53 relative) are three hundred million times smaller and are covered by doubling the
    whole bound.  Returns (bound for g_true [B], bound for g_fake [B], bound for g_aug, a scalar)."""
    u = 2.0 ** -24
    t, f, a = (np.asarray(x, np.float64).reshape(-1) for x in (t, f, a))
    B = len(t)
    m_t, m_a = abs(t.mean()), abs(a.mean())
    delta = abs(t.mean() - a.mean())
    pen_err = (2.0 * abs(gamma) / B) * (u * (m_t + m_a) + 3.0 * u * delta)
    pen_g = 2.0 * abs(gamma) * delta / B
    c = 2.0 * abs(weight) / B
    alpha_r, alpha_f = float(_float(state[0])), float(_float(state[1]))
    g_t = 1.0 / B + pen_g + c * np.abs(t - alpha_f)
    g_f = 1.0 / B + c * np.abs(alpha_r - f)
    bound_t = 2.0 * (u / B + pen_err + 4.0 * u * c * np.abs(t - alpha_f) + u * g_t)
    bound_f = 2.0 * (u / B + 4.0 * u * c * np.abs(alpha_r - f) + u * g_f)
    bound_a = 2.0 * (pen_err + u * pen_g)
    return bound_t, bound_f, bound_a
