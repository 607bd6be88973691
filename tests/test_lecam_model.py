"""The numpy definition of the LeCam regulariser (tests/helpers/lecam_model.py) against independent statements of the same things:
the plain D loss restated with scalar loops, torch float64 autograd of the stated loss, and the corners - a NaN logit, a non-finite
mean, the first accepted observation."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lecam_model as L  # noqa: E402

f32 = np.float32


def logits(B, seed, scale=1.5):
    rng = np.random.default_rng(seed)
    return tuple((rng.standard_normal(B) * scale).astype(np.float32) for _ in range(3))


def state_with(alpha_r, alpha_f, accepted):
    state = L.new_state()
    state[0], state[1], state[2] = L._bits(alpha_r), L._bits(alpha_f), accepted
    return state


def words(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def block_sum_by_loops(values):
    """block_sum() spelled with Python loops over threads, lanes and waves"""
    values = [float(v) for v in values]
    lanes = [0.0] * 256
    for i, v in enumerate(values):
        lanes[i % 256] = float(np.float64(lanes[i % 256]) + np.float64(v))
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [float(np.float64(lanes[k]) + np.float64(lanes[k ^ o])) for k in range(256)]
    total = 0.0
    for w in range(4):
        total = float(np.float64(total) + np.float64(lanes[64 * w]))
    return total


@pytest.mark.parametrize("B", [1, 8, 64, 257, 1000])
def test_block_sum_is_the_stated_order(B):
    v = np.random.default_rng(B).standard_normal(B) * 1e3
    assert L.block_sum(v) == block_sum_by_loops(v)
    assert abs(L.block_sum(v) - float(sum(Fraction(float(x)) for x in v))) <= 1e-12 * np.abs(v).sum()


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    for _ in range(300):
        a, b, c = (f32(x) for x in rng.standard_normal(3) * 10.0 ** rng.integers(-3, 4))
        got = L.fma32(a, b, c)
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        below, above = np.nextafter(got, f32(-np.inf)), np.nextafter(got, f32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(below)) - exact) and err <= abs(Fraction(float(above)) - exact)
    # a case where rounding the product first loses the answer: (1 + 2^-12)^2 - (1 + 2^-11) = 2^-24
    x = f32(1 + 2.0 ** -12)
    assert L.fma32(x, x, -f32(1 + 2.0 ** -11)) == f32(2.0 ** -24) and f32(f32(x * x) - f32(1 + 2.0 ** -11)) == 0
    assert np.isnan(L.fma32(np.nan, 1, 1)) and L.fma32(np.inf, 1, 1) == np.inf


@pytest.mark.parametrize("B", [1, 8, 64, 257])
def test_the_inactive_model_is_the_plain_d_loss_restated(B):
    """weight = 0, too few accepted observations, and both: the plain loss, which is restated here with scalar loops"""
    t, f, a = logits(B, 10 + B)
    gamma = f32(100.0)
    hinge = [float(np.float64(max(f32(1) - ti, f32(0))) + np.float64(max(f32(1) + fi, f32(0)))) for ti, fi in zip(t, f)]
    m_t, m_a = f32(block_sum_by_loops(t) / B), f32(block_sum_by_loops(a) / B)
    delta = f32(m_t - m_a)
    invB = f32(1) / f32(B)
    pen_g = f32(f32(f32(f32(2) * gamma) * delta) * invB)
    d_error = f32(block_sum_by_loops(hinge) / B)
    pen = f32(f32(gamma * delta) * delta)
    total = L.fma32(delta, f32(gamma * delta), d_error)
    want = (np.array([d_error, pen, total, 0], np.float32),
            np.array([f32((-invB if f32(1) - ti >= 0 else f32(0)) + pen_g) for ti in t], np.float32),
            np.array([invB if f32(1) + fi >= 0 else f32(0) for fi in f], np.float32), np.full(B, -pen_g, np.float32))
    for state, weight, warmup in ((state_with(0.5, -0.5, 9), 0.0, 0), (state_with(0.5, -0.5, 9), 0.3, 10),
                                  (state_with(0.5, -0.5, 0), 0.3, 0), (L.new_state(), 0.0, 5)):
        got = L.d_loss(t, f, a, gamma, state, weight, True, warmup)
        assert not L.is_active(state, weight, warmup)
        assert all(np.array_equal(words(g), words(w)) for g, w in zip(got, want))
    plain = L.plain_d_loss(t, f, a, gamma)
    assert np.array_equal(words(plain[0]), words(want[0][:3])) and all(np.array_equal(words(g), words(w)) for g, w in zip(plain[1:], want[1:]))
    # active at exactly max(warmup, 1) accepted observations
    assert L.is_active(state_with(0.5, -0.5, 10), 0.3, 10) and L.is_active(state_with(0.5, -0.5, 1), 0.3, 0)


@pytest.mark.parametrize("one_sided", [True, False])
@pytest.mark.parametrize("B", [8, 64, 257])
def test_active_gradients_agree_with_float64_autograd_of_the_stated_loss(B, one_sided):
    t, f, a = logits(B, 20 + B)
    gamma, weight = 100.0, 0.3
    state = state_with(0.25, -0.375, 3)
    losses, gt, gf, ga = L.d_loss(t, f, a, gamma, state, weight, one_sided, 0)
    T, F, A = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (t, f, a))
    d, e = T - (-0.375), 0.25 - F
    if one_sided:
        d, e = d.clamp(min=0), e.clamp(min=0)
    R = (d * d).mean() + (e * e).mean()
    d_error = ((1 - T).clamp(min=0) + (1 + F).clamp(min=0)).mean()
    pen = gamma * (T.mean() - A.mean()) ** 2
    total = d_error + pen + weight * R
    total.backward()
    bt, bf, ba = L.gradient_bound(t, f, a, gamma, state, weight)
    assert (np.abs(gt.astype(np.float64) - T.grad.numpy()) <= bt).all()
    assert (np.abs(gf.astype(np.float64) - F.grad.numpy()) <= bf).all()
    assert (np.abs(ga.astype(np.float64) - A.grad.numpy()) <= ba).all()
    assert bt.max() < 1e-5 and bf.max() < 1e-6          # the bound is a rounding bound, not a licence
    # the values: a few units of fp32 roundoff of their own size
    values = [v.item() for v in (d_error, pen, total, R)]
    for got, want in zip(losses, values):
        assert abs(float(got) - want) <= 8 * 2.0 ** -24 * max(abs(want), values[0] + values[1])
    # and the regulariser is in them: not the plain gradients
    plain = L.plain_d_loss(t, f, a, gamma)
    assert not np.array_equal(gt, plain[1]) and not np.array_equal(gf, plain[2]) and np.array_equal(words(ga), words(plain[3]))


@pytest.mark.parametrize("one_sided", [True, False])
def test_a_nan_logit_makes_r_nan_and_nothing_is_clamped_away(one_sided):
    state = state_with(0.25, -0.375, 1)
    for which in (0, 1):
        x = list(logits(8, 31))
        x[which] = x[which].copy()
        x[which][3] = np.nan
        losses, gt, gf, ga = L.d_loss(x[0], x[1], x[2], 100.0, state, 0.3, one_sided, 0)
        assert np.isnan(losses[3]) and np.isnan(losses[2]) and np.isnan(losses[0])
        if which == 0:
            assert np.isnan(gt).all()          # the penalty's gradient holds mean t
        else:
            # clamp's gradient mask is false for a NaN: one-sided, the element keeps its plain gradient; two-sided, it is the NaN
            assert np.isnan(gf[3]) == (not one_sided) and np.isfinite(np.delete(gf, 3)).all()
    for inf in (np.inf, -np.inf):
        t, f, a = logits(8, 32)
        t[2] = inf
        losses = L.d_loss(t, f, a, 100.0, state, 0.3, one_sided, 0)[0]
        assert not np.isfinite(losses[2]), "an infinite logit must not leave a finite total"


def test_the_first_accepted_observation_sets_the_anchor_and_later_ones_move_it():
    state, ring = L.new_state(), L.new_ring(4)
    t, f, _ = logits(8, 40)
    rate = L.rate_constant(0.75)
    assert rate == f32(0.25)
    L.observe(t, -f, 7, state, ring, rate)
    s = L.fields(state)
    m_r, m_f = f32(np.float64(L.block_sum(t)) / 8), f32(np.float64(L.block_sum(f)) / 8)
    assert (s["alpha_r"], s["alpha_f"], s["accepted"], s["observations"], s["nonfinite"], s["rows"]) == (m_r, m_f, 1, 1, 0, 1)
    assert L.curve(ring, 0, 1) == [{"iteration": 7, "anchor_real": float(m_r), "anchor_fake": float(m_f), "mean_real": float(m_r),
                                    "mean_fake": float(m_f), "accepted": 1}]
    t2, f2, _ = logits(8, 41)
    L.observe(t2, -f2, 8, state, ring, rate)
    m2 = f32(np.float64(L.block_sum(t2)) / 8)
    assert L.fields(state)["alpha_r"] == f32(m_r + f32(rate * f32(m2 - m_r))) and L.fields(state)["accepted"] == 2
    assert not state[8:].any()


def test_a_non_finite_mean_leaves_the_anchors_alone():
    state, ring = L.new_state(), L.new_ring(2)
    t, f, _ = logits(8, 50)
    rate = f32(0.5)
    L.observe(t, -f, 1, state, ring, rate)
    before = state.copy()
    for k, (bad_t, bad_f) in enumerate(((np.nan, 0), (np.inf, 0), (0, -np.inf), (0, np.nan)), 2):
        t2, f2 = t.copy(), f.copy()
        if bad_t:
            t2[1] = bad_t
        if bad_f:
            f2[5] = bad_f
        L.observe(t2, -f2, k, state, ring, rate)
        s = L.fields(state)
        assert state[0] == before[0] and state[1] == before[1] and s["accepted"] == 1
        assert s["nonfinite"] == k - 1 and s["observations"] == k and s["rows"] == k
        assert L.curve(ring, k - 1, k)[0]["accepted"] == 0
    # a non-finite mean before any accepted observation: still no anchor, still inactive
    fresh, ring = L.new_state(), L.new_ring(2)
    L.observe(np.full(8, np.nan, np.float32), f, 1, fresh, ring, rate)
    assert fresh[0] == 0 and fresh[2] == 0 and fresh[4] == 1 and not L.is_active(fresh, 0.3, 0)
    # an update that would overflow is refused as well
    big = state_with(3e38, -3e38, 1)
    L.observe(np.full(8, -3e38, np.float32), np.full(8, -3e38, np.float32), 1, big, L.new_ring(1), f32(1.0))
    assert L.fields(big)["alpha_r"] == f32(3e38) and L.fields(big)["nonfinite"] == 1 and L.fields(big)["accepted"] == 1
