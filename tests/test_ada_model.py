"""The numpy definition of the adaptive augmentation (tests/helpers/ada_model.py) against its own stated properties: the kernels are
held to the model with == (tests/test_gpu_ada.py), so what is checked here is checked for them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ada_model as A  # noqa: E402

f32 = np.float32


def run(batches, interval=4, target=0.6, step=0.125, p_max=1.0, p=0.0, capacity=8):
    state, ring = A.new_state(p), A.new_ring(capacity)
    trace = []
    for it, x in enumerate(batches, 1):
        A.observe(x, it, state, ring, interval, target, f32(step), p_max)
        trace.append(A.fields(state))
    return state, ring, trace


def test_step_constant_is_one_rounding_of_the_float64_quotient():
    assert A.step_constant(64, 4, 500) == f32(64 * 4 / 500000.0) and A.step_constant(64, 4, 500).dtype == np.float32
    assert A.step_constant(64, 4, float("inf")) == 0.0
    assert A.step_constant(7, 3, 0.021) == f32(1.0)


@pytest.mark.parametrize("p_max", [1.0, 0.7, 0.05])
def test_p_never_leaves_its_range(p_max):
    rng = np.random.default_rng(3)
    # long runs of confident, of undecided and of random logits, with a step that does not divide the range
    batches = [np.full(5, 1.0, f32)] * 60 + [np.full(5, -1.0, f32)] * 60 + [rng.standard_normal(5).astype(f32) for _ in range(80)]
    _, _, trace = run(batches, interval=2, step=0.3, p_max=p_max, p=p_max / 2)
    ps = np.array([t["p"] for t in trace], np.float64)
    assert ps.min() >= 0.0 and ps.max() <= f32(p_max)
    assert ps.max() == f32(p_max) and ps.min() == 0.0          # and it reached and stuck at both ends
    assert trace[-1]["ups"] + trace[-1]["downs"] <= trace[-1]["closed"] == 100


def test_a_window_of_nans_moves_nothing():
    nan = np.full(6, np.nan, f32)
    state, ring, trace = run([np.ones(6, f32)] * 2 + [nan] * 4, interval=2, step=0.25, p=0.5)
    assert [t["p"] for t in trace] == [0.5, 0.75, 0.75, 0.75, 0.75, 0.75]
    last = trace[-1]
    assert (last["r"], last["closed"], last["ups"], last["downs"], last["nan"], last["rows"]) == (1.0, 3, 1, 0, 24, 3)
    assert last["sum"] == last["counted"] == last["seen"] == 0
    # the empty windows' rows repeat the last r and p and say that nothing was counted
    assert [int(ring[k][3]) for k in range(3)] == [12, 0, 0] and ring[1][1] == ring[0][1] and ring[2][2] == ring[0][2]
    # a NaN beside numbers is left out of the sum AND of the denominator: r = (2 - 1) / 3
    _, _, trace = run([np.array([np.nan, 1.0, 2.0, -1.0, np.nan], f32)], interval=1)
    assert trace[0]["r"] == f32(1.0 / 3.0) and trace[0]["nan"] == 2


def test_zeros_count_zero_and_infinities_as_their_sign():
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.inf, 1e-45, -1e-45, 3.0], f32)
    _, ring, trace = run([x], interval=1)
    assert trace[0]["r"] == f32(2.0 / 8.0) and int(ring[0][3]) == 8 and trace[0]["nan"] == 0


def test_r_equal_to_target_leaves_p():
    x = np.array([1.0, 1.0, 1.0, 1.0, -1.0], f32)          # B = 5, sum 3: r = fp32(0.6) = fp32 of the target
    _, _, trace = run([x] * 4, interval=2, target=0.6, step=0.25, p=0.5)
    assert [t["p"] for t in trace] == [0.5] * 4 and trace[-1]["closed"] == 2 and trace[-1]["ups"] == trace[-1]["downs"] == 0
    assert trace[-1]["r"] == f32(0.6)


def test_the_ring_wraps_and_keeps_the_newest_rows():
    _, ring, trace = run([np.ones(3, f32)] * 11, interval=1, step=0.01, capacity=4)
    assert trace[-1]["rows"] == 11
    assert [r["iteration"] for r in A.curve(ring, 7, 11)] == [8, 9, 10, 11]
    assert [r["p"] for r in A.curve(ring, 9, 11)] == [float(trace[9]["p"]), float(trace[10]["p"])]


def test_gate_is_strict_and_touches_nothing_else():
    raw = np.arange(5 * 12, dtype=np.float32).reshape(5, 12) * f32(0.37)
    p = f32(0.3)
    raw[:, 9:] = [[0.0, 0.0, 0.0], [p, np.nextafter(p, f32(0)), np.nextafter(p, f32(1))], [A.GATE_CAP] * 3, [0.1, 0.9, 0.2], [np.nan, 0.0, p]]
    out = A.gate(raw, p, 7)
    assert np.array_equal(out[:, :9].view(np.uint32), raw[:, :9].view(np.uint32))
    assert out[:, 9].tolist() == [0.0, 1.0 + 4.0, 7.0, 2.0, 1.0 + 4.0] and not out[:, 10:].any()          # g == p is OFF
    assert A.gate(raw, p, 2)[:, 9].tolist() == [0.0, 0.0, 2.0, 2.0, 0.0]          # bits outside the policy stay clear
    assert A.gate(raw, 0.0, 7)[:, 9].tolist() == [7.0] * 5          # p = 0 applies nothing, not even g = 0
    assert A.gate(raw, 1.0, 7)[:, 9].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]          # p = 1 applies everything below the cap


def test_gate_keeps_each_op_at_its_probability():
    """10 000 rows at p = 0.3: each op's applied fraction within five binomial sigmas, 5 sqrt(0.21 / 10000) = 0.023"""
    rng = np.random.default_rng(11)
    raw = np.zeros((10000, 12), np.float32)
    raw[:, 9:] = A.gate_uniforms(rng.random((10000, 3)))
    mask = A.gate(raw, 0.3, 7)[:, 9].astype(np.int64)
    for k in range(3):
        applied = float(np.mean((mask >> k & 1) == 0))
        assert abs(applied - 0.3) <= 5.0 * np.sqrt(0.21 / 10000), (k, applied)


def test_gate_uniforms_stay_below_one():
    g = A.gate_uniforms(np.array([0.0, 0.5, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -25, 1.0 - 2.0 ** -24]))
    assert g.dtype == np.float32 and g.max() == A.GATE_CAP < 1.0 and g[0] == 0.0
    assert np.float32(1.0 - 2.0 ** -53) == 1.0          # what the cap is for
