"""The numpy definition of top-k training (tests/helpers/topk_model.py) against independent spellings of the same thing, without a GPU:
the ranks against a brute-force sorted() with the definition's key and against before() pair by pair, k = B against the plain hinge
mean and gradient, ties, signed zeros, NaN first, infinities, a k out of range, the record and the ring."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import topk_model as M  # noqa: E402

f32 = np.float32


def words(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def sorted_order(f):
    """indices in the definition's order by Python's sorted(): NaN first, then higher first, then lower index"""
    def key(i):
        v = float(f[i])
        return (0, 0.0, i) if v != v else (1, -v, i)          # -(-0.0) == -(0.0) as floats: the zeros tie
    return sorted(range(len(f)), key=key)


def inputs():
    rng = np.random.default_rng(2020)
    out = {"gauss": rng.standard_normal(97).astype(np.float32) * f32(1.5),
           "five": rng.choice(np.array([-1.5, -0.25, 0.0, 0.75, 2.0], np.float32), 130),
           "equal": np.full(40, 0.375, np.float32),
           "zeros": np.where(rng.random(33) < 0.5, f32(-0.0), f32(0.0)).astype(np.float32),
           "above": (rng.random(50) + 1.5).astype(np.float32)}
    x = out["gauss"].copy()
    x[[3, 50, 96]] = np.nan
    out["nans"] = x
    x = out["gauss"].copy()
    x[[0, 7]], x[[5, 90]] = np.inf, -np.inf
    out["infs"] = x
    return out


INPUTS = inputs()


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_ranks_are_the_position_in_a_sorted_list_and_the_pairwise_count(name):
    f = INPUTS[name]
    B = len(f)
    rank = M.ranks(f)
    order = sorted_order(f)
    assert [int(rank[i]) for i in order] == list(range(B))
    assert sorted(rank.tolist()) == list(range(B))
    for i in range(0, B, 7):
        assert rank[i] == sum(M.before(f, j, i) for j in range(B))
    for k in (1, 2, B // 2, B - 1, B):
        assert np.array_equal(np.nonzero(M.kept(f, k))[0], np.sort(order[:k]))


def test_the_order_on_the_cases_that_matter():
    f = np.array([1, np.nan, 3, -0.0, 0.0, 3], np.float32)
    assert sorted_order(f) == [1, 2, 5, 0, 3, 4] and M.ranks(f).tolist() == [3, 0, 1, 4, 5, 2]
    assert M.kept(f, 3).tolist() == [False, True, True, False, False, True]          # nan, 3, 3: what torch.topk selects
    assert M.before(f, 3, 4) and not M.before(f, 4, 3)          # -0 and +0 are equal: the lower index first
    f = np.array([np.nan, -np.inf, np.inf, np.nan, 1e38], np.float32)
    assert M.ranks(f).tolist() == [0, 4, 2, 1, 3]
    assert not M.before(f, 0, 0)


@pytest.mark.parametrize("name", ["gauss", "five", "equal", "zeros", "above", "infs"])
def test_k_equal_to_the_batch_is_the_plain_hinge_loss(name):
    f = INPUTS[name]
    B = len(f)
    loss, g = M.plain_g_loss(f)
    for k in (B, 0, -3, B + 1):          # out of range behaves as B
        state, ring = M.new_state(k), M.new_ring(2)
        losses, gk = M.g_loss(f, state, ring)
        assert words(losses)[0] == words(loss)[0] and words(losses)[1] == words(loss)[0]
        assert np.array_equal(words(gk), words(g))
        s = M.fields(state)
        assert s["k"] == k and s["k_used"] == B and s["launches"] == 1 and s["active"] == int(((f32(1) - f) >= 0).sum())
        assert words(s["mean_all"])[0] == words(s["mean_kept"])[0]
    # the plain mean in another spelling: float64 throughout, far inside fp32's rounding of the block-ordered sum
    want = np.maximum(1.0 - f.astype(np.float64), 0.0).mean()
    assert float(loss) == want if np.isinf(want) else abs(float(loss) - want) <= 2.0 ** -23 * want
    assert np.array_equal(g, np.where(f <= 1, f32(-1.0) / f32(B), f32(0)).astype(np.float32))


@pytest.mark.parametrize("name", ["gauss", "five", "zeros", "above", "infs"])
def test_the_loss_over_the_kept_elements(name):
    f = INPUTS[name]
    B = len(f)
    order = sorted_order(f)
    for k in (1, 2, B // 2, B - 1):
        state, ring = M.new_state(k), M.new_ring(4)
        losses, g = M.g_loss(f, state, ring)
        top = np.array(order[:k])
        want = np.maximum(1.0 - f[top].astype(np.float64), 0.0).sum() / k
        assert float(losses[0]) == want if np.isinf(want) else abs(float(losses[0]) - want) <= 2.0 ** -23 * want
        assert words(losses)[1] == words(M.plain_g_loss(f)[0])[0]
        dropped = np.ones(B, bool)
        dropped[top] = False
        assert (words(g)[dropped] == 0).all()          # +0 bits, not -0
        assert np.array_equal(g[top], np.where(f[top] <= 1, -(f32(1) / f32(k)), f32(0)).astype(np.float32))
        s = M.fields(state)
        assert s["k_used"] == k and s["active"] == int((f[top] <= 1).sum()) and s["nonfinite"] == int(name == "infs")
        assert words(s["threshold"])[0] == words(f[order[k - 1]])[0]
        if name != "infs":
            assert s["mean_kept"] >= s["mean_all"] and abs(float(s["mean_kept"]) - f[top].astype(np.float64).mean()) <= 1e-6
        assert ring[0].tolist() == [1, k, s["active"], state[5], state[6], state[7], int(name == "infs"), 0]


def test_all_above_one_has_no_active_element_and_a_zero_loss():
    f = INPUTS["above"]
    state, ring = M.new_state(10), M.new_ring(1)
    losses, g = M.g_loss(f, state, ring)
    assert words(losses).tolist() == [0, 0] and not words(g).any() and M.fields(state)["active"] == 0


def test_a_nan_is_always_selected_and_the_loss_is_a_nan():
    f = INPUTS["nans"]
    for k in (1, 2, 3, 50, len(f)):
        state, ring = M.new_state(k), M.new_ring(1)
        losses, g = M.g_loss(f, state, ring)
        assert np.isnan(losses).all()
        s = M.fields(state)
        assert s["nonfinite"] == 1 and np.isnan(s["mean_all"]) and np.isnan(s["mean_kept"])
        assert (words(g)[[3, 50, 96][:k]] == 0).all()          # selected, but a NaN passes no gradient (clamp's mask)
        assert np.isnan(s["threshold"]) == (k <= 3)
        assert s["active"] == int((M.kept(f, k) & (f <= 1)).sum())


def test_the_record_counts_and_the_ring_wraps():
    f = INPUTS["gauss"]
    state, ring = M.new_state(5), M.new_ring(4)
    for n in range(1, 8):
        bad = n in (3, 6)
        x = f.copy()
        if bad:
            x[n] = np.inf
        state[0] = n + 4
        M.g_loss(x, state, ring)
        s = M.fields(state)
        assert s["launches"] == n and s["k_used"] == n + 4 and s["nonfinite"] == (n >= 3) + (n >= 6)
        assert ring[(n - 1) % 4][0] == n and ring[(n - 1) % 4][1] == n + 4 and ring[(n - 1) % 4][6] == int(bad)
    assert not state[8:].any() and ring[:, 7].tolist() == [0, 0, 0, 0] and ring[:, 0].tolist() == [5, 6, 7, 4]
    assert [row["launch"] for row in M.curve(ring, 3, 7)] == [4, 5, 6, 7]
    state[1] = 0xFFFFFFFF          # the ordinal is a counter mod 2^32
    M.g_loss(f, state, ring)
    assert state[1] == 0 and ring[0xFFFFFFFF % 4][0] == 0
