"""csrc/lecam.hip on the MI355X, the two kernels alone: against the numpy definition (tests/helpers/lecam_model.py) with == on the raw
words, against train.d_loss where the regulariser is inactive, with non-finite logits, through a small ring, between guard words.

B in 1, 8, 64, 257, 1000: one element, part of a wave, one wave's worth, and two sizes at which a thread adds more than one element
(257: a single thread does; 1000: most do, not all)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lecam_model as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 8, 64, 257, 1000]
SENTINEL = 0x7FC0DEAD
GAMMA = 100.0
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def stream():
    return torch.cuda.current_stream().cuda_stream


def words(x):
    return np.ascontiguousarray(x).view(np.uint32)


_LOGITS = {}


def logits(B):
    """(t, f, a), float32 on the host, made once per size: D(real) around +0.5, D(G(z)) around -0.5, so both clamps of the one-sided
    form and both hinge masks see either sign"""
    if B not in _LOGITS:
        rng = np.random.default_rng(900 + B)
        t, f, a = (rng.standard_normal(B) * 1.5 + shift for shift in (0.5, -0.5, 0.4))
        out = tuple(x.astype(np.float32) for x in (t, f, a))
        for x in out:
            x.setflags(write=False)
        _LOGITS[B] = out
    return _LOGITS[B]


def anchors(accepted, alpha_r=0.3125, alpha_f=-0.4375):
    state = L.new_state()
    state[0], state[1], state[2], state[3], state[5] = L._bits(alpha_r), L._bits(alpha_f), accepted, accepted, accepted
    return state


class Guarded:
    """int32 words inside a larger allocation, `offset` words past a 16-byte boundary, between sentinel guards"""

    def __init__(self, values, offset=1):
        values = np.ascontiguousarray(values).view(np.int32)
        self.n, self.offset = values.size, offset
        self.flat = torch.full((values.size + 64,), SENTINEL, dtype=torch.int32, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[32 + offset:32 + offset + values.size]
        self.view.copy_(torch.from_numpy(values.reshape(-1).copy()).to(DEV))

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        return self.view.cpu().numpy().view(np.uint32)

    def intact(self):
        host = self.flat.cpu().numpy()
        return bool((host[:32 + self.offset] == SENTINEL).all() and (host[32 + self.offset + self.n:] == SENTINEL).all())


def launch_d_loss(t, f, a, state, weight, one_sided, warmup, gamma=GAMMA):
    """the raw entry, every buffer between guards; (losses[4], g_true, g_fake, g_aug) as uint32 words, state words afterwards"""
    from locate_amd._lib import check, lib
    B = len(t)
    bufs = [Guarded(x, k % 4) for k, x in enumerate((t, f, a, state))]
    outs = [Guarded(np.full(n, SENTINEL, np.int32), k % 3) for k, n in enumerate((4, B, B, B))]
    check(lib().locate_d_loss_lecam(bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(), B, gamma, bufs[3].ptr(), weight, int(one_sided), warmup,
                                    outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), stream()), "locate_d_loss_lecam")
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + outs)
    for b, x in zip(bufs, (t, f, a, state)):          # inputs and the record are read only
        assert np.array_equal(b.host(), words(x).reshape(-1))
    return [o.host() for o in outs]


def launch_observe(t, g, iteration, state, ring, rate):
    """the raw entry; updates `state` and `ring` (host uint32 arrays) from the device's"""
    from locate_amd._lib import check, lib
    bufs = [Guarded(t, 1), Guarded(g, 2), Guarded(state, 3), Guarded(ring, 0)]
    check(lib().locate_lecam_observe(bufs[0].ptr(), bufs[1].ptr(), len(t), iteration, bufs[2].ptr(), bufs[3].ptr(), len(ring), float(rate),
                                     stream()), "locate_lecam_observe")
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    assert np.array_equal(bufs[0].host(), words(t)) and np.array_equal(bufs[1].host(), words(g))
    state[:] = bufs[2].host()
    ring[:] = bufs[3].host().reshape(ring.shape)


def same_words(got, want):
    return all(np.array_equal(g, words(w).reshape(-1)) for g, w in zip(got, want))


# ---- 1. the loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_sided", [True, False])
@pytest.mark.parametrize("B", SIZES)
def test_the_active_loss_is_the_definition(B, one_sided):
    t, f, a = logits(B)
    state = anchors(5)
    want = L.d_loss(t, f, a, GAMMA, state, 0.3, one_sided, 5)
    got = launch_d_loss(t, f, a, state, 0.3, one_sided, 5)
    assert L.is_active(state, 0.3, 5) and want[0][3] > 0
    assert same_words(got, want)
    assert same_words(launch_d_loss(t, f, a, state, 0.3, one_sided, 5), want)          # two calls, the same bits
    # a negative weight and a warmup of 0 (an anchor has to exist: one accepted observation)
    state = anchors(1, alpha_r=-1.25, alpha_f=2.5)
    assert same_words(launch_d_loss(t, f, a, state, -0.75, one_sided, 0), L.d_loss(t, f, a, GAMMA, state, -0.75, one_sided, 0))


@pytest.mark.parametrize("B", SIZES)
def test_the_inactive_loss_is_train_d_loss_bit_for_bit(B):
    """warmup just above the accepted count, weight = 0, and no accepted observation at all: losses[0 .. 3) and the three gradients are
    what train.d_loss launches, R is 0, and the model says the same"""
    from locate_amd.train import d_loss
    t, f, a = logits(B)
    losses, g_t, g_f, g_a = d_loss(*(torch.from_numpy(x.copy()).to(DEV) for x in (t, f, a)), GAMMA)
    plain = [words(x.cpu().numpy()) for x in (losses, g_t, g_f, g_a)]
    assert g_t._base.shape == (3, B)
    for state, weight, warmup in ((anchors(5), 0.3, 6), (anchors(5), 0.0, 0), (anchors(0), 0.3, 0), (anchors(5), -0.0, 5)):
        got = launch_d_loss(t, f, a, state, weight, True, warmup)
        assert not L.is_active(state, weight, warmup)
        assert np.array_equal(got[0][:3], plain[0]) and got[0][3] == 0
        assert all(np.array_equal(g, p) for g, p in zip(got[1:], plain[1:]))
        assert same_words(got, L.d_loss(t, f, a, GAMMA, state, weight, True, warmup))
    # and one observation later it is active: the same launch, other bits
    got = launch_d_loss(t, f, a, anchors(6), 0.3, True, 6)
    assert got[0][3] != 0          # R; with a single logit the clamp may leave g_true what it was
    assert B == 1 or not np.array_equal(got[1], plain[1])


@pytest.mark.parametrize("one_sided", [True, False])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_the_loss_keeps_a_non_finite_logit(bad, one_sided):
    """in t and in f, separately: the total and R are what the definition says - never a finite number that hides the logit, except
    where the one-sided clamp legitimately removes an infinity of the harmless sign"""
    state = anchors(3)
    for which in (0, 1):
        x = [v.copy() for v in logits(64)]
        x[which][17] = bad
        want = L.d_loss(x[0], x[1], x[2], GAMMA, state, 0.3, one_sided, 0)
        got = launch_d_loss(x[0], x[1], x[2], state, 0.3, one_sided, 0)
        for g, w in zip(got, want):
            w = np.asarray(w, np.float32).reshape(-1)
            g = g.view(np.float32)
            assert np.array_equal(np.isnan(g), np.isnan(w))          # a NaN's payload is the hardware's own
            assert np.array_equal(words(g[~np.isnan(g)]), words(w[~np.isnan(w)]))
        total, R = got[0].view(np.float32)[2], got[0].view(np.float32)[3]
        assert not np.isfinite(total)
        if np.isnan(bad) or not one_sided:
            assert not np.isfinite(R)


# ---- 2. the observer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
def test_the_observer_is_the_definition(B):
    t, f, a = logits(B)
    rate = L.rate_constant(0.99)
    got_state, got_ring = L.new_state(), L.new_ring(3)
    want_state, want_ring = L.new_state(), L.new_ring(3)
    for it, (x, g) in enumerate(((t, -f), (a, t), (f, -a)), 11):          # d_gen = -f: the kernel negates it back
        launch_observe(x, g.astype(np.float32), it, got_state, got_ring, rate)
        L.observe(x, g, it, want_state, want_ring, rate)
        assert np.array_equal(got_state, want_state) and np.array_equal(got_ring, want_ring)
    s = L.fields(got_state)
    assert (s["accepted"], s["observations"], s["nonfinite"], s["rows"]) == (3, 3, 0, 3) and s["alpha_r"] != s["mean_r"]
    # rate 0 leaves an existing anchor where it is, rate 1 moves it by the whole difference
    for rate in (f32(0.0), f32(1.0)):
        launch_observe(t, -f, 14, got_state, got_ring, rate)
        L.observe(t, -f, 14, want_state, want_ring, rate)
        assert np.array_equal(got_state, want_state) and np.array_equal(got_ring, want_ring)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_the_observer_skips_and_counts_a_non_finite_logit(bad):
    t, f, _ = logits(257)
    rate = f32(0.25)
    got_state, got_ring = L.new_state(), L.new_ring(4)
    want_state, want_ring = L.new_state(), L.new_ring(4)

    def both(x, g, it):
        launch_observe(x, g, it, got_state, got_ring, rate)
        L.observe(x, g, it, want_state, want_ring, rate)
        means = got_ring[:, 3:5].copy().view(np.float32)          # a NaN mean's payload is the hardware's own: compare it as a NaN
        nan = np.isnan(means)
        assert np.array_equal(nan, np.isnan(want_ring[:, 3:5].copy().view(np.float32)))
        keep = np.ones(got_ring.shape, bool)
        keep[:, 3:5] = ~nan
        assert np.array_equal(got_ring[keep], want_ring[keep])
        keep = np.ones(16, bool)
        keep[6:8] = ~np.isnan(got_state[6:8].copy().view(np.float32))
        assert np.array_equal(got_state[keep], want_state[keep])

    tb, gb = t.copy(), (-f).astype(np.float32)
    tb[256] = bad          # the one element a thread adds to its first
    both(tb, gb, 1)          # before any anchor exists
    assert got_state[0] == 0 and got_state[1] == 0 and got_state[2] == 0 and got_state[4] == 1
    both(t, gb, 2)
    before = got_state.copy()
    gb2 = gb.copy()
    gb2[3] = bad
    both(t, gb2, 3)
    assert np.array_equal(got_state[:3], before[:3]) and got_state[4] == 2 and got_state[3] == 3 and got_state[5] == 3
    assert [row["accepted"] for row in L.curve(got_ring, 0, 3)] == [0, 1, 0]


def test_a_ring_of_two_rows_through_five_observations():
    t, f, a = logits(8)
    rate = L.rate_constant(0.5)
    got_state, got_ring = L.new_state(), L.new_ring(2)
    want_state, want_ring = L.new_state(), L.new_ring(2)
    for it in range(1, 6):
        x, g = np.roll(t, it), np.roll(f, it) * f32(it)
        launch_observe(x, g, 100 + it, got_state, got_ring, rate)
        L.observe(x, g, 100 + it, want_state, want_ring, rate)
        assert np.array_equal(got_state, want_state) and np.array_equal(got_ring, want_ring)
    assert [row["iteration"] for row in L.curve(got_ring, 3, 5)] == [104, 105] and got_state[5] == 5
    assert got_ring[0, 0] == 105 and got_ring[1, 0] == 104          # row k sits at k % capacity


def test_bad_arguments_are_refused_and_launch_nothing():
    from locate_amd._lib import lib
    t, f, a = (Guarded(x) for x in logits(8))
    state, ring, out = Guarded(L.new_state()), Guarded(L.new_ring(2)), Guarded(np.zeros(4 + 24, np.int32))
    o = out.ptr()
    h = lib()
    ok = (t.ptr(), f.ptr(), a.ptr(), 8, GAMMA, state.ptr(), 0.3, 1, 0, o, o + 16, o + 48, o + 80, stream())
    for k, v in ((0, None), (5, None), (9, None), (12, None), (3, 0), (3, -4), (6, float("nan")), (6, float("inf")), (8, -1), (1, f.ptr() + 2)):
        args = list(ok)
        args[k] = v
        assert h.locate_d_loss_lecam(*args) != 0 and b"locate_d_loss_lecam" in h.locate_last_error()
    ok = (t.ptr(), f.ptr(), 8, 1, state.ptr(), ring.ptr(), 2, 0.01, stream())
    for k, v in ((0, None), (1, None), (4, None), (5, None), (2, 0), (6, 0), (7, float("nan")), (7, -0.25), (7, 1.5), (4, state.ptr() + 1)):
        args = list(ok)
        args[k] = v
        assert h.locate_lecam_observe(*args) != 0 and b"locate_lecam_observe" in h.locate_last_error()
    torch.cuda.synchronize()
    assert not state.host().any() and not ring.host().any() and not out.host().any()


# ---- 3. the class ----------------------------------------------------------------------------------------------------------------------
def test_the_class_drives_both_kernels():
    from locate_amd import LeCam
    B = 64
    t, f, a = logits(B)
    T, F, A = (torch.from_numpy(x.copy()).to(DEV) for x in (t, f, a))
    lecam = LeCam(batch=B, weight=0.3, decay=0.75, warmup=2, one_sided=True, capacity=2, device=DEV)
    state, ring = L.new_state(), L.new_ring(8)
    actives = []
    for it in range(1, 5):
        losses, g_t, g_f, g_a = lecam.d_loss(T, F, A, GAMMA)
        want = L.d_loss(t, f, a, GAMMA, state, 0.3, True, 2)
        assert g_t._base.shape == (3, B) and losses.shape == (4,)
        assert same_words([words(x.cpu().numpy()) for x in (losses, g_t, g_f, g_a)], want)
        actives.append(lecam.status()["active"])
        lecam.observe(T * it, -F, iteration=None)
        L.observe(t * f32(it), -f, it, state, ring, lecam.rate)
    assert actives == [False, False, True, True]
    assert np.array_equal(words(lecam.state.cpu().numpy()), state)
    s = L.fields(state)
    assert lecam.status() == {"anchor_real": float(s["alpha_r"]), "anchor_fake": float(s["alpha_f"]), "observations": 4, "accepted": 4,
                              "nonfinite": 0, "active": True}
    saved = lecam.state_dict()          # before any flush: the two rows the ring of two still holds travel with it
    assert tuple(saved["ring_rows"].shape) == (2, 8) and tuple(saved["curve"].shape) == (0, 8)
    assert lecam.flush() == L.curve(ring, 2, 4) and lecam.curve() == L.curve(ring, 2, 4) and lecam.flush() == []
    other = LeCam(batch=B, weight=0.3, decay=0.75, warmup=2, one_sided=True, capacity=2, device=DEV)
    other.load_state_dict(saved)
    assert torch.equal(other.state, lecam.state) and torch.equal(other.ring, lecam.ring)
    assert other.flush() == L.curve(ring, 2, 4)
    address = lecam.state.data_ptr()
    lecam.load_state_dict(saved)          # into a live one: the addresses a captured graph reads stay
    assert lecam.state.data_ptr() == address and torch.equal(other.state, lecam.state) and torch.equal(other.ring, lecam.ring)
    with pytest.raises(ValueError, match="batches of 64"):
        lecam.observe(T[:8], -F[:8])
