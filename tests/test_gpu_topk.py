"""csrc/topk.hip on the MI355X, the kernel alone: against the numpy definition (tests/helpers/topk_model.py) with == on the raw words
of the losses, the gradient, the record and the ring row - in both selection forms and in the one the library chooses - against
train.g_loss where k = B, with non-finite logits, through a small ring, between guard words, under a captured graph.

B in 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096: one element, two, around one wave's worth, around the block's 256 threads (257: a
single thread holds two elements; 1000: most hold four, not all; 4096: the largest batch, sixteen each), both sides of the size from
which the library sorts instead of counting ranks."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import topk_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096]
KINDS = ["gauss", "five", "equal", "zeros", "above", "nan", "nans", "infs"]
FORMS = (0, 1, 2)          # the library's choice, rank count, sort
SENTINEL = 0x7FC0DEAD
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


def ks(B):
    return sorted({max(1, min(B, k)) for k in (1, 2, B // 2, B - 1, B)})


_LOGITS = {}


def logits(B, kind):
    """(f, ranks(f)), made once per size and kind and left unchanged"""
    if (B, kind) not in _LOGITS:
        rng = np.random.default_rng(7000 + 16 * B + KINDS.index(kind))
        gauss = (rng.standard_normal(B) * 1.5 + 0.25).astype(np.float32)
        spots = rng.permutation(B)
        if kind == "gauss":
            f = gauss
        elif kind == "five":          # heavy ties across every threshold
            f = rng.choice(np.array([-1.5, -0.25, 0.0, 0.75, 2.0], np.float32), B)
        elif kind == "equal":
            f = np.full(B, 0.375, np.float32)
        elif kind == "zeros":          # -0 and +0 are equal: the lower index first, whatever its sign
            f = np.where(rng.random(B) < 0.5, f32(-0.0), f32(0.0)).astype(np.float32)
        elif kind == "above":          # no active element
            f = (rng.random(B) + 1.5).astype(np.float32)
        elif kind == "nan":
            f = gauss
            f[spots[0]] = np.nan
        elif kind == "nans":
            f = gauss
            f[spots[:max(1, min(B // 2, 5))]] = np.nan
            f[spots[0]] = -np.nan          # the sign of a NaN orders nothing
        else:
            f = gauss
            f[spots[0]] = np.inf
            if B > 1:
                f[spots[1]] = -np.inf
            if B > 3:
                f[spots[2]], f[spots[3]] = np.inf, -np.inf
        f.setflags(write=False)
        rank = M.ranks(f)
        rank.setflags(write=False)
        _LOGITS[(B, kind)] = (f, rank)
    return _LOGITS[(B, kind)]


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


def launch(f, state, ring, form=0):
    """the raw entry, every buffer between guards; (losses[2], g) as uint32 words; `state` and `ring` updated from the device's"""
    from locate_amd._lib import check, lib
    B = len(f)
    bufs = [Guarded(f, 1), Guarded(state, 3), Guarded(ring, 2)]
    outs = [Guarded(np.full(2, SENTINEL, np.int32), 1), Guarded(np.full(B, SENTINEL, np.int32), 2)]
    check(lib().locate_g_loss_topk(bufs[0].ptr(), B, bufs[1].ptr(), bufs[2].ptr(), len(ring), form, outs[0].ptr(), outs[1].ptr(), stream()),
          "locate_g_loss_topk")
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + outs)
    assert np.array_equal(bufs[0].host(), words(f))          # the logits are read only
    state[:] = bufs[1].host()
    ring[:] = bufs[2].host().reshape(ring.shape)
    return outs[0].host(), outs[1].host()


def same_floats(got, want):
    """== on the bits, except that where the definition yields a NaN a NaN is required, not its payload"""
    got, want = words(got).reshape(-1), words(want).reshape(-1)
    nan = np.isnan(want.view(np.float32))
    return got.shape == want.shape and np.array_equal(np.isnan(got.view(np.float32)), nan) and np.array_equal(got[~nan], want[~nan])


def same_record(got, want):
    """the 16 words of a record or the 8 of a ring row: words 6, 7 (4, 5 of a row) are the two means"""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    means = slice(6, 8) if got.shape[-1] == M.STATE_WORDS else slice(4, 6)
    rest = np.ones(got.shape[-1], bool)
    rest[means] = False
    return np.array_equal(got[..., rest], want[..., rest]) and same_floats(got[..., means], want[..., means])


def both(f, rank, k, form, got_state=None, got_ring=None, want_state=None, want_ring=None, capacity=3):
    """one launch and the definition from the same record; returns (losses, g) words, the record and the definition's losses"""
    if got_state is None:
        got_state, got_ring, want_state, want_ring = M.new_state(k), M.new_ring(capacity), M.new_state(k), M.new_ring(capacity)
    want = M.g_loss(f, want_state, want_ring, rank)
    got = launch(f, got_state, got_ring, form)
    assert same_floats(got[0], want[0]), (k, form, got[0].view(np.float32), want[0])
    assert np.array_equal(got[1], words(want[1])), (k, form)
    assert same_record(got_state, want_state), (k, form, got_state, want_state)
    assert same_record(got_ring, want_ring), (k, form)
    return got, got_state, want


# ---- 1. the kernel against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", SIZES)
def test_the_launch_is_the_definition(B, kind):
    from locate_amd.train import g_loss
    f, rank = logits(B, kind)
    plain_loss, plain_g = (words(x.cpu().numpy()) for x in g_loss(torch.from_numpy(f.copy()).to(DEV)))
    for k in ks(B):
        for form in FORMS:
            got, state, want = both(f, rank, k, form)
            keep = rank < k
            assert (got[1][~keep] == 0).all()          # dropped elements: +0 bits
            if kind not in ("nan", "nans"):
                assert got[0][1] == plain_loss[0]          # loss_all is locate_g_loss, whatever k
            else:
                assert np.isnan(got[0].view(np.float32)).all() and state[2] == 1          # always selected: nothing is laundered
            if k == B:          # and so are loss_topk and the gradient
                assert np.array_equal(got[1], plain_g) and (kind in ("nan", "nans") or got[0][0] == plain_loss[0])
            if kind == "above":
                assert state[4] == 0 and not got[1].any() and not got[0].any()
            if kind == "infs":
                assert state[2] == 1 and (B == 1 or got[0].view(np.float32)[1] == np.inf)          # -Inf's hinge; B = 1 holds +Inf only


@pytest.mark.parametrize("B", [1, 64, 257, 1000])
def test_a_k_out_of_range_is_the_plain_loss(B):
    from locate_amd.train import g_loss
    f, rank = logits(B, "gauss")
    plain_loss, plain_g = (words(x.cpu().numpy()) for x in g_loss(torch.from_numpy(f.copy()).to(DEV)))
    for k in (0, -3, B + 1, -(1 << 31), (1 << 31) - 1):
        for form in FORMS:
            got, state, _ = both(f, rank, k, form)
            assert got[0][0] == plain_loss[0] and got[0][1] == plain_loss[0] and np.array_equal(got[1], plain_g)
            assert M.fields(state)["k"] == k and state[3] == B          # word 0 is the host's: the kernel leaves it


@pytest.mark.parametrize("form", FORMS)
def test_two_calls_give_the_same_bits_and_the_ring_wraps_at_four(form):
    f, rank = logits(257, "five")
    states = [M.new_state(100), M.new_state(100)]
    rings = [M.new_ring(4), M.new_ring(4)]
    first = None
    for n in range(1, 7):
        got, _, _ = both(f, rank, 100, form, states[0], rings[0], states[1], rings[1])
        first = first or got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
        assert states[0][1] == n and rings[0][(n - 1) % 4][0] == n
    assert rings[0][:, 0].tolist() == [5, 6, 3, 4]          # launch n sits at (n - 1) % capacity
    assert [row["launch"] for row in M.curve(rings[0], 2, 6)] == [3, 4, 5, 6]
    # a non-finite launch counts one in word 2, a finite one after it none; the ordinal is a counter mod 2^32
    bad, bad_rank = logits(257, "infs")
    both(bad, bad_rank, 100, form, states[0], rings[0], states[1], rings[1])
    both(f, rank, 100, form, states[0], rings[0], states[1], rings[1])
    assert states[0][2] == 1 and states[0][1] == 8 and rings[0][6 % 4][6] == 1 and rings[0][7 % 4][6] == 0
    states[0][1] = states[1][1] = 0xFFFFFFFF
    both(f, rank, 100, form, states[0], rings[0], states[1], rings[1])
    assert states[0][1] == 0 and rings[0][3][0] == 0


def test_bad_arguments_are_refused_and_launch_nothing():
    from locate_amd._lib import lib
    f, state, ring, out = Guarded(np.ones(8, np.float32)), Guarded(M.new_state(3)), Guarded(M.new_ring(2)), Guarded(np.zeros(2 + 8, np.int32))
    o = out.ptr()
    h = lib()
    ok = (f.ptr(), 8, state.ptr(), ring.ptr(), 2, 0, o, o + 8, stream())
    for n, v in ((0, None), (2, None), (3, None), (6, None), (7, None), (1, 0), (1, -4), (1, 4097), (4, 0), (4, -1), (5, 3), (5, -1),
                 (0, f.ptr() + 2), (2, state.ptr() + 1)):
        args = list(ok)
        args[n] = v
        assert h.locate_g_loss_topk(*args) != 0 and b"locate_g_loss_topk" in h.locate_last_error()
    torch.cuda.synchronize()
    assert state.host().tolist() == M.new_state(3).tolist() and not ring.host().any() and not out.host().any()


# ---- 2. the class ------------------------------------------------------------------------------------------------------------------------
def test_the_class_drives_the_kernel():
    from locate_amd import TopK
    B = 64
    f, rank = logits(B, "gauss")
    F = torch.from_numpy(f.copy()).to(DEV)
    topk = TopK(batch=B, gamma=0.5, floor=0.25, every=2, capacity=2, device=DEV)
    state, ring = M.new_state(B), M.new_ring(8)
    seen = []
    for it in range(5):
        moved = topk.advance(it)
        state[0] = M.topk_k(B, 0.5, 0.25, it // 2)
        seen.append((moved, topk.k))
        losses, g = topk.g_loss(F * (it + 1))
        want = M.g_loss(f * f32(it + 1), state, ring)
        assert losses.shape == (2,) and g.shape == (B,)
        assert np.array_equal(words(losses.cpu().numpy()), words(want[0])) and np.array_equal(words(g.cpu().numpy()), words(want[1]))
    assert seen == [(False, 64), (False, 64), (True, 32), (False, 32), (True, 16)]
    assert np.array_equal(words(topk.state.cpu().numpy()), state)
    s = M.fields(state)
    assert topk.status() == {"k": 16, "k_used": 16, "launches": 5, "nonfinite": 0, "active": s["active"], "threshold": float(s["threshold"]),
                             "mean_all": float(s["mean_all"]), "mean_kept": float(s["mean_kept"])}
    assert s["mean_kept"] > s["mean_all"] and s["threshold"] > s["mean_all"]
    saved = topk.state_dict()          # before any flush: the two rows the ring of two still holds travel with it
    assert tuple(saved["ring_rows"].shape) == (2, 8) and tuple(saved["curve"].shape) == (0, 8)
    assert topk.flush() == M.curve(ring, 3, 5) and topk.curve() == M.curve(ring, 3, 5) and topk.flush() == []
    other = TopK(batch=B, gamma=0.5, floor=0.25, every=2, capacity=2, device=DEV)
    other.load_state_dict(saved)
    assert torch.equal(other.state, topk.state) and torch.equal(other.ring, topk.ring) and other.k == 16
    assert other.flush() == M.curve(ring, 3, 5)
    address = topk.state.data_ptr()
    topk.set_k(7)
    topk.load_state_dict(saved)          # into a live one: the addresses a captured graph reads stay
    assert topk.state.data_ptr() == address and torch.equal(other.state, topk.state) and torch.equal(other.ring, topk.ring) and topk.k == 16
    with pytest.raises(ValueError, match="batches of 64"):
        topk.g_loss(F[:8])


def test_a_captured_launch_follows_set_k_between_replays():
    from locate_amd import TopK
    B = 65
    f, rank = logits(B, "five")
    F = torch.from_numpy(f.copy()).to(DEV)
    topk = TopK(batch=B, capacity=16, device=DEV)
    state, ring = M.new_state(B), M.new_ring(16)
    topk.g_loss(F)          # the eager warm-up: the record and the ring exist before the capture
    M.g_loss(f, state, ring, rank)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        losses, g = topk.g_loss(F)
    values = set()
    for k in (B, 33, 33, 1, 0, 64, 2):
        topk.set_k(k)
        state[0] = np.array([k], np.int32).view(np.uint32)[0]
        graph.replay()
        want = M.g_loss(f, state, ring, rank)
        assert np.array_equal(words(losses.cpu().numpy()), words(want[0])) and np.array_equal(words(g.cpu().numpy()), words(want[1]))
        assert np.array_equal(words(topk.state.cpu().numpy()), state) and np.array_equal(words(topk.ring.cpu().numpy()), ring)
        values.add(float(losses[0]))
    assert len(values) >= 4 and topk.status()["launches"] == 8          # the capture itself launched nothing
    assert [row["k"] for row in topk.flush()] == [B, B, 33, 33, 1, B, 64, 2]
