"""Host side of the input pipeline (locate_amd/data.py): the random parameter records and the epoch bookkeeping.  No GPU, no
library: the kernel call is replaced by a stub that records what it was asked for."""
import math

import numpy as np
import pytest
import torch

from locate_amd import data
from locate_amd.data import InputPipeline, draw_params

H, W, S = 157, 128, 64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_draws_are_deterministic_per_seed():
    a, b, c = (draw_params(gen(s), 500, H, W, S, True) for s in (7, 7, 8))
    assert a.dtype == data.PARAM_DTYPE and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()


@pytest.mark.parametrize("augment", [False, True])
def test_crops_and_factors_are_in_range(augment):
    r = draw_params(gen(1), 5000, H, W, S, augment)
    assert (r["top"] >= 0).all() and (r["left"] >= 0).all()
    assert (r["top"] + r["side"] <= H).all() and (r["left"] + r["side"] <= W).all()
    lo = int(round(math.sqrt(0.75 * H * W)))
    fallback = (r["side"] == min(H, W)) & (r["top"] == (H - min(H, W)) // 2) & (r["left"] == (W - min(H, W)) // 2)
    assert (((r["side"] >= lo) & (r["side"] <= min(H, W))) | fallback).all()
    assert len(np.unique(r["side"])) > 3 and len(np.unique(r["top"])) > 10
    # both ends of the inclusive position range are reached
    assert ((r["top"] + r["side"]) == H).any() and (r["top"] == 0).any() and ((r["left"] + r["side"]) == W).any()
    if augment:
        for k in ("brightness", "contrast", "saturation"):
            assert (r[k] >= np.float32(0.8)).all() and (r[k] <= np.float32(1.2)).all() and r[k].std() > 0.05
        ops = np.stack([(r["order"] >> (4 * k)) & 15 for k in range(4)], axis=1)
        assert (np.sort(ops, axis=1) == np.arange(4)).all()                       # a permutation of the four ops
        assert len(np.unique(r["order"])) == 24
    else:
        assert not r["flip"].any() and (r["order"] == data.PLAIN_ORDER).all()
        assert (r["brightness"] == 1).all() and (r["contrast"] == 1).all() and (r["saturation"] == 1).all()


def test_fallback_and_flip_shares():
    r = draw_params(gen(3), 20000, H, W, S, True)
    # a try succeeds when sqrt(H W u) rounds to at most 128: p = (128.5^2 / (H W) - 0.75) / 0.25; ten tries
    p = (128.5 ** 2 / (H * W) - 0.75) / 0.25
    analytic = (1 - p) ** 10
    assert abs(analytic - 0.0341) < 1e-3
    centred = (r["side"] == 128) & (r["top"] == (H - 128) // 2) & (r["left"] == 0)
    # the centred square can also be drawn by an accepted try (side 128, top 14 of 30 positions, left 0 is forced)
    accepted_centred = (1 - analytic) * ((128.5 ** 2 - 127.5 ** 2) / (H * W) / 0.25 / p) / (H - 128 + 1)
    share = centred.mean() - accepted_centred
    print("fallback share %.4f (analytic %.4f), flip share %.4f" % (share, analytic, r["flip"].mean()))
    assert abs(share - analytic) < 0.01
    assert abs(r["flip"].mean() - 0.5) < 0.02


class StubStore:
    def __init__(self, n):
        self.N, self.H, self.W, self.device = n, H, W, torch.device("cpu")

    def __len__(self):
        return self.N


class Recorder(InputPipeline):
    """the kernel call replaced: notes the indices and records, fills the outputs with the batch number"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def _run(self, idx, params, out_real, out_aug):
        data.validate(idx, params, self.store.N, H, W, self.side_lo, min(H, W))
        self.calls.append((idx.copy(), params.copy()))
        out_real.fill_(len(self.calls))
        out_aug.fill_(-len(self.calls))


def test_epochs_visit_every_image_once():
    n, batch = 103, 8
    p = Recorder(StubStore(n), S, batch, seed=5)
    per = n // batch
    for _ in range(3 * per):
        real, aug = p.next_batch()
        assert real.shape == (batch, 3, S, S) and aug.shape == real.shape
    assert p.epoch == 2 and p.pos == per
    for e in range(3):
        calls = p.calls[e * per:(e + 1) * per]
        real_idx = np.concatenate([c[0][:batch] for c in calls])
        aug_idx = np.concatenate([c[0][batch:] for c in calls])
        for idx in (real_idx, aug_idx):
            assert len(idx) == per * batch == len(np.unique(idx)) and idx.min() >= 0 and idx.max() < n
        assert not np.array_equal(real_idx, aug_idx)                               # two independent shuffles
        for c in calls:
            assert not c[1]["flip"][:batch].any() and (c[1]["order"][:batch] == data.PLAIN_ORDER).all()
            assert (c[1]["order"][batch:] != data.PLAIN_ORDER).all()
    first = [np.concatenate([c[0] for c in p.calls[e * per:(e + 1) * per]]) for e in range(3)]
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])


def test_overfit_repeats_the_first_pair():
    p = Recorder(StubStore(40), S, 4, seed=1, overfit=True)
    a = [t.clone() for t in p.next_batch()]
    out_r, out_a = torch.zeros(4, 3, S, S), torch.zeros(4, 3, S, S)
    for _ in range(3):
        r, g = p.next_batch(out_r, out_a)
        assert r is out_r and g is out_a and torch.equal(r, a[0]) and torch.equal(g, a[1])
    assert len(p.calls) == 1


def test_state_dict_round_trip_continues_the_sequence():
    n, batch = 50, 4
    p = Recorder(StubStore(n), S, batch, seed=11)
    for _ in range(17):                                      # into the second epoch (12 batches per epoch)
        p.next_batch()
    state = p.state_dict()
    for _ in range(20):                                      # across another epoch boundary
        p.next_batch()
    q = Recorder(StubStore(n), S, batch, seed=999)           # another seed: everything must come from the state
    q.load_state_dict(state)
    for _ in range(20):
        q.next_batch()
    assert (q.epoch, q.pos) == (p.epoch, p.pos)
    for (ia, pa), (ib, pb) in zip(p.calls[17:], q.calls):
        assert np.array_equal(ia, ib) and pa.tobytes() == pb.tobytes()


def test_arguments_are_checked():
    with pytest.raises(ValueError):
        InputPipeline(StubStore(3), S, 4, seed=0)
    with pytest.raises(ValueError):
        InputPipeline(StubStore(30), 30, 4, seed=0)
    p = Recorder(StubStore(30), S, 4, seed=0)
    with pytest.raises(ValueError):
        p.next_batch(out_real=torch.zeros(4, 3, S, S + 4))
    rec = draw_params(gen(0), 2, H, W, S, False)
    with pytest.raises(ValueError):
        data.validate(np.array([0, 30]), rec, 30, H, W, 111, 128)
    rec["top"][1] = H - rec["side"][1] + 1
    with pytest.raises(ValueError):
        data.validate(np.array([0, 1]), rec, 30, H, W, 111, 128)
