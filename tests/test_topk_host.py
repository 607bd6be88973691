"""Top-k training's host side, without a GPU: the schedule of k, construction and its refusals, the state that a resume carries
(unflushed ring rows included), that a reducer beside it is no refusal, and the command line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import topk_model as M  # noqa: E402


def test_plumbing():
    from locate_amd import TopK, build, topk, topk_k
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert TopK is topk.TopK and topk_k is topk.topk_k
    assert EXPECTED_ABI >= 25 and "topk.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "topk.hip"))
    assert len(PROTOTYPES["locate_g_loss_topk"][1]) == 9
    with open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "locate_hip.h")) as f:
        assert "int locate_g_loss_topk(" in f.read()
    # one layout: the package's names of the record's words are the model's
    assert topk.FIELDS == M.FIELDS and topk.STATE_WORDS == M.STATE_WORDS and topk.RING_WORDS == M.RING_WORDS and topk.MAX_BATCH == M.MAX_BATCH
    # both files take the G hinge from the one header
    for name in ("loss.hip", "topk.hip"):
        with open(os.path.join(build.CSRC, name)) as f:
            source = f.read()
        assert '#include "gloss.h"' in source and "g_hinge_term(" in source and "g_hinge_grad(" in source


def test_the_schedule_at_dyadic_settings():
    from locate_amd import topk_k
    # gamma = 1/2, floor = 1/4, B = 64: every product is exact, and so is the hand-made list
    assert [topk_k(64, 0.5, 0.25, p) for p in range(6)] == [64, 32, 16, 16, 16, 16]
    assert [topk_k(64, 0.5, 0.0, p) for p in range(9)] == [64, 32, 16, 8, 4, 2, 1, 1, 1]          # k_min = max(1, 0): 0.5 rounds half up
    assert [topk_k(10, 0.75, 0.5, p) for p in range(5)] == [10, 8, 6, 5, 5]          # 7.5 -> 8 (half up), 5.625 -> 6, 4.21875 -> floor 5
    assert [topk_k(7, 0.5, 0.5, p) for p in range(3)] == [7, 4, 4]          # 3.5 -> 4 = ceil(3.5)
    assert topk_k(64, 1.0, 0.5, 10 ** 6) == 64 and topk_k(1, 0.5, 0.0, 99) == 1 and topk_k(64, 0.5, 1.0, 3) == 64
    assert topk_k(4096, 0.99, 0.5, 10 ** 9) == 2048          # the power underflows to 0: the floor holds
    for B in (1, 5, 64, 1000):
        for gamma in (0.99, 0.75, 0.5, 1.0):
            for floor in (0.0, 0.3, 0.5, 1.0):
                ks = [topk_k(B, gamma, floor, p) for p in range(400)]
                assert ks == [M.topk_k(B, gamma, floor, p) for p in range(400)]
                assert ks[0] == B and all(a >= b for a, b in zip(ks, ks[1:]))          # from B, never up
                assert min(ks) >= max(1, int(np.ceil(floor * B))) and max(ks) <= B


def test_construction_needs_no_gpu_and_refuses_bad_settings():
    from locate_amd import TopK
    a = TopK(batch=64)
    assert (a.gamma, a.floor, a.capacity, a.k) == (0.99, 0.5, 4096, 64) and a._state is None
    assert a.status() == {"k": 64, "k_used": 0, "launches": 0, "nonfinite": 0, "active": 0, "threshold": 0.0, "mean_all": 0.0, "mean_kept": 0.0}
    assert a.flush() == [] and a.curve() == []
    for bad in (dict(batch=0), dict(batch=4097), dict(gamma=0.0), dict(gamma=1.5), dict(gamma=float("nan")), dict(floor=-0.1), dict(floor=1.5),
                dict(floor=float("nan")), dict(every=0), dict(every=1 << 31), dict(capacity=0)):
        with pytest.raises(ValueError):
            TopK(**dict(dict(batch=8), **bad))
    # the schedule moves the host's copy of k; without a device record nothing is copied anywhere
    b = TopK(batch=8, gamma=0.5, floor=0.25, every=3)
    assert [b.scheduled_k(it) for it in range(8)] == [8, 8, 8, 4, 4, 4, 2, 2]
    assert b.advance(2) is False and b.k == 8 and b.advance(3) is True and b.k == 4 and b.advance(5) is False
    assert b.set_k(0) is True and b.k == 0 and b.set_k(-3) is True and b.k == -3 and b.status()["k"] == -3 and b._state is None
    with pytest.raises(ValueError):
        b.set_k(1 << 31)
    # no CPU path: logits that are not on the GPU are refused before anything is launched or allocated
    with pytest.raises(TypeError, match="no CPU path"):
        b.g_loss(torch.zeros(8))
    assert b._state is None


def run_model(n, capacity, k=3):
    state, ring = M.new_state(k), M.new_ring(capacity)
    rng = np.random.default_rng(4)
    for _ in range(n):
        M.g_loss(rng.standard_normal(5).astype(np.float32), state, ring)
    return state, ring


def test_state_dict_round_trip_and_refusal_of_other_settings(tmp_path):
    from locate_amd import TopK
    kw = dict(batch=5, gamma=0.75, floor=0.25, every=7, capacity=4)
    a = TopK(**kw)
    # as a run would leave it: six launches through a ring of four rows, the first three flushed
    state, ring = run_model(6, 4)
    early = run_model(3, 4)[1]
    a._record, a._flushed = state.copy(), 3
    a._curve = early[:3].copy()
    a._pending = np.stack([ring[n % 4] for n in (3, 4, 5)])
    torch.save({"topk": a.state_dict()}, str(tmp_path / "s.torch"))
    saved = torch.load(str(tmp_path / "s.torch"), map_location="cpu", weights_only=True)["topk"]
    assert saved["settings"] == dict(kw) and tuple(saved["record"].shape) == (16,)
    assert tuple(saved["ring_rows"].shape) == (3, 8) and tuple(saved["curve"].shape) == (3, 8)
    b = TopK(**kw)
    b.load_state_dict(saved)
    s = M.fields(state)
    assert b.status() == a.status() and b.k == 3 and b.status()["launches"] == 6 and b.status()["k_used"] == 3
    assert b.status()["threshold"] == float(s["threshold"]) and b.status()["mean_kept"] == float(s["mean_kept"])
    assert b._flushed == 3 and b.curve() == a.curve() == M.curve(early, 0, 3)
    assert b.flush() == M.curve(ring, 3, 6) and b.curve() == M.curve(early, 0, 3) + M.curve(ring, 3, 6) and b.flush() == []
    assert [row["launch"] for row in b.curve()] == [1, 2, 3, 4, 5, 6]
    # a smaller ring keeps the newest unflushed rows
    c = TopK(**dict(kw, capacity=2))
    c.load_state_dict(saved)
    assert c.flush() == M.curve(ring, 4, 6)
    # other settings are refused, each of the four
    for other in (dict(batch=6), dict(gamma=0.5), dict(floor=0.5), dict(every=8)):
        with pytest.raises(ValueError, match="ran with"):
            TopK(**dict(kw, **other)).load_state_dict(saved)
    damaged = saved["record"].clone()
    damaged[1] = 2
    with pytest.raises(ValueError, match="damaged"):
        b.load_state_dict(dict(saved, record=damaged))


def test_a_topk_beside_a_reducer_is_not_refused_and_the_loop_moves_k():
    from locate_amd import TopK, TrainLoop

    class Step:
        reducer_g = reducer_d = None
        augment = lecam = None

        def d_forward_backward(self, latent, real, aug):
            return {"d_true": None}

        def d_optimizer(self):
            pass

        def g_forward_backward(self, latent):
            return {"k_at_the_g_step": self.topk.k}

        def g_optimizer(self):
            pass

    step = Step()
    step.topk = TopK(batch=8, gamma=0.5, floor=0.25, every=2)
    step.reducer_d = step.reducer_g = object()
    loop = TrainLoop(step)          # each rank selects within its shard; k is the same function of the iteration on every rank
    assert [loop.iteration(None, None, None)["k_at_the_g_step"] for _ in range(6)] == [8, 8, 4, 4, 2, 2] and loop.iterations == 6
    loop.iterations = 0          # what a Trainer sets before every iteration: its own count, not the sub-pass's i
    assert loop.iteration(None, None, None)["k_at_the_g_step"] == 8 and loop.i == 7


BASE = ["--store", "none.npy", "--image-size", "64", "--batch", "8", "--out", "nowhere"]


@pytest.mark.parametrize("extra, message", [
    (["--topk-floor", "1.5"], r"--topk-floor must be in \[0, 1\]"),
    (["--topk-floor", "-0.5"], r"--topk-floor must be in \[0, 1\]"),
    (["--topk-floor", "nan"], r"--topk-floor must be in \[0, 1\]"),
    (["--topk-floor", "0.5", "--topk-gamma", "0"], r"--topk-gamma must be in \(0, 1\]"),
    (["--topk-floor", "0.5", "--topk-gamma", "1.25"], r"--topk-gamma must be in \(0, 1\]"),
    (["--topk-floor", "0.5", "--topk-gamma", "nan"], r"--topk-gamma must be in \(0, 1\]"),
    (["--topk-floor", "0.5", "--topk-every", "0"], "--topk-every must be in"),
    (["--topk-gamma", "0.9"], "need --topk-floor"),
    (["--topk-every", "10"], "need --topk-floor"),
    (["--topk-floor"], "expected one argument"),
])
def test_command_line_error_paths(extra, message, capsys):
    import re
    from locate_amd.run import main
    with pytest.raises(SystemExit) as stop:
        main(BASE + extra)
    assert stop.value.code == 2
    assert re.search(message, capsys.readouterr().err)


def test_command_line_defaults():
    from locate_amd.run import parser
    args = parser().parse_args(BASE)
    assert (args.topk_floor, args.topk_gamma, args.topk_every) == (None, 0.99, None)
    args = parser().parse_args(BASE + ["--topk-floor", "0.5", "--topk-gamma", "0.75", "--topk-every", "12"])
    assert (args.topk_floor, args.topk_gamma, args.topk_every) == (0.5, 0.75, 12)
