"""LeCam's host side, without a GPU: construction and its refusals, the state that a resume carries (unflushed ring rows included),
the refusal beside a data-parallel reducer, and the command line's error paths."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lecam_model as L  # noqa: E402


def test_plumbing():
    from locate_amd import LeCam, build, lecam
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert LeCam is lecam.LeCam
    assert EXPECTED_ABI >= 24 and "lecam.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "lecam.hip"))
    assert os.path.exists(os.path.join(build.CSRC, "dloss.h"))
    assert len(PROTOTYPES["locate_d_loss_lecam"][1]) == 14 and len(PROTOTYPES["locate_lecam_observe"][1]) == 9
    with open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "locate_hip.h")) as f:
        header = f.read()
    assert "int locate_d_loss_lecam(" in header and "int locate_lecam_observe(" in header
    # one layout: the package's names of the record's words are the model's
    assert lecam.FIELDS == L.FIELDS and lecam.STATE_WORDS == L.STATE_WORDS and lecam.RING_WORDS == L.RING_WORDS
    for decay in (0.99, 0.999, 0.0, 1.0, 0.75):
        assert lecam.lecam_rate(decay) == L.rate_constant(decay) and lecam.lecam_rate(decay).dtype == np.float32
    # both files take the hinge arithmetic from the one header
    for name in ("loss.hip", "lecam.hip"):
        with open(os.path.join(build.CSRC, name)) as f:
            assert '#include "dloss.h"' in f.read()


def test_construction_needs_no_gpu_and_refuses_bad_settings():
    from locate_amd import LeCam
    a = LeCam(batch=64)
    assert (a.weight, a.decay, a.warmup, a.one_sided, a.capacity) == (0.3, 0.99, 1000, True, 4096)
    assert a.rate == np.float32(1.0 - 0.99) and a._state is None
    assert a.status() == {"anchor_real": 0.0, "anchor_fake": 0.0, "observations": 0, "accepted": 0, "nonfinite": 0, "active": False}
    assert a.flush() == [] and a.curve() == []
    for bad in (dict(batch=0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=1e39), dict(decay=-0.1),
                dict(decay=1.5), dict(decay=float("nan")), dict(warmup=-1), dict(warmup=1 << 31), dict(capacity=0)):
        with pytest.raises(ValueError):
            LeCam(**dict(dict(batch=8), **bad))
    # no CPU path: logits that are not on the GPU are refused before anything is launched or allocated
    x = torch.zeros(8)
    b = LeCam(batch=8)
    with pytest.raises(TypeError, match="no CPU path"):
        b.d_loss(x, x, x, 100.0)
    with pytest.raises(TypeError, match="no CPU path"):
        b.observe(x, x)
    assert b._state is None and b.observations == 0


def run_model(n, capacity, rate):
    state, ring = L.new_state(), L.new_ring(capacity)
    rng = np.random.default_rng(4)
    for it in range(1, n + 1):
        L.observe(rng.standard_normal(5).astype(np.float32), rng.standard_normal(5).astype(np.float32), it, state, ring, rate)
    return state, ring


def test_state_dict_round_trip_and_refusal_of_other_settings(tmp_path):
    from locate_amd import LeCam
    kw = dict(batch=5, weight=0.25, decay=0.75, warmup=2, one_sided=False, capacity=4)
    a = LeCam(**kw)
    # as a run would leave it: six observations through a ring of four rows, the first three flushed
    state, ring = run_model(6, 4, a.rate)
    early = run_model(3, 4, a.rate)[1]
    a._record, a.observations, a._flushed = state.copy(), 6, 3
    a._curve = early[:3].copy()
    a._pending = np.stack([ring[k % 4] for k in (3, 4, 5)])
    torch.save({"lecam": a.state_dict()}, str(tmp_path / "s.torch"))
    saved = torch.load(str(tmp_path / "s.torch"), map_location="cpu", weights_only=True)["lecam"]
    assert saved["settings"] == dict(kw) and tuple(saved["record"].shape) == (16,) and saved["observations"] == 6
    assert tuple(saved["ring_rows"].shape) == (3, 8) and tuple(saved["curve"].shape) == (3, 8)
    b = LeCam(**kw)
    b.load_state_dict(saved)
    assert b.status() == a.status() and b.status()["accepted"] == 6 and b.status()["active"] is True
    assert b.status()["anchor_real"] == float(L.fields(state)["alpha_r"])
    assert (b.observations, b._flushed) == (6, 3) and b.curve() == a.curve() == L.curve(early, 0, 3)
    assert b.flush() == L.curve(ring, 3, 6) and b.curve() == L.curve(early, 0, 3) + L.curve(ring, 3, 6) and b.flush() == []
    # a smaller ring keeps the newest unflushed rows
    c = LeCam(**dict(kw, capacity=2))
    c.load_state_dict(saved)
    assert c.flush() == L.curve(ring, 4, 6)
    # other settings are refused, each of the four
    for other in (dict(weight=0.3), dict(decay=0.5), dict(warmup=3), dict(one_sided=True)):
        with pytest.raises(ValueError, match="ran with"):
            LeCam(**dict(kw, **other)).load_state_dict(saved)
    with pytest.raises(ValueError, match="damaged"):
        b.load_state_dict(dict(saved, observations=2))


def test_a_lecam_beside_a_reducer_is_refused():
    from locate_amd import LeCam, TrainLoop

    class Step:
        reducer_g = reducer_d = None
        augment = None

    step = Step()
    step.lecam = LeCam(batch=2)
    TrainLoop(step)
    for which in ("reducer_d", "reducer_g"):
        setattr(step, which, object())
        with pytest.raises(ValueError, match="LeCam regulariser with a data-parallel reducer"):
            TrainLoop(step)
        setattr(step, which, None)
    step.lecam, step.reducer_d = None, object()
    TrainLoop(step)          # a reducer alone is no business of this check


BASE = ["--store", "none.npy", "--image-size", "64", "--batch", "8", "--out", "nowhere"]


@pytest.mark.parametrize("extra, message", [
    (["--lecam", "inf"], "--lecam must be a finite number"),
    (["--lecam", "nan"], "--lecam must be a finite number"),
    (["--lecam", "0.3", "--lecam-decay", "1.5"], r"--lecam-decay must be in \[0, 1\]"),
    (["--lecam", "0.3", "--lecam-decay", "-0.5"], r"--lecam-decay must be in \[0, 1\]"),
    (["--lecam", "0.3", "--lecam-decay", "nan"], r"--lecam-decay must be in \[0, 1\]"),
    (["--lecam", "0.3", "--lecam-warmup", "-1"], "--lecam-warmup must be in"),
    (["--lecam"], "expected one argument"),
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
    assert (args.lecam, args.lecam_decay, args.lecam_warmup, args.lecam_two_sided) == (None, 0.99, 1000, False)
    args = parser().parse_args(BASE + ["--lecam", "0", "--lecam-two-sided"])
    assert args.lecam == 0.0 and args.lecam_two_sided is True
