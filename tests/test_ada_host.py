"""AdaptiveDiffAugment's host side, without a GPU: the parameter stream it shares with DiffAugment, the gate uniforms, the state that a
resume carries, the refusals, and the command line's error paths."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ada_model as A  # noqa: E402

FULL = "color,translation,cutout"


def rows_of(aug):
    """what draw() would upload, without a device: the class's own draw with the upload left out"""
    aug.upload = lambda rows: rows
    return aug.draw()


def test_plumbing():
    from locate_amd import AdaptiveDiffAugment, DiffAugment, augment, build
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert issubclass(AdaptiveDiffAugment, DiffAugment)
    assert EXPECTED_ABI >= 23 and "ada.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ada.hip"))
    assert len(PROTOTYPES["locate_ada_gate"][1]) == 6 and len(PROTOTYPES["locate_ada_observe"][1]) == 11
    with open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "locate_hip.h")) as f:
        header = f.read()
    assert "int locate_ada_gate(" in header and "int locate_ada_observe(" in header
    # one layout: the package's names of the record's words are the model's
    assert augment.ADA_FIELDS == A.FIELDS and augment.ADA_STATE_WORDS == A.STATE_WORDS and augment.ADA_RING_WORDS == A.RING_WORDS
    assert augment.GATE_WORD == A.GATE_WORD and augment._GATE_CAP == A.GATE_CAP
    assert augment.ada_step(64, 4, 500) == A.step_constant(64, 4, 500)


def test_words_0_to_8_are_diffaugments_draw_after_draw():
    from locate_amd import AdaptiveDiffAugment, DiffAugment
    for policy in (FULL, "translation", "color,cutout"):
        plain = DiffAugment(S=64, batch=5, policy=policy, seed=42, device="cpu")
        adaptive = AdaptiveDiffAugment(S=64, batch=5, policy=policy, seed=42, device="cpu")
        for _ in range(4):
            want, got = rows_of(plain), rows_of(adaptive)
            assert got.shape == (20, 12) and got.dtype == np.float32
            assert np.array_equal(got[:, :9].view(np.uint32), want[:, :9].view(np.uint32))
            assert not want[:, 9:].any()
            g = got[:, 9:]
            assert g.min() >= 0.0 and g.max() < 1.0 and len(np.unique(g)) == g.size


def test_gate_uniforms_are_their_own_stream_and_stay_below_one():
    from locate_amd import AdaptiveDiffAugment
    a = AdaptiveDiffAugment(S=32, batch=2, seed=7, device="cpu")
    want = torch.rand(8, 3, generator=torch.Generator().manual_seed(7 + 0xADA), dtype=torch.float64).numpy()
    assert np.array_equal(rows_of(a)[:, 9:], A.gate_uniforms(want))
    # a generator that returns the largest float64 below 1 everywhere: fp32 rounding would give 1.0, the draw gives the cap
    real_rand = torch.rand

    def almost_one(*size, **kw):
        return torch.full(size, 1.0 - 2.0 ** -53, dtype=kw["dtype"]) if size[1] == 3 else real_rand(*size, **kw)
    torch.rand = almost_one
    try:
        g = rows_of(a)[:, 9:]
    finally:
        torch.rand = real_rand
    assert (g == A.GATE_CAP).all() and g.max() < 1.0


def test_constructor_settings_and_refusals():
    from locate_amd import AdaptiveDiffAugment
    a = AdaptiveDiffAugment(S=64, batch=64, seed=1, device="cpu")
    assert (a.target, a.interval, a.kimg, a.initial_p, a.p_max, a.capacity) == (0.6, 4, 500.0, 0.0, 1.0, 4096)
    assert a.step == np.float32(64 * 4 / 500000.0) and a.step.dtype == np.float32
    assert AdaptiveDiffAugment(S=64, batch=64, device="cpu", kimg=float("inf"), initial_p=1.0).step == 0.0
    assert a.status() == {"p": 0.0, "r_t": 0.0, "updates": 0, "ups": 0, "downs": 0, "nonfinite": 0}          # no device needed
    assert a.flush() == [] and a.curve() == []
    for bad in (dict(kimg=0), dict(kimg=-1.0), dict(kimg=float("nan")), dict(p_max=0.0), dict(p_max=1.5), dict(initial_p=-0.1),
                dict(initial_p=0.8, p_max=0.5), dict(interval=0), dict(target=float("nan")), dict(capacity=0), dict(policy="")):
        with pytest.raises(ValueError):
            AdaptiveDiffAugment(S=64, batch=8, device="cpu", **bad)


def test_state_dict_round_trip_and_cross_class_refusal(tmp_path):
    from locate_amd import AdaptiveDiffAugment, DiffAugment
    kw = dict(S=32, batch=3, policy=FULL, seed=5, device="cpu", target=0.4, interval=3, kimg=2.0, initial_p=0.25, p_max=0.75)
    a = AdaptiveDiffAugment(**kw)
    for _ in range(3):
        rows_of(a)
    # a record as a run would leave it: p moved, a window open
    record, ring = A.new_state(0.25), A.new_ring(4)
    for it in range(1, 5):
        A.observe(np.ones(3, np.float32), it, record, ring, 3, 0.4, a.step, 0.75)
    a._record, a.observations, a._window_seen, a._ring_rows, a._flushed = record.copy(), 4, 1, 1, 1
    a._curve = ring[:1].copy()
    torch.save({"augment": a.state_dict()}, str(tmp_path / "s.torch"))
    saved = torch.load(str(tmp_path / "s.torch"), map_location="cpu", weights_only=True)["augment"]
    assert saved["adaptive"] is True and saved["settings"]["interval"] == 3 and tuple(saved["record"].shape) == (16,)
    b = AdaptiveDiffAugment(**kw)
    b.load_state_dict(saved)
    assert b.status() == a.status() and b.status()["p"] == float(np.float32(0.25) + a.step) and b.status()["ups"] == 1
    assert (b.observations, b._window_seen, b._ring_rows, b._flushed) == (4, 1, 1, 1)
    assert b.curve() == a.curve() == A.curve(ring, 0, 1)
    for _ in range(2):          # both streams continue
        assert np.array_equal(rows_of(a), rows_of(b))
    # other settings, and the other class either way
    with pytest.raises(ValueError, match="ran with"):
        AdaptiveDiffAugment(**dict(kw, interval=4)).load_state_dict(saved)
    with pytest.raises(ValueError, match="AdaptiveDiffAugment"):
        DiffAugment(S=32, batch=3, policy=FULL, seed=5, device="cpu").load_state_dict(saved)
    with pytest.raises(ValueError, match="plain DiffAugment"):
        b.load_state_dict(DiffAugment(S=32, batch=3, policy=FULL, seed=5, device="cpu").state_dict())
    # and a plain state still loads into a plain augment
    DiffAugment(S=32, batch=3, policy=FULL, seed=5, device="cpu").load_state_dict(DiffAugment(S=32, batch=3, policy=FULL, seed=6, device="cpu").state_dict())


def test_an_adaptive_augment_beside_a_reducer_is_refused():
    from locate_amd import AdaptiveDiffAugment, DiffAugment, TrainLoop

    class Step:
        reducer_g = reducer_d = None

    step = Step()
    step.augment = AdaptiveDiffAugment(S=32, batch=2, device="cpu")
    TrainLoop(step)
    step.reducer_d = object()
    with pytest.raises(ValueError, match="data-parallel"):
        TrainLoop(step)
    step.augment = DiffAugment(S=32, batch=2, device="cpu")
    TrainLoop(step)          # a plain augment has no p to steer


BASE = ["--store", "none.npy", "--image-size", "64", "--batch", "8", "--out", "nowhere"]


@pytest.mark.parametrize("extra, message", [
    (["--ada-target", "0.6"], "--ada-target steers --diffaugment"),
    (["--diffaugment", FULL, "--ada-target", "inf"], "--ada-target must be a finite number"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-kimg", "0"], "--ada-kimg must be > 0"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-kimg", "-3"], "--ada-kimg must be > 0"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-interval", "0"], "--ada-interval must be >= 1"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-p-max", "0"], r"--ada-p-max must be in \(0, 1\]"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-p-max", "1.25"], r"--ada-p-max must be in \(0, 1\]"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-initial-p", "0.9", "--ada-p-max", "0.5"], "--ada-initial-p must be in"),
    (["--diffaugment", FULL, "--ada-target", "0.6", "--ada-initial-p", "-0.5"], "--ada-initial-p must be in"),
])
def test_command_line_error_paths(extra, message, capsys):
    import re
    from locate_amd.run import main
    with pytest.raises(SystemExit) as stop:
        main(BASE + extra)
    assert stop.value.code == 2
    assert re.search(message, capsys.readouterr().err)


def test_command_line_defaults_are_the_papers():
    from locate_amd.run import parser
    args = parser().parse_args(BASE)
    assert (args.ada_target, args.ada_kimg, args.ada_interval, args.ada_initial_p, args.ada_p_max) == (None, 500.0, 4, 0.0, 1.0)
