"""The guarded optimizer's host side (locate_amd/guard.py, the hooks in locate_amd/run.py) without a GPU: the model of the verdict
the GPU tests hold the kernel to, what the constructor refuses, the state dictionaries `Nadam` and `GuardedNadam` exchange, and
what the trainer does with the counters - the record per epoch, the stop at the limit, no save behind it."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import guard_model as GM  # noqa: E402


def test_importing_the_module_loads_no_library():
    code = ("import locate_amd.guard, locate_amd._lib as L\n"
            "from locate_amd import GuardedNadam, GuardExhausted\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_scale():
    # no limit, or a norm at or below it: exactly 1
    for max_norm, sumsq in ((0.0, 1e30), (5.0, 25.0), (5.0, 24.0), (1e30, 1e40)):
        skip, scale, c = GM.verdict(sumsq, 0, max_norm)
        assert not skip and scale == np.float32(1.0) and scale.dtype == np.float32 and c["clipped"] == 0
    # above it: max_norm / norm, divided in double, rounded once
    skip, scale, c = GM.verdict(100.0, 0, 5.0)
    assert not skip and scale == np.float32(0.5) and c["clipped"] == 1 and c["last_norm"] == 10.0 and c["last_scale"] == 0.5
    skip, scale, c = GM.verdict(9.0, 0, 1.0)
    assert scale == np.float32(1.0 / 3.0)
    # torch's clip_grad_norm_ would give max_norm / (norm + 1e-6): another number
    assert float(scale) != float(np.float32(1.0 / (3.0 + 1e-6)))
    # a norm that overflows fp32 but not fp64
    skip, scale, c = GM.verdict(1e80, 0, 1.0)
    assert scale == np.float32(1e-40) and scale > 0          # a denormal scale, not zero
    assert GM.scale_within_one_ulp(np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1))) and not GM.scale_within_one_ulp(0.5, 0.5001)


def test_model_skip_and_counters():
    c = None
    skip, scale, c = GM.verdict(4.0, 0, 1.0, True, c)          # clipped
    assert (skip, float(scale)) == (False, 0.5)
    skip, scale, c = GM.verdict(4.0, 3, 1.0, True, c)          # skipped: never clipped, scale exactly 1
    assert skip and scale == np.float32(1.0) and c["last_nonfinite"] == 3
    skip, scale, c = GM.verdict(0.0, 1, 1.0, True, c)
    assert skip and c["consecutive_skips"] == 2 and c["last_norm"] == 0.0
    skip, scale, c = GM.verdict(0.25, 0, 1.0, True, c)         # taken, below the limit
    assert not skip and scale == np.float32(1.0)
    assert {k: c[k] for k in ("steps", "skipped", "clipped", "consecutive_skips")} == {"steps": 4, "skipped": 2, "clipped": 1, "consecutive_skips": 0}
    # skip_nonfinite off: the step is taken and clipped by the norm of the finite elements, the count is still reported
    skip, scale, c = GM.verdict(16.0, 2, 1.0, False, c)
    assert not skip and scale == np.float32(0.25) and c["last_nonfinite"] == 2 and c["skipped"] == 2 and c["clipped"] == 2
    assert GM.ZERO["steps"] == 0          # the model copies its input


def test_model_global_statistics():
    nan, inf = np.float32("nan"), np.float32("inf")
    sumsq, nonfinite, n = GM.global_statistics([np.array([3.0, nan], np.float32), np.array([[4.0], [-inf], [0.0]], np.float32)])
    assert (sumsq, nonfinite, n) == (25.0, 2, 5)


# ---- the optimizer's host side -------------------------------------------------------------------------------------------------------
def params():
    torch.manual_seed(1)
    return [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]


def test_constructor_validation():
    from locate_amd import GuardedNadam, Nadam
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            GuardedNadam(params(), max_norm=bad)
    with pytest.raises(ValueError):
        GuardedNadam(params(), weight_decay=-1.0)          # Nadam's own check still holds
    opt = GuardedNadam(params())
    assert isinstance(opt, Nadam) and opt.max_norm == 0.0 and opt.skip_nonfinite is True
    opt = GuardedNadam(params(), lr=1e-3, max_norm=2, skip_nonfinite=0)
    assert opt.max_norm == 2.0 and opt.skip_nonfinite is False and opt.param_groups[0]["lr"] == 1e-3
    assert set(opt.param_groups[0]) == set(Nadam(params()).param_groups[0])          # the guard's settings are not a group's
    assert opt.counters() == GM.ZERO and list(opt.counters()) == list(GM.ZERO)          # before the first step: no device needed


def test_state_dict_interchange_with_nadam():
    from locate_amd import GuardedNadam, Nadam

    def filled(cls, **kw):
        ps = params()
        opt = cls(ps, lr=1e-3, weight_decay=0.01, **kw)
        for i, p in enumerate(ps):
            st = opt._state_for(p)
            st["exp_avg"].fill_(1.5 + i)
            st["exp_avg_sq"].fill_(2.5 + i)
            st["sched"].copy_(torch.tensor([7.0 + i, 0.123456789012345678], dtype=torch.float64))
        return ps, opt

    _, guarded = filled(GuardedNadam, max_norm=3.0)
    _, plain = filled(Nadam)
    a, b = guarded.state_dict(), plain.state_dict()
    assert a["param_groups"] == b["param_groups"] and sorted(a["state"]) == sorted(b["state"])
    for i in a["state"]:
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "sched"]
        assert all(torch.equal(a["state"][i][k], b["state"][i][k]) and a["state"][i][k].dtype == b["state"][i][k].dtype for k in a["state"][i])
    for src, cls, kw in ((a, Nadam, {}), (b, GuardedNadam, {"max_norm": 9.0, "skip_nonfinite": False})):
        ps = params()
        fresh = cls(ps, **kw)
        fresh.load_state_dict(src)
        assert fresh.param_groups[0]["lr"] == 1e-3 and fresh.param_groups[0]["weight_decay"] == 0.01
        for i, p in enumerate(ps):
            st = fresh.state[p]
            assert st["sched"].dtype == torch.float64 and st["sched"].tolist() == [7.0 + i, 0.123456789012345678]
            assert bool((st["exp_avg"] == 1.5 + i).all()) and bool((st["exp_avg_sq"] == 2.5 + i).all())
        if kw:          # loading a state is not loading the guard's settings or counters
            assert fresh.max_norm == 9.0 and fresh.skip_nonfinite is False and fresh.counters() == GM.ZERO and fresh._guard_tables == {}


def test_counters_state_round_trip():
    from locate_amd import GuardedNadam
    opt = GuardedNadam(params())
    state = {"steps": 40, "skipped": 3, "clipped": 11, "consecutive_skips": 1, "last_norm": 2.5, "last_scale": 0.4, "last_nonfinite": 7}
    assert opt.load_counters_state(state) is opt
    assert opt.counters_state() == state and opt.counters() == state
    with pytest.raises(KeyError):
        opt.load_counters_state({"steps": 1})
    from locate_amd.guard import _decode_verdict, _encode_verdict
    raw = _encode_verdict(state)
    assert len(raw) == 64
    back = _decode_verdict(raw)
    assert {k: back[k] for k in state if k != "last_scale"} == {k: state[k] for k in state if k != "last_scale"}
    assert back["last_scale"] == float(np.float32(0.4))


def test_the_error():
    from locate_amd import GuardExhausted
    err = GuardExhausted(48, "D", 16)
    assert isinstance(err, RuntimeError) and (err.iteration, err.network, err.consecutive_skips) == (48, "D", 16)
    assert "iteration 48" in str(err) and "16 steps" in str(err) and " D " in str(err)


# ---- the trainer's wiring, with stub optimizers ---------------------------------------------------------------------------------------
class StubGuard:
    def __init__(self, **counters):
        self.c = dict(GM.ZERO, **counters)
        self.reads = 0
        self.loaded = None

    def counters(self):
        self.reads += 1
        return dict(self.c)

    def counters_state(self):
        return dict(self.c)

    def load_counters_state(self, state):
        self.loaded = dict(state)


def stub_trainer(out, gen_opt, dis_opt, **kw):
    from locate_amd import Trainer
    net = torch.nn.Linear(2, 2)
    step = types.SimpleNamespace(gen=net, dis=net, gen_opt=gen_opt, dis_opt=dis_opt, minibatches=1)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    t = Trainer(step, pipeline, str(out), **kw)
    t.saves = []
    t.save_state = lambda: t.saves.append(t.iterations) or []
    return t


def test_trainer_without_guards_does_nothing(tmp_path):
    t = stub_trainer(tmp_path, object(), object(), max_iterations=0)
    assert t._guards() == [] and t.max_consecutive_skips == 16
    assert t.run() == 0 and t.saves == [0]
    assert not os.path.exists(str(tmp_path / "error"))
    with pytest.raises(ValueError):
        stub_trainer(tmp_path, object(), object(), max_consecutive_skips=0)


def test_trainer_reads_counters_and_stops_at_the_limit(tmp_path):
    from locate_amd import GuardExhausted
    g, d = StubGuard(steps=20, clipped=4), StubGuard(steps=20, skipped=15, consecutive_skips=15)
    t = stub_trainer(tmp_path, g, d, max_iterations=0)
    assert [tag for tag, _ in t._guards()] == ["G", "D"]
    # below the limit: the counters are read before the save, the state is saved
    assert t.run() == 0 and t.saves == [0] and (g.reads, d.reads) == (1, 1)
    assert not os.path.exists(str(tmp_path / "error" / "nonfinite.json"))
    # the record of an epoch
    path = t._save_guards(3)
    assert path == str(tmp_path / "error" / "3-guard.json")
    with open(path) as f:
        assert json.load(f) == {"G": g.c, "D": d.c}
    # with the progress line
    t.history = types.SimpleNamespace(flush=lambda: [], d=[], g=[])
    t._progress(0, 0, 16, 0, 1, 100, 0.0)
    assert (g.reads, d.reads) == (3, 3)
    # at the limit: GuardExhausted, the json, and no save
    d.c["consecutive_skips"] = 16
    t.iterations, t.saves = 37, []
    for call in (t.run, lambda: t._progress(0, 0, 16, 0, 1, 100, 0.0), lambda: t._save_guards(4)):
        with pytest.raises(GuardExhausted) as info:
            call()
        assert (info.value.iteration, info.value.network, info.value.consecutive_skips) == (37, "D", 16)
    assert t.saves == [] and not os.path.exists(str(tmp_path / "error" / "4-guard.json"))
    with open(str(tmp_path / "error" / "nonfinite.json")) as f:
        report = json.load(f)
    assert report == {"iteration": 37, "epoch": 1, "tensors": [], "guard": {"network": "D", "counters": d.c}}
    assert str(tmp_path / "error" / "nonfinite.json") in t.written
    # a limit of the caller's own; only one of the two guarded
    t = stub_trainer(tmp_path / "b", object(), StubGuard(consecutive_skips=2), max_iterations=0, max_consecutive_skips=2)
    assert [tag for tag, _ in t._guards()] == ["D"]
    with pytest.raises(GuardExhausted):
        t.run()
    assert t.saves == []


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--clip-grad-norm", "0"], ["--clip-grad-norm", "2.5"], ["--no-skip-nonfinite"],
                  ["--clip-grad-norm", "1", "--no-skip-nonfinite", "--max-consecutive-skips", "4"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--clip-grad-norm", "-1"], ["--clip-grad-norm", "nan"], ["--clip-grad-norm", "inf"], ["--clip-grad-norm"],
                  ["--max-consecutive-skips", "0"], ["--max-consecutive-skips", "x"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--clip-grad-norm X" in text and "--no-skip-nonfinite" in text and "--max-consecutive-skips N" in text
