"""The snapshot's host side (locate_amd/snapshot.py, the hooks in locate_amd/run.py) without a GPU: the arena, the numpy model the
GPU tests hold the kernels to (tests/helpers/snapshot_model.py) - its classification against numpy's own isfinite, its commit
logic - what the constructors and the command line refuse, and what the trainer does where it used to stop: roll back, record,
go on; stop as before once the rollbacks are used up or no snapshot exists."""
import json
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import guard_model as GM  # noqa: E402
import snapshot_model as SM  # noqa: E402


def test_importing_the_module_loads_no_library():
    code = ("import locate_amd.snapshot, locate_amd._lib as L\n"
            "from locate_amd import StateSnapshot, TrainingSnapshot, NoSnapshot\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


# ---- the arena ----------------------------------------------------------------------------------------------------------------------
def test_arena_layout():
    from locate_amd.snapshot import arena_layout
    sizes = [0, 1, 3, 4, 5, 4097]
    offsets, slot_bytes = arena_layout(sizes)
    assert offsets == [0, 0, 16, 32, 48, 80] and slot_bytes == 80 + 16400          # 4097 words = 16388 bytes, padded to 16400
    assert all(o % 16 == 0 for o in offsets) and offsets == sorted(offsets)
    for (o, n), nxt in zip(zip(offsets, sizes), offsets[1:] + [slot_bytes]):
        assert o + 4 * n <= nxt and nxt - (o + 4 * n) < 16          # in order, no overlap, less than one 16-byte word of padding
    assert (offsets, slot_bytes) == SM.layout(sizes)
    assert arena_layout([]) == ([], 0) and arena_layout([0, 0]) == ([0, 0], 0) and arena_layout([4]) == ([0], 16)
    with pytest.raises(ValueError):
        arena_layout([3, -1])


# ---- the model's classification against numpy ----------------------------------------------------------------------------------------
def test_model_classification_fp32():
    w = np.array([bits for bits, _ in SM.SPECIAL_F32], dtype=np.uint32)
    finite = np.isfinite(w.view(np.float32))
    assert finite.tolist() == [f for _, f in SM.SPECIAL_F32]          # the table says what numpy says
    assert SM.nonfinite(w, 1) == int((~finite).sum()) == 8
    for bits, f in SM.SPECIAL_F32:
        assert SM.nonfinite(np.array([bits], np.uint32), 1) == (0 if f else 1), hex(bits)
        assert SM.nonfinite(np.array([bits], np.uint32), 0) == 0          # raw words are never judged
    rng = np.random.default_rng(1)
    w = rng.integers(0, 2 ** 32, size=100000, dtype=np.uint64).astype(np.uint32)          # every exponent, ~390 of them all ones
    assert SM.nonfinite(w, 1) == int((~np.isfinite(w.view(np.float32))).sum()) > 100


def test_model_classification_fp64():
    pairs = np.array([p for p, _ in SM.SPECIAL_F64], dtype=np.uint32)          # [k, 2]: low, high
    finite = np.isfinite(pairs.reshape(-1).view(np.float64))
    assert finite.tolist() == [f for _, f in SM.SPECIAL_F64]
    assert SM.nonfinite(pairs.reshape(-1), 2) == int((~finite).sum()) == 4
    for p, f in SM.SPECIAL_F64:
        assert SM.nonfinite(np.array(p, np.uint32), 2) == (0 if f else 1), p
    # a double whose LOW word alone looks like an fp32 NaN is finite - and judged as fp32 the same words would not be
    low_nan = np.array([0x7fc00000, 0x3ff00000], np.uint32)
    assert np.isfinite(low_nan.view(np.float64)[0]) and SM.nonfinite(low_nan, 2) == 0 and SM.nonfinite(low_nan, 1) == 1
    rng = np.random.default_rng(2)
    w = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    w[1::2] |= np.uint32(0x7fe00000)          # most exponents nearly all ones: about half of the doubles are non-finite
    want = int((~np.isfinite(w.view(np.float64))).sum())
    assert SM.nonfinite(w, 2) == want and 1000 < want < 99000
    # Nadam's fresh schedule pair
    from locate_amd.snapshot import SCHED_FILL, _fill_words
    assert np.array(SCHED_FILL, np.uint32).view(np.float64).tolist() == [0.0, 1.0]
    assert _fill_words((7,)) == (7, 7, 7, 7) and _fill_words((1, 2)) == (1, 2, 1, 2) and _fill_words(SCHED_FILL) == SCHED_FILL
    with pytest.raises(ValueError):
        _fill_words((1, 2, 3))


# ---- the model's commit logic --------------------------------------------------------------------------------------------------------
def test_model_commit_sequence():
    f32 = lambda *v: SM.words(np.array(v, np.float32))          # noqa: E731
    model = SM.Model([(5, 1, (0,)), (4, 2, (0, 0, 0, 0x3ff00000)), (3, 1, (0xabc,)), (0, 1, (0,)), (2, 0, (0,))])
    names = ["a", "sched", "later", "empty", "raw"]
    assert model.offsets == [0, 32, 48, 64, 64] and model.slot_bytes == 80
    sched = SM.words(np.array([3.0, 0.5], np.float64))
    raw = np.array([0x7f800000, 0xffffffff], np.uint32)          # an fp32 Inf and a NaN in a kind-0 entry: not judged
    live = [f32(1, -2, 3, -0.0, 5e-41), sched, None, f32(), raw]
    assert model.restore(live) is None          # nothing committed yet
    # 1. the first take goes to slot 0
    assert model.take(live, 3) and model.status(names) == {"good": 0, "iteration": 3, "taken": 1, "rejected": 0, "last_rejected_iteration": 0,
                                                          "last_rejected_count": 0, "last_rejected_tensor": None}
    image = model.slots[0].copy()
    assert image[:5].tolist() == live[0].tolist() and image[5:8].tolist() == [0, 0, 0]          # the tensor, then its padding
    assert image[8:12].tolist() == sched.tolist() and image[12:15].tolist() == [0xabc] * 3 and image[16:18].tolist() == raw.tolist()
    assert not model.slots[1].any()
    # 2. a rejected take: good and its iteration stay, the good slot keeps its bytes, the OTHER slot was written
    bad = [f32(1, float("nan"), 3, float("inf"), 5), SM.words(np.array([float("inf"), 0.5], np.float64)), f32(7, 8, 9), f32(), raw]
    assert model.destination() == 1 and not model.take(bad, 5)
    assert model.status(names) == {"good": 0, "iteration": 3, "taken": 1, "rejected": 1, "last_rejected_iteration": 5,
                                   "last_rejected_count": 3, "last_rejected_tensor": "a"}
    assert np.array_equal(model.slots[0], image) and model.slots[1][1] == bad[0][1] and model.destination() == 1
    # 3. the next good take lands in the SAME slot, over what the rejected one wrote, and flips
    good = [f32(9, 8, 7, 6, 5), sched, f32(7, 8, 9), f32(), raw]
    assert model.take(good, 6) and model.destination() == 0
    assert model.status(names) == {"good": 1, "iteration": 6, "taken": 2, "rejected": 1, "last_rejected_iteration": 5,
                                   "last_rejected_count": 3, "last_rejected_tensor": "a"}
    assert np.array_equal(model.slots[0], image) and model.slots[1][:5].tolist() == good[0].tolist()
    # 4. restore from the good slot: every live tensor, the ones that do not exist skipped
    iteration, back = model.restore([bad[0], bad[1], None, f32(), raw])
    assert iteration == 6 and back[2] is None and back[3].size == 0
    assert back[0].tolist() == good[0].tolist() and back[1].tolist() == sched.tolist() and back[4].tolist() == raw.tolist()
    # a tensor that appeared after a take is restored to its fill
    model.take([good[0], sched, None, f32(), raw], 7)
    assert model.restore(good)[1][2].tolist() == [0xabc] * 3


# ---- what the constructors refuse ----------------------------------------------------------------------------------------------------
def tiny_step(**extra):
    from locate_amd import Discriminator, Generator, Nadam, NetConfig
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    return types.SimpleNamespace(gen=G, dis=D, gen_opt=Nadam(G.parameters(), lr=cfg.glr), dis_opt=Nadam(D.parameters(), lr=cfg.dlr),
                                 minibatches=1, reducer_g=None, reducer_d=None, **extra)


def test_snapshot_argument_errors():
    from locate_amd import StateSnapshot, TrainingSnapshot
    with pytest.raises(TypeError, match="GPU"):
        TrainingSnapshot(tiny_step())          # the networks are on the CPU: there is no CPU path
    step = tiny_step()
    step.reducer_d = object()
    with pytest.raises(ValueError, match="data parallelism"):
        TrainingSnapshot(step)
    t = torch.zeros(8)
    with pytest.raises(TypeError):
        StateSnapshot([("t", lambda: t, 8, 1, (0,))], "cuda:0")          # a CPU tensor, refused before any device memory is taken
    with pytest.raises(TypeError):
        StateSnapshot([("t", lambda: None, 8, 1, (0,))], "cpu")
    for entry in (("t", lambda: None, -1, 1, (0,)), ("t", lambda: None, 8, 3, (0,)), ("t", lambda: None, 3, 2, (0,)),
                  ("t", lambda: None, 8, 1, (0, 0, 0)), ("t", lambda: None, 8, 1, (-1,))):
        with pytest.raises(ValueError):
            StateSnapshot([entry], "cuda:0")
    with pytest.raises(ValueError):
        StateSnapshot([("t", lambda: None, 0, 1, (0,))], "cuda:0")          # nothing to copy
    # iteration < 1: before the first G-step D's u / v are not trainable yet, and a restore would not return that
    blank = TrainingSnapshot.__new__(TrainingSnapshot)
    for iteration in (0, -1):
        with pytest.raises(ValueError, match="iteration"):
            blank.take(iteration)


def test_the_commit_record_layout():
    from locate_amd.snapshot import COMMIT_BYTES, RECORD_BYTES, _COMMIT, _decode_commit
    assert struct.calcsize(_COMMIT) == COMMIT_BYTES == 64 and struct.calcsize("<Qqqi4I4x") == RECORD_BYTES == 48
    raw = struct.pack(_COMMIT, 1, 0x7fffffff, 0, 48, 5, 2, 40, 17, 1, 0)
    assert _decode_commit(raw, ["a", "b"]) == {"good": 1, "iteration": 48, "taken": 5, "rejected": 2, "last_rejected_iteration": 40,
                                             "last_rejected_count": 17, "last_rejected_tensor": "b"}
    assert _decode_commit(struct.pack(_COMMIT, -1, 0x7fffffff, 0, 0, 0, 0, 0, 0, -1, 0), ["a"])["last_rejected_tensor"] is None


# ---- the trainer's policy, with stand-ins --------------------------------------------------------------------------------------------
class StubSnapshot:
    """records take / restore; restore() returns `good` or raises NoSnapshot while it is None"""

    def __init__(self, good=None, on_restore=None):
        self.good, self.on_restore, self.calls = good, on_restore, []

    def take(self, iteration):
        self.calls.append(("take", iteration))
        self.good = iteration

    def restore(self):
        from locate_amd import NoSnapshot
        self.calls.append(("restore",))
        if self.good is None:
            raise NoSnapshot("nothing committed")
        if self.on_restore:
            self.on_restore()
        return self.good


class StubStats:
    """check() raises NonFiniteError once per entry of `failures` (the iteration it names), then passes"""

    def __init__(self, failures=()):
        self.failures, self.records, self.checks, self.last_iteration = list(failures), [], 0, None

    def record(self, iteration):
        self.records.append(iteration)
        self.last_iteration = iteration
        return self

    def check(self):
        from locate_amd import NonFiniteError
        self.checks += 1
        if self.failures:
            raise NonFiniteError(self.failures.pop(0), [("D/w", 2), ("D/w.grad", 9)])
        return self


class StubGuard:
    def __init__(self, **counters):
        self.c = dict(GM.ZERO, **counters)

    def counters(self):
        return dict(self.c)

    def counters_state(self):
        return dict(self.c)

    def load_counters_state(self, state):
        self.c = dict(state)


def stub_trainer(out, gen_opt=None, dis_opt=None, **kw):
    from locate_amd import Trainer
    net = torch.nn.Linear(2, 2)
    step = types.SimpleNamespace(gen=net, dis=net, gen_opt=gen_opt or object(), dis_opt=dis_opt or object(), minibatches=1)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    t = Trainer(step, pipeline, str(out), **kw)
    t.saves = []
    t.save_state = lambda: t.saves.append(t.iterations) or []
    t.history = types.SimpleNamespace(flush=lambda: [], d=[], g=[])
    return t


def progress(t):
    t._progress(0, 0, t.iterations, 0, 1, 100, 0.0)


def read(path):
    with open(str(path)) as f:
        return json.load(f)


def test_trainer_argument_errors(tmp_path):
    with pytest.raises(ValueError, match="stats"):
        stub_trainer(tmp_path, snapshot=StubSnapshot())          # neither statistics nor a guard: nothing would trigger a rollback
    for kw in ({"rollback_every": 0}, {"rollback_every": -4}, {"max_rollbacks": -1}):
        with pytest.raises(ValueError):
            stub_trainer(tmp_path, snapshot=StubSnapshot(), stats=StubStats(), **kw)
    t = stub_trainer(tmp_path, snapshot=StubSnapshot(), stats=StubStats())
    assert (t.rollback_every, t.max_rollbacks, t.rollbacks) == (256, 3, 0)
    assert stub_trainer(tmp_path, snapshot=StubSnapshot(), dis_opt=StubGuard()).snapshot is not None          # a guard alone will do
    assert stub_trainer(tmp_path).snapshot is None          # and without one nothing asks for statistics


def test_trainer_takes_at_the_progress_line(tmp_path):
    snap, stats = StubSnapshot(), StubStats()
    t = stub_trainer(tmp_path, snapshot=snap, stats=stats, rollback_every=8)
    for iterations, want in ((4, []), (8, [("take", 8)]), (12, [("take", 8)]), (15, [("take", 8)]), (16, [("take", 8), ("take", 16)])):
        t.iterations = iterations
        progress(t)
        assert snap.calls == want, iterations
    assert stats.checks == 5 and not os.path.exists(str(tmp_path / "error"))


def test_trainer_rolls_back_where_it_used_to_stop(tmp_path):
    from locate_amd import NonFiniteError
    snap, stats = StubSnapshot(good=16), StubStats(failures=[21])
    t = stub_trainer(tmp_path, snapshot=snap, stats=stats, rollback_every=4, max_iterations=40)
    t.iterations = 24
    progress(t)          # the check fails: restore, record, go on - and no take behind a check that did not pass
    want = [{"iteration": 21, "to_iteration": 16, "epoch": 1, "cause": "nonfinite", "tensors": [["D/w", 2], ["D/w.grad", 9]]}]
    assert snap.calls == [("restore",)] and t.rollbacks == 1
    assert read(tmp_path / "error" / "rollbacks.json") == want and str(tmp_path / "error" / "rollbacks.json") in t.written
    assert not os.path.exists(str(tmp_path / "error" / "nonfinite.json")) and not os.path.exists(str(tmp_path / "error" / "rollbacks.json.tmp"))
    assert stats.records == []          # at a progress line nothing more is recorded
    t.iterations = 28
    progress(t)          # the next one passes: a take
    assert snap.calls == [("restore",), ("take", 28)]
    # before a save: the restored state is recorded and checked, then saved
    t.iterations, stats.failures = 40, [40]
    assert t.run() == 40 and t.saves == [40]
    assert snap.calls[2:] == [("restore",)] and stats.records == [40, 40] and t.rollbacks == 2
    want.append({"iteration": 40, "to_iteration": 28, "epoch": 1, "cause": "nonfinite", "tensors": [["D/w", 2], ["D/w.grad", 9]]})
    assert read(tmp_path / "error" / "rollbacks.json") == want
    # the third failure is still rolled back; the FOURTH, with max_rollbacks = 3, is what it always was: the json, no save, the error
    stats.failures = [41]
    progress(t)
    assert t.rollbacks == 3 and len(read(tmp_path / "error" / "rollbacks.json")) == 3
    assert not os.path.exists(str(tmp_path / "error" / "nonfinite.json"))
    stats.failures, t.saves, before = [43], [], list(snap.calls)
    stats.last_iteration = None          # as after another iteration
    with pytest.raises(NonFiniteError) as info:
        t.run()
    assert info.value.iteration == 43 and t.saves == [] and snap.calls == before and t.rollbacks == 3
    assert read(tmp_path / "error" / "nonfinite.json") == {"iteration": 43, "epoch": 1, "tensors": [["D/w", 2], ["D/w.grad", 9]]}
    assert len(read(tmp_path / "error" / "rollbacks.json")) == 3


def test_no_snapshot_falls_through(tmp_path):
    from locate_amd import NonFiniteError
    snap, stats = StubSnapshot(good=None), StubStats(failures=[5])
    t = stub_trainer(tmp_path, snapshot=snap, stats=stats, max_iterations=6)
    t.iterations = 6
    with pytest.raises(NonFiniteError):
        t.run()
    assert snap.calls == [("restore",)] and t.saves == [] and t.rollbacks == 0
    assert read(tmp_path / "error" / "nonfinite.json") == {"iteration": 5, "epoch": 1, "tensors": [["D/w", 2], ["D/w.grad", 9]]}
    assert not os.path.exists(str(tmp_path / "error" / "rollbacks.json"))
    # max_rollbacks = 0: the snapshot is not even asked
    snap, stats = StubSnapshot(good=3), StubStats(failures=[5])
    t = stub_trainer(tmp_path / "zero", snapshot=snap, stats=stats, max_iterations=6, max_rollbacks=0)
    t.iterations = 6
    with pytest.raises(NonFiniteError):
        t.run()
    assert snap.calls == [] and t.saves == [] and os.path.exists(str(tmp_path / "zero" / "error" / "nonfinite.json"))


def test_an_exhausted_guard_rolls_back_too(tmp_path):
    from locate_amd import GuardExhausted
    guard = StubGuard(steps=40, skipped=16, consecutive_skips=16)
    snap = StubSnapshot(good=20, on_restore=lambda: guard.c.update(consecutive_skips=0))          # as TrainingSnapshot.restore does
    stats = StubStats()
    t = stub_trainer(tmp_path, dis_opt=guard, snapshot=snap, stats=stats, max_iterations=40, max_rollbacks=1)
    t.iterations = 40
    assert t.run() == 40 and t.saves == [40]
    counters = dict(guard.c, consecutive_skips=16)
    assert read(tmp_path / "error" / "rollbacks.json") == [{"iteration": 40, "to_iteration": 20, "epoch": 1, "cause": "guard",
                                                           "guard": {"network": "D", "counters": counters}}]
    assert stats.records == [40, 40]          # the state the guard's rollback restored was recorded and checked before the save
    assert not os.path.exists(str(tmp_path / "error" / "nonfinite.json"))
    guard.c["consecutive_skips"], t.saves = 16, []          # again: the one rollback is used up
    with pytest.raises(GuardExhausted):
        t.run()
    assert t.saves == [] and read(tmp_path / "error" / "nonfinite.json")["guard"]["network"] == "D"


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--rollback-every", "0"], ["--rollback-every", "64", "--stats-every", "16"], ["--max-rollbacks", "0"],
                  ["--rollback-every", "64", "--clip-grad-norm", "0", "--max-rollbacks", "5"], ["--rollback-every", "8", "--no-skip-nonfinite"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--rollback-every", "-1", "--stats-every", "16"], ["--max-rollbacks", "-1"], ["--rollback-every", "x"], ["--rollback-every"],
                  ["--rollback-every", "64"]):          # the last: neither statistics nor a guard
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--rollback-every N" in text and "--max-rollbacks N" in text
