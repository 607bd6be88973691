"""The run statistics' host side (locate_amd/stats.py, the hooks in locate_amd/run.py) without a GPU: which entries there are and
in which order, what is refused, the error a bad record raises, the saved file, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def tiny_networks():
    from locate_amd import Discriminator, Generator, NetConfig
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    return Generator(cfg), Discriminator(cfg)


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.stats, locate_amd._lib as L\n"
            "from locate_amd import RunStatistics, NonFiniteError, tensor_statistics\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'liblocate_hip' not in maps, 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_entries_and_their_order():
    from locate_amd import RunStatistics
    G, D = tiny_networks()
    stats = RunStatistics(G, D)
    want = ["G/" + n for n, _ in G.named_parameters()] + ["D/" + n for n, _ in D.named_parameters()]
    assert stats.entry_names() == want and len(want) > 50          # before the first backward: no gradient entry
    assert any(n.endswith("weight_u") for n in want) and any(n.endswith("weight_v") for n in want)
    # gradient entries appear only where .grad exists, directly behind their parameter
    g_names, d_names = [n for n, _ in G.named_parameters()], [n for n, _ in D.named_parameters()]
    given = {"G/" + g_names[0], "G/" + g_names[5], "D/" + d_names[-1]}
    for tag, net in (("G", G), ("D", D)):
        for n, p in net.named_parameters():
            if tag + "/" + n in given:
                p.grad = torch.zeros_like(p)
    names = stats.entry_names()
    assert [n for n in names if not n.endswith(".grad")] == want
    assert {n[:-len(".grad")] for n in names if n.endswith(".grad")} == given
    for n in given:
        assert names[names.index(n) + 1] == n + ".grad"
    G.zero_grad()
    D.zero_grad()
    assert stats.entry_names() == want


def test_cpu_tensors_are_rejected():
    from locate_amd import RunStatistics, tensor_statistics
    with pytest.raises(TypeError):
        tensor_statistics([torch.zeros(4)])
    with pytest.raises(TypeError):
        tensor_statistics([np.zeros(4, np.float32)])
    with pytest.raises(ValueError):
        tensor_statistics([])
    stats = RunStatistics(*tiny_networks())
    with pytest.raises(TypeError):
        stats.record(1)
    assert stats.flush() == [] and stats.rows == [] and stats.last_iteration is None and stats.check() is stats


def test_argument_validation():
    from locate_amd import RunStatistics, Trainer
    G, D = tiny_networks()
    for capacity in (0, -3):
        with pytest.raises(ValueError):
            RunStatistics(G, D, capacity=capacity)
    assert RunStatistics(G, D, capacity=1).capacity == 1 and RunStatistics(G, D).capacity == 256
    import types
    from locate_amd import Nadam, NetConfig, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    with pytest.raises(ValueError):
        Trainer(step, pipeline, "OUT", stats=RunStatistics(G, D), stats_every=-1)
    off = Trainer(step, pipeline, "OUT")
    assert off.stats is None and off.stats_every == 16
    marker = RunStatistics(G, D)
    on = Trainer(step, pipeline, "OUT", stats=marker, stats_every=0)
    assert on.stats is marker and on.stats_every == 0 and on.written == []


def test_the_error():
    from locate_amd import NonFiniteError
    err = NonFiniteError(7, [("D/a.weight", 1), ("D/a.weight.grad", 12), ("G/b", 3), ("G/c", 4), ("G/d", 5), ("G/e", 6)])
    assert isinstance(err, RuntimeError) and err.iteration == 7
    assert err.tensors[:2] == [("D/a.weight", 1), ("D/a.weight.grad", 12)] and len(err.tensors) == 6
    text = str(err)
    assert "iteration 7" in text and "6 tensors" in text and "D/a.weight (1)" in text and "G/c (4)" in text
    assert "G/d" not in text and "2 more" in text          # the first few are named
    assert "1 tensor:" in str(NonFiniteError(3, [("G/x", 2)]))


def hand_made_rows():
    f64, f32, u32 = np.float64, np.float32, np.uint32
    early = ("G/a", "G/b", "D/c")
    late = ("G/a", "G/a.grad", "G/b", "D/c", "D/c.grad")
    return [
        {"iteration": 2, "names": early, "sumsq": np.array([9.0, 16.0, 4.0], f64), "absmax": np.array([3, 4, 2], f32),
         "nonfinite": np.zeros(3, u32), "total": 0, "first": -1},
        {"iteration": 4, "names": late, "sumsq": np.array([1.0, 36.0, 0.0, 25.0, 64.0], f64), "absmax": np.array([1, 6, 0, 5, 8], f32),
         "nonfinite": np.array([0, 0, 7, 0, 2], u32), "total": 9, "first": 2},
    ]


class Net(torch.nn.Module):
    def __init__(self, names):
        super().__init__()
        for n in names:
            setattr(self, n, torch.nn.Parameter(torch.zeros(2)))


def test_saved_file_and_global_norms(tmp_path):
    from locate_amd import NonFiniteError, RunStatistics
    stats = RunStatistics(Net(["a", "b"]), Net(["c"]))
    stats.rows = hand_made_rows()
    assert stats.names == ["G/a", "G/a.grad", "G/b", "D/c", "D/c.grad"]
    norms = stats.global_norms()
    assert norms == [{"iteration": 2, "G/weight": 5.0, "G/grad": 0.0, "D/weight": 2.0, "D/grad": 0.0},
                     {"iteration": 4, "G/weight": 1.0, "G/grad": 6.0, "D/weight": 5.0, "D/grad": 8.0}]
    (path,) = stats.save(str(tmp_path / "error"), 3)
    assert path == str(tmp_path / "error" / "3-stats.npz") and sorted(os.listdir(str(tmp_path / "error"))) == ["3-stats.npz"]
    with np.load(path) as z:          # no pickled objects inside
        assert sorted(z.files) == ["absmax", "iterations", "names", "nonfinite", "sumsq"]
        assert z["names"].tolist() == stats.names and z["iterations"].tolist() == [2, 4] and z["iterations"].dtype == np.int64
        assert z["sumsq"].dtype == np.float64 and z["absmax"].dtype == np.float32 and z["nonfinite"].dtype == np.uint32
        # an entry that did not exist at a record: NaN / 0 / 0
        assert np.array_equal(z["sumsq"], np.array([[9, np.nan, 16, 4, np.nan], [1, 36, 0, 25, 64]], np.float64), equal_nan=True)
        assert z["absmax"].tolist() == [[3, 0, 4, 2, 0], [1, 6, 0, 5, 8]]
        assert z["nonfinite"].tolist() == [[0, 0, 0, 0, 0], [0, 0, 7, 0, 2]]
    # check() names the first bad record once, and keeps the rows
    with pytest.raises(NonFiniteError) as info:
        stats.check()
    assert info.value.iteration == 4 and info.value.tensors == [("G/b", 7), ("D/c.grad", 2)]
    assert stats.check() is stats and len(stats.rows) == 2
    assert stats.clear().rows == [] and stats.names == [] and stats.global_norms() == []


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--stats-every", "0"], ["--stats-every", "16"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--stats-every", "-1"], ["--stats-every", "often"], ["--stats-every"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--stats-every N" in capsys.readouterr().out
