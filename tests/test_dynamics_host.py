"""The run dynamics' host side (locate_amd/dynamics.py, the hooks in locate_amd/run.py) without a GPU: which entries and layers there
are and in which order, what is refused, the ratios and the saved file, and the command line."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT


def tiny_networks():
    from locate_amd import Discriminator, Generator, NetConfig
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    return Generator(cfg), Discriminator(cfg)


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.dynamics, locate_amd._lib as L\n"
            "from locate_amd import RunDynamics, tensor_deltas\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'liblocate_hip' not in maps, 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_entries_and_layers_and_their_order():
    from locate_amd import RunDynamics, RunStatistics, SpectralNorm
    G, D = tiny_networks()
    dyn = RunDynamics(G, D)
    want = ["G/" + n for n, _ in G.named_parameters()] + ["D/" + n for n, _ in D.named_parameters()]
    assert dyn.entry_names() == want and len(want) > 50
    assert dyn.entry_names() == RunStatistics(G, D).entry_names()          # before the first backward: the weight entries, so the files join
    assert any(n.endswith("weight_u") for n in want) and any(n.endswith("weight_v") for n in want)
    # one layer per SpectralNorm module, generator first, in modules() order, named after its weight_bar
    layers = dyn.layer_names()
    bars = [n for n in want if n.endswith("weight_bar")]
    assert layers == bars and len(layers) > 10 and len(set(layers)) == len(layers)
    assert len(layers) == sum(isinstance(m, SpectralNorm) for net in (G, D) for m in net.modules())
    first_d = next(i for i, n in enumerate(layers) if n.startswith("D/"))
    assert all(n.startswith("G/") for n in layers[:first_d]) and all(n.startswith("D/") for n in layers[first_d:])
    by_module = ["%s/%s.module.weight_bar" % (tag, name) for tag, net in (("G", G), ("D", D)) for name, m in net.named_modules()
                 if isinstance(m, SpectralNorm)]
    assert layers == by_module
    # sigma_rounds = 0 turns the part off
    assert RunDynamics(G, D, sigma_rounds=0).layer_names() == [] and RunDynamics(G, D, sigma_rounds=0).entry_names() == want


class Net(torch.nn.Module):
    def __init__(self, names, size=2):
        super().__init__()
        for n in names:
            setattr(self, n, torch.nn.Parameter(torch.zeros(size)))


def test_zero_element_parameters_are_skipped():
    from locate_amd import RunDynamics
    net = Net(["a", "b"])
    net.empty = torch.nn.Parameter(torch.zeros(0))
    assert RunDynamics(net, Net(["c"])).entry_names() == ["G/a", "G/b", "D/c"]


def test_what_is_refused():
    from locate_amd import RunDynamics, tensor_deltas
    G, D = tiny_networks()
    for capacity in (0, -3):
        with pytest.raises(ValueError):
            RunDynamics(G, D, capacity=capacity)
    with pytest.raises(ValueError):
        RunDynamics(G, D, sigma_rounds=-1)
    dyn = RunDynamics(G, D)
    assert (dyn.capacity, dyn.sigma_rounds) == (256, 4) and RunDynamics(G, D, capacity=1, sigma_rounds=0).capacity == 1
    with pytest.raises(ValueError):
        dyn.record(1)          # before any mark()
    with pytest.raises(TypeError):
        dyn.mark()          # parameters on the CPU: there is no CPU path
    with pytest.raises(ValueError):
        dyn.record(1)          # the refused mark() does not count
    assert dyn.flush() == [] and dyn.rows == [] and dyn.last_iteration is None and dyn.ratios() == []
    with pytest.raises(ValueError):
        RunDynamics(torch.nn.Module(), torch.nn.Module()).mark()          # nothing to follow
    with pytest.raises(TypeError):
        tensor_deltas([torch.zeros(4)], [torch.zeros(4)])
    with pytest.raises(TypeError):
        tensor_deltas([np.zeros(4, np.float32)], [np.zeros(4, np.float32)])
    with pytest.raises(ValueError):
        tensor_deltas([], [])
    with pytest.raises(ValueError):
        tensor_deltas([torch.zeros(4)], [torch.zeros(4), torch.zeros(4)])


def hand_made_rows():
    f64, f32, u32 = np.float64, np.float32, np.uint32
    names = ("G/a", "G/b.weight_u", "G/c", "D/d", "D/e.weight_v")
    layers = ("G/a", "D/d")
    return [
        {"iteration": 2, "names": names, "delta_sumsq": np.array([9.0, 100.0, 16.0, 0.0, 7.0], f64), "base_sumsq": np.array([900.0, 1.0, 1600.0, 4.0, 1.0], f64),
         "delta_absmax": np.array([3, 10, 4, 0, 2], f32), "unchanged": np.array([0, 0, 1, 2, 0], u32), "nonfinite": np.zeros(5, u32),
         "layers": layers, "sigma_train": np.array([2.0, 0.5], f32), "sigma_top": np.array([3.0, 0.5], f32)},
        {"iteration": 4, "names": names, "delta_sumsq": np.array([1.0, 0.0, 3.0, 1.0, 0.0], f64), "base_sumsq": np.array([0.0, 1.0, 0.0, 16.0, 0.0], f64),
         "delta_absmax": np.array([1, 0, 1, 1, 0], f32), "unchanged": np.zeros(5, u32), "nonfinite": np.array([0, 0, 7, 0, 0], u32),
         "layers": layers, "sigma_train": np.array([4.0, 1.0], f32), "sigma_top": np.array([4.0, 1.25], f32)},
    ]


def test_ratios_and_the_saved_file(tmp_path):
    from locate_amd import RunDynamics
    dyn = RunDynamics(Net(["a", "c"]), Net(["d"]))
    dyn.rows = hand_made_rows()
    first, second = dyn.ratios()
    assert first["iteration"] == 2 and second["iteration"] == 4
    assert first["update"].tolist() == [0.1, 10.0, 0.1, 0.0, np.sqrt(7.0)] and first["lipschitz"].tolist() == [1.5, 1.0]
    # per network, over the entries that are not u / v: sqrt((9 + 16) / (900 + 1600)) and sqrt(0 / 4)
    assert first["G/update"] == 0.1 and first["D/update"] == 0.0
    # a base of 0: NaN, per entry and per network; the others are what they are
    assert np.isnan(second["update"][[0, 2, 4]]).all() and second["update"][[1, 3]].tolist() == [0.0, 0.25]
    assert np.isnan(second["G/update"]) and second["D/update"] == 0.25 and second["lipschitz"].tolist() == [1.0, 1.25]
    assert sorted(first) == ["D/update", "G/update", "iteration", "lipschitz", "update"]
    (path,) = dyn.save(str(tmp_path / "error"), 3)
    assert path == str(tmp_path / "error" / "3-dynamics.npz") and sorted(os.listdir(str(tmp_path / "error"))) == ["3-dynamics.npz"]
    with np.load(path) as z:          # no pickled objects inside
        assert sorted(z.files) == ["D_update", "G_update", "base_sumsq", "delta_absmax", "delta_sumsq", "iterations", "layers", "lipschitz",
                                   "names", "nonfinite", "sigma_top", "sigma_train", "unchanged", "update"]
        assert z["names"].tolist() == list(hand_made_rows()[0]["names"]) and z["layers"].tolist() == ["G/a", "D/d"]
        assert z["iterations"].tolist() == [2, 4] and z["iterations"].dtype == np.int64
        for key, dtype, width in (("delta_sumsq", np.float64, 5), ("base_sumsq", np.float64, 5), ("delta_absmax", np.float32, 5),
                                  ("unchanged", np.uint32, 5), ("nonfinite", np.uint32, 5), ("update", np.float64, 5),
                                  ("sigma_train", np.float32, 2), ("sigma_top", np.float32, 2), ("lipschitz", np.float64, 2)):
            assert z[key].dtype == dtype and z[key].shape == (2, width), key
        assert z["delta_sumsq"].tolist() == [[9, 100, 16, 0, 7], [1, 0, 3, 1, 0]] and z["nonfinite"].tolist() == [[0] * 5, [0, 0, 7, 0, 0]]
        assert z["sigma_top"].tolist() == [[3.0, 0.5], [4.0, 1.25]] and z["lipschitz"].tolist() == [[1.5, 1.0], [1.0, 1.25]]
        assert np.array_equal(z["update"], np.array([first["update"], second["update"]]), equal_nan=True)
        assert np.array_equal(z["G_update"], np.array([0.1, np.nan]), equal_nan=True) and z["D_update"].tolist() == [0.0, 0.25]
    assert dyn.clear().rows == [] and dyn.ratios() == []
    # no records: a file of empty arrays with the entries' names
    (path,) = dyn.save(str(tmp_path / "error"), 4)
    with np.load(path) as z:
        assert z["names"].tolist() == ["G/a", "G/c", "D/d"] and z["delta_sumsq"].shape == (0, 3) and z["iterations"].shape == (0,)
        assert z["layers"].shape == (0,) and z["sigma_top"].shape == (0, 0)


def trainer_arguments(G, D):
    from locate_amd import Nadam, NetConfig, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    return step, pipeline


def test_trainer_arguments():
    from locate_amd import RunDynamics, Trainer
    G, D = tiny_networks()
    step, pipeline = trainer_arguments(G, D)
    with pytest.raises(ValueError):
        Trainer(step, pipeline, "OUT", dynamics=RunDynamics(G, D), dynamics_every=-1)
    off = Trainer(step, pipeline, "OUT")
    assert off.dynamics is None and off.dynamics_every == 0
    marker = RunDynamics(G, D)
    on = Trainer(step, pipeline, "OUT", dynamics=marker, dynamics_every=16)
    assert on.dynamics is marker and on.dynamics_every == 16 and on.written == []


def test_command_line(monkeypatch, capsys, tmp_path):
    import locate_amd
    from locate_amd import RunDynamics, _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--dynamics-every", "0"], ["--dynamics-every", "16"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--dynamics-every", "-1"], ["--dynamics-every", "often"], ["--dynamics-every"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--dynamics-every N" in capsys.readouterr().out

    # what main() hands to the Trainer: everything in front of it replaced by stand-ins that need no GPU
    seen = []

    class Recorder:
        def __init__(self, *args, **kwargs):
            seen.append(kwargs)
            raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", lambda: ("gfx950", 256, 64))
    monkeypatch.setattr(locate_amd, "Generator", lambda cfg: Net(["a"]))
    monkeypatch.setattr(locate_amd, "Discriminator", lambda cfg: Net(["b"]))
    monkeypatch.setattr(locate_amd, "get_model", lambda net, lr, dev, cfg: (net, None))
    monkeypatch.setattr(locate_amd, "TrainStep", lambda *a, **k: types.SimpleNamespace())
    monkeypatch.setattr(locate_amd, "DeviceImageStore", lambda *a, **k: None)
    monkeypatch.setattr(locate_amd, "InputPipeline", lambda *a, **k: None)
    monkeypatch.setattr(run, "Trainer", Recorder)
    base[-1] = str(tmp_path / "OUT")
    with pytest.raises(Reached):
        run.main(base)
    with pytest.raises(Reached):
        run.main(base + ["--dynamics-every", "4"])
    without, with_flag = seen
    assert without["dynamics"] is None and without["dynamics_every"] == 0 and without["stats"] is None
    assert isinstance(with_flag["dynamics"], RunDynamics) and with_flag["dynamics_every"] == 4
    assert with_flag["dynamics"].entry_names() == ["G/a", "D/b"]
