"""The manifold metrics' host side (locate_amd/manifold.py, the hooks in locate_amd/run.py) without a GPU: import and construction,
what is refused, the metrics from counts, the trainer's record with a stand-in, and the command line."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.manifold, locate_amd._lib as L\n"
            "from locate_amd import ManifoldMetrics, kth_radius, within\n"
            "mm = ManifoldMetrics(S=64)\n"
            "assert (mm.S, mm.k, mm.images, mm.seed, mm.chunk) == (64, 3, 4096, 999, 64) and str(mm.device) == 'cuda'\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_the_abi_is_declared_and_bound():
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert EXPECTED_ABI >= 16
    header = open(os.path.join(ROOT, "include", "locate_hip.h")).read()
    for name in ("locate_nn_within_workspace_bytes", "locate_nn_within"):
        assert name in PROTOTYPES and name + "(" in header
    assert len(PROTOTYPES["locate_nn_within"][1]) == 15 and len(PROTOTYPES["locate_nn_within_workspace_bytes"][1]) == 3


def test_construction_and_what_is_refused():
    from locate_amd import ManifoldMetrics, kth_radius, within
    mm = ManifoldMetrics(S=32, k=2, images=16, seed=5, chunk=8, device="cuda:0")
    assert (mm.S, mm.k, mm.images, mm.seed, mm.chunk) == (32, 2, 16, 5, 8) and not mm.has_reference and mm.baseline is None
    for bad in (dict(k=0), dict(k=9), dict(S=6), dict(images=0), dict(chunk=0)):
        with pytest.raises(ValueError):
            ManifoldMetrics(**dict(dict(S=64), **bad))
    with pytest.raises(RuntimeError):
        mm.evaluate(None)
    with pytest.raises(TypeError):
        ManifoldMetrics(S=64, device="cpu").reference_from_store(types.SimpleNamespace())
    with pytest.raises(TypeError):
        mm.between(torch.zeros(2, 3, 32, 32))
    cpu = (torch.zeros(2, 64, dtype=torch.int8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        within(cpu, cpu, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        kth_radius(cpu, 1)
    with pytest.raises(ValueError):
        within(cpu[:2], cpu, torch.zeros(2, dtype=torch.int64))


def test_the_metrics_are_true_divisions_of_the_counts():
    from locate_amd.manifold import COUNTS, metrics
    assert COUNTS == ("precise", "recalled", "hit_sum", "covered")
    value = metrics({"precise": 2, "recalled": 3, "hit_sum": 4, "covered": 1}, m=3, n=4, k=2)
    assert value == {"precision": 2 / 3, "recall": 3 / 4, "density": 4 / 6, "coverage": 1 / 4}


class FakeManifold:
    def __init__(self):
        self.calls = []

    def evaluate(self, gen, latents=None):
        self.calls.append((gen, latents))
        p = 0.25 if gen == "EMA" else 0.5
        return {"images": 4, "real_images": 4, "k": 3, "precision": p, "recall": 0.75, "density": 1.25, "coverage": 0.5,
                "counts": {"precise": int(4 * p), "recalled": 3, "hit_sum": 15, "covered": 2}, "nonfinite": 0,
                "baseline": {"precision": 1.0, "recall": 1.0, "density": 1.0, "coverage": 1.0,
                             "counts": {"precise": 4, "recalled": 4, "hit_sum": 12, "covered": 4}}}


def fake_trainer(out, **kw):
    """a Trainer with only what `_manifold` reads: no networks, no GPU"""
    from locate_amd import Trainer
    t = Trainer.__new__(Trainer)
    t.out, t.gen, t.iterations, t.average = str(out), "GEN", 12, kw.get("average")
    t.manifold = kw.get("manifold")
    return t


def test_the_trainers_record(tmp_path):
    keys = ["baseline", "counts", "coverage", "density", "epoch", "images", "iterations", "k", "nonfinite", "precision", "real_images", "recall"]
    mm = FakeManifold()
    t = fake_trainer(tmp_path, manifold=mm)
    os.makedirs(str(tmp_path / "error"))
    path = str(tmp_path / "error" / "manifold.json")
    assert t._manifold(0) == path and os.path.exists(path) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == keys and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["precision"]) == (1, 12, 0.5)
    assert mm.calls == [("GEN", None)]          # the metric's own fixed latents
    # a later epoch - or a resumed run - appends to the list it finds; with an average, its record goes under "average"
    t.average = types.SimpleNamespace(generator="EMA")
    t.iterations = 24
    assert t._manifold(1) == path
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and sorted(rec2[1]) == sorted(keys + ["average"])
    assert sorted(rec2[1]["average"]) == [k for k in keys if k not in ("epoch", "iterations", "baseline")]
    assert rec2[1]["average"]["precision"] == 0.25 and rec2[1]["precision"] == 0.5 and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 24)
    assert os.listdir(str(tmp_path / "error")) == ["manifold.json"]


def test_trainer_without_manifold_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    assert Trainer(step, pipeline, "OUT").manifold is None
    marker = FakeManifold()
    on = Trainer(step, pipeline, "OUT", manifold=marker)
    assert on.manifold is marker and on.written == [] and marker.calls == []          # nothing is evaluated before an epoch ends


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    args = run.parser().parse_args(base)
    assert (args.manifold, args.manifold_k) == (0, 3)
    args = run.parser().parse_args(base + ["--manifold", "4096", "--manifold-k", "5"])
    assert (args.manifold, args.manifold_k) == (4096, 5)

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for extra in ([], ["--manifold", "0"], ["--manifold", "64"], ["--manifold", "64", "--manifold-k", "8"], ["--manifold", "64", "--manifold-k", "1"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--manifold", "-1"], ["--manifold", "many"], ["--manifold"], ["--manifold", "64", "--manifold-k", "0"],
                  ["--manifold", "64", "--manifold-k", "9"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--manifold IMAGES" in text and "--manifold-k K" in text
    assert "--manifold" in run.__doc__ and "manifold" in run.Trainer.__doc__
