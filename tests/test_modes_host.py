"""The binned mode coverage's host side (locate_amd/modes.py, the hooks in locate_amd/run.py) without a GPU: import and construction,
what is refused, the trainer's record with a stand-in, and the command line."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.modes, locate_amd._lib as L\n"
            "from locate_amd import BinnedModes, centroids, group_sums, kmeans_codes, ndb_statistics\n"
            "bm = BinnedModes(S=64)\n"
            "assert (bm.S, bm.bins, bm.images, bm.samples, bm.iterations, bm.alpha, bm.seed, bm.chunk) == (64, 128, 16384, 4096, 10, 0.05, 999, 64)\n"
            "assert str(bm.device) == 'cuda' and ndb_statistics([1, 1], [1, 1])['ndb'] == 0\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_the_abi_is_declared_and_bound():
    from locate_amd import build
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert EXPECTED_ABI >= 21 and "modes.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "modes.hip"))
    header = open(os.path.join(ROOT, "include", "locate_hip.h")).read()
    for name, count in (("locate_nn_group_sums_workspace_bytes", 3), ("locate_nn_group_sums", 10), ("locate_nn_centroids", 10)):
        assert name in PROTOTYPES and name + "(" in header and len(PROTOTYPES[name][1]) == count, name
    with open(os.path.join(build.CSRC, "runtime.hip")) as f:
        assert "return %d;" % EXPECTED_ABI in f.read()


def test_construction_and_what_is_refused():
    from locate_amd import BinnedModes, centroids, group_sums, kmeans_codes
    bm = BinnedModes(S=32, bins=4, images=16, samples=8, iterations=3, alpha=0.1, seed=5, chunk=8, device="cuda:0")
    assert (bm.S, bm.bins, bm.images, bm.samples, bm.iterations, bm.alpha, bm.seed, bm.chunk) == (32, 4, 16, 8, 3, 0.1, 5, 8)
    assert not bm.has_reference and bm.baseline is None and bm.converged_at is None
    assert BinnedModes(S=32, bins=16, images=16).bins == 16 and BinnedModes(S=32, bins=1, images=1).bins == 1
    for bad in (dict(bins=17, images=16), dict(bins=0), dict(S=6), dict(S=0), dict(images=0, bins=1), dict(samples=0), dict(chunk=0),
                dict(iterations=-1), dict(alpha=0.0), dict(alpha=1.0), dict(bins=65536, images=70000)):
        with pytest.raises(ValueError):
            BinnedModes(**dict(dict(S=64), **bad))
    with pytest.raises(RuntimeError):
        bm.evaluate(None)
    with pytest.raises(RuntimeError):
        bm.between(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError):
        bm.save_picture("x.png", {"order": [0]})
    with pytest.raises(TypeError):
        BinnedModes(S=64, device="cpu").reference_from_store(types.SimpleNamespace())
    bm.centres = "set"
    with pytest.raises(TypeError):
        bm.between(torch.zeros(2, 3, 32, 32))
    codes, labels = torch.zeros(4, 64, dtype=torch.int8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        group_sums(codes, labels, 2)
    with pytest.raises(TypeError):
        centroids(torch.zeros(2, 64, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 4, codes[:2])
    with pytest.raises(TypeError):
        kmeans_codes((codes, torch.zeros(4, dtype=torch.int64), labels), 2)


def test_the_initial_rows_are_distinct_and_not_flagged():
    from locate_amd.modes import initial_rows
    flags = [0, 3, 0, 0, 1, 0, 0]
    ok = [0, 2, 3, 5, 6]
    perm = torch.randperm(5, generator=torch.Generator().manual_seed(21))
    assert initial_rows(flags, 5, 21).tolist() == [ok[i] for i in perm.tolist()]
    assert initial_rows(torch.tensor(flags), 2, 21).tolist() == [ok[i] for i in perm[:2].tolist()]
    for K in (0, 6):
        with pytest.raises(ValueError):
            initial_rows(flags, K, 21)


class FakeModes:
    def __init__(self):
        self.calls, self.pictures = [], []

    def evaluate(self, gen, latents=None):
        self.calls.append((gen, latents))
        f = [3, 1] if gen == "EMA" else [0, 4]
        return {"bins": 2, "images": 8, "samples": 4, "alpha": 0.05, "ndb": 1, "ndb_over_k": 0.5, "js": 0.25, "missing": f.count(0),
                "real_counts": [4, 4], "fake_counts": f, "z": [-2.5, 2.5], "different": [True, True], "order": [0, 1], "nonfinite": 0,
                "kmeans": {"iterations": 10, "converged_at": 4, "inertia": [9, 5, 5]},
                "baseline": {"ndb": 0, "ndb_over_k": 0.0, "js": 0.01, "missing": 0, "fake_counts": [2, 2]}}

    def save_picture(self, path, record):
        self.pictures.append((path, record["fake_counts"]))
        open(path, "wb").close()
        return path


def fake_trainer(out, **kw):
    """a Trainer with only what `_modes` reads: no networks, no GPU"""
    from locate_amd import Trainer
    t = Trainer.__new__(Trainer)
    t.out, t.gen, t.iterations, t.average = str(out), "GEN", 12, kw.get("average")
    t.modes = kw.get("modes")
    return t


def test_the_trainers_record(tmp_path):
    keys = sorted(FakeModes().evaluate("GEN")) + ["epoch", "iterations"]
    bm = FakeModes()
    t = fake_trainer(tmp_path, modes=bm)
    os.makedirs(str(tmp_path / "error"))
    path, png = str(tmp_path / "error" / "modes.json"), str(tmp_path / "1-modes.png")
    assert t._modes(0) == [path, png] and os.path.exists(path) and os.path.exists(png) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == sorted(keys) and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["missing"]) == (1, 12, 1)
    assert bm.calls == [("GEN", None)] and bm.pictures == [(png, [0, 4])]          # the metric's own fixed latents; the live record's picture
    # a later epoch - or a resumed run - appends to the list it finds; with an average, its record goes under "average"
    t.average = types.SimpleNamespace(generator="EMA")
    t.iterations = 24
    assert t._modes(1) == [path, str(tmp_path / "2-modes.png")]
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and sorted(rec2[1]) == sorted(keys + ["average"])
    assert sorted(rec2[1]["average"]) == sorted(k for k in keys if k not in ("epoch", "iterations", "baseline"))
    assert rec2[1]["average"]["fake_counts"] == [3, 1] and rec2[1]["fake_counts"] == [0, 4] and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 24)
    assert bm.pictures[-1] == (str(tmp_path / "2-modes.png"), [0, 4])
    assert os.listdir(str(tmp_path / "error")) == ["modes.json"]


def test_trainer_without_modes_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    assert Trainer(step, pipeline, "OUT").modes is None
    marker = FakeModes()
    on = Trainer(step, pipeline, "OUT", modes=marker)
    assert on.modes is marker and on.written == [] and marker.calls == []          # nothing is evaluated before an epoch ends


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    args = run.parser().parse_args(base)
    assert (args.modes, args.modes_bins, args.modes_images) == (0, 128, 16384)
    args = run.parser().parse_args(base + ["--modes", "4096", "--modes-bins", "64", "--modes-images", "8192"])
    assert (args.modes, args.modes_bins, args.modes_images) == (4096, 64, 8192)

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for extra in ([], ["--modes", "0"], ["--modes", "64"], ["--modes", "64", "--modes-bins", "1"],
                  ["--modes", "64", "--modes-bins", "200", "--modes-images", "200"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--modes", "-1"], ["--modes", "many"], ["--modes"], ["--modes", "64", "--modes-bins", "0"], ["--modes", "64", "--modes-bins", "-3"],
                  ["--modes", "64", "--modes-images", "-1"], ["--modes", "64", "--modes-bins", "201", "--modes-images", "200"],
                  ["--modes", "64", "--modes-images", "100"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--modes SAMPLES" in text and "--modes-bins K" in text and "--modes-images IMAGES" in text
    assert "--modes" in run.__doc__ and "--modes-bins" in run.__doc__ and "--modes-images" in run.__doc__ and "modes" in run.Trainer.__doc__
