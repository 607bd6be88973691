"""The nearest-neighbour search's host side (locate_amd/neighbours.py, the hooks in locate_amd/run.py) without a GPU: the canonical
record, construction, what is refused, the trainer's record and file names with a stand-in, and the command line."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.neighbours, locate_amd._lib as L\n"
            "from locate_amd import NearestNeighbours, encode_images, nearest\n"
            "nn = NearestNeighbours(S=64, k=3, images=64, seed=999, device='cuda:0')\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


@pytest.mark.parametrize("H,W", [(10, 14), (14, 10), (12, 12), (10, 40)])
def test_the_canonical_record_is_valid_and_is_the_fallback_of_draw_params(H, W):
    from locate_amd.data import PLAIN_ORDER, draw_params, validate
    from locate_amd.neighbours import canonical_params
    rec = canonical_params(5, H, W)
    side = min(H, W)
    validate(np.arange(5), rec, 5, H, W, side, side)          # side_lo = side_hi = min(H, W): the plan of the bank
    assert (rec["side"] == side).all() and (rec["top"] == (H - side) // 2).all() and (rec["left"] == (W - side) // 2).all()
    assert (rec["flip"] == 0).all() and (rec["order"] == PLAIN_ORDER).all()
    assert (rec["brightness"] == 1).all() and (rec["contrast"] == 1).all() and (rec["saturation"] == 1).all()
    if (H, W) == (10, 40):          # sqrt(400 U(0.75, 1)) >= 17 > 10: no try fits, every record is the fallback
        drawn = draw_params(torch.Generator().manual_seed(1), 5, H, W, 8, False)
        assert drawn.tobytes() == rec.tobytes()


def test_construction_and_what_is_refused():
    from locate_amd import NearestNeighbours, encode_images, nearest
    from locate_amd.neighbours import row_bytes
    assert [row_bytes(S) for S in (4, 8, 12, 20, 64, 256)] == [64, 192, 448, 1216, 12288, 196608]
    nn = NearestNeighbours(S=64, k=3, images=64, seed=999, device="cuda:0")
    assert (nn.S, nn.k, nn.images, nn.seed, nn.row_bytes) == (64, 3, 64, 999, 12288) and not nn.has_reference
    for bad in (dict(k=0), dict(k=9), dict(S=6), dict(images=0), dict(chunk=0)):
        with pytest.raises(ValueError):
            NearestNeighbours(**dict(dict(S=64), **bad))
    with pytest.raises(RuntimeError):
        nn.search(torch.zeros(2, 3, 64, 64))
    with pytest.raises(RuntimeError):
        nn.evaluate(None)
    with pytest.raises(RuntimeError):
        nn.save_picture("x.png", None)
    with pytest.raises(TypeError):
        NearestNeighbours(S=64, device="cpu").reference_from_store(types.SimpleNamespace())
    with pytest.raises(TypeError):
        encode_images(torch.zeros(2, 3, 8, 8))
    cpu = (torch.zeros(2, 64, dtype=torch.int8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        nearest(cpu, cpu)


class FakeNeighbours:
    def __init__(self):
        self.calls = []

    def evaluate(self, gen, latents=None):
        self.calls.append(("evaluate", gen, latents))
        tag = 0.5 if gen == "EMA" else 1.0
        return {"images": 2, "k": 2, "index": [[3, 1], [0, -1]], "d2": [[5, 9], [0, -1]], "rms": [0.1 * tag, 0.0],
                "generated_to_real": {"min": 0.0, "median": 0.05 * tag}, "generated_to_generated": {"min": 0.2, "median": 0.2},
                "real_to_real": {"min": 0.3, "median": 0.4}, "real_among_themselves": {"min": 0.5, "median": 0.6}, "nonfinite": 0}

    def save_picture(self, path, gen, latents=None):
        self.calls.append(("picture", gen, latents))
        with open(path, "wb") as f:
            f.write(b"png")
        return path


def fake_trainer(out, **kw):
    """a Trainer with only what `_nearest` reads: no networks, no GPU"""
    from locate_amd import Trainer
    t = Trainer.__new__(Trainer)
    t.out, t.gen, t.iterations, t.average = str(out), "GEN", 12, kw.get("average")
    t.neighbours = kw.get("neighbours")
    t._sampler = types.SimpleNamespace(fixed_noise="LATENTS")
    return t


def test_the_trainers_record_and_file_names(tmp_path):
    keys = ["epoch", "generated_to_generated", "generated_to_real", "images", "index", "iterations", "k", "nonfinite", "real_among_themselves",
            "real_to_real"]
    nn = FakeNeighbours()
    t = fake_trainer(tmp_path, neighbours=nn)
    os.makedirs(str(tmp_path / "error"))
    written = t._nearest(0)
    path = str(tmp_path / "error" / "neighbours.json")
    assert written == [path, str(tmp_path / "error" / "1-neighbours.png")]
    assert all(os.path.exists(f) for f in written) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == keys and (rec[0]["epoch"], rec[0]["iterations"]) == (1, 12)
    assert rec[0]["index"] == [[3, 1], [0, -1]] and rec[0]["generated_to_real"] == {"min": 0.0, "median": 0.05}
    assert nn.calls == [("evaluate", "GEN", "LATENTS"), ("picture", "GEN", "LATENTS")]          # the sampler's fixed latents
    # a later epoch appends; with an average, its record goes under "average" and its picture beside the first
    t.average = types.SimpleNamespace(generator="EMA")
    t.iterations = 24
    written = t._nearest(1)
    assert written == [path, str(tmp_path / "error" / "2-neighbours.png"), str(tmp_path / "error" / "2-neighbours.ema.png")]
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and sorted(rec2[1]) == sorted(keys + ["average"])
    assert sorted(rec2[1]["average"]) == [k for k in keys if k not in ("epoch", "iterations")]
    assert rec2[1]["average"]["generated_to_real"]["median"] == 0.025 and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 24)
    assert sorted(os.listdir(str(tmp_path / "error"))) == ["1-neighbours.png", "2-neighbours.ema.png", "2-neighbours.png", "neighbours.json"]


def test_trainer_without_neighbours_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    assert Trainer(step, pipeline, "OUT").neighbours is None
    marker = FakeNeighbours()
    on = Trainer(step, pipeline, "OUT", neighbours=marker)
    assert on.neighbours is marker and on.written == [] and marker.calls == []          # nothing is evaluated before an epoch ends


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run
    args = run.parser().parse_args(["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"])
    assert (args.neighbours, args.neighbours_k) == (0, 3)
    args = run.parser().parse_args(["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT", "--neighbours", "64", "--neighbours-k", "5"])
    assert (args.neighbours, args.neighbours_k) == (64, 5)

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--neighbours", "0"], ["--neighbours", "64"], ["--neighbours", "64", "--neighbours-k", "8"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--neighbours", "-1"], ["--neighbours", "many"], ["--neighbours"], ["--neighbours", "64", "--neighbours-k", "0"],
                  ["--neighbours", "64", "--neighbours-k", "9"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--neighbours IMAGES" in text and "--neighbours-k K" in text
