"""The radial power spectrum's host side (locate_amd/spectrum.py, the hooks in locate_amd/run.py) without a GPU: import and
construction, what is refused, the gap arithmetic, the trainer's record with a stand-in, and the command line."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

KEYS = ["baseline", "bins", "fake", "gap_db", "high_gap_db", "images", "max_abs_gap_db", "nonfinite", "real", "window"]


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.spectrum, locate_amd._lib as L\n"
            "from locate_amd import RadialSpectrum, dft_tables, radial_bins, radial_spectrum, spectrum_summary\n"
            "rs = RadialSpectrum(S=64)\n"
            "assert (rs.S, rs.images, rs.seed, rs.chunk, rs.window, rs.bins) == (64, 4096, 999, 64, 'none', 46) and str(rs.device) == 'cuda'\n"
            "assert radial_bins(64)[0].shape == (64, 33) and dft_tables(32, 'hann')[0].shape == (32, 32)\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_the_abi_is_declared_bound_and_built():
    from locate_amd import build
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert EXPECTED_ABI >= 18 and "spectrum.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "spectrum.hip"))
    header = open(os.path.join(ROOT, "include", "locate_hip.h")).read()
    for name, args in (("locate_spectrum_workspace_bytes", 2), ("locate_spectrum_planes", 11), ("locate_spectrum_summary_workspace_bytes", 1),
                       ("locate_spectrum_summary", 9)):
        assert name in PROTOTYPES and name + "(" in header and len(PROTOTYPES[name][1]) == args
    with open(os.path.join(build.CSRC, "runtime.hip")) as f:
        assert "return %d;" % EXPECTED_ABI in f.read()
    source = open(os.path.join(build.CSRC, "spectrum.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in source


def test_construction_and_what_is_refused():
    from locate_amd import RadialSpectrum, radial_bins, radial_spectrum, spectrum_summary
    from locate_amd.spectrum import dft_tables
    rs = RadialSpectrum(S=32, images=16, seed=5, chunk=8, window="hann", device="cuda:0")
    assert (rs.S, rs.images, rs.seed, rs.chunk, rs.window, rs.bins) == (32, 16, 5, 8, "hann", 24) and not rs.has_reference and rs.baseline is None
    for bad in (dict(S=16), dict(S=48), dict(S=512), dict(images=0), dict(chunk=0), dict(window="hamming")):
        with pytest.raises(ValueError):
            RadialSpectrum(**dict(dict(S=64), **bad))
    for S in (0, 16, 48, 100, 512):
        with pytest.raises(ValueError):
            radial_bins(S)
        with pytest.raises(ValueError):
            dft_tables(S)
    with pytest.raises(ValueError):
        dft_tables(32, "blackman")
    with pytest.raises(RuntimeError):
        rs.evaluate(None)
    with pytest.raises(RuntimeError):
        rs.distance(torch.zeros(16, 3, 32, 32))
    with pytest.raises(TypeError):
        rs.between(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    with pytest.raises(TypeError):
        rs.set_reference(torch.zeros(16, 3, 32, 32))
    with pytest.raises(TypeError):
        radial_spectrum(torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        radial_spectrum(torch.zeros(2, 3, 32, 32), window="hamming")
    with pytest.raises(TypeError):
        spectrum_summary(torch.zeros(2, 3, 24, dtype=torch.float64))
    with pytest.raises(TypeError):
        RadialSpectrum(S=32, device="cpu").latents(8)


def test_gap_arithmetic():
    from locate_amd.spectrum import gap_record
    R = 24
    real = [[1.0] * R, [2.0] * R, [4.0] * R]
    fake = [[10.0] * R, [2.0] * R, [0.04] * R]
    fake[1] = [2.0] * 8 + [4.0] * 16          # S / 4 = 8: the high band of channel 1 is 3.01 dB up
    rec = gap_record(real, fake, 32)
    assert sorted(rec) == ["fake", "gap_db", "high_gap_db", "max_abs_gap_db", "real"] and rec["real"] == real and rec["fake"] == fake
    assert rec["gap_db"][0] == [10.0] * R and rec["gap_db"][2] == [10.0 * math.log10(0.04 / 4.0)] * R
    assert rec["gap_db"][1][:8] == [0.0] * 8 and rec["gap_db"][1][8] == 10.0 * math.log10(2.0)
    assert rec["high_gap_db"][0] == 10.0 and abs(rec["high_gap_db"][1] - 10.0 * math.log10(2.0)) < 1e-12 and abs(rec["high_gap_db"][2] + 20.0) < 1e-12
    assert rec["max_abs_gap_db"] == max(abs(v) for row in rec["gap_db"] for v in row) and abs(rec["max_abs_gap_db"] - 20.0) < 1e-12
    json.dumps(rec)


class FakeSpectrum:
    def __init__(self):
        self.calls = []

    def evaluate(self, gen):
        self.calls.append(gen)
        from locate_amd.spectrum import gap_record
        lift = 2.0 if gen == "EMA" else 4.0
        value = {"bins": 24, "images": 4, "window": "none"}
        value.update(gap_record([[1.0] * 24] * 3, [[lift] * 24] * 3, 32))
        value["nonfinite"] = 0
        value["baseline"] = dict(gap_record([[1.0] * 24] * 3, [[1.0] * 24] * 3, 32), nonfinite=0)
        return value


def fake_trainer(out, **kw):
    """a Trainer with only what `_spectrum` reads: no networks, no GPU"""
    from locate_amd import Trainer
    t = Trainer.__new__(Trainer)
    t.out, t.gen, t.iterations, t.average = str(out), "GEN", 12, kw.get("average")
    t.spectrum = kw.get("spectrum")
    return t


def test_the_trainers_record(tmp_path):
    keys = sorted(KEYS + ["epoch", "iterations"])
    rs = FakeSpectrum()
    t = fake_trainer(tmp_path, spectrum=rs)
    os.makedirs(str(tmp_path / "error"))
    path = str(tmp_path / "error" / "spectrum.json")
    assert t._spectrum(0) == path and os.path.exists(path) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == keys and (rec[0]["epoch"], rec[0]["iterations"]) == (1, 12)
    assert abs(rec[0]["high_gap_db"][0] - 10 * math.log10(4.0)) < 1e-12 and rec[0]["baseline"]["max_abs_gap_db"] == 0.0
    assert rs.calls == ["GEN"]
    t.average = types.SimpleNamespace(generator="EMA")
    t.iterations = 24
    assert t._spectrum(1) == path
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and sorted(rec2[1]) == sorted(keys + ["average"])
    assert sorted(rec2[1]["average"]) == [k for k in keys if k not in ("epoch", "iterations", "baseline")]
    assert abs(rec2[1]["average"]["high_gap_db"][2] - 10 * math.log10(2.0)) < 1e-12 and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 24)
    assert os.listdir(str(tmp_path / "error")) == ["spectrum.json"]


def test_trainer_without_spectrum_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    assert Trainer(step, pipeline, "OUT").spectrum is None
    marker = FakeSpectrum()
    on = Trainer(step, pipeline, "OUT", spectrum=marker)
    assert on.spectrum is marker and on.written == [] and marker.calls == []          # nothing is evaluated before an epoch ends


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    args = run.parser().parse_args(base)
    assert (args.spectrum_images, args.spectrum_window) == (0, "none")
    args = run.parser().parse_args(base + ["--spectrum-images", "4096", "--spectrum-window", "hann"])
    assert (args.spectrum_images, args.spectrum_window) == (4096, "hann")

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for extra in ([], ["--spectrum-images", "0"], ["--spectrum-images", "64"], ["--spectrum-images", "64", "--spectrum-window", "hann"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--spectrum-images", "-1"], ["--spectrum-images", "many"], ["--spectrum-images"], ["--spectrum-images", "64", "--spectrum-window", "hamming"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    with pytest.raises(SystemExit):          # a size the kernels do not take is refused before the GPU is asked for
        run.main(["--store", "S.npy", "--image-size", "16", "--batch", "8", "--out", "OUT", "--spectrum-images", "64"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--spectrum-images N" in text and "--spectrum-window" in text
    assert "--spectrum-images" in run.__doc__ and "spectrum" in run.Trainer.__doc__


def test_tables_need_no_gpu():
    from locate_amd.spectrum import dft_tables, radial_bins
    bins, mult = radial_bins(256)
    assert mult.size == 182 and int(mult.sum()) == 256 * 256 and bins.shape == (256, 129)
    c, s = dft_tables(128)
    assert c.dtype == np.float32 and float(c[1, 32]) == 0.0 and float(s[1, 32]) == 1.0 and float(c[64, 3]) == -1.0
