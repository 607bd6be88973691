"""The multi-scale SSIM's host side (locate_amd/msssim.py, the hooks in locate_amd/run.py) without a GPU: import and construction,
what is refused, the trainer's record with a stand-in, and the command line."""
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT

KEYS = ["clamped", "levels", "mean", "nonfinite", "pairs", "real", "std"]


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.msssim, locate_amd._lib as L\n"
            "from locate_amd import MultiScaleSSIM, ms_ssim, ms_ssim_levels, ms_ssim_value, window_taps\n"
            "m = MultiScaleSSIM(S=64)\n"
            "assert (m.S, m.pairs, m.seed, m.chunk, m.real) == (64, 4096, 999, 64, None) and str(m.device) == 'cuda'\n"
            "assert window_taps(64).shape == (5, 11) and locate_amd.msssim.SIZES == (32, 64, 128, 256)\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_the_abi_is_declared_bound_and_built():
    from locate_amd import build
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert EXPECTED_ABI >= 19 and "msssim.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "msssim.hip"))
    header = open(os.path.join(ROOT, "include", "locate_hip.h")).read()
    for name, args in (("locate_msssim_workspace_bytes", 2), ("locate_msssim_pairs", 11)):
        assert name in PROTOTYPES and name + "(" in header and len(PROTOTYPES[name][1]) == args
    with open(os.path.join(build.CSRC, "runtime.hip")) as f:
        assert "return %d;" % EXPECTED_ABI in f.read()


def test_the_source_accumulates_no_product_in_fp32():
    """How it is checked: in csrc/msssim.hip every `float` value is a plane element, a pointer to one, or the 2 x 2 mean (exact in
    fp32: four values of at most 16 bits); so no line may hold a float accumulation (`+=` on a float, fmaf, a float-typed sum of
    products), every accumulator is declared double, the filter chains are fma() on doubles, and contraction is off for the whole
    file.  The GPU test's bright near-flat texture is the check that matters: fp32 accumulation misses it by 60000 bounds."""
    source = open(os.path.join(ROOT, "locate_amd", "csrc", "msssim.hip")).read()
    code = "\n".join(line.split("//")[0] for line in source.splitlines())
    assert "#pragma clang fp contract(off)" in code
    assert "fmaf" not in code and "__fmaf" not in code and "atomic" not in code
    assert code.count("fma(") >= 4
    for line in code.splitlines():
        if re.search(r"\bfloat\b[^;]*=", line) and "*" in line.split("=", 1)[1]:
            # a float assigned from an expression with `*`: only pointer arithmetic / dereferences, or the exact 2 x 2 mean
            assert "0.25f" in line or "reinterpret_cast" in line or re.search(r"float\* \w+ = ", line), line
    assert not re.search(r"float\s+\w+\s*\+=", code)


def test_construction_and_what_is_refused():
    from locate_amd import MultiScaleSSIM, ms_ssim, ms_ssim_levels, ms_ssim_value
    m = MultiScaleSSIM(S=32, pairs=8, seed=5, chunk=4, device="cuda:0")
    assert (m.S, m.pairs, m.seed, m.chunk) == (32, 8, 5, 4) and m.real is None
    for bad in (dict(S=16), dict(S=48), dict(S=512), dict(pairs=0), dict(pairs=-3), dict(chunk=3), dict(chunk=63), dict(chunk=0)):
        with pytest.raises(ValueError):
            MultiScaleSSIM(**dict(dict(S=64), **bad))
    img = torch.zeros(4, 3, 32, 32)
    with pytest.raises(TypeError):
        m.between(img, img)
    with pytest.raises(TypeError):
        m.among(img)
    with pytest.raises(TypeError):
        ms_ssim(img, img)
    with pytest.raises(TypeError):
        ms_ssim_value(torch.zeros(4, 2, 5, dtype=torch.float64))
    triple = (torch.zeros(4, 3072, dtype=torch.int8), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        ms_ssim_levels(triple, triple)
    with pytest.raises(ValueError):
        ms_ssim_levels(triple[:2], triple)
    with pytest.raises(TypeError):
        MultiScaleSSIM(S=32, device="cpu").latents(8)
    with pytest.raises(TypeError):
        MultiScaleSSIM(S=32, device="cpu").reference_from_pipeline(None)


class FakeMetric:
    def __init__(self):
        self.calls = []

    def _value(self, mean):
        return {"pairs": 4, "mean": mean, "std": 0.125, "clamped": 1, "nonfinite": 0, "levels": {"ssim": [mean] * 5, "cs": [0.5] * 5}}

    def evaluate(self, gen):
        self.calls.append(gen)
        return dict(self._value(0.25 if gen == "EMA" else 0.5), real=self._value(0.125))

    def evaluate_against(self, a, b):
        self.calls.append((a, b))
        return self._value(0.75)


def fake_trainer(out, **kw):
    """a Trainer with only what `_msssim` reads: no networks, no GPU"""
    from locate_amd import Trainer
    t = Trainer.__new__(Trainer)
    t.out, t.gen, t.iterations, t.average = str(out), "GEN", 12, kw.get("average")
    t.msssim = kw.get("msssim")
    return t


def test_the_trainers_record(tmp_path):
    keys = sorted(KEYS + ["epoch", "iterations"])
    metric = FakeMetric()
    t = fake_trainer(tmp_path, msssim=metric)
    os.makedirs(str(tmp_path / "error"))
    path = str(tmp_path / "error" / "msssim.json")
    assert t._msssim(0) == path and os.path.exists(path) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == keys and (rec[0]["epoch"], rec[0]["iterations"]) == (1, 12)
    assert rec[0]["mean"] == 0.5 and rec[0]["real"]["mean"] == 0.125 and sorted(rec[0]["levels"]) == ["cs", "ssim"]
    assert metric.calls == ["GEN"]
    t.average = types.SimpleNamespace(generator="EMA")
    t.iterations = 24
    assert t._msssim(1) == path
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and sorted(rec2[1]) == sorted(keys + ["average", "average_to_live"])
    assert sorted(rec2[1]["average"]) == [k for k in KEYS if k != "real"] and rec2[1]["average"]["mean"] == 0.25
    assert sorted(rec2[1]["average_to_live"]) == [k for k in KEYS if k != "real"] and rec2[1]["average_to_live"]["mean"] == 0.75
    assert metric.calls == ["GEN", "GEN", "EMA", ("GEN", "EMA")] and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 24)
    assert os.listdir(str(tmp_path / "error")) == ["msssim.json"]


def test_trainer_without_the_metric_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    assert Trainer(step, pipeline, "OUT").msssim is None
    marker = FakeMetric()
    on = Trainer(step, pipeline, "OUT", msssim=marker)
    assert on.msssim is marker and on.written == [] and marker.calls == []          # nothing is evaluated before an epoch ends


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    assert run.parser().parse_args(base).msssim_pairs == 0
    assert run.parser().parse_args(base + ["--msssim-pairs", "4096"]).msssim_pairs == 4096

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    for extra in ([], ["--msssim-pairs", "0"], ["--msssim-pairs", "1"], ["--msssim-pairs", "64"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--msssim-pairs", "-1"], ["--msssim-pairs", "many"], ["--msssim-pairs"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    with pytest.raises(SystemExit):          # a size the kernels do not take is refused before the GPU is asked for
        run.main(["--store", "S.npy", "--image-size", "16", "--batch", "8", "--out", "OUT", "--msssim-pairs", "64"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run.main(["--help"])
    text = capsys.readouterr().out
    assert "--msssim-pairs N" in text
    assert "--msssim-pairs" in run.__doc__ and "msssim" in run.Trainer.__doc__


def test_the_chunk_the_command_line_chooses_is_even():
    from locate_amd import MultiScaleSSIM
    for n in (1, 2, 3, 31, 32, 33, 4096):
        chunk = min(64, 2 * n) // 2 * 2
        assert MultiScaleSSIM(32, pairs=n, chunk=chunk).chunk == min(64, 2 * n)
