"""bench.py's command line and its output dump, on the host: a plain run leaves the extra measurements to --full, and
--dump-outputs writes the same float32 arrays, within the size cap, every time it is given the same tensors."""
import sys

import numpy as np
import torch

import bench


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)


def test_dump_outputs_is_repeatable_and_capped(tmp_path):
    torch.manual_seed(0)
    big = torch.nn.Linear(1500, 1000)                      # 1.5 M parameters: written as a sample
    small = torch.nn.Linear(10, 3)
    out = {"d_error": torch.tensor(0.25), "generated": torch.randn(2, 3, 8, 8), "note": "not a tensor"}
    for d in ("a", "b"):
        bench.dump_outputs(out, {"G": big, "D": small}, str(tmp_path / d))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["D_parameters.npy", "G_parameters.npy", "d_error.npy", "generated.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "generated.npy").shape == (2, 3, 8, 8)
    assert np.array_equal(np.load(tmp_path / "a" / "generated.npy"), out["generated"].numpy())
    g = np.load(tmp_path / "a" / "G_parameters.npy")
    assert g.shape == (bench.DUMP_MAX_ELEMENTS,)
    flat = torch.cat([p.detach().reshape(-1) for p in big.parameters()]).numpy()
    assert np.isin(g, flat).all()
