"""The format audit's host side (locate_amd/formats.py, the tap in locate_amd/ops.py, the hooks in locate_amd/run.py) without a GPU:
which entries there are and in which order, how a weight's address finds its slots, what is refused, the decoded rows, the report
and the saved file, and the command line."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import formats_model as M  # noqa: E402


def tiny_networks():
    from locate_amd import Discriminator, Generator, NetConfig
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    return Generator(cfg), Discriminator(cfg)


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.formats, locate_amd._lib as L\n"
            "from locate_amd import FormatAudit, format_errors, ops\n"
            "assert ops.CONTRACTION_TAP is None\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_abi_and_build_list():
    from locate_amd import build
    from locate_amd._lib import EXPECTED_ABI, PROTOTYPES
    assert EXPECTED_ABI >= 17 and "formats.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "formats.hip"))
    with open(os.path.join(ROOT, "include", "locate_hip.h")) as f:
        header = f.read()
    names = ["locate_formats_count", "locate_formats_name", "locate_formats_max_views", "locate_formats_view_record_bytes",
             "locate_formats_base_record_bytes", "locate_formats_format_record_bytes", "locate_formats_workspace_bytes", "locate_formats_audit"]
    for name in names:
        assert name in PROTOTYPES and name + "(" in header
    assert len(PROTOTYPES["locate_formats_audit"][1]) == 6
    with open(os.path.join(build.CSRC, "runtime.hip")) as f:
        assert "return %d;" % EXPECTED_ABI in f.read()


def test_entries_and_their_order():
    from locate_amd import FormatAudit, SpectralNorm
    from locate_amd.formats import ROLES
    G, D = tiny_networks()
    audit = FormatAudit(G, D)          # no GPU needed
    assert ROLES == ("fwd.x", "fwd.w", "dgrad.gy", "dgrad.w", "wgrad.x", "wgrad.gy")
    dense = ["%s/%s.module.weight_bar" % (tag, name) for tag, net in (("G", G), ("D", D)) for name, m in net.named_modules()
             if isinstance(m, SpectralNorm) and getattr(m.module, "groups", 1) == 1]
    names = [n for n, _ in audit.layers]
    assert names == dense and len(names) > 10 and len(set(names)) == len(names)
    assert any(isinstance(m.module, torch.nn.ConvTranspose2d) for m in G.modules() if isinstance(m, SpectralNorm))
    assert any(isinstance(m.module, torch.nn.Linear) for m in G.modules() if isinstance(m, SpectralNorm))
    entries = audit.entries()
    assert entries == [(n, r) for n in names for r in ROLES]
    assert all(audit.slot(n, r) == i for i, (n, r) in enumerate(entries))
    # a weight's address finds its layer, whatever view of it the contraction is handed
    keys = audit.key_map()
    assert len(keys) == len(names)
    for i, (_, w) in enumerate(audit.layers):
        assert keys[w.data_ptr()] == i and keys[w.detach().view(w.shape[0], -1).data_ptr()] == i
    with pytest.raises(ValueError):
        FormatAudit(G, D, capacity=0)
    with pytest.raises(ValueError):
        FormatAudit(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2))          # nothing that reaches a dense contraction
    with pytest.raises(TypeError):
        with audit.iteration(1):          # the networks are on the CPU
            pass
    from locate_amd import ops
    assert ops.CONTRACTION_TAP is None


def test_views_of_tensors():
    from locate_amd.formats import _pack, _view, format_errors
    with pytest.raises(TypeError):
        format_errors([torch.ones(3)])          # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError):
        _view(np.ones(3, dtype=np.float32), 2)
    with pytest.raises(ValueError):
        format_errors([])
    t = types.SimpleNamespace(data_ptr=lambda: 0x1000)
    rec = _pack([(t, 2, 3, 5, 17, 1)])
    assert len(rec) == 40 and rec == (0x1000).to_bytes(8, "little") + b"".join(v.to_bytes(4, "little") for v in (2, 3, 5, 0)) + \
        (17).to_bytes(8, "little") + (1).to_bytes(4, "little") + bytes(4)


def synthetic_slots(records):
    """model records -> the int64 words the kernel would leave"""
    from locate_amd.formats import SLOT_WORDS
    words = np.zeros((len(records), SLOT_WORDS), dtype=np.int64)
    u, f = words.view(np.uint64), words.view(np.float64)
    for i, r in enumerate(records):
        if r is None:
            continue
        u[i, :4] = r["n"], r["zeros"], r["nonfinite"], r["calls"]
        f[i, 4] = r["sumsq"]
        u[i, 5] = r["absmax"]
        u[i, 6:38] = r["hist"]
        for k, fr in enumerate(r["formats"]):
            f[i, 38 + 4 * k] = fr["err_sumsq"]
            u[i, 39 + 4 * k:42 + 4 * k] = fr["flushed"], fr["subnormal"], fr["clamped"]
    return words


def test_decode_report_and_saved_file(tmp_path):
    from locate_amd import FormatAudit
    from locate_amd.formats import decode, snr_db
    G, D = tiny_networks()
    audit = FormatAudit(G, D)
    e = len(audit.entries())
    x = M.fixture((2, 33, 5), "plain", 1)
    model = [M.audit(x, 1), M.audit(x, 2)]
    words = synthetic_slots([model[0], None, model[1]] + [None] * (e - 3))
    row = decode(words)
    assert int(row["n"][0]) == 330 and int(row["nonfinite"][2]) == model[1]["nonfinite"] > 0 and row["absmax"][0] == np.float32(1.5 * 2 ** 20)
    assert row["hist"][2].tolist() == model[1]["hist"] and row["clamped"][0].tolist() == [f["clamped"] for f in model[0]["formats"]]
    assert row["err_sumsq"][2].tolist() == [f["err_sumsq"] for f in model[1]["formats"]]
    assert snr_db([4.0, 0.0, 1.0], [[1.0] * 5, [0.0] * 5, [0.0] * 5])[:, 0].tolist()[::2] == [10 * np.log10(4.0), np.inf]
    assert np.isnan(snr_db([0.0], [[0.0] * 5])).all()
    row["iteration"] = 7
    audit.rows = [row, dict(row, iteration=9)]
    report = audit.report()
    assert [r["iteration"] for r in report] == [7, 9] and report[0]["entries"] == audit.entries() and report[0]["formats"] == M.NAMES
    finite = model[0]["n"] - model[0]["nonfinite"]
    assert report[0]["flushed"][0].tolist() == [f["flushed"] / finite for f in model[0]["formats"]]
    assert report[0]["snr_db"][0, 4] == 10 * np.log10(model[0]["sumsq"] / model[0]["formats"][4]["err_sumsq"]) > 40
    assert np.isnan(report[0]["snr_db"][1]).all() and np.isnan(report[0]["flushed"][1]).all()
    (path,) = audit.save(str(tmp_path / "error"), 3)
    assert path == str(tmp_path / "error" / "3-formats.npz") and not os.path.exists(path + ".tmp")
    with np.load(path) as z:
        assert sorted(z.files) == ["absmax", "calls", "clamped", "err_sumsq", "flushed", "formats", "hist", "iterations", "n", "names",
                                   "nonfinite", "roles", "snr_db", "subnormal", "sumsq", "zeros"]
        assert z["iterations"].tolist() == [7, 9] and z["formats"].tolist() == list(M.NAMES)
        assert [tuple(p) for p in zip(z["names"].tolist(), z["roles"].tolist())] == audit.entries()
        assert z["n"].shape == (2, e) and z["n"].dtype == np.uint64 and z["hist"].shape == (2, e, 32) and z["err_sumsq"].shape == (2, e, 5)
        assert z["sumsq"][1, 2] == model[1]["sumsq"] and z["absmax"].dtype == np.float32 and z["subnormal"][0, 0].tolist() == \
            [f["subnormal"] for f in model[0]["formats"]]
        assert np.array_equal(z["snr_db"], np.stack([report[0]["snr_db"], report[1]["snr_db"]]), equal_nan=True)
    assert audit.clear().rows == [] and audit.flush() == []
    (path,) = audit.save(str(tmp_path / "error"), 4)          # no records: empty arrays with the entries' names
    with np.load(path) as z:
        assert z["iterations"].shape == (0,) and z["err_sumsq"].shape == (0, e, 5) and len(z["names"]) == e


def trainer_arguments(G, D):
    from locate_amd import Nadam, NetConfig, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=1)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    return step, pipeline


def test_trainer_arguments():
    from locate_amd import FormatAudit, Trainer
    G, D = tiny_networks()
    step, pipeline = trainer_arguments(G, D)
    with pytest.raises(ValueError):
        Trainer(step, pipeline, "OUT", formats=FormatAudit(G, D), formats_every=-1)
    off = Trainer(step, pipeline, "OUT")
    assert off.formats is None and off.formats_every == 0
    marker = FormatAudit(G, D)
    on = Trainer(step, pipeline, "OUT", formats=marker, formats_every=16)
    assert on.formats is marker and on.formats_every == 16 and on.written == []
    one = dict(epochs=1, miniter_function=lambda e: 1)
    assert Trainer(step, pipeline, "OUT", graphed=True, **one).graphed          # a graphed run without an audit is what it was
    with pytest.raises(ValueError, match="replayed graph runs no Python"):
        Trainer(step, pipeline, "OUT", graphed=True, formats=marker, formats_every=2, **one)


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--formats-every", "0"], ["--formats-every", "2"], ["--graph"], ["--graph", "--formats-every", "0"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--formats-every", "-1"], ["--formats-every", "often"], ["--formats-every"], ["--graph", "--formats-every", "2"]):
        with pytest.raises(SystemExit):
            run.main(base + extra)
    assert "not with --graph" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--formats-every N" in capsys.readouterr().out
