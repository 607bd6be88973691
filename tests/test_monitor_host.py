"""The training monitor's host side (locate_amd/monitor.py, locate_amd/run.py) without a GPU: the PNG container, the loss
curves' moving average as the reference codes it, the outer loop's schedule and file names, and the refusals."""
import os
import types

import numpy as np
import pytest
import torch

from locate_amd import LossHistory, NetConfig, Trainer, image_grid
from locate_amd import monitor, run


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 4), (5, 7, 4), (88, 328, 4)):
        rgba = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = str(tmp_path / ("p%d.png" % shape[0]))
        assert monitor.write_png(path, rgba) == path and not os.path.exists(path + ".tmp")
        assert np.array_equal(monitor.read_png(path), rgba)
        assert np.array_equal(monitor.read_png(monitor.write_png(path, torch.from_numpy(rgba), level=9)), rgba)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), rgba)
    with pytest.raises(ValueError):
        monitor.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        monitor.write_png(str(tmp_path / "bad.png"), np.zeros((4, 4, 4), np.float32))


def test_read_png_refuses_what_it_does_not_decode(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    path = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(path)          # colour type 2
    with pytest.raises(ValueError):
        monitor.read_png(path)
    with open(path, "wb") as f:
        f.write(b"not a png")
    with pytest.raises(ValueError):
        monitor.read_png(path)


def test_moving_average_is_the_reference_formula_as_coded():
    """main.py:226-232 evaluated literally: weights j = 1 .. W, divisor (W^2 - W) / 2 - not the weights' sum."""
    series = [0.5, -1.25, 2.0, 3.5, 0.125, -0.75, 1.0, 4.0, 2.25]
    for W in (2, 4, 8):
        h = LossHistory(mean_window=W)
        h.d, h.g = list(series), [2 * v for v in series]
        div = (W ** 2 - W) / 2
        want = [sum(series[i + j - 1] * j for j in range(1, W + 1)) / div for i in range(len(series) - W)]
        ma_d, ma_g = h.moving_average()
        assert ma_d == want and len(ma_d) == len(series) - W
        assert ma_g == [sum(2 * series[i + j - 1] * j for j in range(1, W + 1)) / div for i in range(len(series) - W)]
    # worked by hand, W = 2: divisor 1, entries s[i] + 2 s[i + 1]
    h = LossHistory(mean_window=2)
    h.d = h.g = [1.0, 2.0, 4.0]
    assert h.moving_average()[0] == [5.0]          # one entry: len - W
    for n in (0, 3, 4):          # len <= W: nothing
        h = LossHistory(mean_window=4)
        h.d = h.g = [1.0] * n
        assert h.moving_average() == ([], [])
    with pytest.raises(ValueError):
        LossHistory(mean_window=1)


def test_loss_history_files(tmp_path):
    import json
    h = LossHistory(mean_window=2)
    h.d, h.g = [1.0, 2.0, 4.0], [0.5, 0.25, 0.125]
    files = h.save(str(tmp_path / "error"), 3)
    assert files[0] == str(tmp_path / "error" / "3.json")
    rec = json.load(open(files[0]))
    assert rec["d"] == [1.0, 2.0, 4.0] and rec["d_moving_average"] == [5.0] and rec["g_moving_average"] == [1.0] and rec["mean_window"] == 2
    again = LossHistory()
    again.load_state_dict(h.state_dict())
    assert again.d == h.d and again.g == h.g and again.mean_window == 2


def _trainer(batch, batches=100, **kw):
    from locate_amd import Discriminator, Generator, Nadam, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    minibatches = kw.pop("step_minibatches", 8)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=minibatches)
    pipeline = types.SimpleNamespace(batch=batch, batches_per_epoch=batches)
    return Trainer(step, pipeline, "OUT", **kw)


def test_schedule_numbers():
    """libs/config.py:19-30 and main.py:109-116 by hand: MINIBATCHES = 8, MAIN_N = 1024.
    batch 16: print_every = 1024 // max(16, 64) = 16, image_intervall = 16 * 1024 // 16 = 1024;
    batch 64: print_every = 1024 // 64 = 16, image_intervall = 16384 // 64 = 256;
    epoch e: miniter = 8 (e + 1) = 8, 16, 24; sub-passes (e + 1)^2 = 1, 4, 9."""
    for batch, every, interval in ((16, 16, 1024), (64, 16, 256)):
        t = _trainer(batch)
        for e, miniter, subs in ((0, 8, 1), (1, 16, 4), (2, 24, 9)):
            assert t.schedule(e) == {"miniter": miniter, "subepochs": subs, "print_every": every, "image_interval": interval}
    assert _trainer(256).schedule(0)["print_every"] == 4 and _trainer(256).schedule(0)["image_interval"] == 64
    assert _trainer(4096).schedule(0)["print_every"] == 1 and _trainer(4096).schedule(0)["image_interval"] == 4
    assert _trainer(32768).schedule(0)["image_interval"] == 1          # max(1, 0)
    # the benchmark's schedule: MINIBATCHES = 1 gives miniter = 1 in the first epoch
    t = _trainer(64, step_minibatches=1)
    assert [t.schedule(e)["miniter"] for e in range(3)] == [1, 2, 3]
    # the schedule functions are arguments
    t = _trainer(64, miniter_function=lambda e: 1, subepoch_function=lambda e: 2, image_interval_function=lambda b: 2,
                 print_every_function=lambda b: 3)
    assert t.schedule(5) == {"miniter": 1, "subepochs": 2, "print_every": 3, "image_interval": 2}


def test_file_names():
    """main.py:204-205, 221: {sub+1:0{sub_len}d}-{i:0{batch_len}d}.png with sub_len = len(str(subepochs)), batch_len = len(str(batches))"""
    assert run.picture_name(0, 256, 1, 12662) == "1-00256.png"
    assert run.picture_name(0, None, 1, 12662) == "1-END.png"
    assert run.picture_name(2, 7, 16, 99) == "03-07.png"
    assert run.picture_name(15, None, 16, 99) == "16-END.png"
    t = _trainer(16, batches=3165)
    assert t.picture_path(0, 0, 1024) == os.path.join("OUT", "1", "1-1024.png")
    assert t.picture_path(3, 4, 24) == os.path.join("OUT", "4", "05-0024.png")          # epoch 3: 16 sub-passes
    assert t.picture_path(3, 15, None) == os.path.join("OUT", "4", "16-END.png")


def test_graphed_needs_whole_iterations():
    with pytest.raises(ValueError):
        _trainer(64, graphed=True, epochs=1)                                   # MINIBATCHES = 8: miniter = 8
    with pytest.raises(ValueError):
        _trainer(64, step_minibatches=1, graphed=True, epochs=2)                # miniter = 2 in the second epoch
    with pytest.raises(ValueError):
        _trainer(64, step_minibatches=1, graphed=True)                          # open-ended: the schedule grows
    with pytest.raises(ValueError):
        _trainer(64, step_minibatches=1, graphed=True, epochs=1, diters=2)
    assert _trainer(64, step_minibatches=1, graphed=True, epochs=1).graphed
    assert _trainer(64, graphed=True, epochs=3, miniter_function=lambda e: 1).graphed


def test_cpu_tensors_are_rejected():
    with pytest.raises(TypeError):
        image_grid(torch.zeros(4, 3, 8, 8))
    with pytest.raises(TypeError):
        image_grid(np.zeros((4, 3, 8, 8), np.float32))
    from locate_amd import Generator, Sampler
    with pytest.raises(TypeError):
        Sampler(Generator(NetConfig(image_size=32, base_feature_factor=1)), images=4)
    with pytest.raises(TypeError):
        LossHistory().record({"d_error": torch.zeros(()), "g_error": torch.zeros(())})
    assert monitor.grid_geometry(13, 32, 8, 8) == (8, 2, 88, 328) and monitor.grid_geometry(1, 16, 8, 2) == (1, 1, 20, 20)
