"""The sliced Wasserstein metric's host side (locate_amd/metric.py, the hook in locate_amd/run.py) without a GPU: the level
sizes, the seeded tables, the refusals, and a run loop that is unchanged without the metric."""
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def test_pyramid_levels():
    from locate_amd import pyramid_levels
    assert pyramid_levels(16) == [16]
    assert pyramid_levels(64) == [64, 32, 16]
    assert pyramid_levels(256) == [256, 128, 64, 32, 16]
    assert pyramid_levels(64, min_size=32) == [64, 32]
    for bad in (8, 15, 48, 100, 0):
        with pytest.raises(ValueError):
            pyramid_levels(bad)


def test_seed_reproduces_positions_and_directions():
    from locate_amd import SlicedWasserstein
    kw = dict(images=6, nhoods_per_image=5, dir_repeats=3, dirs_per_repeat=7, device="cpu")          # tables only: no GPU is touched
    a, b, c = SlicedWasserstein(64, seed=5, **kw), SlicedWasserstein(64, seed=5, **kw), SlicedWasserstein(64, seed=6, **kw)
    assert a.sizes == [64, 32, 16]
    assert a.directions.dtype == torch.float32 and tuple(a.directions.shape) == (147, 21)
    assert torch.equal(a.directions, b.directions) and not torch.equal(a.directions, c.directions)
    assert float((a.directions.double().square().sum(0).sqrt() - 1).abs().max()) <= 1e-6
    for which in ("reference", "candidate"):
        assert len(a.positions[which]) == 3
        for l, s in enumerate(a.sizes):
            p = a.positions[which][l]
            assert p.dtype == torch.int32 and tuple(p.shape) == (30, 2)
            assert int(p.min()) >= 0 and int(p.max()) <= s - 7
            assert torch.equal(p, b.positions[which][l]) and not torch.equal(p, c.positions[which][l])
        assert not torch.equal(a.positions["reference"][l], a.positions["candidate"][l])
    # the 16 x 16 level of a larger table reaches both ends of [0, 9]
    big = SlicedWasserstein(16, images=64, nhoods_per_image=16, device="cpu").positions["reference"][0]
    assert int(big.min()) == 0 and int(big.max()) == 9
    assert not a.has_reference
    with pytest.raises(RuntimeError):
        a.distance(torch.zeros(6, 3, 64, 64))
    with pytest.raises(ValueError):
        SlicedWasserstein(48, device="cpu")
    with pytest.raises(ValueError):
        SlicedWasserstein(64, images=0, device="cpu")


def test_importing_the_metric_loads_no_library():
    code = ("import sys, locate_amd.metric, locate_amd._lib as L\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'liblocate_hip' not in maps, 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_cpu_tensors_are_rejected():
    from locate_amd import SlicedWasserstein, descriptor_stats, laplacian_pyramid, project_descriptors, sorted_distance
    from locate_amd import metric
    x = torch.zeros(2, 3, 32, 32)
    pos = torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(TypeError):
        laplacian_pyramid(x)
    with pytest.raises(TypeError):
        metric.pyr_down(x)
    with pytest.raises(TypeError):
        metric.pyr_residual(x, torch.zeros(2, 3, 16, 16))
    with pytest.raises(TypeError):
        descriptor_stats(x, pos, 2)
    with pytest.raises(TypeError):
        project_descriptors(x, pos, 2, torch.zeros(147, 4), torch.zeros(6))
    with pytest.raises(TypeError):
        sorted_distance(torch.zeros(8), torch.zeros(8))
    with pytest.raises(TypeError):
        laplacian_pyramid(x.numpy())
    swd = SlicedWasserstein(32, images=2, nhoods_per_image=2, dir_repeats=1, dirs_per_repeat=2, device="cpu")
    with pytest.raises(TypeError):
        swd.set_reference(x)
    with pytest.raises(TypeError):
        swd.between(x, x)
    from locate_amd import Generator, NetConfig
    swd._reference = [[None]]          # as if set: the refusal of a CPU generator comes before anything is computed
    with pytest.raises(TypeError):
        swd.evaluate(Generator(NetConfig(image_size=32, base_feature_factor=1)))


def test_trainer_without_the_metric_is_unchanged():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, Trainer, TrainStep
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    plain, off = Trainer(step, pipeline, "OUT"), Trainer(step, pipeline, "OUT", swd=None)
    assert plain.swd is None and off.swd is None and off.written == []
    for e, miniter, subs in ((0, 8, 1), (1, 16, 4), (2, 24, 9)):          # libs/config.py:19-30, main.py:109-116
        assert off.schedule(e) == plain.schedule(e) == {"miniter": miniter, "subepochs": subs, "print_every": 16, "image_interval": 1024}
    assert off.picture_path(3, 4, 24) == os.path.join("OUT", "4", "05-024.png")          # 16 sub-passes, 100 batches
    marker = object()
    assert Trainer(step, pipeline, "OUT", swd=marker).swd is marker          # kept as given; nothing is evaluated before an epoch ends
    from locate_amd import run
    with pytest.raises(SystemExit):          # the flag exists; without the required arguments argparse still exits
        run.main(["--swd-images", "16"])
