"""The averaged generator's host side (locate_amd/average.py, the hooks in locate_amd/run.py) without a GPU: what it refuses, its
saved state, and a run loop that is unchanged without it."""
import io
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def tiny_generator():
    from locate_amd import Generator, NetConfig
    return Generator(NetConfig(image_size=32, base_feature_factor=1))


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.average, locate_amd._lib as L\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'liblocate_hip' not in maps, 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_a_cpu_generator_is_rejected():
    from locate_amd import AveragedGenerator
    G = tiny_generator()
    state = torch.random.get_rng_state()
    with pytest.raises(TypeError):
        AveragedGenerator(G, beta=0.999)
    with pytest.raises(ValueError):          # the arguments are checked first
        AveragedGenerator(G)
    with pytest.raises(ValueError):
        AveragedGenerator(G, beta=0.9, half_life_images=10, batch=2)
    assert torch.equal(torch.random.get_rng_state(), state)


def host_side(gen, updates, one_minus_beta):
    """an AveragedGenerator's saved-state half around a CPU generator: the constructor itself refuses one (there is no CPU path
    for update()), while state_dict() / load_state_dict() only copy tensors"""
    from locate_amd import AveragedGenerator
    avg = object.__new__(AveragedGenerator)
    avg.generator, avg.updates, avg.one_minus_beta = gen, updates, one_minus_beta
    return avg


def test_state_dict_round_trip():
    from locate_amd import Generator, NetConfig
    a, b = host_side(tiny_generator(), 7, 0.25), host_side(tiny_generator(), 0, 0.25)
    assert not torch.equal(a.generator.noise, b.generator.noise)
    state = a.state_dict()
    assert state["updates"] == 7 and state["one_minus_beta"] == 0.25 and torch.equal(state["noise"], a.generator.noise)
    assert sorted(k for k in state if k not in ("noise", "updates", "one_minus_beta")) == sorted(a.generator.state_dict())
    assert all(v.device.type == "cpu" and v.data_ptr() != a.generator.state_dict()[k].data_ptr() for k, v in state.items() if torch.is_tensor(v) and k != "noise")
    assert sorted(a.generator_state_dict()) == sorted(a.generator.state_dict())
    blob = io.BytesIO()
    torch.save(state, blob)
    blob.seek(0)
    state = torch.load(blob, map_location="cpu", weights_only=True)          # tensors and numbers only
    before = {k: v.data_ptr() for k, v in b.generator.state_dict(keep_vars=True).items()}
    versions = {k: v._version for k, v in b.generator.state_dict(keep_vars=True).items()}
    assert b.load_state_dict(state) is b and b.updates == 7
    for k, v in b.generator.state_dict(keep_vars=True).items():
        assert torch.equal(v, a.generator.state_dict()[k]), k
        assert v.data_ptr() == before[k] and v._version > versions[k], k          # in place, and the panel cache will notice
    assert torch.equal(b.generator.noise, a.generator.noise)
    fresh = tiny_generator()
    fresh.load_state_dict(a.generator_state_dict(), strict=True)
    # refusals leave the target as it was
    other_beta = host_side(tiny_generator(), 0, 0.5)
    keep = {k: v.clone() for k, v in other_beta.generator.state_dict().items()}
    with pytest.raises(ValueError):
        other_beta.load_state_dict(state)
    other_shape = host_side(Generator(NetConfig(image_size=32, base_feature_factor=2)), 0, 0.25)
    with pytest.raises(ValueError):
        other_shape.load_state_dict(state)
    missing = dict(state)
    missing.pop(sorted(a.generator.state_dict())[0])
    with pytest.raises(ValueError):
        host_side(tiny_generator(), 0, 0.25).load_state_dict(missing)
    assert other_beta.updates == 0 and all(torch.equal(v, keep[k]) for k, v in other_beta.generator.state_dict().items())


TODAYS_STATE_KEYS = ["epoch", "fixed_noise", "history", "i", "iterations", "latent_state", "pipeline", "sub"]


def test_trainer_without_an_average_is_unchanged(tmp_path, monkeypatch, capsys):
    from locate_amd import Discriminator, Nadam, NetConfig, Trainer, TrainStep
    from locate_amd import run
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = tiny_generator(), Discriminator(cfg)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr), Nadam(D.parameters(), lr=cfg.dlr), minibatches=8)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100, state_dict=lambda: {"epoch": 0, "pos": 0})
    plain, off = Trainer(step, pipeline, "OUT"), Trainer(step, pipeline, "OUT", average=None)
    assert plain.average is None and off.average is None and off.written == []
    for e, miniter, subs in ((0, 8, 1), (1, 16, 4), (2, 24, 9)):
        assert off.schedule(e) == plain.schedule(e) == {"miniter": miniter, "subepochs": subs, "print_every": 16, "image_interval": 1024}
    assert off.picture_path(3, 4, 24) == os.path.join("OUT", "4", "05-024.png")
    marker = object()
    assert Trainer(step, pipeline, "OUT", average=marker).average is marker          # kept as given; nothing runs before an iteration

    # what save_state() writes, with the device-side pieces replaced by host stand-ins
    monkeypatch.setattr(run, "save_checkpoint", lambda out, *nets: [os.path.join(out, "netG.torch")])
    stub = types.SimpleNamespace(state_dict=lambda: {"w": torch.ones(2), "noise": torch.zeros(1), "updates": 3, "one_minus_beta": 0.5},
                                 generator_state_dict=lambda: {"w": torch.ones(2)})
    for tag, average in (("off", None), ("on", stub)):
        out = tmp_path / tag
        out.mkdir()
        t = Trainer(step, pipeline, str(out), average=average)
        t._sampler = types.SimpleNamespace(fixed_noise=torch.zeros(4, G.g_in))
        files = [os.path.relpath(f, str(out)) for f in t.save_state()]
        state = torch.load(str(out / "trainer.torch"), map_location="cpu", weights_only=True)
        if average is None:
            assert files == ["netG.torch", "trainer.torch"] and sorted(state) == TODAYS_STATE_KEYS
            assert sorted(os.listdir(str(out))) == ["trainer.torch"]
        else:
            assert files == ["netG.torch", "netG_ema.torch", "trainer.torch"] and sorted(state) == sorted(TODAYS_STATE_KEYS + ["average"])
            assert state["average"]["updates"] == 3 and sorted(os.listdir(str(out))) == ["netG_ema.torch", "trainer.torch"]
            assert sorted(torch.load(str(out / "netG_ema.torch"), weights_only=True)) == ["w"]

    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--ema-half-life IMAGES" in capsys.readouterr().out
