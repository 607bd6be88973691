"""The sample metrics' shared Python layer (locate_amd/sampling.py, `CanonicalViews` in locate_amd/neighbours.py) without a GPU: the
import, the bookkeeping of `sampling` on a CPU generator with no forward pass, what is refused, and the table of the fixed latents."""
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd.sampling, locate_amd._lib as L\n"
            "from locate_amd.sampling import FixedLatents, batches, plain_batches, sampling, _gpu, _ptr, _stream, _spectral_state\n"
            "from locate_amd.monitor import _spectral_state as moved\n"
            "assert moved is _spectral_state and _ptr(None) is None\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def tiny_generator():
    from locate_amd import Generator, NetConfig
    return Generator(NetConfig(image_size=32, base_feature_factor=1))


def snapshot(uv):
    return [p.detach().clone() for p in uv], [p.data_ptr() for p in uv]


def restored(uv, before):
    return all(torch.equal(p, q) for p, q in zip(uv, before[0])) and [p.data_ptr() for p in uv] == before[1]


def test_the_context_restores_u_v_modes_and_grad_mode():
    from locate_amd.sampling import _spectral_state, sampling
    a, b = tiny_generator().train(), tiny_generator().eval()
    uv = _spectral_state(a) + _spectral_state(b)
    assert len(_spectral_state(a)) > 0 and len(uv) == 2 * len(_spectral_state(a))
    before = snapshot(uv)
    assert torch.is_grad_enabled()
    with sampling("Owner", a, b, device_type="cpu"):
        assert not torch.is_grad_enabled() and not a.training and not b.training
        for p in uv:
            p.data.add_(1.0)          # what a forward's power iteration does: in place
        assert not restored(uv, before)
    assert torch.is_grad_enabled() and a.training and not b.training
    assert restored(uv, before)


def test_the_context_restores_when_the_body_raises():
    from locate_amd.sampling import _spectral_state, sampling
    a, b = tiny_generator().eval(), tiny_generator().train()
    uv = _spectral_state(a) + _spectral_state(b)
    before = snapshot(uv)

    class Mid(Exception):
        pass

    with pytest.raises(Mid):
        with sampling("Owner", a, b, device_type="cpu"):
            for p in uv:
                p.data.add_(1.0)
            raise Mid()
    assert torch.is_grad_enabled() and not a.training and b.training
    assert restored(uv, before)


def metrics():
    from locate_amd import BinnedModes, ManifoldMetrics, MultiScaleSSIM, NearestNeighbours, RadialSpectrum, SlicedWasserstein
    return (SlicedWasserstein, RadialSpectrum, NearestNeighbours, ManifoldMetrics, MultiScaleSSIM, BinnedModes)


def test_a_generator_on_the_cpu_is_refused_by_name():
    from locate_amd.sampling import _spectral_state
    gen = tiny_generator()
    before = snapshot(_spectral_state(gen))
    for cls in metrics():
        metric = cls(S=32)
        with pytest.raises(TypeError, match="^%s computes on the GPU only; the generator is on cpu$" % cls.__name__):
            with metric._sampling(gen):
                raise AssertionError("entered")
        with pytest.raises(TypeError, match="^%s computes on the GPU only; its device is cpu$" % cls.__name__):
            cls(S=32, device="cpu").latents(8)
    assert gen.training and restored(_spectral_state(gen), before) and torch.is_grad_enabled()


def test_the_latent_table():
    """seed offset and count per class: the draws are torch.randn(count, g_in, generator=<seeded seed + offset>) on the device"""
    from locate_amd.sampling import FixedLatents
    sizes = types.SimpleNamespace(images=5, pairs=7, samples=11)
    table = [(cls.__name__, cls.latent_seed, cls._latent_count(sizes)) for cls in metrics()]
    assert table == [("SlicedWasserstein", 3, 5), ("RadialSpectrum", 3, 5), ("NearestNeighbours", 6, 5), ("ManifoldMetrics", 8, 5),
                     ("MultiScaleSSIM", 9, 14), ("BinnedModes", 11, 11)]
    assert all(issubclass(cls, FixedLatents) and cls.latents is FixedLatents.latents and cls._need_gpu is FixedLatents._need_gpu for cls in metrics())


def test_canonical_views_without_a_store():
    from locate_amd.neighbours import CanonicalViews
    views = CanonicalViews(8)
    assert (views.S, views.store) == (8, None)
    for call in (views.views, views.encode):
        with pytest.raises(RuntimeError, match="^reference_from_store\\(\\) first$"):
            call(range(3))
    with pytest.raises(ValueError, match="image size 6: the input pipeline writes 16-byte groups"):
        CanonicalViews(6)
