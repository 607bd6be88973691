"""The sample metrics' shared Python layer on the MI355X (locate_amd/sampling.py, `CanonicalViews` in locate_amd/neighbours.py): the
batches of `sampling` + `batches` are the generator's own eval-mode forwards and leave u / v, their addresses and the mode as they
were, for one generator and for two; the canonical views of a store are encoded chunk by chunk into Pillow's bytes minus 128.
The network is the tiny fixture of tests/test_gpu_swd.py (32 x 32, base width 1)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import neighbours_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def build_tiny():
    from locate_amd import Generator, NetConfig
    z = load_golden("g8_tiny_e2e")
    G = Generator(NetConfig(image_size=32, base_feature_factor=1))
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    G.noise = T(z["G/noise"])
    G = G.to(DEV)
    G.batched_spectral_norm = True
    return G


def latents(G, n=20):
    return torch.randn(n, G.g_in, generator=torch.Generator().manual_seed(3)).to(DEV)


def snapshot(uv):
    return [p.detach().clone() for p in uv], [p.data_ptr() for p in uv]


def restored(uv, before):
    return all(torch.equal(p, q) for p, q in zip(uv, before[0])) and [p.data_ptr() for p in uv] == before[1]


def plain_forwards(gens, lat, chunk, uv, before):
    """the same slices through gen.eval() by hand, one after the other as the iterator runs them (a forward advances u / v, so a
    chunk sees what the chunks before it left); then u / v reset to `before` and the modes put back"""
    modes = [g.training for g in gens]
    with torch.no_grad():
        for g in gens:
            g.eval()
        out = [[g(lat[at:at + chunk]).clone() for g in gens] for at in range(0, lat.shape[0], chunk)]
        for g, mode in zip(gens, modes):
            g.train(mode)
        assert not restored(uv, before)          # the forwards did move u / v: the restore below is not vacuous
        for p, q in zip(uv, before[0]):
            p.data.copy_(q)
    return out


@pytest.mark.parametrize("training", [True, False])
def test_batches_are_the_generators_own_forwards_and_leave_no_trace(training):
    from locate_amd.sampling import _spectral_state, batches, sampling
    G = build_tiny().train(training)
    lat = latents(G)
    uv = _spectral_state(G)
    before = snapshot(uv)
    assert len(uv) > 0
    want = plain_forwards([G], lat, 8, uv, before)
    with sampling("Test", G):
        assert not G.training and not torch.is_grad_enabled()
        got = [x.clone() for x in batches(G, lat, 8)]
    assert [x.shape[0] for x in got] == [8, 8, 4] and all(tuple(x.shape[1:]) == (3, 32, 32) for x in got)
    assert all(torch.equal(x, w[0]) for x, w in zip(got, want))
    assert restored(uv, before) and G.training == training and torch.is_grad_enabled()


def test_two_generators_give_the_pairs_of_one_slice():
    import copy
    from locate_amd.sampling import _spectral_state, batches, sampling
    A = build_tiny().train()
    B = copy.deepcopy(A).eval()
    rng = torch.Generator(device=DEV)
    rng.manual_seed(5)
    with torch.no_grad():
        for p in B.parameters():
            if p.dim() > 1:          # another network: the pair is not twice the same picture
                p.add_(0.05 * p.abs().max() * torch.randn(p.shape, device=DEV, generator=rng))
    lat = latents(A)
    uv = _spectral_state(A) + _spectral_state(B)
    before = snapshot(uv)
    want = plain_forwards([A, B], lat, 8, uv, before)
    with sampling("Test", A, B):
        got = [[x.clone() for x in pair] for pair in batches([A, B], lat, 8)]
    assert [len(pair) for pair in got] == [2, 2, 2] and [pair[0].shape[0] for pair in got] == [8, 8, 4]
    assert all(torch.equal(x, w) for pair, wpair in zip(got, want) for x, w in zip(pair, wpair))
    assert not torch.equal(got[0][0], got[0][1])
    assert restored(uv, before) and A.training and not B.training


def test_canonical_views_are_encoded_chunk_by_chunk(monkeypatch):
    from locate_amd import BinnedModes, DeviceImageStore, ManifoldMetrics, neighbours
    from locate_amd.modes import initial_rows
    images = np.random.default_rng(15).integers(0, 256, size=(37, 10, 14, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)
    monkeypatch.setattr(neighbours, "BANK_CHUNK", 16)          # three chunks, the last one short
    sizes, encode_into = [], neighbours._encode_into

    def counted(x, codes, norms, flags):
        sizes.append(int(x.shape[0]))
        return encode_into(x, codes, norms, flags)
    monkeypatch.setattr(neighbours, "_encode_into", counted)
    want = NM.bank_codes(images, 8)
    codes, norms, flags = (t.cpu().numpy() for t in neighbours.CanonicalViews(8, store).encode(range(37)))
    assert sizes == [16, 16, 5] and codes.shape == (37, 192) and np.array_equal(codes, want)
    assert np.array_equal(norms, NM.norms(want)) and not flags.any()
    # the two metrics that hold a CanonicalViews: the real set is the model's rows at real_index
    del sizes[:]
    mm = ManifoldMetrics(S=8, k=3, images=37, seed=21, device=DEV).reference_from_store(store)
    assert sizes == [16, 16, 5] and sorted(mm.real_index) == list(range(37)) and mm.baseline is None
    assert np.array_equal(mm.real[0].cpu().numpy(), want[mm.real_index]) and np.array_equal(mm.real[1].cpu().numpy(), NM.norms(want[mm.real_index]))
    # with no Lloyd round the centres are rows of the real set: all of them, in the order of `initial_rows`
    del sizes[:]
    bm = BinnedModes(S=8, bins=37, images=37, samples=8, iterations=0, seed=21, device=DEV).reference_from_store(store)
    assert sizes == [16, 16, 5]          # the patched chunk size reaches modes.py
    at = initial_rows(np.zeros(37, np.int32), 37, 21 + 12).numpy()
    assert np.array_equal(bm.centres[0].cpu().numpy(), want[np.asarray(bm.real_index)[at]]) and bm.real_counts == [1] * 37
