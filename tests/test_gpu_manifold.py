"""Precision / recall / density / coverage on the MI355X: the within kernels of csrc/neighbours.hip at the C ABI and through
locate_amd/manifold.py against the numpy model (tests/helpers/manifold_model.py) - integers, so everything is compared with == -
and the behaviour around a running training: an evaluation between two iterations, eager or replayed, leaves the trajectory where
it would be.  Outputs and workspace hold 0x55 garbage before every ABI-level call: nothing may depend on their contents."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import manifold_model as M  # noqa: E402
import neighbours_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
INT64_MAX = 2 ** 63 - 1


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def triple(codes, flags=None):
    """a (codes, norms, flags) device triple of raw int8 rows"""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    flags = np.zeros(codes.shape[0], np.int32) if flags is None else np.asarray(flags, np.int32)
    return dev(codes, np.int8), dev(NM.norms(codes), np.int64), dev(flags, np.int32)


def garbage(n, dtype):
    return torch.full((max(int(n), 1) * torch.empty(0, dtype=dtype).element_size(),), 0x55, dtype=torch.uint8, device=DEV).view(dtype)


def abi_within(q, r, radius2, qflags=None, rflags=None, skip=None, covered=True):
    """locate_nn_within on raw int8 rows; rflags None: the null pointer.  Returns (hits, covered or None) as numpy."""
    from locate_amd._lib import check, lib
    L = lib()
    Q, N = q.shape[0], r.shape[0]
    tq, tr = triple(q, qflags), triple(r, rflags)
    rad, sk = dev(radius2, np.int64), dev(skip, np.int32)
    hits = garbage(Q, torch.int32)
    cov = garbage(N, torch.int32) if covered else None
    bytes_ = L.locate_nn_within_workspace_bytes(Q, N, 1 if covered else 0)
    assert bytes_ == 4 * (Q * -(-N // 128) + (N * -(-Q // 64) if covered else 0))
    ws = garbage(bytes_ // 4, torch.int32)
    check(L.locate_nn_within(p(tq[0]), p(tq[1]), p(tq[2]), Q, p(tr[0]), p(tr[1]), None if rflags is None else p(tr[2]), N, q.shape[1], p(rad), p(sk),
                             p(hits), p(cov), p(ws), stream()), "locate_nn_within")
    return hits.cpu().numpy(), None if cov is None else cov.cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0]) and (got[1] is None or np.array_equal(got[1], want[1]))


# ---- 1. the pattern: about half of the pairs count, the median pair of every column sits on the <= boundary ----------------------------
# (1, 1, 64): one pair; (64, 128, 128): one whole tile, one whole stage; (65, 129, 192): one row over in both directions, a half-filled
# last stage; (130, 257, 448): three tiles each way - more than one word in every sum - and 3.5 stages
@pytest.mark.parametrize("Q,N,row", [(1, 1, 64), (64, 128, 128), (65, 129, 192), (130, 257, 448)])
def test_pattern_against_the_model(Q, N, row):
    rng = np.random.default_rng(Q + N + row)
    q, r = rng.integers(-128, 128, size=(Q, row), dtype=np.int8), rng.integers(-128, 128, size=(N, row), dtype=np.int8)
    d2 = M.distances(q, r)
    radius2 = np.sort(d2, axis=0)[(Q - 1) // 2]          # a median that is an element of its column: that pair has d2 == radius2
    want = M.within(d2, radius2)
    assert (d2 == radius2[None, :]).any(0).all() and want[1].min() >= 1 and (Q == 1 or 0 < want[0].sum() < Q * N)
    got = abi_within(q, r, radius2)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert same(got, want), (int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum()))


# ---- 2. the boundary --------------------------------------------------------------------------------------------------------------
def test_boundary():
    rng = np.random.default_rng(21)
    q = rng.integers(-128, 128, size=(1, 192), dtype=np.int8)
    r = rng.integers(-128, 128, size=(1, 192), dtype=np.int8)
    d2 = int(M.distances(q, r)[0, 0])
    assert d2 > 0
    for radius, want in ((d2, 1), (d2 - 1, 0), (d2 + 1, 1), (0, 0), (-1, 0), (INT64_MAX, 1), (-INT64_MAX - 1, 0)):
        hits, cov = abi_within(q, r, [radius])
        assert hits.tolist() == [want] and cov.tolist() == [want], radius
    # a duplicate row: distance 0 counts at radius 0 and not at -1
    both = np.concatenate([r, q])
    hits, cov = abi_within(q, both, [0, 0])
    assert hits.tolist() == [1] and cov.tolist() == [0, 1]
    hits, cov = abi_within(q, both, [-1, -1])
    assert hits.tolist() == [0] and cov.tolist() == [0, 0]
    # the largest radius counts every pair
    q, r = rng.integers(-128, 128, size=(5, 64), dtype=np.int8), rng.integers(-128, 128, size=(7, 64), dtype=np.int8)
    hits, cov = abi_within(q, r, [INT64_MAX] * 7)
    assert hits.tolist() == [7] * 5 and cov.tolist() == [5] * 7


# ---- 3. masking: the pad rows of a tile are all-zero rows too, at distance 0 from an all-zero query ----------------------------------
def test_pad_rows_of_the_tile_are_not_counted():
    q, r = np.zeros((65, 64), np.int8), np.zeros((129, 64), np.int8)
    for radius in (INT64_MAX, 0):
        hits, cov = abi_within(q, r, [radius] * 129)
        assert (hits == 129).all() and hits.shape == (65,) and (cov == 65).all() and cov.shape == (129,)


# ---- 4. flags and skip --------------------------------------------------------------------------------------------------------------
def test_flags_and_skip():
    rng = np.random.default_rng(22)
    q = rng.integers(-128, 128, size=(70, 192), dtype=np.int8)
    r = rng.integers(-128, 128, size=(300, 192), dtype=np.int8)
    r[:70] = q          # the queries are part of the references
    d2 = M.distances(q, r)
    radius2 = np.sort(d2, axis=0)[40]
    radius2[[5, 131]] = -1
    qflags, rflags = np.zeros(70, np.int32), np.zeros(300, np.int32)
    qflags[[3, 64, 69]] = (1, 5, 192)
    rflags[[0, 8, 127, 128, 299]] = 1
    skip = np.arange(70)
    skip[10] = -1          # none: its own row counts, distance 0
    skip[11] = 250
    want = M.within(d2, radius2, qflags, rflags, skip)
    got = abi_within(q, r, radius2, qflags, rflags, skip)
    assert same(got, want)
    assert (got[0][[3, 64, 69]] == 0).all() and (got[1][[0, 8, 127, 128, 299, 5, 131]] == 0).all()
    # a flagged query adds to no reference's count; skip removes exactly that pair
    plain = abi_within(q, r, radius2)
    assert same(plain, M.within(d2, radius2))
    only_skip = abi_within(q, r, radius2, skip=skip)
    mine = np.array([j for j in range(70) if j not in (5, 10, 11)])          # rows whose own pair (d2 = 0, a ball) was removed
    assert np.array_equal(plain[0][mine] - only_skip[0][mine], np.ones(mine.size, np.int32)) and plain[0][10] == only_skip[0][10]
    assert np.array_equal(plain[1][mine] - only_skip[1][mine], np.ones(mine.size, np.int32))
    # no flags on the reference side: the null pointer; no `covered`: the null pointer, and no workspace for it
    assert same(abi_within(q, r, radius2, qflags, None, skip), M.within(d2, radius2, qflags, None, skip))
    hits, cov = abi_within(q, r, radius2, qflags, rflags, skip, covered=False)
    assert cov is None and np.array_equal(hits, want[0])


# ---- 5. rows past the int32 accumulator ---------------------------------------------------------------------------------------------
def test_segments_rows_past_the_int32_accumulator():
    """rows of 65600 bytes: one whole segment and one stage of a second (the upper half of that stage beyond the row).  q0 . r0 =
    128^2 65600 > 2^30: the first segment's int32 sum is 2^30 and has left the accumulator when the row ends - the accumulator
    alone is not the dot product - and 2 q0 . r0 > 2^31: the distance in int32 arithmetic would be wrong"""
    row = 65600
    rng = np.random.default_rng(23)
    q = np.stack([np.full(row, -128, np.int8), np.full(row, 127, np.int8)])
    r = np.stack([np.full(row, -128, np.int8), np.full(row, 127, np.int8), rng.integers(-128, 128, size=row, dtype=np.int8)])
    assert row > 65536 and row % 64 == 0 and 128 * 128 * row > 2 ** 30
    d2 = M.distances(q, r)
    assert d2[0, 0] == 0 and d2[0, 1] == 255 * 255 * row
    for radius2 in ([0, 0, 0], d2[0], d2[1], d2.max(0), d2.min(0), d2.min(0) - 1, [d2[0, 1] - 1, d2[0, 1], d2[1, 2]]):
        assert same(abi_within(q, r, radius2), M.within(d2, radius2)), radius2


# ---- 6. chunks, determinism, and the search after the refactoring ---------------------------------------------------------------------
def test_chunks_and_determinism():
    from locate_amd import within
    rng = np.random.default_rng(24)
    q, r = rng.integers(-128, 128, size=(130, 192), dtype=np.int8), rng.integers(-128, 128, size=(257, 192), dtype=np.int8)
    d2 = M.distances(q, r)
    radius2 = np.sort(d2, axis=0)[64]
    qflags = np.zeros(130, np.int32)
    qflags[77] = 1
    skip = rng.integers(-1, 257, size=130)
    want = M.within(d2, radius2, qflags, None, skip)
    tq, tr, rad, sk = triple(q, qflags), triple(r), dev(radius2, np.int64), dev(skip, np.int32)
    whole = within(tq, (tr[0], tr[1], None), rad, skip=sk)
    assert whole[0].dtype == torch.int32 and whole[1].dtype == torch.int32 and tuple(whole[0].shape) == (130,) and tuple(whole[1].shape) == (257,)
    assert same(tuple(t.cpu().numpy() for t in whole), want)
    for chunk in (64, 100, 1):
        parts = within(tq, (tr[0], tr[1], None), rad, skip=sk, query_chunk=chunk)
        assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), chunk
    again = within(tq, (tr[0], tr[1], None), rad, skip=sk)
    assert torch.equal(again[0], whole[0]) and torch.equal(again[1], whole[1])
    hits, none = within(tq, tr, rad, skip=sk, covered=False, query_chunk=64)
    assert none is None and torch.equal(hits, whole[0])
    for bad in (dict(query_chunk=0), dict(skip=sk[:5])):
        with pytest.raises(ValueError):
            within(tq, tr, rad, **bad)
    with pytest.raises(ValueError):
        within(tq, tr, rad[:5])
    with pytest.raises(ValueError):
        within(tq, tr, rad.to(torch.int32))


def test_the_search_still_equals_its_model():
    from locate_amd import nearest
    rng = np.random.default_rng(25)
    q, r = rng.integers(-128, 128, size=(130, 448), dtype=np.int8), rng.integers(-128, 128, size=(257, 448), dtype=np.int8)
    r[200] = r[3]
    for k in (1, 8):
        d2, index = nearest(triple(q), triple(r), k=k)
        want = NM.topk(M.distances(q, r), k)
        assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(index.cpu().numpy(), want[1])


# ---- 7. what the entry point refuses ---------------------------------------------------------------------------------------------------
def test_what_the_entry_point_refuses():
    from locate_amd._lib import LocateError, check, lib
    L = lib()
    q, r = triple(np.zeros((2, 64), np.int8)), triple(np.zeros((3, 64), np.int8))
    rad = torch.zeros(4, dtype=torch.int64, device=DEV)
    hits, cov = torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(64, dtype=torch.int32, device=DEV)
    assert L.locate_nn_within_workspace_bytes(2, 3, 1) == 4 * (2 + 3) and L.locate_nn_within_workspace_bytes(65, 129, 0) == 4 * 65 * 2
    assert L.locate_nn_within_workspace_bytes(65, 129, 1) == 4 * (65 * 2 + 129 * 2) and L.locate_nn_within_workspace_bytes(0, 3, 1) == 0

    def off(t, n):
        return ctypes.c_void_p(t.data_ptr() + n)
    args = lambda **kw: [kw.get("qc", p(q[0])), kw.get("qn", p(q[1])), kw.get("qf", p(q[2])), kw.get("Q", 2), kw.get("rc", p(r[0])), p(r[1]), None,  # noqa: E731
                         kw.get("N", 3), kw.get("row", 64), kw.get("rad", p(rad)), None, kw.get("hits", p(hits)), kw.get("cov", p(cov)),
                         kw.get("ws", p(ws)), stream()]
    assert L.locate_nn_within(*args()) == 0 and L.locate_nn_within(*args(cov=None)) == 0
    assert hits[:2].tolist() == [3, 3] and cov[:3].tolist() == [2, 2, 2]
    for bad in (dict(Q=0), dict(N=0), dict(N=-1), dict(row=96), dict(row=0), dict(row=262144 + 64), dict(qc=None), dict(qn=None), dict(qf=None),
                dict(rc=None), dict(rad=None), dict(hits=None), dict(ws=None), dict(qc=off(q[0], 8)), dict(rc=off(r[0], 8)), dict(qn=off(q[1], 4)),
                dict(rad=off(rad, 4)), dict(qf=off(q[2], 2)), dict(hits=off(hits, 2)), dict(cov=off(cov, 2)), dict(ws=off(ws, 2))):
        status = L.locate_nn_within(*args(**bad))
        assert status != 0 and b"locate_nn_within" in L.locate_last_error(), bad
        with pytest.raises(LocateError):
            check(status, "locate_nn_within")


# ---- 8. end to end: radii, the record, the properties --------------------------------------------------------------------------------
def test_kth_radius_against_the_model():
    from locate_amd import encode_images, kth_radius
    rng = np.random.default_rng(26)
    x = rng.uniform(-1, 1, size=(6, 3, 8, 8)).astype(np.float32)
    x[2, 0, 0, 0] = np.nan
    t = encode_images(torch.from_numpy(x).to(DEV))
    model = NM.encode(x)
    for k in (1, 3, 4, 5, 8):          # four unflagged others: k = 5 and 8 give "no ball"
        got = kth_radius(t, k)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), M.kth_radius(model, k)), k
    assert kth_radius(t, 4).cpu()[2] == -1 and (kth_radius(t, 4).cpu()[[0, 1, 3, 4, 5]] > 0).all() and (kth_radius(t, 5).cpu() == -1).all()


STORE16 = np.random.default_rng(27).integers(0, 256, size=(16, 10, 14, 3), dtype=np.uint8)


def test_between_against_the_models_record():
    from locate_amd import DeviceImageStore, ManifoldMetrics
    store = DeviceImageStore(STORE16, DEV)
    codes = NM.bank_codes(STORE16, 8)
    rows = lambda index: M.triple(codes[index])          # noqa: E731
    rng = np.random.default_rng(28)
    fake = rng.uniform(-1, 1, size=(11, 3, 8, 8)).astype(np.float32)
    fake[:4] = (codes[:4, :192].astype(np.float32).reshape(4, 3, 8, 8) + 128) / 127.5 - 1 + rng.uniform(-0.02, 0.02, size=(4, 3, 8, 8)).astype(np.float32)
    fake[7, 1, 2, 3] = np.inf
    # with a baseline: 8 of the 16 images are the real set, the other 8 the second one
    mm = ManifoldMetrics(S=8, k=2, images=8, seed=31, device=DEV).reference_from_store(store)
    order = torch.randperm(16, generator=torch.Generator().manual_seed(31 + 7)).tolist()
    assert mm.real_index == order[:8] and np.array_equal(mm.real[0].cpu().numpy(), codes[order[:8]])
    assert np.array_equal(mm.real_radius.cpu().numpy(), M.kth_radius(rows(order[:8]), 2))
    baseline = M.baseline(rows(order[8:]), rows(order[:8]), 2)
    assert mm.baseline == baseline and sorted(baseline) == ["counts", "coverage", "density", "precision", "recall"]
    value = mm.between(torch.from_numpy(fake).to(DEV))
    assert value == M.between(NM.encode(fake), rows(order[:8]), 2, baseline)
    assert value["nonfinite"] == 1 and value["images"] == 11 and value["real_images"] == 8 and value["counts"]["precise"] <= 10
    assert sorted(value) == ["baseline", "counts", "coverage", "density", "images", "k", "nonfinite", "precision", "real_images", "recall"]
    assert json.loads(json.dumps(value)) == value
    # a given real set instead of the cached one
    other = rng.uniform(-1, 1, size=(9, 3, 8, 8)).astype(np.float32)
    assert mm.between(torch.from_numpy(fake).to(DEV), real=torch.from_numpy(other).to(DEV)) == M.record(fake, other, 2, baseline)
    # without a baseline: the store holds fewer than 2 x images
    small = ManifoldMetrics(S=8, k=3, images=9, seed=31, device=DEV).reference_from_store(store)
    assert small.baseline is None and small.real_index == order[:9]
    assert small.between(torch.from_numpy(fake).to(DEV)) == M.between(NM.encode(fake), rows(order[:9]), 3, None)
    # more images asked for than the store holds: all of it
    assert len(ManifoldMetrics(S=8, k=3, images=64, seed=31, device=DEV).reference_from_store(store).real_index) == 16


def cluster_images(centres, per, seed, S=8):
    """fp32 images: `per` noise fields, the same around every centre value - the modes are translates of each other"""
    noise = np.random.default_rng(seed).integers(-3, 4, size=(per, 3, S, S))
    codes = np.concatenate([c + noise for c in centres])          # byte codes, away from the clamp
    return ((codes + 128) / 127.5 - 1).astype(np.float32)          # the encoder maps these back exactly


def test_the_properties_hold_on_the_device():
    from locate_amd import ManifoldMetrics
    mm = ManifoldMetrics(S=8, k=3, images=64, device=DEV)
    real = cluster_images([-90, -30, 30, 90], 16, seed=4)
    fake = cluster_images([-90, -30, 30, 90], 16, seed=5)
    assert np.array_equal(NM.encode(real)[0][:16, :192], (-90 + np.random.default_rng(4).integers(-3, 4, size=(16, 3, 8, 8))).reshape(16, 192))
    R, G = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    itself = mm.between(R, real=R)
    assert itself == M.record(real, real, 3) and itself["precision"] == itself["recall"] == itself["coverage"] == 1.0 and itself["density"] >= 1.0
    full, dropped = mm.between(G, real=R), mm.between(G[:32], real=R)
    assert full == M.record(fake, real, 3) and dropped == M.record(fake[:32], real, 3)
    assert full["precision"] == dropped["precision"] > 0.0
    assert dropped["recall"] < full["recall"] and dropped["coverage"] < full["coverage"] and dropped["coverage"] <= 0.5
    apart = mm.between(torch.from_numpy(cluster_images([-100], 12, seed=2)).to(DEV), real=torch.from_numpy(cluster_images([100], 12, seed=3)).to(DEV))
    assert (apart["precision"], apart["recall"], apart["density"], apart["coverage"]) == (0.0, 0.0, 0.0, 0.0)


# ---- 9. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) ---------------------
def build_tiny():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1)
    inputs = tuple(T(z["step1/" + k]).to(DEV) for k in ("latent", "real", "aug"))
    return G, D, step, inputs


def training_state(G, D, step):
    """every parameter (u and v included) and every Nadam state tensor, by name"""
    torch.cuda.synchronize()
    state = {"G/" + k: v.detach().clone() for k, v in G.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in D.state_dict().items()})
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        for name, q in net.named_parameters():
            for k, v in opt.state.get(q, {}).items():
                if torch.is_tensor(v):
                    state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
    return state


STORE = np.random.default_rng(16).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
_CACHE = {}


def small_metric():
    """the metric over STORE at 32 x 32 (built once: nothing below changes it)"""
    if "mm" not in _CACHE:
        from locate_amd import DeviceImageStore, ManifoldMetrics
        _CACHE["mm"] = ManifoldMetrics(S=32, k=3, images=16, seed=4, chunk=8, device=DEV).reference_from_store(DeviceImageStore(STORE, DEV))
    return _CACHE["mm"]


def test_evaluate_is_the_model_applied_to_the_generated_images():
    G, _, _, _ = build_tiny()
    mm = small_metric()
    assert mm.baseline is not None
    first = mm.evaluate(G)
    assert G.training and tuple(mm.latents(G.g_in).shape) == (16, G.g_in)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(4 + 8)
    assert torch.equal(mm.latents(G.g_in), torch.randn(16, G.g_in, device=DEV, generator=rng))
    images = mm._generate(G, mm.latents(G.g_in))
    real = tuple(t.cpu().numpy() for t in mm.real)
    assert np.array_equal(real[0], NM.bank_codes(STORE, 32)[mm.real_index])
    assert first == M.between(NM.encode(images.cpu().numpy()), real, 3, mm.baseline)
    assert mm.evaluate(G) == first and first["images"] == 16 and first["nonfinite"] == 0
    G.eval()
    own = torch.randn(5, G.g_in, generator=torch.Generator().manual_seed(1)).to(DEV)
    value = mm.evaluate(G, latents=own)
    assert not G.training and value["images"] == 5


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_an_evaluation_between_iterations_has_no_side_effect(launch):
    from locate_amd.graph import GraphedTrainStep

    def run(measure):
        G, D, step, (lat, real, aug) = build_tiny()
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
        values, losses = [], []
        for i in range(6):
            out = runner.replay() if runner is not None else step(lat, real, aug)
            losses.append((out["d_error"].detach().clone(), out["g_error"].detach().clone()))
            if measure and i == 2:
                mm = small_metric()
                values = [mm.evaluate(G), mm.evaluate(G)]
                assert G.training
        return training_state(G, D, step), losses, values

    plain, plain_losses, _ = run(False)
    watched, losses, values = run(True)
    assert sorted(plain) == sorted(watched)
    bad = [k for k in plain if not torch.equal(plain[k], watched[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain_losses, losses))
    assert values[0] == values[1] and values[0]["images"] == 16


# ---- 10. the trainer ---------------------------------------------------------------------------------------------------------------------
def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, files in os.walk(str(root)) for f in files)


def test_trainer_records_the_metrics(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, ManifoldMetrics, Trainer
    store = DeviceImageStore(STORE, DEV)

    def trainer(out, with_manifold):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        mm = ManifoldMetrics(S=32, k=2, images=8, seed=3, chunk=8, device=DEV).reference_from_store(store) if with_manifold else None
        t = Trainer(step, pipeline, str(out), epochs=1, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                    image_interval_function=lambda batch: 2, manifold=mm)
        return t, G, D, step, mm

    t, G1, D1, step1, mm = trainer(tmp_path / "with", True)
    assert t.run() == 4
    path = os.path.join(str(tmp_path / "with"), "error", "manifold.json")
    assert path in t.written and os.path.exists(path) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    direct = mm.evaluate(G1)          # the weights are the saved ones
    assert len(rec) == 1 and rec[0] == dict(direct, epoch=1, iterations=4) and rec[0]["baseline"] is not None and "average" not in rec[0]
    assert (rec[0]["images"], rec[0]["real_images"], rec[0]["k"]) == (8, 8, 2)

    plain, G2, D2, step2, _ = trainer(tmp_path / "without", False)
    assert plain.run() == 4
    extra = [os.path.join("error", "manifold.json")]
    assert listing(tmp_path / "without") == [f for f in listing(tmp_path / "with") if f not in extra]
    assert sorted(set(listing(tmp_path / "with")) - set(listing(tmp_path / "without"))) == extra
    strip = lambda files, root: [os.path.relpath(f, str(root)) for f in files if "manifold" not in f]      # noqa: E731
    assert strip(plain.written, tmp_path / "without") == strip(t.written, tmp_path / "with")
    a, b = training_state(G1, D1, step1), training_state(G2, D2, step2)
    assert sorted(a) == sorted(b) and not [k for k in a if not torch.equal(a[k], b[k])]


def test_trainer_records_the_average_too(tmp_path):
    """with an average: its record, without the baseline, goes under the key "average" """
    from locate_amd import AveragedGenerator, DeviceImageStore, InputPipeline, ManifoldMetrics, Trainer
    store = DeviceImageStore(STORE, DEV)
    G3, _, step, _ = build_tiny()
    mm3 = ManifoldMetrics(S=32, k=2, images=8, seed=3, chunk=8, device=DEV).reference_from_store(store)
    t3 = Trainer(step, InputPipeline(store, 32, 8, seed=11), str(tmp_path / "average"), epochs=1, images=13, seed=3, miniter_function=lambda e: 1,
                 subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, manifold=mm3,
                 average=AveragedGenerator(G3, half_life_images=64, batch=8))
    assert t3.run() == 4
    rec = json.load(open(os.path.join(str(tmp_path / "average"), "error", "manifold.json")))
    ema = mm3.evaluate(t3.average.generator)
    assert len(rec) == 1 and rec[0]["average"] == {k: v for k, v in ema.items() if k != "baseline"}
    assert {k: v for k, v in rec[0].items() if k != "average"} == dict(mm3.evaluate(G3), epoch=1, iterations=4)


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, STORE)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--manifold", "16", "--manifold-k", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    rec = json.load(open(os.path.join(out, "error", "manifold.json")))
    assert len(rec) == 1 and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["images"], rec[0]["real_images"], rec[0]["k"]) == (1, 4, 16, 16, 2)
    assert rec[0]["baseline"] is not None and rec[0]["baseline"]["counts"]["hit_sum"] == int(rec[0]["baseline"]["density"] * 2 * 16)
    assert rec[0]["precision"] == rec[0]["counts"]["precise"] / 16 and rec[0]["coverage"] == rec[0]["counts"]["covered"] / 16
    assert not [f for f in listing(out) if "neighbours" in f]
