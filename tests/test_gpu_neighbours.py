"""Exact nearest neighbours on the MI355X: the encoder and the search of csrc/neighbours.hip against the numpy model
(tests/helpers/neighbours_model.py) - integers, so everything is compared with == - the bank built from a store, and the behaviour
around a running training: an evaluation between two iterations, eager or replayed, leaves the trajectory where it would be."""
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
import neighbours_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def triple(codes, flags=None):
    """a (codes, norms, flags) device triple of raw int8 rows"""
    codes = np.ascontiguousarray(codes, dtype=np.int8)
    flags = np.zeros(codes.shape[0], np.int32) if flags is None else np.asarray(flags, np.int32)
    return (torch.from_numpy(codes).to(DEV), torch.from_numpy(M.norms(codes)).to(DEV), torch.from_numpy(flags).to(DEV))


def search(q, r, k, qflags=None, rflags=None, skip=None):
    from locate_amd import nearest
    sk = None if skip is None else torch.from_numpy(np.asarray(skip, np.int32)).to(DEV)
    d2, index = nearest(triple(q, qflags), triple(r, rflags), k=k, skip=sk)
    assert d2.dtype == torch.int64 and index.dtype == torch.int32 and tuple(d2.shape) == tuple(index.shape) == (q.shape[0], k)
    return d2.cpu().numpy(), index.cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. the encoder ----------------------------------------------------------------------------------------------------------------
def encoder_input(S, seed):
    """random values in [-1.5, 1.5]; exactly -1, 1, -0.0, a denormal and the ends of the clamp; every half-way point
    (n + 0.5) / 127.5 - 1; NaN, +Inf and -Inf planted in two images"""
    rng = np.random.default_rng(seed)
    E = 3 * S * S
    n = np.arange(255)
    special = np.concatenate([np.array([-1.0, 1.0, -0.0, 1e-40, -1.5, 1.5, 0.0, np.nextafter(np.float32(-1), np.float32(0))], dtype=np.float32),
                              ((n + 0.5) / 127.5 - 1).astype(np.float32)])
    count = -(-special.size // E) + 3
    x = rng.uniform(-1.5, 1.5, size=(count, E)).astype(np.float32)
    x.reshape(-1)[E:E + special.size] = special          # image 0 stays random
    x[0, 5], x[0, E - 1], x[count - 1, 0], x[count - 1, 7] = np.nan, np.inf, -np.inf, np.nan
    return x.reshape(count, 3, S, S)


def abi_encode(xd, n, S):
    from locate_amd._lib import check, lib
    L = lib()
    rb = L.locate_nn_row_bytes(S)
    codes = torch.full((n, rb), 0x55, dtype=torch.int8, device=DEV)
    norms = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    check(L.locate_nn_encode(p(xd), n, S, p(codes), p(norms), p(flags), stream()), "locate_nn_encode")
    return codes.cpu().numpy(), norms.cpu().numpy(), flags.cpu().numpy()


# S = 4: 48 bytes padded to 64; S = 8: 192 bytes, no pad; S = 5: 75 elements, no multiple of 4 - the scalar loads
@pytest.mark.parametrize("S", [4, 8, 5])
def test_encoder_against_the_model(S):
    from locate_amd._lib import lib
    x = encoder_input(S, S)
    n = x.shape[0]
    want = M.encode(x)
    assert lib().locate_nn_row_bytes(S) == M.row_bytes(S) == want[0].shape[1]
    assert want[2][0] == 2 and want[2][n - 1] == 2 and not want[2][1:n - 1].any()
    for offset in (0, 4, 1):          # floats: aligned, 16 bytes on (still the 16-byte loads), 4 bytes on (the scalar ones)
        buf = torch.zeros(x.size + offset, dtype=torch.float32, device=DEV)
        xd = buf[offset:]
        xd.copy_(torch.from_numpy(x).reshape(-1))
        assert xd.data_ptr() % 16 == (4 * offset) % 16
        codes, norms, flags = abi_encode(xd, n, S)
        assert np.array_equal(codes, want[0]), (offset, int((codes != want[0]).sum()))
        assert not codes[:, 3 * S * S:].any()          # the pad
        assert np.array_equal(norms, want[1]) and np.array_equal(flags, want[2])


def test_encode_images_is_the_entry_point():
    from locate_amd import encode_images
    x = encoder_input(8, 1)
    codes, norms, flags = encode_images(torch.from_numpy(x).to(DEV))
    assert codes.dtype == torch.int8 and norms.dtype == torch.int64 and flags.dtype == torch.int32
    want = M.encode(x)
    assert np.array_equal(codes.cpu().numpy(), want[0]) and np.array_equal(norms.cpu().numpy(), want[1]) and np.array_equal(flags.cpu().numpy(), want[2])


# ---- 2. the lane map: exact integer data, one-hot against an asymmetric ramp ---------------------------------------------------------
def ramp(N, row):
    j, b = np.arange(N)[:, None], np.arange(row)[None, :]
    return (((7 * j + 3 * b) % 251) - 125).astype(np.int8)


def one_hot(positions, row):
    q = np.zeros((len(positions), row), dtype=np.int8)
    q[np.arange(len(positions)), positions] = 127
    return q


def test_lane_map_one_hot_against_a_ramp():
    """every 16-byte group of a 128-byte stage, both lane halves of every 32-byte step: d2 of every (i, j) pair"""
    positions = [0, 17, 34, 51, 68, 85, 102, 119, 15, 16, 31, 32, 63, 64, 127]
    q, r = one_hot(positions, 128), ramp(8, 128)
    want = M.distances(q, r)
    d2, index = search(q, r, 8)
    full = np.full_like(want, -1)
    np.put_along_axis(full, index.astype(np.int64), d2, axis=1)
    assert np.array_equal(full, want)
    assert same((d2, index), M.topk(want, 8))


def test_lane_map_every_row_and_column_of_the_block_tile():
    """128 references x 64 queries - every wave, every accumulator register, both query tiles: k = 8 through windows of 8 references"""
    positions = [(5 * i + 3) % 128 for i in range(64)]
    q, r = one_hot(positions, 128), ramp(128, 128)
    want = M.distances(q, r)
    full = np.full_like(want, -1)
    for w in range(16):
        rflags = np.ones(128, np.int32)
        rflags[8 * w:8 * w + 8] = 0
        d2, index = search(q, r, 8, rflags=rflags)
        assert (index >= 8 * w).all() and (index < 8 * w + 8).all()
        np.put_along_axis(full, index.astype(np.int64), d2, axis=1)
    assert np.array_equal(full, want)


@pytest.mark.parametrize("S", [4, 8])
def test_signs(S):
    row = M.row_bytes(S)
    lo, hi = np.zeros((1, row), np.int8), np.zeros((1, row), np.int8)
    lo[0, :3 * S * S], hi[0, :3 * S * S] = -128, 127
    for a, b in ((lo, hi), (hi, lo)):
        d2, index = search(a, b, 1)
        assert d2.tolist() == [[255 * 255 * 3 * S * S]] and index.tolist() == [[0]]
    d2, _ = search(lo, lo, 1)
    assert d2.tolist() == [[0]]


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------
QS, NS, KS = (1, 3, 64, 65, 130), (1, 5, 127, 128, 129, 1000), (1, 3, 8)


# rows of 64 bytes from five values (ties everywhere, both extremes), of 448 (S = 12: 3.5 stages) and 1216 bytes (S = 20: 9.5 stages)
@pytest.mark.parametrize("row", [64, 448, 1216])
def test_shapes(row):
    rng = np.random.default_rng(row)
    if row == 64:
        q, r = (rng.choice(np.array([-128, -1, 0, 1, 127], dtype=np.int8), size=(n, row)) for n in (max(QS), max(NS)))
    else:
        q, r = (rng.integers(-128, 128, size=(n, row), dtype=np.int8) for n in (max(QS), max(NS)))
    from locate_amd import nearest
    want = M.distances(q, r)          # once: every case is a corner of it, on the device too
    tq, tr = triple(q), triple(r)
    for Q in QS:
        for N in NS:
            for k in KS:
                d2, index = nearest(tuple(t[:Q] for t in tq), tuple(t[:N] for t in tr), k=k)
                got = (d2.cpu().numpy(), index.cpu().numpy())
                assert got[0].shape == (Q, k) and same(got, M.topk(want[:Q, :N], k)), (Q, N, k)
                if k > N:
                    assert (got[1][:, N:] == -1).all() and (got[0][:, N:] == -1).all()


def test_ties_resolve_to_the_lower_index_across_tiles():
    rng = np.random.default_rng(11)
    r = rng.integers(-128, 128, size=(400, 192), dtype=np.int8)
    r[300] = r[5]          # another tile
    r[9] = r[5]            # the same tile, another lane
    r[37] = r[5]           # the same tile, another wave
    q = np.stack([r[5], r[300], rng.integers(-128, 128, size=192, dtype=np.int8)])
    d2, index = search(q, r, 8)
    assert index[0, :4].tolist() == [5, 9, 37, 300] and d2[0, :4].tolist() == [0, 0, 0, 0] and index[1, :4].tolist() == [5, 9, 37, 300]
    assert same((d2, index), M.topk(M.distances(q, r), 8))


def test_skip_and_flags():
    rng = np.random.default_rng(12)
    q = rng.integers(-128, 128, size=(70, 192), dtype=np.int8)
    r = rng.integers(-128, 128, size=(300, 192), dtype=np.int8)
    r[:70] = q          # the queries are part of the bank
    qflags, rflags = np.zeros(70, np.int32), np.zeros(300, np.int32)
    qflags[[3, 64, 69]] = (1, 5, 192)
    rflags[[0, 8, 127, 128, 299]] = 1
    skip = np.arange(70)
    skip[10] = -1          # none: its own row comes first, distance 0
    skip[11] = 250
    want = M.distances(q, r)
    for k in (1, 8):
        d2, index = search(q, r, k, qflags, rflags, skip)
        assert same((d2, index), M.topk(want, k, qflags, rflags, skip))
        assert (index[[3, 64, 69]] == -1).all() and (d2[[3, 64, 69]] == -1).all()
        assert index[10, 0] == 10 and d2[10, 0] == 0 and index[11, 0] == 11 and (index[12] != 12).all()
        assert not np.isin(index, [0, 8, 127, 128, 299]).any()
    # no flags on the reference side: the pointer may be null
    from locate_amd import nearest
    tq, tr = triple(q), triple(r)
    d2, index = nearest(tq, (tr[0], tr[1], None), k=3)
    assert same((d2.cpu().numpy(), index.cpu().numpy()), M.topk(want, 3))


def test_nonfinite_images_are_flagged_and_never_returned():
    from locate_amd import encode_images, nearest
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, size=(6, 3, 8, 8)).astype(np.float32)
    x[2, 0, 0, 0], x[4, 2, 7, 7] = np.nan, np.inf
    t = encode_images(torch.from_numpy(x).to(DEV))
    d2, index = nearest(t, t, k=8)
    want = M.nearest(M.encode(x), M.encode(x), 8)
    assert same((d2.cpu().numpy(), index.cpu().numpy()), want)
    index = index.cpu().numpy()
    assert (index[[2, 4]] == -1).all() and not np.isin(index, [2, 4]).any() and (index[0, :4] >= 0).all() and (index[0, 4:] == -1).all()


def test_segments_rows_past_the_int32_accumulator():
    """rows of 134848 bytes - three segments, the last one short - whose operands hold the extremes: 128^2 row > 2^31"""
    row = 134848
    rng = np.random.default_rng(14)
    q = np.stack([np.full(row, -128, np.int8), np.full(row, 127, np.int8)])
    r = np.stack([np.full(row, -128, np.int8), np.full(row, 127, np.int8), rng.integers(-128, 128, size=row, dtype=np.int8)])
    assert 128 * 128 * row > 2 ** 31
    want = M.distances(q, r)
    assert want[0, 1] == 255 * 255 * row and want[0, 0] == 0
    assert same(search(q, r, 3), M.topk(want, 3))


def test_what_the_entry_point_refuses():
    from locate_amd import nearest
    from locate_amd._lib import LocateError, check, lib
    L = lib()
    q, r = triple(np.zeros((2, 64), np.int8)), triple(np.zeros((3, 64), np.int8))
    for k in (0, 9):
        with pytest.raises(ValueError):
            nearest(q, r, k=k)
    with pytest.raises(ValueError):
        nearest(q, triple(np.zeros((3, 128), np.int8)))
    d2, index = torch.empty(2, 3, dtype=torch.int64, device=DEV), torch.empty(2, 3, dtype=torch.int32, device=DEV)
    ws = torch.empty(64, dtype=torch.int64, device=DEV)
    assert L.locate_nn_search_workspace_bytes(2, 3, 3) == 2 * 1 * 3 * 8 and L.locate_nn_search_workspace_bytes(65, 129, 8) == 65 * 2 * 8 * 8
    args = lambda **kw: [kw.get("qc", p(q[0])), p(q[1]), p(q[2]), 2, p(r[0]), p(r[1]), None, 3, kw.get("row", 64), None, kw.get("k", 3), p(d2), p(index),  # noqa: E731
                         kw.get("ws", p(ws)), stream()]
    assert L.locate_nn_search(*args()) == 0
    misaligned = ctypes.c_void_p(q[0].data_ptr() + 8)
    for bad in (dict(k=0), dict(k=9), dict(row=96), dict(row=0), dict(row=262144 + 64), dict(qc=None), dict(qc=misaligned), dict(ws=None)):
        with pytest.raises(LocateError):
            check(L.locate_nn_search(*args(**bad)), "locate_nn_search")


# ---- 4. the bank --------------------------------------------------------------------------------------------------------------------
def test_bank_from_a_store(monkeypatch):
    from locate_amd import DeviceImageStore, NearestNeighbours, neighbours
    images = np.random.default_rng(15).integers(0, 256, size=(37, 10, 14, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)
    monkeypatch.setattr(neighbours, "BANK_CHUNK", 16)          # three transform calls, the last one short
    nn = NearestNeighbours(S=8, k=3, images=9, seed=21, device=DEV).reference_from_store(store)
    want = M.bank_codes(images, 8)
    codes, norms, flags = (t.cpu().numpy() for t in nn.bank)
    assert codes.shape == (37, 192) and np.array_equal(codes, want)          # Pillow's bytes - 128
    assert np.array_equal(norms, M.norms(want)) and not flags.any()
    # the baselines
    drawn = torch.randperm(37, generator=torch.Generator().manual_seed(21 + 5))[:9].tolist()
    assert nn.baseline_index == drawn
    bank = (want, M.norms(want), np.zeros(37, np.int32))
    r2r, among = M.baselines(bank, drawn, 8)
    assert nn.real_to_real == r2r and nn.real_among_themselves == among and r2r["median"] > 0 and among["min"] >= r2r["min"]
    # every image finds itself
    views = nn.canonical_views(range(37))
    value = nn.search(views)
    assert [row[0] for row in value["index"]] == list(range(37)) and [row[0] for row in value["d2"]] == [0] * 37
    assert value == M.record(views.cpu().numpy(), bank, 3, 8, r2r, among)
    assert value["generated_to_real"] == {"min": 0.0, "median": 0.0} and value["nonfinite"] == 0 and value["images"] == 37
    # limit: the first images
    short = NearestNeighbours(S=8, k=2, images=64, seed=21, device=DEV).reference_from_store(store, limit=20)
    assert np.array_equal(short.bank[0].cpu().numpy(), want[:20]) and len(short.baseline_index) == 20
    assert max(max(row) for row in short.search(views)["index"]) < 20


# ---- 5. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) ---------------------
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


def small_search():
    """a searcher over STORE at 32 x 32 (built once: nothing below changes it)"""
    if "nn" not in _CACHE:
        from locate_amd import DeviceImageStore, NearestNeighbours
        _CACHE["nn"] = NearestNeighbours(S=32, k=3, images=16, seed=4, chunk=8, device=DEV).reference_from_store(DeviceImageStore(STORE, DEV))
    return _CACHE["nn"]


def test_evaluate_is_the_model_applied_to_the_generated_images():
    G, _, _, _ = build_tiny()
    nn = small_search()
    first = nn.evaluate(G)
    assert G.training and tuple(nn.latents(G.g_in).shape) == (16, G.g_in)
    images = nn.generate(G)
    assert tuple(images.shape) == (16, 3, 32, 32)
    bank = tuple(t.cpu().numpy() for t in nn.bank)
    assert np.array_equal(bank[0], M.bank_codes(STORE, 32))
    assert first == M.record(images.cpu().numpy(), bank, 3, 32, nn.real_to_real, nn.real_among_themselves)
    assert nn.evaluate(G) == first
    assert sorted(first) == ["d2", "generated_to_generated", "generated_to_real", "images", "index", "k", "nonfinite", "real_among_themselves",
                             "real_to_real", "rms"]
    assert first["images"] == 16 and first["k"] == 3 and first["nonfinite"] == 0 and all(len(row) == 3 for row in first["index"])
    # the caller's latents, and eval mode restored too
    G.eval()
    own = torch.randn(5, G.g_in, generator=torch.Generator().manual_seed(1)).to(DEV)
    value = nn.evaluate(G, latents=own)
    assert not G.training and value["images"] == 5
    assert value == M.record(nn.generate(G, own).cpu().numpy(), bank, 3, 32, nn.real_to_real, nn.real_among_themselves)


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_an_evaluation_between_iterations_has_no_side_effect(launch, tmp_path):
    from locate_amd.graph import GraphedTrainStep

    def run(measure):
        G, D, step, (lat, real, aug) = build_tiny()
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
        values, losses = [], []
        for i in range(6):
            out = runner.replay() if runner is not None else step(lat, real, aug)
            losses.append((out["d_error"].detach().clone(), out["g_error"].detach().clone()))
            if measure and i == 2:
                nn = small_search()
                values = [nn.evaluate(G), nn.evaluate(G)]
                nn.save_picture(str(tmp_path / "n.png"), G)
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


def test_the_picture(tmp_path):
    from locate_amd.monitor import grid_geometry, read_png
    G, _, _, _ = build_tiny()
    nn = small_search()
    path = nn.save_picture(str(tmp_path / "n.png"), G)
    rgba = read_png(path)
    _, _, GH, GW = grid_geometry(16 * 4, 32, nrow=4, padding=2)
    assert rgba.shape == (GH, GW, 4) and (rgba[..., 3] == 255).all()
    # the tile right of sample i is the canonical view of its nearest image: the store's bytes
    value = nn.evaluate(G)
    for i in (0, 7, 15):
        want = M.canonical_u8(STORE[value["index"][i][0]], 32)
        tile = rgba[2 + 34 * i:2 + 34 * i + 32, 2 + 34:2 + 34 + 32, :3]
        assert np.abs(tile.astype(np.int64) - want.astype(np.int64)).max() <= 1          # the grid scales by 255 in fp32 and truncates


# ---- 6. the trainer and the command line ---------------------------------------------------------------------------------------------
def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, files in os.walk(str(root)) for f in files)


def test_trainer_records_the_neighbours(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, NearestNeighbours, Trainer
    store = DeviceImageStore(STORE, DEV)

    def trainer(out, with_neighbours):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        nn = NearestNeighbours(S=32, k=2, images=8, seed=3, chunk=8, device=DEV).reference_from_store(store) if with_neighbours else None
        t = Trainer(step, pipeline, str(out), epochs=1, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                    image_interval_function=lambda batch: 2, neighbours=nn)
        return t, G, D, step, nn

    t, G1, D1, step1, nn = trainer(tmp_path / "with", True)
    assert t.run() == 4
    path = os.path.join(str(tmp_path / "with"), "error", "neighbours.json")
    picture = os.path.join(str(tmp_path / "with"), "error", "1-neighbours.png")
    assert path in t.written and picture in t.written and os.path.exists(path) and os.path.exists(picture) and not os.path.exists(path + ".tmp")
    rec = json.load(open(path))
    assert len(rec) == 1 and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["images"], rec[0]["k"]) == (1, 4, 13, 2)
    direct = nn.evaluate(G1, latents=t.sampler.fixed_noise)          # the sampler's latents; the weights are the saved ones
    assert rec[0]["index"] == direct["index"] and rec[0]["generated_to_real"] == direct["generated_to_real"]
    assert sorted(rec[0]) == sorted(["epoch", "iterations"] + [k for k in direct if k not in ("d2", "rms")])

    plain, G2, D2, step2, _ = trainer(tmp_path / "without", False)
    assert plain.run() == 4
    extra = [os.path.join("error", "1-neighbours.png"), os.path.join("error", "neighbours.json")]
    assert listing(tmp_path / "without") == [f for f in listing(tmp_path / "with") if f not in extra]
    assert sorted(set(listing(tmp_path / "with")) - set(listing(tmp_path / "without"))) == extra
    strip = lambda files, root: [os.path.relpath(f, str(root)) for f in files if "neighbours" not in f]      # noqa: E731
    assert strip(plain.written, tmp_path / "without") == strip(t.written, tmp_path / "with")
    a, b = training_state(G1, D1, step1), training_state(G2, D2, step2)
    assert sorted(a) == sorted(b) and not [k for k in a if not torch.equal(a[k], b[k])]


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, STORE)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--neighbours", "16", "--neighbours-k", "2"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    rec = json.load(open(os.path.join(out, "error", "neighbours.json")))
    assert len(rec) == 1 and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["images"], rec[0]["k"]) == (1, 4, 16, 2)
    assert all(len(row) == 2 and all(0 <= j < 32 for j in row) for row in rec[0]["index"])
    assert rec[0]["real_to_real"]["median"] > 0 and rec[0]["generated_to_real"]["median"] > 0
    assert os.path.exists(os.path.join(out, "error", "1-neighbours.png"))
