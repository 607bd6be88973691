"""The binned mode coverage on the MI355X: the group-sum and centroid kernels of csrc/modes.hip at the C ABI, k-means and the NDB record
through locate_amd/modes.py, all against the numpy model (tests/helpers/modes_model.py) - integers, so everything is compared with == -
and the behaviour around a running training: an evaluation between two iterations, eager or replayed, leaves the trajectory where it
would be.  Outputs and workspace hold 0x55 garbage before every ABI-level call: nothing may depend on their contents."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import modes_model as MM  # noqa: E402
import neighbours_model as NM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def garbage(n, dtype):
    return torch.full((max(int(n), 1) * torch.empty(0, dtype=dtype).element_size(),), 0x55, dtype=torch.uint8, device=DEV).view(dtype)


def workspace_bytes(M, K, row):
    """the formula include/locate_hip.h documents"""
    slots = -(-M // 64) + K + 1
    return 4 * (slots * (row + 1) + 2 * (K + 1))


def abi_group_sums(codes, order, starts, K, codes_dev=None, offset=0):
    """locate_nn_group_sums on raw int8 rows; returns sums int32 [K, row] as numpy.  codes_dev / offset: the rows as they lie on the device"""
    from locate_amd._lib import check, lib
    L = lib()
    N, row = codes.shape
    M = len(order)
    c = dev(codes, np.int8) if codes_dev is None else codes_dev
    o, s = dev(order, np.int32), dev(starts, np.int32)
    sums = garbage(K * row, torch.int32)
    bytes_ = L.locate_nn_group_sums_workspace_bytes(M, K, row)
    assert bytes_ == workspace_bytes(M, K, row)
    ws = garbage(bytes_ // 4, torch.int32)
    check(L.locate_nn_group_sums(p(c, offset), N, row, p(o), M, p(s), K, p(sums), p(ws), stream()), "locate_nn_group_sums")
    return sums.cpu().numpy().reshape(K, row)


def abi_centroids(sums, starts, M, previous, in_place=False):
    """locate_nn_centroids; returns (codes int8 [K, row], norms int64 [K], moved int32 [K]) as numpy"""
    from locate_amd._lib import check, lib
    K, row = sums.shape
    s, st, prev = dev(sums, np.int32), dev(starts, np.int32), dev(previous, np.int8)
    out = prev if in_place else garbage(K * row, torch.int8)
    norms, moved = garbage(K, torch.int64), garbage(K, torch.int32)
    check(lib().locate_nn_centroids(p(s), p(st), K, M, row, p(prev), p(out), p(norms), p(moved), stream()), "locate_nn_centroids")
    return out.cpu().numpy().reshape(K, row), norms.cpu().numpy(), moved.cpu().numpy()


# ---- 1. group sums at the raw ABI -----------------------------------------------------------------------------------------------------
def layout(name, M, K, N, rng):
    """(order [M], starts [K + 1]) of the named arrangement"""
    order = rng.integers(0, N, size=M)
    cuts = np.sort(rng.integers(0, M + 1, size=K + 1))
    cuts[0], cuts[-1] = 0, M
    if name == "one_group":          # all rows in group 0: it spans every slab
        cuts[:] = M
        cuts[0] = 0
    elif name == "singles":          # group k is row k alone; the groups past M are empty
        cuts = np.minimum(np.arange(K + 1), M)
    elif name == "empties":          # empty groups at the front, in the middle and at the end
        cuts[:min(2, K)] = 0
        cuts[K // 2] = cuts[max(K // 2 - 1, 0)]
        cuts[-min(2, K):] = M if K > 1 else cuts[-1]
        cuts = np.sort(cuts)
    elif name == "front":          # the leading rows are in no group
        cuts = np.maximum(cuts, min(M - 1, 1 + M // 3))
    elif name == "subset":          # distinct rows, fewer than N
        order = rng.permutation(N)[:M] if M <= N else order
    elif name == "repeats":
        order = rng.integers(0, min(N, 3), size=M)
    elif name == "invalid":          # -1 and N among valid ones, and some far out
        order[rng.random(M) < 0.3] = -1
        order[rng.random(M) < 0.2] = N
        order[::7] = (2 ** 31 - 1, -2 ** 31, N + 5, -2)[M % 4]
    elif name == "decrease":          # one value falls back: an empty group and an overlap; the last exceeds M, one is negative
        cuts[K // 2 + 1 if K > 1 else 1] = cuts[K // 2] // 2
        cuts[-1] = M + 50
        cuts[0] = -3
    return order, cuts


LAYOUTS = ("mixed", "one_group", "singles", "empties", "front", "subset", "repeats", "invalid", "decrease")
CASES = [(row, M, K, name) for row in (64, 192, 1216, 3072) for (M, K) in ((257, 3), (1000, 129)) for name in LAYOUTS]
CASES += [(192, M, K, "mixed") for M in (1, 2, 255, 256, 257, 1000) for K in (1, 3, 128, 129, 300)]
CASES += [(192, 257, 300, "singles"), (64, 256, 128, "decrease"), (1216, 255, 300, "empties"), (3072, 2, 1, "one_group")]


@pytest.mark.parametrize("row,M,K,name", CASES)
def test_group_sums_against_the_model(row, M, K, name):
    rng = np.random.default_rng(row + 7 * M + 13 * K + len(name))
    N = 300 if name != "subset" else 1200
    codes = rng.integers(-128, 128, size=(N, row), dtype=np.int8)
    order, starts = layout(name, M, K, N, rng)
    want = MM.group_sums(codes, order, starts, K)
    got = abi_group_sums(codes, order, starts, K)
    assert got.dtype == np.int32 and np.array_equal(got, want), int((got != want).sum())
    sizes = MM.group_sizes(starts, K, M)
    assert not got[[k for k in range(K) if sizes[k] == 0]].any()          # an empty group: a row of zeros
    if name == "one_group":
        assert sizes[0] == M and (M <= 64 or np.array_equal(got[0], codes[order].astype(np.int64).sum(0)))
    if name == "decrease" and K > 1:
        assert 0 in sizes and sizes[-1] > 0


def test_group_sums_of_rows_longer_than_65536_bytes():
    row = NM.row_bytes(148)
    assert row == 65728
    rng = np.random.default_rng(3)
    codes = rng.integers(-128, 128, size=(3, row), dtype=np.int8)
    order, starts = [2, 0, 0, 1, 3, 2, -1], [1, 4, 4, 7]
    assert np.array_equal(abi_group_sums(codes, order, starts, 3), MM.group_sums(codes, order, starts, 3))


# ---- 2. the accumulator is int32 --------------------------------------------------------------------------------------------------------
def test_sums_of_seventy_thousand_extreme_rows_are_exact():
    M = 70000
    for value in (-128, 127):
        codes = np.full((M, 64), value, dtype=np.int8)
        got = abi_group_sums(codes, np.arange(M), [0, M], 1)
        assert got.shape == (1, 64) and (got == value * M).all() and abs(value * M) > 2 ** 23


def test_what_the_entry_points_refuse():
    from locate_amd._lib import LocateError, check, lib
    L = lib()
    big = 2 ** 24
    codes = torch.zeros(4, 64, dtype=torch.int8, device=DEV)
    order = torch.zeros(big, dtype=torch.int32, device=DEV)          # as long as the refused call says: nothing could be read past it
    starts = T([0, 4], dtype=torch.int32).to(DEV)
    sums, ws = garbage(64, torch.int32), garbage(4096, torch.int32)
    assert L.locate_nn_group_sums_workspace_bytes(big, 1, 64) == 0 and L.locate_nn_group_sums_workspace_bytes(big - 1, 1, 64) == workspace_bytes(big - 1, 1, 64)
    assert L.locate_nn_group_sums_workspace_bytes(4, 0, 64) == 0 and L.locate_nn_group_sums_workspace_bytes(4, 65536, 64) == 0
    assert L.locate_nn_group_sums_workspace_bytes(4, 1, 96) == 0 and L.locate_nn_group_sums_workspace_bytes(4, 1, 262144 + 64) == 0
    args = lambda **kw: [kw.get("codes", p(codes)), kw.get("N", 4), kw.get("row", 64), kw.get("order", p(order)), kw.get("M", 4),  # noqa: E731
                         kw.get("starts", p(starts)), kw.get("K", 1), kw.get("sums", p(sums)), kw.get("ws", p(ws)), stream()]
    status = L.locate_nn_group_sums(*args(M=big))
    assert status != 0 and b"locate_nn_group_sums" in L.locate_last_error()
    torch.cuda.synchronize()
    assert (sums.cpu() == 0x55555555).all() and (ws.cpu() == 0x55555555).all()          # no launch: not a word was written
    for bad in (dict(M=0), dict(M=-1), dict(K=0), dict(K=65536), dict(N=0), dict(row=0), dict(row=96), dict(row=262144 + 64), dict(codes=None),
                dict(order=None), dict(starts=None), dict(sums=None), dict(ws=None), dict(codes=p(codes, 8)), dict(ws=p(ws, 8)),
                dict(order=p(order, 2)), dict(starts=p(starts, 2)), dict(sums=p(sums, 2))):
        status = L.locate_nn_group_sums(*args(**bad))
        assert status != 0 and b"locate_nn_group_sums" in L.locate_last_error(), bad
        with pytest.raises(LocateError):
            check(status, "locate_nn_group_sums")
    assert L.locate_nn_group_sums(*args()) == 0 and not sums.cpu()[:64].any()
    prev, out = torch.zeros(64, dtype=torch.int8, device=DEV), garbage(64, torch.int8)
    norms, moved = garbage(1, torch.int64), garbage(1, torch.int32)
    cargs = lambda **kw: [kw.get("sums", p(sums)), kw.get("starts", p(starts)), kw.get("K", 1), kw.get("M", 4), kw.get("row", 64),  # noqa: E731
                          kw.get("prev", p(prev)), kw.get("out", p(out)), kw.get("norms", p(norms)), kw.get("moved", p(moved)), stream()]
    for bad in (dict(M=big), dict(M=0), dict(K=0), dict(K=65536), dict(row=32), dict(row=262144 + 64), dict(sums=None), dict(starts=None), dict(prev=None),
                dict(out=None), dict(norms=None), dict(moved=None), dict(sums=p(sums, 4)), dict(prev=p(prev, 8)), dict(out=p(out, 8)),
                dict(norms=p(norms, 4)), dict(moved=p(moved, 2)), dict(starts=p(starts, 2))):
        status = L.locate_nn_centroids(*cargs(**bad))
        assert status != 0 and b"locate_nn_centroids" in L.locate_last_error(), bad
    torch.cuda.synchronize()
    assert (out.cpu() == 0x55).all() and moved.cpu().tolist() == [0x55555555]
    assert L.locate_nn_centroids(*cargs()) == 0 and not out.cpu().any() and norms.cpu().tolist() == [0] and moved.cpu().tolist() == [0]


# ---- 3. the rounded mean ----------------------------------------------------------------------------------------------------------------
def test_centroids_against_the_model():
    rng = np.random.default_rng(5)
    K, row, M = 12, 192, 1000
    starts = [3, 5, 7, 9, 11, 11, 16, 23, 23, 400, 300, 1001, 2000]          # n = 2 2 2 2 0 5 7 0 377 0 700 0 (the last two clamp to M)
    sizes = MM.group_sizes(starts, K, M)
    assert sizes == [2, 2, 2, 2, 0, 5, 7, 0, 377, 0, 700, 0]
    sums = np.zeros((K, row), dtype=np.int64)
    for k, n in enumerate(sizes):
        if n:
            sums[k, :180] = rng.integers(-128 * n, 127 * n + 1, size=180)          # 180 .. 191: the pad, sums 0
    sums[:4, 0] = (-3, -1, 1, 3)          # halves, negative and positive
    sums[:4, 1] = (-256, 254, -255, 253)          # the ends, and the halves next to them
    sums[5, :3] = (-128 * 5, 127 * 5, -2)
    sums[6, :3] = (-128 * 7, 127 * 7, 3)
    sums[8, :2] = (-128 * 377, 127 * 377)
    sums[10, :4] = (-128 * 700, 127 * 700, 350, -350)
    previous = rng.integers(-128, 128, size=(K, row), dtype=np.int8)
    previous[:, 180:] = 0
    previous[1] = MM.centroids(sums, starts, M, previous)[0][1]          # a centre that is where its mean is: it does not move
    want = MM.centroids(sums, starts, M, previous)
    assert want[0][:4, 0].tolist() == [-1, 0, 1, 2] and want[0][:4, 1].tolist() == [-128, 127, -127, 127] and want[0][10, :4].tolist() == [-128, 127, 1, 0]
    got = abi_centroids(sums, starts, M, previous)
    assert got[0].dtype == np.int8 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    empty = [k for k in range(K) if sizes[k] == 0]
    assert np.array_equal(got[0][empty], previous[empty]) and not got[2][empty].any() and got[2][1] == 0 and got[2][0] > 0
    assert not got[0][:, 180:].any() and np.array_equal(got[1], NM.norms(got[0]))
    in_place = abi_centroids(sums, starts, M, previous, in_place=True)
    assert all(np.array_equal(a, b) for a, b in zip(in_place, got))
    again = abi_centroids(sums, starts, M, previous)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


# ---- 4. the same words from call to call, whatever the alignment --------------------------------------------------------------------------
def test_two_calls_give_the_same_words():
    rng = np.random.default_rng(6)
    N, row, M, K = 300, 1216, 1000, 129
    codes = rng.integers(-128, 128, size=(N, row), dtype=np.int8)
    order, starts = layout("mixed", M, K, N, rng)
    first = abi_group_sums(codes, order, starts, K)
    assert np.array_equal(first, abi_group_sums(codes, order, starts, K)) and np.array_equal(first, MM.group_sums(codes, order, starts, K))
    buffer = garbage(N * row + 64, torch.int8)
    buffer[16:16 + N * row] = dev(codes, np.int8).reshape(-1)
    assert np.array_equal(first, abi_group_sums(codes, order, starts, K, codes_dev=buffer, offset=16))


# ---- 5. Lloyd's algorithm ---------------------------------------------------------------------------------------------------------------
def images_of_codes(codes, S):
    """fp32 [n, 3, S, S] whose codes are `codes` [n, 3 S S]: the encoder maps (code + 128) / 127.5 - 1 back exactly"""
    return ((np.asarray(codes, dtype=np.float64) + 128) / 127.5 - 1).astype(np.float32).reshape(-1, 3, S, S)


def test_kmeans_equals_the_models_lloyd():
    from locate_amd import encode_images, kmeans_codes
    rng = np.random.default_rng(11)
    N, K, S, rounds, seed = 300, 7, 8, 6, 77
    centres = rng.integers(-90, 91, size=(5, 192))
    x = images_of_codes(np.clip(centres[rng.integers(0, 5, size=N)] + rng.integers(-20, 21, size=(N, 192)), -128, 127), S)
    x[17, 0, 0, 0], x[200, 2, 7, 7] = np.nan, np.inf
    flags = np.zeros(N, np.int32)
    flags[[17, 200]] = 1
    ok = np.flatnonzero(flags == 0)
    initial = ok[torch.randperm(N - 2, generator=torch.Generator().manual_seed(seed))[:K].numpy()]
    x[initial[4]] = x[initial[1]]          # two identical rows among the initial centres: centre 4 gets no row in the first round
    model = NM.encode(x)
    assert np.array_equal(model[2] != 0, flags != 0) and np.array_equal(model[0][initial[4]], model[0][initial[1]])
    want = MM.lloyd(model, initial, rounds)
    assert want[4][0][4] == 0 and all(a >= b for a, b in zip(want[3], want[3][1:])) and want[3][0] > want[3][-1] and want[4].any()
    triple = encode_images(torch.from_numpy(x).to(DEV))
    assert np.array_equal(triple[0].cpu().numpy(), model[0])
    centres_t, labels, counts, inertia, moved = kmeans_codes(triple, K, iterations=rounds, seed=seed)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and inertia.dtype == torch.int64 and moved.dtype == torch.int32
    assert tuple(inertia.shape) == (rounds + 1,) and tuple(moved.shape) == (rounds, K) and inertia.is_cuda
    assert np.array_equal(centres_t[0].cpu().numpy(), want[0]) and np.array_equal(centres_t[1].cpu().numpy(), NM.norms(want[0]))
    assert not centres_t[2].cpu().any()
    assert np.array_equal(labels.cpu().numpy(), want[1]) and np.array_equal(counts.cpu().numpy(), want[2])
    assert inertia.cpu().tolist() == want[3] and np.array_equal(moved.cpu().numpy(), want[4])
    got = inertia.cpu().tolist()
    assert all(a >= b for a, b in zip(got, got[1:]))
    with pytest.raises(ValueError):
        kmeans_codes(triple, N - 1, iterations=1, seed=seed)          # 298 rows are not flagged


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
SEED, S6, BINS, IMAGES, SAMPLES = 41, 16, 16, 512, 256


def prototypes():
    """16 smooth pictures, far apart: byte = 128 + 70 cos(a y + phase) cos(b x) per channel with its own (a, b, phase)"""
    y, x = np.meshgrid(np.arange(S6), np.arange(S6), indexing="ij")
    out = np.empty((16, S6, S6, 3))
    for k in range(16):
        for c in range(3):
            out[k, :, :, c] = 128 + 70 * np.cos((1 + k % 4) * np.pi * y / S6 + c) * np.cos((1 + k // 4) * np.pi * x / S6 + 0.5 * k)
    return np.rint(out)


def synthetic_store():
    """(store uint8 [800, 16, 16, 3], the prototype of every store image): the images k-means starts from - known from the seeds - are
    one of each prototype, so every bin is one prototype; the others are drawn at random"""
    rng = np.random.default_rng(12)
    N = 800
    order = torch.randperm(N, generator=torch.Generator().manual_seed(SEED + 10)).tolist()
    start = [order[i] for i in torch.randperm(IMAGES, generator=torch.Generator().manual_seed(SEED + 12))[:BINS].tolist()]
    which = rng.integers(0, 16, size=N)
    which[start] = np.arange(16)
    store = np.clip(prototypes()[which] + rng.integers(-2, 3, size=(N, S6, S6, 3)), 0, 255).astype(np.uint8)
    return store, which, order


def fakes(which, seed):
    noise = np.random.default_rng(seed).integers(-2, 3, size=(len(which), S6, S6, 3))
    codes = (np.clip(prototypes()[which] + noise, 0, 255) - 128).transpose(0, 3, 1, 2).reshape(len(which), -1)
    return images_of_codes(codes, S6)


def model_reference(store, order):
    """the model's centres, counts, k-means summary and baseline for the synthetic store"""
    bank = NM.bank_codes(store, S6)
    real = bank[order[:IMAGES]]
    initial = torch.randperm(IMAGES, generator=torch.Generator().manual_seed(SEED + 12))[:BINS].numpy()
    centres, _, counts, inertia, moved = MM.lloyd((real, NM.norms(real), np.zeros(IMAGES, np.int32)), initial, 10)
    kmeans = {"iterations": 10, "converged_at": MM.converged_at(moved), "inertia": inertia}
    second = bank[order[IMAGES:IMAGES + SAMPLES]]
    base = MM.record((second, NM.norms(second), np.zeros(SAMPLES, np.int32)), centres, counts, 0.05, kmeans, None)
    return centres, counts, kmeans, {key: base[key] for key in ("ndb", "ndb_over_k", "js", "missing", "fake_counts")}


def same_record(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        if key in ("js", "z", "ndb_over_k"):
            assert got[key] == pytest.approx(want[key], rel=1e-12, abs=0.0), key
        elif key == "baseline":
            assert sorted(got[key]) == sorted(want[key]) and got[key]["js"] == pytest.approx(want[key]["js"], rel=1e-12, abs=0.0)
            assert all(got[key][k] == want[key][k] for k in want[key] if k != "js")
        else:
            assert got[key] == want[key], key


def test_binned_modes_end_to_end(tmp_path):
    from locate_amd import BinnedModes, DeviceImageStore
    store, which, order = synthetic_store()
    centres, counts, kmeans, baseline = model_reference(store, order)
    critical = 1.959963984540054
    # what the test relies on, on the model alone: every bin is one prototype, all fakes -> few different bins, six prototypes left out ->
    # exactly those six bins are missing, and no |z| sits on the critical value
    rng = np.random.default_rng(13)
    all_which, some_which = rng.integers(0, 16, size=SAMPLES), rng.integers(0, 10, size=SAMPLES)
    x_all, x_some = fakes(all_which, 14), fakes(some_which, 15)
    assert kmeans["converged_at"] is not None and counts.tolist() == [int((which[order[:IMAGES]] == k).sum()) for k in range(16)]
    want_all = MM.record(NM.encode(x_all), centres, counts, 0.05, kmeans, baseline)
    want_some = MM.record(NM.encode(x_some), centres, counts, 0.05, kmeans, baseline)
    assert want_all["fake_counts"] == [int((all_which == k).sum()) for k in range(16)] and want_all["ndb"] <= 2 and baseline["ndb"] <= 2
    assert want_some["fake_counts"][10:] == [0] * 6 and all(want_some["different"][10:]) and sorted(want_some["order"][:6]) == list(range(10, 16))
    assert want_some["missing"] == 6 and min(want_some["fake_counts"][:10]) > 0
    for rec in (want_all, want_some):
        assert min(abs(abs(z) - critical) for z in rec["z"]) > 1e-9

    bm = BinnedModes(S=S6, bins=BINS, images=IMAGES, samples=SAMPLES, seed=SEED, device=DEV).reference_from_store(DeviceImageStore(store, DEV))
    assert bm.real_index == order[:IMAGES] and np.array_equal(bm.centres[0].cpu().numpy(), centres)
    assert bm.real_counts == counts.tolist() and bm.inertia == kmeans["inertia"] and bm.converged_at == kmeans["converged_at"]
    # (a) fakes from every prototype: the model's record
    got_all = bm.between(torch.from_numpy(x_all).to(DEV))
    same_record(got_all, want_all)
    assert json.loads(json.dumps(got_all)) == got_all and got_all["baseline"]["ndb"] == baseline["ndb"]
    # (b) six prototypes are never drawn
    got_some = bm.between(torch.from_numpy(x_some).to(DEV))
    same_record(got_some, want_some)
    assert got_some["fake_counts"][10:] == [0] * 6 and all(got_some["different"][10:]) and sorted(got_some["order"][:6]) == list(range(10, 16))
    assert got_some["missing"] == 6
    # (c) a sample that holds a NaN falls into no bin
    x_nan = x_all.copy()
    x_nan[5, 1, 3, 3] = np.nan
    got_nan = bm.between(torch.from_numpy(x_nan).to(DEV))
    same_record(got_nan, MM.record(NM.encode(x_nan), centres, counts, 0.05, kmeans, baseline))
    assert got_nan["nonfinite"] == 1 and sum(got_nan["fake_counts"]) == SAMPLES - 1 == sum(got_all["fake_counts"]) - 1 and got_nan["samples"] == SAMPLES
    # the picture: 16 centres in one row of 16, padding 2
    path = bm.save_picture(str(tmp_path / "modes.png"), got_some)
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n" and not os.path.exists(path + ".tmp")
    shown = bm.centre_images()
    assert tuple(shown.shape) == (16, 3, S6, S6) and np.array_equal(NM.encode(shown.cpu().numpy())[0], centres)
    # a store too small for the baseline; more images asked for than it holds
    small = BinnedModes(S=S6, bins=4, images=700, samples=200, iterations=2, seed=SEED, device=DEV).reference_from_store(DeviceImageStore(store, DEV))
    assert small.baseline is None and len(small.real_index) == 700 and small.between(torch.from_numpy(x_all).to(DEV))["baseline"] is None
    assert len(BinnedModes(S=S6, bins=4, images=5000, samples=8, iterations=1, seed=SEED, device=DEV).reference_from_store(DeviceImageStore(store, DEV)).real_index) == 800


# ---- 7. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) ---------------------
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
    if "bm" not in _CACHE:
        from locate_amd import BinnedModes, DeviceImageStore
        _CACHE["bm"] = BinnedModes(S=32, bins=4, images=16, samples=8, iterations=3, seed=4, chunk=8, device=DEV).reference_from_store(DeviceImageStore(STORE, DEV))
    return _CACHE["bm"]


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
                bm = small_metric()
                values = [bm.evaluate(G), bm.evaluate(G)]
                assert G.training
        return training_state(G, D, step), losses, values

    plain, plain_losses, _ = run(False)
    watched, losses, values = run(True)
    assert sorted(plain) == sorted(watched)
    bad = [k for k in plain if not torch.equal(plain[k], watched[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain_losses, losses))
    assert values[0] == values[1] and values[0]["samples"] == 8 and sum(values[0]["fake_counts"]) + values[0]["nonfinite"] == 8
    assert values[0]["baseline"] is not None and sum(values[0]["real_counts"]) == 16
