"""The run dynamics on the MI355X: the delta kernel through the raw C ABI against the model (tests/helpers/dynamics_model.py) - every
size class, the alignments, denormal and infinite deltas, NaN on either side, guards around every buffer, the three modes, the same
bits from call to call and from table to table - the shadow power iterations against the training's own kernels and against an
SVD, and `RunDynamics` around a running training: it reports what the model says of the weights before and after an iteration and
leaves the trajectory where a run without it would be."""
import ctypes
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dynamics_model as M  # noqa: E402
import test_gpu_stats as S  # noqa: E402  (the guarded arena and the tiny training set-up)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, SENTINEL, SENTINEL64, CHUNK = S.GUARD, S.SENTINEL, S.SENTINEL64, S.CHUNK
SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 8193, 3 * 4096 + 2]
POS_NAN, NEG_NAN = S.POS_NAN, S.NEG_NAN
f32 = S.f32


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def pass_raw(tensors, mode, null_outputs=False):
    """tensors: [(address of w, address of base, n), ...], none empty.  One call of locate_dyn_pass with guarded records and a
    guarded workspace; returns the raw int64 [n, 4] records - all sentinels when the mode writes none."""
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_dyn_tensor_record_bytes() == 32 and L.locate_dyn_record_bytes() == 32 and L.locate_dyn_chunk_elems() == CHUNK
    rec, chunks = bytearray(), []
    for i, (w, base, n) in enumerate(tensors):
        rec += struct.pack("<QQqi4x", w, base, n, len(chunks))
        chunks.extend((i, c) for c in range(-(-n // CHUNK)))
    assert L.locate_dyn_workspace_bytes(len(chunks)) == 32 * len(chunks) and L.locate_dyn_workspace_bytes(0) == 0
    t_dev = torch.frombuffer(rec, dtype=torch.uint8).clone().to(DEV)
    c_dev = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(DEV)
    k = len(tensors)
    out = torch.full((GUARD + k + GUARD, 4), SENTINEL64, dtype=torch.int64, device=DEV)          # guards | records | guards
    ws = torch.full((GUARD + len(chunks) + GUARD, 4), SENTINEL64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    check(L.locate_dyn_pass(p(t_dev), p(c_dev), k, len(chunks), mode, None if null_outputs else p(out[GUARD]),
                            None if null_outputs else p(ws[GUARD]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_dyn_pass")
    torch.cuda.synchronize()
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (out[:GUARD] == SENTINEL64).all() and (out[GUARD + k:] == SENTINEL64).all(), "a guard around the records was written"
    assert (ws[:GUARD] == SENTINEL64).all() and (ws[GUARD + len(chunks):] == SENTINEL64).all(), "a guard around the workspace was written"
    if not mode & 1:
        assert (out == SENTINEL64).all() and (ws == SENTINEL64).all(), "a rebase wrote a record"
    return out[GUARD:GUARD + k].copy()


def decode(words):
    from locate_amd.dynamics import _decode
    return _decode(words)


def bits32(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def last_bits(rng, w, spread=3):
    """w with its bit patterns moved by up to `spread` units in the last place (never across zero: w holds normals)"""
    moved = w.view(np.int32) + rng.integers(-spread, spread + 1, size=w.size, dtype=np.int32)
    return moved.view(np.float32).copy()


def contents(rng):
    """[(what, w, base)]"""
    cases = []
    for n in SIZES:
        w = S.normals(rng, n)
        cases.append(("normals %d" % n, w, last_bits(rng, w)))
    w = S.normals(rng, 4097)
    cases.append(("base == w", w, w.copy()))
    zeros = f32([0x00000000, 0x80000000] * 130 + [0x80000000])
    cases.append(("zeros of both signs", zeros, f32([0x80000000, 0x80000000, 0x00000000, 0x00000000] * 65 + [0x00000000])))
    low = rng.integers(0x00800000, 0x00800000 + 1000, size=4099, dtype=np.int64) | (rng.integers(0, 2, size=4099, dtype=np.int64) << 31)
    w = low.astype(np.uint32).view(np.float32)
    cases.append(("denormal deltas", w, (low + rng.integers(1, 50, size=4099)).astype(np.uint32).view(np.float32)))
    w, base = S.normals(rng, 4097), None
    base = last_bits(rng, w)
    for at in (0, 2000, 4096):
        w[at], base[at] = np.float32(3e38), np.float32(-3e38)
    cases.append(("finite operands, infinite delta", w, base))
    w = S.normals(rng, 8193)
    base = last_bits(rng, w)
    w[4096 + 2000] = base[4096 + 2000] = np.inf
    w[5], base[5] = -np.inf, -np.inf
    w[6], base[6] = np.inf, -np.inf
    cases.append(("Inf - Inf", w, base))
    w = S.normals(rng, 3 * 4096 + 2)
    base = last_bits(rng, w)
    w[-1], w[4096] = NEG_NAN, POS_NAN
    cases.append(("NaN in w, last of a tail chunk and first of a chunk", w, base))
    w = S.normals(rng, 4097)
    base = last_bits(rng, w)
    base[-1], base[17] = POS_NAN, NEG_NAN
    cases.append(("NaN in base, alone in a tail chunk", w, base))
    w = np.tile(f32([0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]), 66)[:261]
    cases.append(("all NaN on both sides", w, w.copy()))
    return cases


ALIGNMENTS = ((0, 0), (1, 0), (0, 3))          # offsets of (w, base) from a 16-byte boundary, in elements


def arenas(cases):
    """the live tensors and their bases, each case at every alignment: two guarded allocations"""
    live, base, what = S.Arena(), S.Arena(), []
    for name, w, b in cases:
        for ow, ob in ALIGNMENTS:
            live.add(w, ow)
            base.add(b, ob)
            what.append("%s, offsets %d/%d" % (name, ow, ob))
    return live.upload(), base.upload(), what


def rebased(live, base):
    """the words of the whole base allocation after a rebase: every slot holds its tensor's bits, every guard its sentinel"""
    want = base.host().copy()
    for i, (start, n) in enumerate(base.spans):
        want[start:start + n] = live.values(i).view(np.int32)
    return want


def check_records(words, live, base, what):
    got = decode(words)
    for i in range(len(what)):
        n = live.spans[i][1]
        w_dsq, w_bsq, w_absmax, w_same, w_bad = M.delta_record(live.values(i), base.values(i))
        print("%-70s n %6d  delta_sumsq %.17g (model %.17g)  base_sumsq %.17g (model %.17g)  bound %.3g  absmax %.9g  unchanged %d  nonfinite %d"
              % (what[i], n, got[0][i], w_dsq, got[1][i], w_bsq, M.sumsq_tolerance(n), got[2][i], got[3][i], got[4][i]))
        assert (int(got[3][i]), int(got[4][i])) == (w_same, w_bad), what[i]
        assert bits32(got[2][i]) == bits32(w_absmax), what[i]
        assert M.sums_close(float(got[0][i]), w_dsq, n) and M.sums_close(float(got[1][i]), w_bsq, n), what[i]
        assert words[i, 3] >> 32 == 0, what[i]          # pad
    return got


def test_kernel_against_the_model():
    rng = np.random.default_rng(33)
    cases = contents(rng)
    live, base, what = arenas(cases)
    others, other_bases = S.Arena(), S.Arena()
    for n in (7, 4096, 5000, 1, 12289):
        others.add(S.normals(rng, n), int(rng.integers(0, 4)))
        other_bases.add(S.normals(rng, n), int(rng.integers(0, 4)))
    others.upload()
    other_bases.upload()
    k = len(what)
    table = [(live.ptr(i), base.ptr(i), live.spans[i][1]) for i in range(k)]
    # ---- mode 1: the records, and nothing else is written
    words = pass_raw(table, 1)
    dsq, bsq, absmax, same, bad = check_records(words, live, base, what)
    assert live.untouched() and base.untouched()
    by_name = {w: i for i, w in enumerate(what)}
    for offsets in ALIGNMENTS:
        tail = ", offsets %d/%d" % offsets
        i = by_name["base == w" + tail]
        assert (dsq[i], absmax[i], same[i], bad[i]) == (0.0, 0.0, 4097, 0) and words[i, 0] == 0 and bsq[i] > 0          # +0.0, not -0.0
        i = by_name["zeros of both signs" + tail]
        assert (dsq[i], bsq[i], absmax[i], same[i], bad[i]) == (0.0, 0.0, 0.0, 261, 0) and words[i, 0] == 0 and words[i, 1] == 0
        i = by_name["denormal deltas" + tail]
        assert 0.0 < absmax[i] < 1.1754944e-38 and 0.0 < dsq[i] < 1e-70 and same[i] == 0          # denormals are not flushed
        i = by_name["finite operands, infinite delta" + tail]
        assert bad[i] == 3 and np.isfinite(dsq[i]) and np.isfinite(absmax[i]) and bsq[i] > 2.6e77          # the base's own 3e38 are summed
        i = by_name["Inf - Inf" + tail]
        assert bad[i] == 3 and np.isfinite(bsq[i]) and same[i] >= 2          # Inf == Inf, though Inf - Inf is NaN
        i = by_name["NaN in w, last of a tail chunk and first of a chunk" + tail]
        assert bad[i] == 2
        i = by_name["NaN in base, alone in a tail chunk" + tail]
        assert bad[i] == 2
        i = by_name["all NaN on both sides" + tail]
        assert (dsq[i], bsq[i], absmax[i], same[i], bad[i]) == (0.0, 0.0, 0.0, 0, 261) and words[i, 0] == 0 and words[i, 1] == 0
    # the same contents at every alignment: the same record
    for i in range(0, k, len(ALIGNMENTS)):
        for j in range(1, len(ALIGNMENTS)):
            assert np.array_equal(words[i], words[i + j]), what[i + j]
    # a second call: the same bits
    assert np.array_equal(pass_raw(table, 1), words)
    # the same tensors in reverse order, interleaved with others: every tensor keeps its bits
    mixed, where = [], {}
    for j, i in enumerate(reversed(range(k))):
        where[i] = len(mixed)
        mixed.append(table[i])
        if j % 3 == 0:
            o = (j // 3) % len(others.spans)
            mixed.append((others.ptr(o), other_bases.ptr(o), others.spans[o][1]))
    words2 = pass_raw(mixed, 1)
    for i in range(k):
        assert np.array_equal(words2[where[i]], words[i]), what[i]
    assert live.untouched() and base.untouched() and others.untouched() and other_bases.untouched()
    # ---- mode 3: mode 1's records of the base as it was, and the base becomes the tensor, bit for bit, inside its guards
    want_base = rebased(live, base)
    assert np.array_equal(pass_raw(table, 3), words)
    assert live.untouched() and np.array_equal(base.dev.cpu().numpy(), want_base)
    # ---- mode 2 on a fresh copy of the bases: the same arena, no record (pass_raw looks), also with null outputs
    for null_outputs in (False, True):
        base.upload()
        assert base.untouched()
        pass_raw(table2 := [(live.ptr(i), base.ptr(i), live.spans[i][1]) for i in range(k)], 2, null_outputs)
        assert live.untouched() and np.array_equal(base.dev.cpu().numpy(), want_base)
    # ---- mode 1 after the rebase: nothing has moved
    after = pass_raw(table2, 1)
    dsq, bsq, absmax, same, bad = decode(after)
    for i in range(k):
        w = live.values(i)
        nan = int(np.isnan(w).sum())
        assert (dsq[i], bits32(absmax[i]), int(same[i]), int(bad[i])) == (0.0, 0, w.size - nan, int((~np.isfinite(w)).sum())), what[i]
        assert after[i, 0] == 0 and M.sums_close(float(bsq[i]), M.delta_record(w, w)[1], w.size), what[i]
    assert np.array_equal(base.dev.cpu().numpy(), want_base)


def test_more_chunks_than_the_largest_grid():
    from locate_amd._lib import lib
    cap = lib().locate_dyn_max_blocks()
    assert 0 < cap <= 4096
    n = (cap + 3) * CHUNK + 5
    bufs = []
    for _ in range(2):
        buf = torch.ones(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
        flat = buf.view(torch.int32)
        flat[:GUARD] = SENTINEL
        flat[GUARD + n:] = SENTINEL
        bufs.append((buf, flat))
    w, base = bufs[0][0][GUARD:GUARD + n], bufs[1][0][GUARD:GUARD + n]
    two, nan, huge = (cap + 1) * CHUNK + 7, (cap + 2) * CHUNK + 4095, n - 1          # all beyond the first grid-stride round
    w[two] = 2.0
    w[nan] = float("nan")
    base[huge] = -1e30
    table = [(w.data_ptr(), base.data_ptr(), n)]
    before = [flat.cpu().numpy() for _, flat in bufs]
    words = pass_raw(table, 1)
    dsq, bsq, absmax, same, bad = decode(words)
    big = float(np.float32(1.0) - np.float32(-1e30))          # 1 + 1e30 in fp32
    want_d = math.fsum([1.0, big * big])          # the terms are exact
    want_b = math.fsum([float(n - 1), float(np.float32(-1e30)) ** 2])
    print("n %d  delta_sumsq %.17g (model %.17g)  base_sumsq %.17g (model %.17g)  bound %.3g" % (n, dsq[0], want_d, bsq[0], want_b, M.sumsq_tolerance(n)))
    assert (int(same[0]), int(bad[0])) == (n - 3, 1) and absmax[0] == np.float32(big)
    assert M.sums_close(float(dsq[0]), want_d, n) and M.sums_close(float(bsq[0]), want_b, n)
    assert all(np.array_equal(flat.cpu().numpy(), b) for (_, flat), b in zip(bufs, before))          # both were only read
    base[huge] = 1.0
    words = pass_raw(table, 1)
    dsq, bsq, absmax, same, bad = decode(words)
    assert (dsq[0], bsq[0], absmax[0], int(same[0]), int(bad[0])) == (1.0, float(n), 1.0, n - 2, 1)          # integers below 2^53: exact
    # both at once: the same record, and the base is the tensor
    assert np.array_equal(pass_raw(table, 3), words)
    torch.cuda.synchronize()
    host_w, host_b = (flat.cpu().numpy() for _, flat in bufs)
    assert np.array_equal(host_w, before[0]) and np.array_equal(host_b, host_w)          # guards included: both hold the sentinels there
    dsq, bsq, absmax, same, bad = decode(pass_raw(table, 1))
    assert (dsq[0], absmax[0], int(same[0]), int(bad[0])) == (0.0, 0.0, n - 1, 1) and bsq[0] == float(n + 2)          # n - 2 ones and one 4


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    for args in ((None, p, 1, 1, 1, p, p), (p, None, 1, 1, 1, p, p), (p, p, 0, 1, 1, p, p), (p, p, 1, 0, 1, p, p), (p, p, -1, 1, 1, p, p),
                 (p, p, 1, -1, 2, p, p), (p, p, 1, 1, 0, p, p), (p, p, 1, 1, 4, p, p), (p, p, 1, 1, -1, p, p),
                 (p, p, 1, 1, 1, None, p), (p, p, 1, 1, 1, p, None), (p, p, 1, 1, 3, None, p), (p, p, 1, 1, 3, p, None),
                 (p, p, 1, 1, 1, odd, p), (p, p, 1, 1, 1, p, odd), (p, p, 1, 1, 3, odd, p), (p, p, 1, 1, 3, p, odd),
                 (None, p, 1, 1, 2, None, None), (p, None, 1, 1, 2, None, None), (p, p, 0, 1, 2, None, None)):
        assert L.locate_dyn_pass(*args, None) == 1, args
        assert b"locate_dyn_pass" in L.locate_last_error()
    torch.cuda.synchronize()
    assert not buf.any()          # nothing was launched
    # a table whose entries are damaged - here all zeros: null tensors of no elements - launches and writes nothing
    out = torch.full((8, 4), SENTINEL64, dtype=torch.int64, device=DEV)
    for mode in (1, 2, 3):
        assert L.locate_dyn_pass(p, p, 1, 1, mode, ctypes.c_void_p(out[2].data_ptr()), ctypes.c_void_p(out[4].data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert not buf.any() and bool((out == SENTINEL64).all())


def test_tensor_deltas():
    from locate_amd import tensor_deltas
    rng = np.random.default_rng(34)
    cases = contents(rng)[6:]          # the larger sizes of normals and the special contents
    live, base, what = arenas(cases)
    k = len(what)
    words = pass_raw([(live.ptr(i), base.ptr(i), live.spans[i][1]) for i in range(k)], 1)
    dsq, bsq, absmax, same, bad = decode(words)
    ws, bs = [live.view(i) for i in range(k)], [base.view(i) for i in range(k)]
    empty = live.dev.view(torch.float32)[5:5]
    got = tensor_deltas(ws[:3] + [empty] + ws[3:], bs[:3] + [empty] + bs[3:])
    assert all(t.is_cuda for t in got)
    assert [t.dtype for t in got] == [torch.float64, torch.float64, torch.float32, torch.int64, torch.int64]
    g = [t.cpu().numpy() for t in got]
    assert [float(a[3]) for a in g] == [0.0] * 5          # the zero-element pair reports zeros
    keep = [j for j in range(k + 1) if j != 3]
    assert np.array_equal(g[0][keep].view(np.int64), dsq.view(np.int64)) and np.array_equal(g[1][keep].view(np.int64), bsq.view(np.int64))
    assert np.array_equal(g[2][keep].view(np.int32), absmax.view(np.int32))
    assert np.array_equal(g[3][keep], same.astype(np.int64)) and np.array_equal(g[4][keep], bad.astype(np.int64))
    alone = tensor_deltas([empty], [empty])
    assert [float(t[0]) for t in alone] == [0.0] * 5 and [tuple(t.shape) for t in alone] == [(1,)] * 5
    with pytest.raises(ValueError):
        tensor_deltas([ws[0]], [bs[len(ALIGNMENTS)]])          # sizes differ: 4096 against 4097
    with pytest.raises(TypeError):
        tensor_deltas([ws[0]], [bs[0].double()])
    with pytest.raises(TypeError):
        tensor_deltas([live.dev.view(torch.float32)[0:64:2]], [bs[0]])          # strided
    assert live.untouched() and base.untouched()


# ---- sigma ----------------------------------------------------------------------------------------------------------------------
def spectral_layers(*nets):
    from locate_amd import SpectralNorm
    return [m.module for net in nets for m in net.modules() if isinstance(m, SpectralNorm)]


def power_iteration_by_hand(layers):
    """one locate_sn_power_iter_batched over clones of (W_bar, u, v) of the layers, every buffer this function's own: sigma [n]"""
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_sn_table_record_bytes() == 80
    keep, buf, geometry = [], bytearray(), []
    sigma = torch.zeros(len(layers), 2, dtype=torch.float32, device=DEV)
    for i, m in enumerate(layers):
        w, u, v = (t.detach().clone() for t in (m.weight_bar, m.weight_u, m.weight_v))
        h = w.shape[0]
        wd = w.numel() // h
        nch = (h + 63) // 64
        wv, t, s, tpart = (torch.zeros(size, dtype=torch.float32, device=DEV) for size in (h, wd, h, nch * wd))
        keep += [w, u, v, wv, t, s, tpart]
        buf += struct.pack("<8Q4i", w.data_ptr(), u.data_ptr(), v.data_ptr(), sigma[i].data_ptr(), wv.data_ptr(), t.data_ptr(), s.data_ptr(),
                           tpart.data_ptr(), h, wd, nch, 0)
        geometry.append((h, wd))
    table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(DEV)
    check(L.locate_sn_power_iter_batched(ctypes.c_void_p(table.data_ptr()), len(layers), max(h for h, _ in geometry), max(wd for _, wd in geometry),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_sn_power_iter_batched")
    torch.cuda.synchronize()
    return sigma[:, 0].clone()


def test_sigma_train_is_what_a_forward_would_divide_by():
    from locate_amd import RunDynamics, ops
    G, D, step, (lat, real, aug) = S.build_tiny()
    for _ in range(2):          # u / v leave their initial values
        step(lat, real, aug)
    torch.cuda.synchronize()
    before = {"%s/%s" % (tag, n): p.detach().clone() for tag, net in (("G", G), ("D", D)) for n, p in net.named_parameters()}
    dyn = RunDynamics(G, D, capacity=2, sigma_rounds=2)
    dyn.mark().record(2)
    (row,) = dyn.flush()
    torch.cuda.synchronize()
    # every parameter of both networks - u and v among them - keeps its bits
    after = {"%s/%s" % (tag, n): p.detach() for tag, net in (("G", G), ("D", D)) for n, p in net.named_parameters()}
    changed = [n for n in before if not torch.equal(before[n].view(torch.int32), after[n].view(torch.int32))]
    assert not changed, changed[:4]
    layers = spectral_layers(G, D)
    assert list(row["layers"]) == dyn.layer_names() and len(row["layers"]) == len(layers) > 10
    by_hand = power_iteration_by_hand(layers)
    assert torch.equal(torch.from_numpy(row["sigma_train"]), by_hand.cpu())
    for i, m in enumerate(layers):
        u, v = m.weight_u.detach().clone(), m.weight_v.detach().clone()
        sigma, _ = ops.sn_power_iteration(m.weight_bar.detach().clone(), u, v)
        err = rel_err(row["sigma_train"][i:i + 1], sigma[:1].cpu())
        assert err <= 1e-6, (row["layers"][i], err)          # the project's bound for batched against per-layer (tests/test_gpu_ops.py)
    assert (row["sigma_train"] > 0).all() and (row["sigma_top"] >= row["sigma_train"] * np.float32(1 - 1e-5)).all()
    assert not row["delta_sumsq"].any() and not row["nonfinite"].any()          # nothing ran between mark() and record()
    assert row["unchanged"].tolist() == [p.numel() for _, p in dyn._parameters()]
    changed = [n for n in before if not torch.equal(before[n].view(torch.int32), after[n].view(torch.int32))]
    assert not changed, changed[:4]


class FourLayers(torch.nn.Module):
    def __init__(self):
        from locate_amd import SpectralNorm
        super().__init__()
        self.layers = torch.nn.ModuleList(SpectralNorm(torch.nn.Linear(40, 24)) for _ in M.FIXTURE_SEEDS)


def test_sigma_top_converges_to_the_top_singular_value():
    from locate_amd import RunDynamics
    torch.manual_seed(12)
    net = FourLayers()
    tops = []
    for sn, seed in zip(net.layers, M.FIXTURE_SEEDS):
        W, _ = M.sigma_fixture(seed)
        with torch.no_grad():
            sn.module.weight_bar.copy_(torch.from_numpy(W))
        tops.append(M.top_singular_value(W))
    net = net.to(DEV)
    dyn = RunDynamics(net, torch.nn.Module(), sigma_rounds=4)
    assert dyn.layer_names() == ["G/layers.%d.module.weight_bar" % i for i in range(4)]
    dyn.mark()
    for i in (1, 2, 3):
        dyn.record(i)
    rows = dyn.flush()
    for row in rows:
        print(row["iteration"], "sigma_train", row["sigma_train"].tolist(), "sigma_top", row["sigma_top"].tolist(), "svd", tops)
        assert (row["sigma_top"] >= row["sigma_train"] * np.float32(1 - 1e-5)).all()
        assert np.array_equal(row["sigma_train"], rows[0]["sigma_train"])          # the live u / v do not move here: the same bits every time
    # twelve rounds in all: the model alone is within 1e-9 (tests/test_dynamics_model.py); 1e-5 is the per-op fp32 bound of SURVEY 8(c)
    for got, want in zip(rows[2]["sigma_top"], tops):
        assert abs(float(got) - want) <= 1e-5 * want, (float(got), want)
    ratios = dyn.ratios()
    assert all((r["lipschitz"] >= 1 - 1e-5).all() for r in ratios)
    # reset_sigma(): the top set starts again from the live u / v, so one record repeats the first one
    dyn.reset_sigma().record(4)
    (again,) = dyn.flush()
    assert np.array_equal(again["sigma_top"], rows[0]["sigma_top"]) and np.array_equal(again["sigma_train"], rows[0]["sigma_train"])


# ---- beside a training run --------------------------------------------------------------------------------------------------------
def host_weights(G, D):
    torch.cuda.synchronize()
    return {"%s/%s" % (tag, n): p.detach().cpu().numpy().copy() for tag, net in (("G", G), ("D", D)) for n, p in net.named_parameters()}


@pytest.mark.parametrize("launch_mode", ["eager", "graphed"])
def test_records_beside_a_training_run(launch_mode):
    from locate_amd import RunDynamics
    from locate_amd.graph import GraphedTrainStep

    def run(recorded):
        G, D, step, (lat, real, aug) = S.build_tiny()
        dyn = RunDynamics(G, D, capacity=2) if recorded else None          # a ring shorter than the run: it flushes itself
        snaps, losses = [], []
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch_mode == "graphed" else None
        for i in range(1, 7):
            followed = recorded and i % 2 == 0
            if followed:
                before = host_weights(G, D)
                dyn.mark()
            out = runner.replay() if runner is not None else step(lat, real, aug)
            losses.append((out["d_error"].detach().clone(), out["g_error"].detach().clone()))
            if followed:
                snaps.append((before, host_weights(G, D)))
                dyn.record(i)
        return S.training_state(G, D, step), losses, dyn, snaps

    plain, plain_losses, _, _ = run(False)
    followed, losses, dyn, snaps = run(True)
    # (a) the training is where it would be without the records: weights, u / v, both optimizers' states, the losses
    assert sorted(plain) == sorted(followed)
    bad = [k for k in plain if not torch.equal(plain[k], followed[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch_mode, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain) and any("/opt/" in k for k in plain)
    assert len(losses) == 6 and all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(plain_losses, losses))
    # (b) every record is the model applied to the weights before and after its iteration
    assert len(dyn.rows) == 2          # the full ring was read when the third record came
    dyn.flush()
    rows = dyn.rows
    assert [r["iteration"] for r in rows] == [2, 4, 6] and dyn.last_iteration == 6
    moved = 0
    for row, (before, after) in zip(rows, snaps):
        assert list(row["names"]) == list(before) == dyn.entry_names()
        for j, name in enumerate(row["names"]):
            n = before[name].size
            w_dsq, w_bsq, w_absmax, w_same, w_bad = M.delta_record(after[name], before[name])
            where = (launch_mode, row["iteration"], name)
            assert (int(row["unchanged"][j]), int(row["nonfinite"][j])) == (w_same, w_bad) and w_bad == 0, where
            assert bits32(row["delta_absmax"][j]) == bits32(w_absmax), where
            assert M.sums_close(float(row["delta_sumsq"][j]), w_dsq, n) and M.sums_close(float(row["base_sumsq"][j]), w_bsq, n), where
            if name.endswith("weight_bar"):
                assert row["unchanged"][j] < n, where          # the step moved the layer
                moved += 1
    assert moved >= 3 * 10
    # (c) the ratios: finite and positive wherever a layer moved
    for r in dyn.ratios():
        bars = [j for j, name in enumerate(rows[0]["names"]) if name.endswith("weight_bar")]
        assert np.isfinite(r["update"][bars]).all() and (r["update"][bars] > 0).all()
        assert np.isfinite(r["G/update"]) and r["G/update"] > 0 and np.isfinite(r["D/update"]) and r["D/update"] > 0
        assert np.isfinite(r["lipschitz"]).all() and (r["lipschitz"] > 0).all()


def test_trainer_and_the_command_line(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, RunDynamics, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, recorded):
        G, D, step, _ = S.build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        extra = dict(dynamics=RunDynamics(G, D), dynamics_every=2) if recorded else {}
        return Trainer(step, pipeline, str(out), epochs=2, max_iterations=4, images=13, seed=3, miniter_function=lambda e: 1,
                       subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, **extra)

    def files(out):
        return sorted(os.path.relpath(os.path.join(d, f), str(out)) for d, _, fs in os.walk(str(out)) for f in fs)

    keys = ["D_update", "G_update", "base_sumsq", "delta_absmax", "delta_sumsq", "iterations", "layers", "lipschitz", "names", "nonfinite",
            "sigma_top", "sigma_train", "unchanged", "update"]

    def check_file(path, entries=None):
        with np.load(path) as z:
            assert sorted(z.files) == keys
            names, layers = z["names"].tolist(), z["layers"].tolist()
            assert z["iterations"].tolist() == [2, 4] and len(names) > 50 and len(layers) > 10
            assert entries is None or names == entries
            for key in ("delta_sumsq", "base_sumsq", "delta_absmax", "unchanged", "nonfinite", "update"):
                assert z[key].shape == (2, len(names)), key
            for key in ("sigma_train", "sigma_top", "lipschitz"):
                assert z[key].shape == (2, len(layers)), key
            assert z["G_update"].shape == z["D_update"].shape == (2,) and not z["nonfinite"].any()
            bars = [j for j, n in enumerate(names) if n.endswith("weight_bar")]
            assert layers == [names[j] for j in bars]
            assert np.isfinite(z["update"][:, bars]).all() and (z["update"][:, bars] > 0).all()
            assert np.isfinite(z["lipschitz"]).all() and (z["lipschitz"] > 0).all()
            assert np.isfinite(z["G_update"]).all() and np.isfinite(z["D_update"]).all()

    out = tmp_path / "on"
    t = trainer(out, True)
    assert t.run() == 4
    assert t.dynamics.last_iteration == 4 and t.dynamics.rows == []          # an epoch's records leave with its file
    check_file(str(out / "error" / "1-dynamics.npz"), t.dynamics.entry_names())
    assert os.path.join(str(out), "error", "1-dynamics.npz") in t.written
    plain = trainer(tmp_path / "off", False)
    assert plain.run() == 4 and plain.dynamics is None
    assert [f for f in files(out) if f != os.path.join("error", "1-dynamics.npz")] == files(tmp_path / "off")          # the parent's list
    assert not any("dynamics" in f for f in files(tmp_path / "off"))
    for name in ("netG.torch", "netD.torch"):          # and the run itself is the run without records
        a, b = (torch.load(str(folder / name), map_location="cpu", weights_only=True) for folder in (out, tmp_path / "off"))
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a), name
    a, b = (torch.load(str(folder / "trainer.torch"), map_location="cpu", weights_only=True) for folder in (out, tmp_path / "off"))
    assert sorted(a) == sorted(b)          # nothing of it goes into trainer.torch
    # the command line
    store_file = str(tmp_path / "store.npy")
    np.save(store_file, images)
    cli = str(tmp_path / "cli")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store_file, "--image-size", "32", "--batch", "8", "--out", cli, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--dynamics-every", "2", "--max-iterations", "4"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    check_file(os.path.join(cli, "error", "1-dynamics.npz"))
    assert not os.path.exists(os.path.join(cli, "error", "1-stats.npz"))
