"""The run statistics on the MI355X: the kernel through the raw C ABI against the model (tests/helpers/stats_model.py) - every size
class, both alignments, denormals, squares that overflow fp32, NaN and Inf at the places where a chunk's code paths change, guards
around every buffer, the same bits from call to call and from table to table - and `RunStatistics` around a running training: it
reports what the model says of the weights and gradients the step left, leaves the trajectory where a run without it would be,
and stops a poisoned run before its last good state is overwritten."""
import ctypes
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stats_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
GUARD = 32                           # sentinel words on either side of every buffer
SENTINEL = 0x7FC0DEAD                # as int32: a NaN with a payload of its own - a read past a tensor's end would be counted
SENTINEL64 = 0x5EAD5EAD5EAD5EAD      # around the outputs
CHUNK = 4096


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


class Arena:
    """float32 tensors inside ONE allocation, each between sentinel guards, each at a chosen offset (in elements) from a 16-byte
    boundary; the whole allocation is compared afterwards, so a write anywhere is seen"""

    def __init__(self):
        self.words, self.spans, self.size = [], [], 0

    def add(self, values, offset):
        assert self.size % 4 == 0 and 0 <= offset < 4
        values = np.ascontiguousarray(values, dtype=np.float32).view(np.int32)
        start = self.size + GUARD + offset
        total = -(-(GUARD + offset + values.size + GUARD) // 4) * 4
        piece = np.full(total, SENTINEL, dtype=np.int32)
        piece[GUARD + offset:GUARD + offset + values.size] = values
        self.words.append(piece)
        self.spans.append((start, values.size))
        self.size += total
        return len(self.spans) - 1

    def host(self):
        return np.concatenate(self.words)

    def upload(self):
        self.dev = torch.from_numpy(self.host()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.spans[i][0]

    def view(self, i):
        start, n = self.spans[i]
        return self.dev.view(torch.float32)[start:start + n]

    def values(self, i):
        start, n = self.spans[i]
        return self.host()[start:start + n].view(np.float32)

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host())


def reduce_raw(tensors):
    """tensors: [(device address, n), ...], none empty.  One call of locate_stats_reduce with guarded outputs and a guarded
    workspace; returns the raw int64 [n, 2] records and the summary (total, first)."""
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_stats_tensor_record_bytes() == 24 and L.locate_stats_record_bytes() == 16 and L.locate_stats_chunk_elems() == CHUNK
    rec, chunks = bytearray(), []
    for i, (address, n) in enumerate(tensors):
        rec += struct.pack("<Qqi4x", address, n, len(chunks))
        chunks.extend((i, c) for c in range(-(-n // CHUNK)))
    assert L.locate_stats_workspace_bytes(len(chunks)) == 16 * len(chunks)
    t_dev = torch.frombuffer(rec, dtype=torch.uint8).clone().to(DEV)
    c_dev = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(DEV)
    k = len(tensors)
    out = torch.full((GUARD + 1 + k + GUARD, 2), SENTINEL64, dtype=torch.int64, device=DEV)          # guards | summary | records | guards
    ws = torch.full((GUARD + len(chunks) + GUARD, 2), SENTINEL64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    check(L.locate_stats_reduce(p(t_dev), p(c_dev), k, len(chunks), p(out[GUARD + 1]), p(out[GUARD]), p(ws[GUARD]),
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_stats_reduce")
    torch.cuda.synchronize()
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    assert (out[:GUARD] == SENTINEL64).all() and (out[GUARD + 1 + k:] == SENTINEL64).all(), "a guard around the records was written"
    assert out[GUARD, 1] == SENTINEL64, "the summary is 8 bytes"
    assert (ws[:GUARD] == SENTINEL64).all() and (ws[GUARD + len(chunks):] == SENTINEL64).all(), "a guard around the workspace was written"
    total, first = np.ascontiguousarray(out[GUARD, :1]).view(np.uint32)[0], np.ascontiguousarray(out[GUARD, :1]).view(np.int32)[1]
    return out[GUARD + 1:GUARD + 1 + k].copy(), (int(total), int(first))


def decode(words):
    from locate_amd.stats import _decode
    return _decode(words)


def normals(rng, n):
    """mixed signs, magnitudes over 40 binades"""
    return (rng.standard_normal(n) * 2.0 ** rng.uniform(-20, 20, size=n)).astype(np.float32)


SIZES = [1, 3, 4, 5, 255, 4095, 4096, 4097, 8193, 3 * 4096 + 2]
POS_NAN, NEG_NAN = f32([0x7FC12345])[0], f32([0xFFC00001])[0]


def contents(rng):
    """[(what, values)], the finite ones first"""
    cases = [("normals %d" % n, normals(rng, n)) for n in SIZES]
    sub = rng.integers(1, 0x800000, size=4099, dtype=np.int64) | (rng.integers(0, 2, size=4099, dtype=np.int64) << 31)
    cases.append(("all denormal", sub.astype(np.uint32).view(np.float32)))
    cases.append(("zeros of both signs", f32([0x00000000, 0x80000000] * 130 + [0x80000000])))
    big = (10.0 ** rng.uniform(19, 38.47, size=4097) * rng.choice([-1.0, 1.0], size=4097)).astype(np.float32)
    big[-1], big[17] = np.float32(3e38), -np.float32(1e19)
    cases.append(("squares overflow fp32", big))
    cases.append(("small integers", rng.integers(-8, 9, size=8193).astype(np.float32)))
    n_finite = len(cases)
    x = normals(rng, 4097)
    x[0] = np.inf
    cases.append(("+Inf first", x))
    x = normals(rng, 8193)
    x[4096 + 2000] = -np.inf
    cases.append(("-Inf inside a full chunk", x))
    x = normals(rng, 3 * 4096 + 2)
    x[-1], x[4096] = NEG_NAN, POS_NAN
    cases.append(("NaN last of a tail chunk and first of a chunk", x))
    x = normals(rng, 4097)
    x[-1] = POS_NAN
    cases.append(("NaN alone in a tail chunk", x))
    x = normals(rng, 5)
    x[-1], x[0] = NEG_NAN, np.inf
    cases.append(("NaN last of five", x))
    cases.append(("all NaN", np.tile(f32([0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]), 66)[:261]))
    return cases, n_finite


def test_kernel_against_the_model():
    from locate_amd import tensor_statistics
    rng = np.random.default_rng(21)
    cases, n_finite = contents(rng)
    arena, what = Arena(), []
    for name, values in cases:          # each once at a 16-byte-aligned base, once one element past one
        for offset in (0, 1):
            arena.add(values, offset)
            what.append("%s, offset %d" % (name, offset))
    others = Arena()
    for n in (7, 4096, 5000, 1, 12289):
        others.add(normals(rng, n), int(rng.integers(0, 4)))
    arena.upload()
    others.upload()
    k = len(what)
    table = [(arena.ptr(i), arena.spans[i][1]) for i in range(k)]
    words, (total, first) = reduce_raw(table)
    sumsq, absmax, nonfinite = decode(words)
    want = [M.statistics(arena.values(i)) for i in range(k)]
    for i in range(k):
        n = arena.spans[i][1]
        w_sumsq, w_absmax, w_nonfinite = want[i]
        rel = abs(sumsq[i] - w_sumsq) / w_sumsq if w_sumsq else float(sumsq[i] != 0.0)
        print("%-56s n %6d  sumsq %.17g  model %.17g  rel %.3g (bound %.3g)  absmax %.9g  nonfinite %d"
              % (what[i], n, sumsq[i], w_sumsq, rel, M.sumsq_tolerance(n), absmax[i], nonfinite[i]))
        assert nonfinite[i] == w_nonfinite, what[i]
        assert absmax[i:i + 1].view(np.uint32)[0] == np.array([w_absmax]).view(np.uint32)[0], what[i]
        assert M.sumsq_close(float(sumsq[i]), w_sumsq, n), what[i]
    by_name = {w: i for i, w in enumerate(what)}
    for offset in (0, 1):
        i = by_name["all NaN, offset %d" % offset]
        assert (sumsq[i], absmax[i], nonfinite[i]) == (0.0, 0.0, 261) and words[i, 0] == 0          # +0.0, not -0.0
        i = by_name["zeros of both signs, offset %d" % offset]
        assert (sumsq[i], absmax[i], nonfinite[i]) == (0.0, 0.0, 0) and words[i, 0] == 0
        i = by_name["small integers, offset %d" % offset]
        assert sumsq[i] == float((arena.values(i).astype(np.float64) ** 2).sum()) and sumsq[i] == want[i][0] and sumsq[i] > 1e4
        i = by_name["all denormal, offset %d" % offset]
        assert 0.0 < absmax[i] < 1.1754944e-38 and 0.0 < sumsq[i] < 1e-70          # denormals are not flushed
        i = by_name["squares overflow fp32, offset %d" % offset]
        assert absmax[i] == np.float32(3e38) and sumsq[i] > 3.4e38
        i = by_name["+Inf first, offset %d" % offset]
        assert nonfinite[i] == 1 and np.isfinite(absmax[i]) and np.isfinite(sumsq[i])          # the Inf is left out of both
    # the same contents at the two alignments: the same record
    for i in range(0, k, 2):
        assert np.array_equal(words[i], words[i + 1]), what[i]
    # the summary
    assert total == sum(w[2] for w in want) and first == 2 * n_finite and total > 500
    finite_only, summary = reduce_raw(table[:2 * n_finite])
    assert summary == (0, -1) and np.array_equal(finite_only, words[:2 * n_finite])
    # the sources and their guards are as they were
    assert arena.untouched() and others.untouched()
    # a second call: the same bits
    again, summary_again = reduce_raw(table)
    assert np.array_equal(again, words) and summary_again == (total, first)
    # the same tensors in reverse order, interleaved with others: every tensor keeps its bits
    mixed, where = [], {}
    for j, i in enumerate(reversed(range(k))):
        where[i] = len(mixed)
        mixed.append(table[i])
        if j % 3 == 0:
            o = (j // 3) % len(others.spans)
            mixed.append((others.ptr(o), others.spans[o][1]))
    words2, (total2, first2) = reduce_raw(mixed)
    for i in range(k):
        assert np.array_equal(words2[where[i]], words[i]), what[i]
    assert total2 == total and first2 == 0          # the all-NaN tensor leads that table
    assert arena.untouched() and others.untouched()
    # the public entry: the same records, a zero-element tensor skipped (and reported as zeros)
    views = [arena.view(i) for i in range(k)]
    empty = arena.dev.view(torch.float32)[5:5]
    s, a, c = tensor_statistics(views[:3] + [empty] + views[3:])
    assert s.is_cuda and a.is_cuda and c.is_cuda and (s.dtype, a.dtype, c.dtype) == (torch.float64, torch.float32, torch.int64)
    s, a, c = s.cpu().numpy(), a.cpu().numpy(), c.cpu().numpy()
    assert (s[3], a[3], c[3]) == (0.0, 0.0, 0)
    keep = [j for j in range(k + 1) if j != 3]
    assert np.array_equal(s[keep].view(np.int64), sumsq.view(np.int64)) and np.array_equal(a[keep].view(np.int32), absmax.view(np.int32))
    assert np.array_equal(c[keep], nonfinite.astype(np.int64))
    s1, a1, c1 = tensor_statistics([empty])
    assert (float(s1[0]), float(a1[0]), int(c1[0])) == (0.0, 0.0, 0)
    assert arena.untouched()


def test_more_chunks_than_the_largest_grid():
    from locate_amd._lib import lib
    cap = lib().locate_stats_max_blocks()
    assert 0 < cap <= 4096
    n = (cap + 3) * CHUNK + 5
    buf = torch.ones(GUARD + n + GUARD, dtype=torch.float32, device=DEV)
    flat = buf.view(torch.int32)
    flat[:GUARD] = SENTINEL
    flat[GUARD + n:] = SENTINEL
    x = buf[GUARD:GUARD + n]
    two, nan, huge = (cap + 1) * CHUNK + 7, (cap + 2) * CHUNK + 4095, n - 1          # all beyond the first grid-stride round
    x[two] = 2.0
    x[nan] = float("nan")
    x[huge] = 1e30
    table = [(x.data_ptr(), n)]
    words, summary = reduce_raw(table)
    sumsq, absmax, nonfinite = decode(words)
    want = math.fsum([float(n - 3), 4.0, float(np.float32(1e30)) ** 2])          # n - 3 ones, one 2.0, one 1e30: the terms are exact
    print("n %d  sumsq %.17g  model %.17g  rel %.3g (bound %.3g)" % (n, sumsq[0], want, abs(sumsq[0] - want) / want, M.sumsq_tolerance(n)))
    assert nonfinite[0] == 1 and summary == (1, 0) and absmax[0] == np.float32(1e30)
    assert M.sumsq_close(float(sumsq[0]), want, n)
    x[huge] = 1.0
    words, summary = reduce_raw(table)
    sumsq, absmax, nonfinite = decode(words)
    assert nonfinite[0] == 1 and summary == (1, 0) and absmax[0] == 2.0
    assert sumsq[0] == float(n + 2)          # n - 2 ones and one 4: every partial sum is an integer below 2^53
    again, _ = reduce_raw(table)
    assert np.array_equal(again, words)
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    assert int((host[GUARD:GUARD + n] != np.array([1.0], np.float32).view(np.int32)[0]).sum()) == 2          # the tensor was only read


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    for args in ((None, p, 1, 1, p, p, p), (p, None, 1, 1, p, p, p), (p, p, 0, 1, p, p, p), (p, p, 1, 0, p, p, p), (p, p, -1, 1, p, p, p),
                 (p, p, 1, 1, None, p, p), (p, p, 1, 1, p, None, p), (p, p, 1, 1, p, p, None), (p, p, 1, 1, odd, p, p), (p, p, 1, 1, p, p, odd)):
        assert L.locate_stats_reduce(*args, None) == 1
        assert b"locate_stats_reduce" in L.locate_last_error()
    torch.cuda.synchronize()
    assert not buf.any()          # nothing was launched


# ---- beside a training run: the tiny fixture network of tests/test_gpu_average.py (32 x 32, base width 1, batch 8) -----------------
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


def host_entries(G, D):
    """what a record taken now should describe: host copies of every parameter and of every gradient there is, in entry order"""
    torch.cuda.synchronize()
    out = {}
    for tag, net in (("G", G), ("D", D)):
        for name, p in net.named_parameters():
            out["%s/%s" % (tag, name)] = p.detach().cpu().numpy().copy()
            if p.grad is not None:
                out["%s/%s.grad" % (tag, name)] = p.grad.detach().cpu().numpy().copy()
    return out


@pytest.mark.parametrize("launch_mode", ["eager", "graphed"])
def test_records_beside_a_training_run(launch_mode):
    from locate_amd import NonFiniteError, RunStatistics
    from locate_amd.graph import GraphedTrainStep

    def run(recorded):
        G, D, step, (lat, real, aug) = build_tiny()
        stats = RunStatistics(G, D, capacity=4) if recorded else None          # a ring shorter than the run: it flushes itself
        snaps = []
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch_mode == "graphed" else None
        for i in range(1, 7):
            if runner is not None:
                runner.replay()
            else:
                step(lat, real, aug)
            if recorded:
                snaps.append(host_entries(G, D))
                stats.record(i)
        return training_state(G, D, step), stats, snaps, (G, D)

    plain, _, _, _ = run(False)
    followed, stats, snaps, (G, D) = run(True)
    # (a) the training is where it would be without the records
    assert sorted(plain) == sorted(followed)
    bad = [k for k in plain if not torch.equal(plain[k], followed[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch_mode, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain) and any("/opt/" in k for k in plain)
    # (b) every record is the model applied to the weights and gradients at that point
    assert len(stats.rows) == 4          # the full ring was read when the fifth record came
    stats.flush()
    rows = list(stats.rows)
    assert [r["iteration"] for r in rows] == [1, 2, 3, 4, 5, 6] and stats.last_iteration == 6
    for row, snap in zip(rows, snaps):
        assert list(row["names"]) == list(snap)
        assert row["total"] == 0 and row["first"] == -1 and not row["nonfinite"].any()
        for j, name in enumerate(row["names"]):
            w_sumsq, w_absmax, w_nonfinite = M.statistics(snap[name])
            assert w_nonfinite == 0
            assert row["absmax"][j:j + 1].view(np.uint32)[0] == np.array([w_absmax]).view(np.uint32)[0], (launch_mode, row["iteration"], name)
            assert M.sumsq_close(float(row["sumsq"][j]), w_sumsq, snap[name].size), (launch_mode, row["iteration"], name, row["sumsq"][j], w_sumsq)
    names = list(rows[-1]["names"])
    want = []
    for tag, net in (("G", G), ("D", D)):
        for n, p in net.named_parameters():
            want += ["%s/%s" % (tag, n)] + (["%s/%s.grad" % (tag, n)] if p.grad is not None else [])
    assert names == want and names == stats.entry_names() == stats.names
    plain_names = [n for n in names if not n.endswith(".grad")]
    assert plain_names == ["G/" + n for n, _ in G.named_parameters()] + ["D/" + n for n, _ in D.named_parameters()]
    unused = [n for n, p in G.named_parameters() if p.grad is None]
    print("%s: %d entries, %d of them gradients; %d generator parameters without one" % (launch_mode, len(names), len(names) - len(plain_names), len(unused)))
    assert len([n for n in unused if n.endswith("i_norm.weight")]) == 6 and not any("G/%s.grad" % n in names for n in unused)
    first, last = (dict(zip(r["names"], r["sumsq"])) for r in (rows[0], rows[-1]))
    changed = sum(int(first[n] != last[n]) for n in first if n in last)
    assert changed >= 10, "the training did not move the weights: nothing was tested"
    norms = stats.global_norms()
    assert len(norms) == 6 and all(v > 0 and np.isfinite(v) for r in norms for v in r.values())
    assert stats.check() is stats
    # (c) a NaN in one element of one discriminator weight
    name, weight = next((n, p) for n, p in D.named_parameters() if n.endswith("weight_bar") and p.numel() > 16)
    with torch.no_grad():
        weight.view(-1)[11] = float("nan")
    stats.record(7)
    with pytest.raises(NonFiniteError) as info:
        stats.check()
    assert info.value.iteration == 7 and info.value.tensors == [("D/" + name, 1)] and ("D/" + name) in str(info.value)
    assert len(stats.rows) == 7 and all(a is b for a, b in zip(stats.rows, rows)) and stats.rows[6]["total"] == 1          # the six are kept
    assert stats.rows[6]["first"] == names.index("D/" + name)
    assert stats.flush() == [] and stats.check() is stats          # raised once


def test_trainer_and_resume(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, NonFiniteError, RunStatistics, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, recorded=True):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        stats = RunStatistics(G, D) if recorded else None
        return Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                       subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, stats=stats, stats_every=2)

    def files(out):
        return sorted(os.path.relpath(os.path.join(d, f), str(out)) for d, _, fs in os.walk(str(out)) for f in fs)

    out = tmp_path / "on"
    t = trainer(out, 4)
    assert t.run() == 4
    assert t.stats.last_iteration == 4 and t.stats.rows == []          # an epoch's records leave with its file
    with np.load(str(out / "error" / "1-stats.npz")) as z:
        assert z["iterations"].tolist() == [2, 4] and z["sumsq"].shape == (2, len(z["names"])) and not z["nonfinite"].any()
        assert z["names"].tolist() == t.stats.entry_names() and np.isfinite(z["sumsq"]).all() and (z["absmax"] > 0).any()
    plain = trainer(tmp_path / "off", 4, recorded=False)
    assert plain.run() == 4
    assert [f for f in files(out) if f != os.path.join("error", "1-stats.npz")] == files(tmp_path / "off")
    assert os.path.join(str(out), "error", "1-stats.npz") in t.written
    for name in ("netG.torch", "netD.torch", "trainer.torch"):          # and the run itself is the run without records
        a, b = (torch.load(str(folder / name), map_location="cpu", weights_only=True) for folder in (out, tmp_path / "off"))
        if name != "trainer.torch":
            assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a), name
        else:
            assert sorted(a) == sorted(b)

    def content(name):
        with open(str(out / name), "rb") as f:
            return f.read()
    before = {name: content(name) for name in ("trainer.torch", "netD.torch", "netG.torch")}
    pname, weight = next((n, p) for n, p in t.dis.named_parameters() if n.endswith("weight_bar") and p.numel() > 16)
    with torch.no_grad():
        weight.view(-1)[5] = float("nan")
    t.max_iterations = 8
    with pytest.raises(NonFiniteError) as info:
        t.run()
    assert info.value.iteration == 6 and ("D/" + pname) in [n for n, _ in info.value.tensors]
    assert {name: content(name) for name in before} == before          # the last good save, byte for byte
    with open(str(out / "error" / "nonfinite.json")) as f:
        report = json.load(f)
    assert sorted(report) == ["epoch", "iteration", "tensors"] and report["iteration"] == 6 and report["epoch"] == 2
    assert ("D/" + pname) in [n for n, _ in report["tensors"]] and all(c > 0 for _, c in report["tensors"])
    assert not os.path.exists(str(out / "error" / "2-stats.npz"))
    fresh = trainer(out, 8)
    assert fresh.resume().iterations == 4
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for net in (fresh.gen, fresh.dis) for p in net.parameters())


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--stats-every", "2", "--max-iterations", "4"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    with np.load(os.path.join(out, "error", "1-stats.npz")) as z:
        assert z["iterations"].tolist() == [2, 4] and not z["nonfinite"].any() and z["sumsq"].shape[1] == len(z["names"]) > 100
        assert any(n.endswith(".grad") for n in z["names"].tolist())
    assert not os.path.exists(os.path.join(out, "error", "nonfinite.json"))
