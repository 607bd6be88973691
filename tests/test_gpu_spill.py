"""The snapshot's spill to disk on the MI355X (locate_amd/spill.py, csrc/digest.hip), bits compared as integers throughout, against
what is not the code under test: the numpy digest and the independent file reader of tests/helpers/spill_model.py at the operator
level - eagerly and inside a captured graph - and, in a run of the tiny fixture network, the uninterrupted run: a run that was
abandoned and continued from a spill file in fresh objects must continue the uninterrupted one bit for bit.  A crash is simulated
by abandoning the objects; no test kills a process."""
import ctypes
import functools
import json
import os
import shutil
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spill_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
CHUNK = 4096
SIZES = [0, 1, 3, 4095, 4096, 4097, 8193, 40000]
VIEW_N = 5001
SENTINEL = 0x5e471e15
PAD = 8          # sentinel words on either side: 32 bytes, so a tensor behind them is 16-byte aligned
SPECIALS = [0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001, 0x00000001, 0x807fffff, 0x80000000, 0x00000000, 0x7f7fffff]


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def as_i32(words):
    return T(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32))


def random_words(rng, n):
    """uint32 words: fp32 values over 16 binades with NaN, Inf, denormal and -0.0 bit patterns sprinkled in"""
    w = PM.words((rng.standard_normal(n) * 2.0 ** rng.uniform(-8, 8, size=n)).astype(np.float32)).copy()
    if n >= 3:
        at = rng.choice(n, size=min(n, len(SPECIALS)), replace=False)
        w[at] = np.array(SPECIALS, np.uint32)[:at.size]
    return w


class Pool:
    """tensors of given word counts, each inside a buffer of sentinel words; `lead` extra words put a tensor off the 16-byte grid"""

    def __init__(self, specs, seed):
        rng = np.random.default_rng(seed)
        self.buffers, self.tensors, self.host = [], [], []
        for n, dtype, lead in specs:
            buf = torch.full((PAD + lead + n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
            w = random_words(rng, n)
            view = buf[PAD + lead:PAD + lead + n]
            if n:
                view.copy_(as_i32(w))
            self.buffers.append(buf)
            self.tensors.append(view if dtype == torch.int32 else view.view(dtype))
            self.host.append(w)
            assert self.tensors[-1].is_contiguous() and (n == 0 or self.tensors[-1].data_ptr() % 16 == 4 * lead)

    def sentinels_intact(self):
        torch.cuda.synchronize()
        for buf, w in zip(self.buffers, self.host):
            lead = buf.numel() - w.size - 2 * PAD
            if not (bool((buf[:PAD + lead] == SENTINEL).all()) and bool((buf[PAD + lead + w.size:] == SENTINEL).all())):
                return False
            if w.size and not torch.equal(buf[PAD + lead:PAD + lead + w.size].cpu(), as_i32(w)):
                return False          # an input was written
        return True


def operator_pool(seed=1):
    return Pool([(n, torch.float32, 0) for n in SIZES] + [(VIEW_N, torch.float32, 1), (4, torch.float64, 0), (9, torch.int32, 0)], seed)


def guarded(n_words):
    """an int64 device array of n_words * 2 values inside sentinel values -> (buffer, the array)"""
    buf = torch.full((2 + 2 * n_words + 2,), SENTINEL, dtype=torch.int64, device=DEV)
    return buf, buf[2:2 + 2 * n_words]


def raw_digest(tensors, counts, order=None):
    """locate_digest through the C ABI over `tensors` in table order `order` -> (uint64 [n, 2] in the ORIGINAL order, intact?)"""
    from locate_amd._lib import lib
    L = lib()
    order = list(range(len(tensors))) if order is None else order
    rec = b"".join(struct.pack("<Qq", tensors[i].data_ptr() if counts[i] else 0, counts[i]) for i in order)
    pairs, first = [], []
    for k, i in enumerate(order):
        first.append(len(pairs))
        pairs += [(k, c) for c in range((counts[i] + CHUNK - 1) // CHUNK)]
    first.append(len(pairs))
    records = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(DEV)
    chunks = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(DEV)
    first_dev = torch.tensor(first, dtype=torch.int32).to(DEV)
    pbuf, partials = guarded(len(pairs))
    obuf, out = guarded(len(order))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    status = L.locate_digest(ptr(records), ptr(chunks), ptr(first_dev), len(order), len(pairs), ptr(partials), ptr(out),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0, L.locate_last_error()
    torch.cuda.synchronize()
    intact = all(int(b[0]) == int(b[1]) == int(b[-1]) == int(b[-2]) == SENTINEL for b in (pbuf, obuf))
    got = out.cpu().numpy().view(np.uint64).reshape(-1, 2)
    back = np.empty_like(got)
    back[order] = got
    return back, intact


def model_digests(host):
    return np.array([PM.digest(w) for w in host], dtype=np.uint64)


# ---- 1. the operator against the model -------------------------------------------------------------------------------------------
def test_digest_against_the_model():
    from locate_amd import digest_model, tensor_digests
    from locate_amd._lib import lib
    assert (lib().locate_digest_record_bytes(), lib().locate_digest_chunk_elems()) == (16, CHUNK)
    pool = operator_pool()
    counts = [w.size for w in pool.host]
    want = model_digests(pool.host)
    assert want[0].tolist() == [0, 0] and [digest_model(w) for w in pool.host] == [tuple(r) for r in want.tolist()]
    got, intact = raw_digest(pool.tensors, counts)
    assert intact and pool.sentinels_intact()
    assert np.array_equal(got, want), "tensors %s differ from the model" % np.nonzero((got != want).any(axis=1))[0].tolist()
    again, _ = raw_digest(pool.tensors, counts)
    assert np.array_equal(again, got)          # two calls, the same bits
    order = list(reversed(range(len(counts))))
    order = order[3:] + order[:3]
    moved, intact = raw_digest(pool.tensors, counts, order)          # another place in the table, another grid position
    assert intact and np.array_equal(moved, want)
    public = tensor_digests(pool.tensors)
    assert public.dtype == torch.uint64 and tuple(public.shape) == (len(counts), 2) and public.device.type == "cuda"
    assert np.array_equal(public.cpu().numpy(), want) and pool.sentinels_intact()
    assert tensor_digests([pool.tensors[0]]).cpu().numpy().tolist() == [[0, 0]]          # nothing but an empty tensor: no launch
    # a flipped bit changes A; two swapped unequal words leave A and change B
    which = SIZES.index(8193)
    t = pool.tensors[which].view(torch.int32)
    t[5000] ^= 0x00400000
    flipped = tensor_digests(pool.tensors).cpu().numpy()
    assert flipped[which, 0] != want[which, 0] and np.array_equal(np.delete(flipped, which, 0), np.delete(want, which, 0))
    t[5000] ^= 0x00400000
    a, b = int(t[17]), int(t[8000])
    assert a != b
    t[17], t[8000] = b, a
    swapped = tensor_digests(pool.tensors).cpu().numpy()
    assert swapped[which, 0] == want[which, 0] and swapped[which, 1] != want[which, 1]
    for bad in (torch.zeros(4), torch.zeros(8, 2, device=DEV)[:, 0], torch.zeros(4, dtype=torch.float16, device=DEV)):
        with pytest.raises(TypeError):
            tensor_digests([bad])


def test_more_chunks_than_the_grid():
    from locate_amd import tensor_digests
    n = 2049 * CHUNK + 1          # the 2048 blocks go round the chunk table twice; the last chunk holds one word
    big = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    small = torch.arange(7, dtype=torch.int32, device=DEV)
    got = tensor_digests([small, big]).cpu().numpy()
    assert got.tolist() == [list(PM.digest(small.cpu().numpy())), list(PM.digest(big.cpu().numpy()))]


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.full((64,), SENTINEL, dtype=torch.int64, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    good = [p, p, p, 1, 1, p, p]          # records chunks first n_tensors n_chunks partials out
    for at, value in ((0, None), (1, None), (2, None), (5, None), (6, None), (3, 0), (3, -1), (4, 0), (4, -2), (5, odd), (6, odd)):
        args = list(good)
        args[at] = value
        assert L.locate_digest(*args, None) == 1, args
        assert b"locate_digest" in L.locate_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())          # nothing was launched


# ---- 2. inside a captured graph ------------------------------------------------------------------------------------------------------
def test_inside_a_graph():
    from locate_amd.spill import _digest_table, _launch_digest
    pool = Pool([(4097, torch.float32, 0), (VIEW_N, torch.float32, 1), (4, torch.float64, 0), (0, torch.float32, 0)], 5)
    counts = [w.size for w in pool.host]
    table = _digest_table([t.data_ptr() if n else 0 for t, n in zip(pool.tensors, counts)], counts, DEV)          # before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = _launch_digest(table, torch.cuda.current_stream())
    rng = np.random.default_rng(6)
    for replay in range(2):
        for i, (t, n) in enumerate(zip(pool.tensors, counts)):
            if n:
                pool.host[i] = random_words(rng, n)
                t.view(torch.int32).copy_(as_i32(pool.host[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), model_digests(pool.host)), "replay %d" % replay
    assert pool.sentinels_intact()


# ---- 3. a StateSnapshot's slot on disk -------------------------------------------------------------------------------------------------
NAMES = ["a", "view", "pair", "later", "empty", "raw", "big"]
LATER = NAMES.index("later")
LATER_FILL = (0x3fc00000, 0xbf800000)          # 1.5, -1.0 alternating


class Rig:
    """a StateSnapshot over tensors inside sentinel buffers, like tests/test_gpu_snapshot.py's; `later` stays hidden: its getter
    returns None.  big: words of one more entry that makes the device-to-host copy long enough to be overtaken."""

    def __init__(self, folder, big=16, keep=2):
        from locate_amd import SnapshotSpill, StateSnapshot
        self.specs = [(4097, torch.float32, 0, 1), (VIEW_N, torch.float32, 1, 1), (4, torch.float64, 0, 2), (77, torch.float32, 0, 1),
                      (0, torch.float32, 0, 1), (9, torch.int32, 0, 0), (big, torch.float32, 0, 1)]
        self.pool = Pool([(n, dtype, lead) for n, dtype, lead, _ in self.specs], 11)
        named = []
        for i, (name, (n, _, _, kind)) in enumerate(zip(NAMES, self.specs)):
            getter = (lambda: None) if i == LATER else (lambda t=self.pool.tensors[i]: t)
            fill = LATER_FILL if i == LATER else ((0, 0, 0, 0x3ff00000) if kind == 2 else (0,))
            named.append((name, getter, n, kind, fill))
        self.snapshot = StateSnapshot(named, DEV)
        self.spill = SnapshotSpill(self.snapshot, str(folder), keep=keep)
        self.folder = str(folder)

    def load(self, seed):
        """finite contents (a take must commit) -> the live tensors; returns them as words per entry (the fill for `later`)"""
        rng = np.random.default_rng(100 + seed)
        state = {}
        for i, (name, (n, dtype, _, kind)) in enumerate(zip(NAMES, self.specs)):
            if i == LATER:
                state[name] = np.array((list(LATER_FILL) * n)[:n], np.uint32)
                continue
            if kind == 2:
                w = PM.words(np.array([float(seed), 0.996 ** seed]))
            elif kind == 0:
                w = np.array((SPECIALS * 2)[seed:seed + n], np.uint32)          # never judged: Inf and NaN patterns among them
            else:
                w = PM.words(rng.standard_normal(n).astype(np.float32)).copy()
                if n >= 3:
                    w[:3] = [0x00000001, 0x80000000, 0x7f7fffff]
            if n:
                self.pool.tensors[i].view(torch.int32).copy_(as_i32(w))
            self.pool.host[i] = w
            state[name] = w
        return state

    def xor(self, mask):
        """every live word ^ mask, by a device operation that does not make the host wait; returns the state like load().  A mask
        that leaves the exponent fields alone keeps finite values finite."""
        state = {}
        for i, (name, (n, _, _, _)) in enumerate(zip(NAMES, self.specs)):
            if i != LATER and n:
                self.pool.tensors[i].view(torch.int32).bitwise_xor_(int(np.array([mask], np.uint32).view(np.int32)[0]))
                self.pool.host[i] = self.pool.host[i] ^ np.uint32(mask)
            state[name] = np.array((list(LATER_FILL) * n)[:n], np.uint32) if i == LATER else self.pool.host[i]
        return state

    def path(self, k):
        return os.path.join(self.folder, "spill-%d.bin" % k)


def assert_file_holds(path, state, iteration):
    from locate_amd import read_spill
    found = read_spill(path)
    assert found.header["iteration"] == iteration
    for name, w in state.items():
        assert np.array_equal(PM.words(found.arrays[name]), w), "%s: %s differs" % (path, name)
    return found


def test_a_slot_goes_to_disk(tmp_path):
    rig = Rig(tmp_path / "spill")
    state = rig.load(1)
    host = {"iterations": 1, "t": torch.arange(5, dtype=torch.float64), "names": ["x", "y"], "nested": {"flag": True, "v": 0.5}}
    assert rig.spill.begin() is False and rig.spill.status()["begun"] == 0          # no slot committed
    rig.spill.take(1, host)
    assert rig.spill.begin() is True
    rig.spill.wait()
    status = rig.spill.status()
    assert (status["begun"], status["written"], status["skipped_busy"], status["last_iteration"]) == (1, 1, 0, 1)
    assert status["last_path"] == rig.path(0) and status["last_seconds"] > 0 and os.listdir(rig.folder) == ["spill-0.bin"]
    found = assert_file_holds(rig.path(0), state, 1)
    # byte for byte the good slot, the zero padding between the entries included
    header, arena, _ = PM.read_file(rig.path(0))
    good = rig.snapshot.status()["good"]
    assert arena == rig.snapshot.slot(good).cpu().numpy().tobytes() and header["slot_bytes"] == rig.snapshot.slot_bytes
    assert [e["name"] for e in header["entries"]] == NAMES and [e["offset"] for e in header["entries"]] == rig.snapshot.offsets
    assert [e["existed"] for e in header["entries"]] == [i != LATER for i in range(len(NAMES))]
    assert found.arrays["later"].tolist() == ([1.5, -1.0] * 39)[:77] and found.arrays["later"].dtype == np.float32
    assert found.arrays["pair"].dtype == np.float64 and found.arrays["pair"].shape == (2,) and found.arrays["raw"].dtype == np.int32
    assert found.arrays["empty"].shape == (0,) and found.arrays["view"].shape == (VIEW_N,)
    for e in header["entries"]:          # the device's digests, as the independent model computes them from the file
        assert list(PM.digest(PM.entry_words(header, arena, e["name"]))) == e["digest"], e["name"]
    got = found.host_state
    assert got["iterations"] == 1 and got["names"] == ["x", "y"] and got["nested"] == {"flag": True, "v": 0.5} and torch.equal(got["t"], host["t"])
    assert rig.spill.begin() is False and rig.spill.status()["begun"] == 1          # nothing newer
    assert rig.pool.sentinels_intact()
    rig.spill.close()
    with pytest.raises(RuntimeError):
        rig.spill.begin()


# ---- 4. ordering: a take behind begin() does not reach the slot in flight --------------------------------------------------------------
def test_a_take_waits_for_the_copy_in_flight(tmp_path):
    from locate_amd import SnapshotSpill, read_spill
    rig = Rig(tmp_path / "spill", big=(8 << 20) + 3)          # 32 MB: the copy takes milliseconds, the takes behind it microseconds
    states = {1: rig.load(1)}
    rig.spill.take(1, {"iterations": 1})
    assert rig.spill.begin()
    for k, mask in ((2, 0x80000000), (3, 0x00000001)):          # take(2) writes the other slot, take(3) the one that is being copied
        states[k] = rig.xor(mask)          # device operations only: the host does not wait, the takes are issued at once
        rig.spill.take(k, {"iterations": k})
    assert not np.array_equal(states[1]["big"], states[3]["big"])
    rig.spill.wait()
    assert rig.snapshot.status()["iteration"] == 3 and rig.snapshot.status()["good"] == 0
    assert_file_holds(rig.path(0), states[1], 1)
    assert rig.spill.begin()
    rig.spill.wait()
    assert_file_holds(rig.path(1), states[3], 3)
    assert_file_holds(rig.path(0), states[1], 1)          # both files are valid
    assert SnapshotSpill.latest(rig.folder).header["iteration"] == 3
    states[4] = rig.load(4)
    rig.spill.take(4, {"iterations": 4})
    assert rig.spill.begin()
    rig.spill.wait()
    assert sorted(os.listdir(rig.folder)) == ["spill-0.bin", "spill-1.bin"]          # keep = 2: the third replaced the oldest
    assert_file_holds(rig.path(0), states[4], 4)
    assert read_spill(rig.path(1)).header["iteration"] == 3
    assert rig.spill.status()["written"] == 3 and rig.pool.sentinels_intact()
    # a new spill over the same folder goes on behind the newest file
    assert SnapshotSpill(rig.snapshot, rig.folder)._next == 1


# ---- 5. a busy writer ------------------------------------------------------------------------------------------------------------------
def test_begin_while_the_writer_is_busy(tmp_path):
    rig = Rig(tmp_path / "spill")
    rig.spill._hold = threading.Event()          # the writer waits here before it touches a job
    rig.load(1)
    rig.spill.take(1)
    assert rig.spill.begin() is True
    state = rig.load(2)
    rig.spill.take(2)
    assert rig.spill.begin() is False and rig.spill.begin() is False
    assert rig.spill.status()["skipped_busy"] == 2 and rig.spill.status()["begun"] == 1 and not os.listdir(rig.folder)
    rig.spill._hold.set()
    rig.spill.wait()
    assert rig.spill.status()["written"] == 1
    assert rig.spill.begin() is True
    rig.spill.wait()
    found = assert_file_holds(rig.path(1), state, 2)
    assert found.host_state is None
    # an error in the writer is kept and raised on the caller's thread
    rig.load(3)
    rig.spill.take(3)
    shutil.rmtree(rig.folder)          # the rename has nowhere to go
    assert rig.spill.begin() is True
    with pytest.raises(OSError):
        rig.spill.wait()
    rig.spill.wait()          # raised once


# ---- 6. in a run: the tiny fixture network of the snapshot and guard tests (g8, 32 x 32, base width 1, batch 8) ---------------------------
def build_tiny():
    from locate_amd import AveragedGenerator, Discriminator, Generator, GuardedNadam, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    step = TrainStep(G, D, GuardedNadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     GuardedNadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1)
    average = AveragedGenerator(G, beta=0.9)
    return G, D, step, average


@functools.lru_cache(maxsize=None)
def inputs():
    """x1 .. x8 as (latent, real, aug) on the device: the fixture's batch, then seeded ones"""
    z = load_golden("g8_tiny_e2e")
    first = tuple(T(z["step1/" + k]) for k in ("latent", "real", "aug"))
    gen = torch.Generator().manual_seed(77)
    rest = [tuple(torch.randn(t.shape, generator=gen) if k == 0 else torch.randn(t.shape, generator=gen).clamp(-1, 1) for k, t in enumerate(first))
            for _ in range(7)]
    return tuple(tuple(t.to(DEV) for t in x) for x in [first] + rest)


def training_state(G, D, step, average):
    """every parameter (u and v included), every Nadam state tensor, the average's tensors and its count, by name"""
    torch.cuda.synchronize()
    state = {"G/" + k: v.detach().clone() for k, v in G.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in D.state_dict().items()})
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        for name, q in net.named_parameters():
            for k, v in opt.state.get(q, {}).items():
                if torch.is_tensor(v):
                    state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
    state.update({"A/" + k: v.detach().clone() for k, v in average.generator.state_dict().items()})
    state["A/updates"] = torch.tensor([average.updates])
    state["G/noise"] = G.noise.detach().clone()
    state["D/uv_trainable"] = torch.tensor([p.requires_grad for n, p in D.named_parameters() if n.endswith(("weight_u", "weight_v"))])
    return state


class Run:
    """iterate(k) runs the step on x_k, then the average's update: eagerly, or - `graphed` - the first call builds a
    GraphedTrainStep (its two warm-up iterations belong to that call, as in the trainer) and every call is a replay"""

    def __init__(self, mode, folder=None):
        from locate_amd import SnapshotSpill, TrainingSnapshot
        self.mode = mode
        self.G, self.D, self.step, self.average = build_tiny()
        self.spill = SnapshotSpill(TrainingSnapshot(self.step, self.average), str(folder)) if folder is not None else None
        self.runner = None
        self.losses = []

    def iterate(self, *ks):
        from locate_amd.graph import GraphedTrainStep
        for k in ks:
            x = inputs()[k - 1]
            if self.mode == "eager":
                out = self.step(*x)
            else:
                if self.runner is None:
                    self.runner = GraphedTrainStep(self.step, *x, warmup=2)
                out = self.runner.replay(*x)
            self.losses.append(torch.stack([out["d_error"].detach().reshape(()), out["g_error"].detach().reshape(())]).clone())
            self.average.update()
        return self

    def host_state(self):
        uv = [p.requires_grad for n, p in self.D.named_parameters() if n.endswith(("weight_u", "weight_v"))]
        return {"noise": self.G.noise.detach().cpu(), "dis_uv_trainable": bool(uv) and all(uv),
                "average": {"updates": int(self.average.updates), "one_minus_beta": float(self.average.one_minus_beta)}}

    def take(self, iteration):
        self.spill.take(iteration, self.host_state())
        return self

    def state(self):
        return training_state(self.G, self.D, self.step, self.average)


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def differing(a, b):
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))[:6]
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


def same_losses(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def uninterrupted(mode):
    """Run A: x1 .. x6 without a snapshot or a spill; the states after iterations 1, 3 and 6 and the losses"""
    run = Run(mode)
    states = {}
    for k in range(1, 7):
        run.iterate(k)
        if k in (1, 3, 6):
            states[k] = run.state()
    return states, [l.clone() for l in run.losses]


@pytest.mark.parametrize("at", [3, 1])
def test_an_abandoned_run_continues_from_its_spill(tmp_path, at):
    """at = 1: D's u / v gain Nadam state only at the second D-step - the file says they did not exist, and the restored optimizer
    must have no state for them, exactly like the uninterrupted run after iteration 1"""
    from locate_amd import SnapshotSpill, restore_training_state
    states, losses = uninterrupted("eager")
    assert any(k.endswith("weight_u") for k in states[3]) and any(k.endswith("/sched") for k in states[3]) and any(k.startswith("A/") for k in states[3])
    late = [k for k in states[3] if k not in states[1]]
    assert late and all("/opt/" in k and ("weight_u" in k or "weight_v" in k) for k in late), late[:4]
    run = Run("eager", tmp_path / "spill").iterate(*range(1, at + 1)).take(at)
    assert run.spill.begin()
    run.iterate(7, 8)          # while the copy is in flight
    run.spill.wait()
    assert len(differing(states[3], run.state())) > 50, "the run did not move on"
    del run          # the crash
    found = SnapshotSpill.latest(str(tmp_path / "spill"))
    assert found.header["iteration"] == at and found.skipped == ()
    hidden = sorted(e["name"] for e in found.header["entries"] if not e["existed"])
    assert set(late) <= set(hidden) if at == 1 else not set(late) & set(hidden)
    fresh = Run("eager")
    assert restore_training_state(found, fresh.step, fresh.average) == at
    bad = differing(states[at], fresh.state())          # the same keys: no state the uninterrupted run did not have
    assert not bad, "after the restore %d of %d tensors differ from the uninterrupted run, first %s" % (len(bad), len(states[at]), bad[:4])
    fresh.iterate(*range(at + 1, 7))
    bad = differing(states[6], fresh.state())
    assert not bad, "at iteration 6, %d of %d tensors differ, first %s" % (len(bad), len(states[6]), bad[:4])
    assert same_losses(losses[at:], fresh.losses)
    # a spill that does not fit is refused before anything is written
    other = Run("eager")
    before = other.state()
    header = json.loads(json.dumps(found.header))
    arrays = dict(found.arrays)
    name = next(k for k in arrays if k.startswith("D/") and arrays[k].size > 4)
    arrays[name] = arrays[name].reshape(-1)[:-1]
    with pytest.raises(ValueError):
        restore_training_state((header, arrays, found.host_state), other.step, other.average)
    arrays = {k: v for k, v in found.arrays.items() if k != name}
    with pytest.raises(ValueError):
        restore_training_state((header, arrays, found.host_state), other.step, other.average)
    assert not differing(before, other.state())


# ---- 7. a run that spills and never resumes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_a_spill_that_is_never_read_changes_nothing(tmp_path, mode):
    states, losses = uninterrupted(mode)
    run = Run(mode, tmp_path / "spill")
    begun = []
    for k in range(1, 7):
        run.iterate(k)
        if k in (3, 5, 6):
            begun.append(run.spill.begin())
        if k in (2, 4, 5):
            run.take(k)
    run.spill.wait()
    assert not differing(states[6], run.state())
    assert same_losses(losses, run.losses)
    assert begun[0] is True and run.spill.status()["written"] + run.spill.status()["skipped_busy"] == 3 and run.spill.status()["written"] >= 1


# ---- 8. the trainer, end to end ------------------------------------------------------------------------------------------------------
class Crash(Exception):
    pass


def make_trainer(out, store, crash_at=None, **kw):
    from locate_amd import InputPipeline, RunStatistics, Trainer, TrainingSnapshot
    G, D, step, average = build_tiny()
    pipeline = InputPipeline(store, 32, 8, seed=11)
    kw.setdefault("max_iterations", 12)
    t = Trainer(step, pipeline, str(out), epochs=1, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                image_interval_function=lambda batch: 1000, print_every_function=lambda batch: 2, average=average, stats=RunStatistics(G, D),
                stats_every=1, snapshot=TrainingSnapshot(step, average), rollback_every=2, **kw)
    assert pipeline.batches_per_epoch == 12
    iteration = t._iteration

    def crashing_iteration():
        if t.iterations + 1 == crash_at:
            raise Crash()
        return iteration()
    t._iteration = crashing_iteration
    return t


def trainer_state(t):
    return training_state(t.gen, t.dis, t.step, t.average)


@pytest.fixture(scope="module")
def crashed(tmp_path_factory):
    """Run A: 12 iterations without a spill -> its final state.  Run B: spill_every = 4, abandoned in iteration 11 -> its folder"""
    from locate_amd import DeviceImageStore
    store = DeviceImageStore(np.random.default_rng(6).integers(0, 256, size=(96, 78, 64, 3), dtype=np.uint8), DEV)
    root = tmp_path_factory.mktemp("spill_trainer")
    a = make_trainer(root / "a", store)
    assert a.run() == 12 and a.spill is None and not os.path.exists(str(root / "a" / "spill"))
    assert not os.path.exists(str(root / "a" / "error" / "resumes.json"))
    want = trainer_state(a)
    b = make_trainer(root / "b", store, crash_at=11, spill_every=4)
    with pytest.raises(Crash):
        b.run()
    assert b.iterations == 10 and not os.path.exists(str(root / "b" / "trainer.torch")) and not os.path.exists(str(root / "b" / "netG.torch"))
    b.spill.wait()          # run() has waited already: the writer is idle
    status = b.spill.status()
    assert status["begun"] == status["written"] >= 2 and 4 <= status["last_iteration"] <= 10
    del a, b
    return store, root, want, status["last_iteration"]


def test_trainer_resumes_from_the_spill(crashed, tmp_path):
    store, root, want, spilled = crashed
    out = tmp_path / "b"
    shutil.copytree(str(root / "b"), str(out))
    # an older save beside the newer spill: the spill wins
    older = make_trainer(out, store, max_iterations=2)
    assert older.run() == 2 and older.spill is None
    assert torch.load(str(out / "trainer.torch"), map_location="cpu", weights_only=True)["iterations"] == 2
    t = make_trainer(out, store, spill_every=4).resume()
    assert t.iterations == spilled and 4 <= spilled <= 10 and (t.epoch, t.sub, t.i) == (0, 0, spilled)
    with open(str(out / "error" / "resumes.json")) as f:
        assert json.load(f) == {"from": "spill", "iterations": spilled}
    assert t.run() == 12
    bad = differing(want, trainer_state(t))
    assert not bad, "resumed at %d: %d of %d tensors differ from the uninterrupted run, first %s" % (spilled, len(bad), len(want), bad[:4])
    # now the save is the newer one: the save wins
    assert torch.load(str(out / "trainer.torch"), map_location="cpu", weights_only=True)["iterations"] == 12
    t = make_trainer(out, store, spill_every=4).resume()
    assert t.iterations == 12
    with open(str(out / "error" / "resumes.json")) as f:
        assert json.load(f) == {"from": "save", "iterations": 12}
    assert not differing(want, trainer_state(t))


def test_trainer_passes_over_a_corrupt_spill(crashed, tmp_path):
    from locate_amd import SnapshotSpill, read_spill
    store, root, want, spilled = crashed
    out = tmp_path / "b"
    shutil.copytree(str(root / "b"), str(out))
    files = sorted(os.listdir(str(out / "spill")))
    assert files == ["spill-0.bin", "spill-1.bin"]
    at = {f: read_spill(str(out / "spill" / f)).header["iteration"] for f in files}
    newest = max(at, key=at.get)
    assert at[newest] == spilled
    header, _, _ = PM.read_file(str(out / "spill" / newest))
    largest = max(header["entries"], key=lambda e: e["n_words"])
    where = os.path.getsize(str(out / "spill" / newest)) - header["blob_bytes"] - header["slot_bytes"] + largest["offset"] + 2
    with open(str(out / "spill" / newest), "r+b") as f:          # one bit of one weight, on disk
        f.seek(where)
        byte = f.read(1)
        f.seek(where)
        f.write(bytes([byte[0] ^ 0x01]))
    older = min(at.values())
    assert SnapshotSpill.latest(str(out / "spill")).skipped == (str(out / "spill" / newest),)
    t = make_trainer(out, store, spill_every=4).resume()          # no trainer.torch: not an error while a valid spill exists
    assert t.iterations == older < spilled
    with open(str(out / "error" / "resumes.json")) as f:
        assert json.load(f) == {"from": "spill", "iterations": older}
    assert t.run() == 12
    assert not differing(want, trainer_state(t))


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_flags(tmp_path):
    """batch 512: the reference's progress interval is 1024 // max(batch, 64) = 2 iterations, so takes follow iterations 2, 4
    and 6 and the spills begin at 4 and 6"""
    from locate_amd import SnapshotSpill
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(6 * 512, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    base = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--epochs", "1", "--minibatches", "1",
            "--images", "16", "--stats-every", "1", "--max-iterations", "6"]
    done = subprocess.run(base + ["--batch", "512", "--out", out, "--spill-every", "2", "--rollback-every", "2"], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "6 iterations" in done.stdout
    files = sorted(os.listdir(os.path.join(out, "spill")))
    assert files and all(f in ("spill-0.bin", "spill-1.bin") for f in files), files
    found = SnapshotSpill.latest(os.path.join(out, "spill"))
    assert found is not None and found.skipped == () and found.header["iteration"] in (2, 4) and found.host_state["iterations"] == found.header["iteration"]
    assert not os.path.exists(os.path.join(out, "error", "resumes.json"))          # nothing was resumed
    # without the flag: no folder, no record
    done = subprocess.run(base + ["--batch", "8", "--out", out + "2", "--rollback-every", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert not os.path.exists(os.path.join(out + "2", "spill")) and not os.path.exists(os.path.join(out + "2", "error", "resumes.json"))
