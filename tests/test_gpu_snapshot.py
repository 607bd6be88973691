"""The last-good snapshot on the MI355X (locate_amd/snapshot.py, csrc/snapshot.hip), bits compared as int32 throughout, against what
is not the code under test: the numpy model of take, commit and restore (tests/helpers/snapshot_model.py) at the operator level -
eagerly and inside a captured graph, where the decision is taken at replay time - and, in a run of the tiny fixture network, the
uninterrupted run: a run that wandered off, or was poisoned, and came back must continue the uninterrupted one bit for bit, which
catches a forgotten panel re-pack, a stale maximum word, a missed version bump, a moment, a schedule pair, u / v or the average."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import snapshot_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
CHUNK = 4096
SIZES = [1, 3, 4095, 4096, 4097, 8193, 40000]          # the project's chunk-edge sizes
VIEW_N = 5001                                          # a view one element into a larger buffer: 4-byte alignment only
LATER_N = 77                                           # an entry whose getter returns None
RAW_N = 9                                              # a kind-0 entry
SENTINEL = 0x5e471e15
PAD = 8                                                # sentinel words on either side of every live tensor
VIEW, PAIR, LATER, EMPTY, RAW = (len(SIZES) + k for k in range(5))
NAMES = ["t%d" % n for n in SIZES] + ["view", "pair", "later", "empty", "raw"]
LATER_FILL = (0x3fc00000, 0xbf800000)                  # 1.5, -1.0 alternating
FINITE_SPECIALS = [bits for bits, finite in SM.SPECIAL_F32 if finite]
ALL_SPECIALS = [bits for bits, _ in SM.SPECIAL_F32]


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def entries():
    return [(n, 1, (0,)) for n in SIZES] + [(VIEW_N, 1, (0,)), (4, 2, SM.fill_words((0, 0, 0, 0x3ff00000)).tolist()), (LATER_N, 1, LATER_FILL),
                                            (0, 1, (0,)), (RAW_N, 0, (0,))]


@functools.lru_cache(maxsize=None)
def host_contents(seed):
    """uint32 words per entry (None for `later`): fp32 over 16 binades with the FINITE special patterns sprinkled in; the raw
    entry holds every special pattern, Inf and NaN included - it is never judged"""
    rng = np.random.default_rng(300 + seed)
    out = []
    for n in SIZES + [VIEW_N]:
        w = SM.words((rng.standard_normal(n) * 2.0 ** rng.uniform(-8, 8, size=n)).astype(np.float32)).copy()
        if n >= 3:
            at = rng.choice(n, size=min(n, len(FINITE_SPECIALS)), replace=False)
            w[at] = np.array(FINITE_SPECIALS, np.uint32)[:at.size]
        out.append(w)
    out.append(SM.words(np.array([float(seed + 1), 0.996 ** (seed + 1)], np.float64)).copy())
    out.append(None)
    out.append(np.zeros(0, np.uint32))
    out.append(np.array((ALL_SPECIALS * 2)[seed:seed + RAW_N], np.uint32))
    return tuple(out)


class Rig:
    """every live tensor sits inside a larger buffer of sentinel words; `later` exists but its getter hides it until show_later"""

    def __init__(self):
        from locate_amd import StateSnapshot
        self.buffers, self.tensors = [], []
        for i, (n, kind, _) in enumerate(entries()):
            lead = PAD + 1 if i == VIEW else PAD          # PAD words = 32 bytes: 16-byte aligned; one more word: 4 bytes past it
            buf = torch.full((lead + n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
            words = buf[lead:lead + n]
            if i == PAIR:
                t = words.view(torch.float64)
            elif i == RAW:
                t = words
            else:
                t = words.view(torch.float32)
            if i == VIEW:
                assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            elif n:
                assert t.data_ptr() % 16 == 0
            self.buffers.append(buf)
            self.tensors.append(t)
        self.show_later = False
        named = []
        for i, (name, (n, kind, fill)) in enumerate(zip(NAMES, entries())):
            getter = (lambda: self.tensors[LATER] if self.show_later else None) if i == LATER else (lambda t=self.tensors[i]: t)
            named.append((name, getter, n, kind, fill))
        self.snapshot = StateSnapshot(named, DEV)
        self.model = SM.Model(entries())
        self.host = None

    def words(self, i):
        t = self.tensors[i]
        return t.view(torch.int32) if t.numel() else t

    def load(self, contents):
        """contents -> the live tensors; the model's view of them is kept"""
        self.host = [None if w is None else w.copy() for w in contents]
        for i, w in enumerate(self.host):
            if w is not None and w.size:
                self.words(i).copy_(T(w.view(np.int32)))
        return self

    def poke(self, which, where, bits):
        self.host[which][where] = bits
        self.words(which)[where] = int(np.array([bits], np.uint32).view(np.int32)[0])

    def live(self):
        """what the model is given: `later` only once it shows"""
        return [(SM.words(self.tensors[LATER].cpu().numpy()) if self.show_later else None) if i == LATER else w for i, w in enumerate(self.host)]

    def take(self, iteration):
        self.snapshot.take(iteration)
        return self.model.take(self.live(), iteration)

    def buffer_bits(self):
        torch.cuda.synchronize()
        return [b.clone() for b in self.buffers]

    def slot_bits(self, i):
        torch.cuda.synchronize()
        return self.snapshot.slot(i).cpu().numpy().view(np.uint32).copy()

    def assert_matches_model(self, what):
        for i in (0, 1):
            got, want = self.slot_bits(i), self.model.slots[i]
            assert got.shape == want.shape, what
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "%s: slot %d differs from the model in %d words, first at word %d" % (what, i, bad.size, bad[0])
        assert self.snapshot.status() == self.model.status(NAMES), what


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the operator against the model -------------------------------------------------------------------------------------------
def test_take_against_the_model():
    from locate_amd.snapshot import arena_layout
    rig = Rig().load(host_contents(0))
    s = rig.snapshot
    assert (s.offsets, s.slot_bytes) == arena_layout([n for n, _, _ in entries()]) == (rig.model.offsets, rig.model.slot_bytes)
    assert s.slot(0).dtype == torch.uint8 and s.slot(0).numel() == s.slot_bytes and s.slot(0).data_ptr() % 16 == 0
    assert s.status() == rig.model.status(NAMES) and s.status()["good"] == -1
    before = rig.buffer_bits()
    assert rig.take(3)
    rig.assert_matches_model("first take")          # byte for byte, the zero padding and the fill of `later` included
    assert same(before, rig.buffer_bits()), "the take wrote a live tensor"
    assert not rig.slot_bits(1).any() and s.status()["good"] == 0 and s.status()["iteration"] == 3
    off = s.offsets[LATER] // 4
    assert rig.slot_bits(0)[off:off + 5].tolist() == [0x3fc00000, 0xbf800000, 0x3fc00000, 0xbf800000, 0x3fc00000]
    # the second take goes to the other slot and leaves the first alone
    first = rig.slot_bits(0)
    rig.load(host_contents(1))
    before = rig.buffer_bits()
    assert rig.take(4)
    rig.assert_matches_model("second take")
    assert np.array_equal(rig.slot_bits(0), first) and same(before, rig.buffer_bits()) and s.status()["good"] == 1
    # the same table at the same addresses: one device table was built
    assert len(s._tables) == 1


# ---- 2. rejection ----------------------------------------------------------------------------------------------------------------------
NAN, INF = 0x7fc00001, 0xff800000
PLACES = {"first of a tensor": (SIZES.index(4097), 0, NAN, 1), "last of a tensor": (SIZES.index(40000), 39999, INF, 1),
          "the 1-element tensor": (SIZES.index(1), 0, 0x7f800001, 1),
          "the scalar head of the misaligned view": (VIEW, 1, NAN, 1), "its tail": (VIEW, VIEW_N - 1, INF, 1),
          "the step of the fp64 pair": (PAIR, 1, 0x7ff80000, 1),          # word 1: the HIGH word of the first double
          "the second chunk of 8193": (SIZES.index(8193), 5000, NAN, 1),
          "an fp32 Inf in a raw entry": (RAW, 4, 0x7f800000, 0)}


@pytest.mark.parametrize("place", list(PLACES))
def test_rejection(place):
    which, where, bits, counted = PLACES[place]
    rig = Rig().load(host_contents(2))
    rig.poke(RAW, 4, 0)
    assert rig.take(1)
    good = rig.slot_bits(0)
    clean = int(rig.host[which][where])
    rig.poke(which, where, bits)
    committed = rig.take(2)
    rig.assert_matches_model(place)
    state = rig.snapshot.status()
    if not counted:          # a raw word is never judged: the take commits
        assert committed and (state["good"], state["iteration"], state["rejected"]) == (1, 2, 0)
        return
    assert not committed
    assert (state["good"], state["iteration"], state["taken"], state["rejected"]) == (0, 1, 1, 1)
    assert (state["last_rejected_iteration"], state["last_rejected_count"], state["last_rejected_tensor"]) == (2, 1, NAMES[which])
    assert np.array_equal(rig.slot_bits(0), good), "a rejected take wrote the good slot"
    # the word cleaned: the next take commits into the slot the rejected one wrote
    rig.poke(which, where, clean)
    assert rig.take(3)
    rig.assert_matches_model(place + ", cleaned")
    state = rig.snapshot.status()
    assert (state["good"], state["iteration"], state["taken"], state["rejected"], state["last_rejected_iteration"]) == (1, 3, 2, 1, 2)
    assert np.array_equal(rig.slot_bits(0), good)


def test_rejection_counts_every_word_and_names_the_first_tensor():
    rig = Rig().load(host_contents(2))
    bad = [bits for bits, finite in SM.SPECIAL_F32 if not finite]
    for k, bits in enumerate(bad):
        rig.poke(SIZES.index(40000), 4090 + k, bits)          # across the first chunk edge
    rig.poke(VIEW, 2, NAN)
    rig.poke(PAIR, 3, 0xfff00000)
    rig.poke(PAIR, 0, 0x7fc00000)          # a LOW word that looks like an fp32 NaN: not counted
    assert not rig.take(9)
    rig.assert_matches_model("many bad words")
    state = rig.snapshot.status()
    assert (state["good"], state["last_rejected_count"], state["last_rejected_tensor"]) == (-1, len(bad) + 2, "t40000")


# ---- 3. restore writes what it should and nothing else ------------------------------------------------------------------------------
def test_restore():
    from locate_amd import NoSnapshot
    rig = Rig().load(host_contents(3))
    untouched = rig.buffer_bits()
    with pytest.raises(NoSnapshot):
        rig.snapshot.restore()
    assert same(untouched, rig.buffer_bits())
    assert rig.take(5)
    want = rig.buffer_bits()
    rig.load(host_contents(4))
    assert not same(want, rig.buffer_bits())
    versions = [t._version for t in rig.tensors]
    assert rig.snapshot.restore() == 5
    got = rig.buffer_bits()
    bad = [NAMES[i] for i, (a, b) in enumerate(zip(want, got)) if not torch.equal(a, b)]
    assert not bad, "after the restore %s differ from the snapshot (sentinels included)" % bad
    for i, t in enumerate(rig.tensors):
        if i in (LATER, EMPTY):
            assert t._version == versions[i], NAMES[i]          # not in the table / nothing to write
        else:
            assert t._version > versions[i], NAMES[i]
        assert int(rig.buffers[i][0]) == SENTINEL and int(rig.buffers[i][-1]) == SENTINEL
    assert (rig.buffers[LATER] == SENTINEL).all()          # the entry that was None: untouched
    # a tensor that appeared since the take is restored to its fill - fresh state - and only it
    rig.show_later = True
    assert rig.snapshot.restore() == 5
    got = rig.buffer_bits()
    assert all(torch.equal(a, b) for i, (a, b) in enumerate(zip(want, got)) if i != LATER)
    later = got[LATER].cpu().numpy().view(np.uint32)
    assert later[:PAD].tolist() == [SENTINEL] * PAD and later[-PAD:].tolist() == [SENTINEL] * PAD
    assert later[PAD:-PAD].tolist() == (list(LATER_FILL) * LATER_N)[:LATER_N]
    assert len(rig.snapshot._tables) == 1          # rebuilt for the new address, the old table dropped
    # and a take now copies it
    rig.host = [None if w is None else w.copy() for w in host_contents(3)]          # what the live tensors hold again
    assert rig.take(6)
    rig.assert_matches_model("with the late tensor")


def test_unsuitable_tensors_are_refused():
    from locate_amd import StateSnapshot
    strided = torch.zeros(8, 2, device=DEV)[:, 0]
    half = torch.zeros(8, dtype=torch.float16, device=DEV)
    for t, n in ((strided, 8), (half, 4), (torch.zeros(8, dtype=torch.int64, device=DEV), 16)):
        with pytest.raises(TypeError):
            StateSnapshot([("t", lambda t=t: t, n, 1, (0,))], DEV)
    with pytest.raises(ValueError):
        StateSnapshot([("t", lambda: torch.zeros(8, device=DEV), 9, 1, (0,))], DEV)


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.zeros(512, dtype=torch.uint8, device=DEV)
    p, q = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 256)
    odd = ctypes.c_void_p(buf.data_ptr() + 4)
    good = [p, p, 1, 1, p, q, p]          # records chunks n_tensors n_chunks slot0 slot1 commit
    for at, value in ((0, None), (1, None), (4, None), (5, None), (6, None), (2, 0), (2, -1), (3, 0), (3, -2), (4, odd), (5, odd), (6, odd), (5, p)):
        args = list(good)
        args[at] = value
        assert L.locate_snapshot_take(*args, 1, None) == 1, args
        assert b"locate_snapshot_take" in L.locate_last_error()
    for args in ([None, p, 1, 1, p], [p, None, 1, 1, p], [p, p, 0, 1, p], [p, p, 1, 0, p], [p, p, 1, 1, None], [p, p, 1, 1, odd]):
        assert L.locate_snapshot_restore(*args, None) == 1, args
        assert b"locate_snapshot_restore" in L.locate_last_error()
    torch.cuda.synchronize()
    assert not buf.any()          # nothing was launched: a commit launch would have counted a take
    assert (L.locate_snapshot_record_bytes(), L.locate_snapshot_commit_bytes(), L.locate_snapshot_chunk_elems()) == (48, 64, CHUNK)


# ---- 4. more chunks than the grid ------------------------------------------------------------------------------------------------------
def test_more_chunks_than_the_copy_grid():
    from locate_amd import StateSnapshot
    n = (2048 + 150) * CHUNK + 5          # 9.0 M words: the 2048 blocks go round the chunk table twice
    torch.manual_seed(5)
    big = torch.randn(n, device=DEV)
    small = torch.randn(7, device=DEV)
    s = StateSnapshot([("small", lambda: small, 7, 1, (0,)), ("big", lambda: big, n, 1, (0,))], DEV)
    big[n - 2] = float("nan")          # in the last, partial chunk
    big[2100 * CHUNK + 17] = float("inf")          # and in a chunk only the second round reaches
    s.take(1)
    state = s.status()
    assert (state["good"], state["rejected"], state["last_rejected_count"], state["last_rejected_tensor"]) == (-1, 1, 2, "big")
    off = s.offsets[1]
    assert torch.equal(s.slot(0)[off:off + 4 * n].view(torch.int32), big.view(torch.int32))          # rejected, but copied whole
    big[n - 2], big[2100 * CHUNK + 17] = 1.0, 2.0
    s.take(2)
    state = s.status()
    assert (state["good"], state["iteration"], state["taken"], state["rejected"]) == (0, 2, 1, 1)
    assert torch.equal(s.slot(0)[off:off + 4 * n].view(torch.int32), big.view(torch.int32))
    assert torch.equal(s.slot(0)[:28].view(torch.int32), small.view(torch.int32)) and not s.slot(0)[28:off].any() and not s.slot(1).any()
    kept = big.clone()
    big.zero_()
    assert s.restore() == 2 and torch.equal(big.view(torch.int32), kept.view(torch.int32))


# ---- 5. inside a captured graph ------------------------------------------------------------------------------------------------------
def test_inside_a_graph():
    rig = Rig().load(host_contents(5))
    assert rig.take(1)          # eagerly once: the table exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rig.snapshot.take(7)
    rig.assert_matches_model("a capture runs nothing")
    written = []
    for replay, (seed, poison) in enumerate(((6, False), (7, True), (8, False))):
        rig.load(host_contents(seed))
        if poison:
            rig.poke(SIZES.index(4096), 4095, NAN)
            rig.poke(VIEW, VIEW_N - 2, INF)
        written.append(rig.model.destination())
        committed = rig.model.take(rig.live(), 7)
        graph.replay()
        rig.assert_matches_model("replay %d" % replay)
        assert committed == (not poison)
    assert written == [1, 0, 0]          # alternating; the rejected take's slot is written again
    state = rig.snapshot.status()
    assert (state["good"], state["taken"], state["rejected"], state["last_rejected_count"], state["last_rejected_tensor"]) == (0, 3, 1, 2, "t4096")


# ---- 6. in a run: the tiny fixture network of tests/test_gpu_guard.py (g8, 32 x 32, base width 1, batch 8) ------------------------------
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


class Run:
    """iterate(k) runs the step on x_k, then the average's update: eagerly, or - `graphed` - the first call builds a
    GraphedTrainStep (its two warm-up iterations belong to that call, as in the trainer) and every call is a replay"""

    def __init__(self, mode, snapshot=True):
        from locate_amd import TrainingSnapshot
        self.mode = mode
        self.G, self.D, self.step, self.average = build_tiny()
        self.snapshot = TrainingSnapshot(self.step, self.average) if snapshot else None
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

    def state(self):
        """every parameter (u and v included), every Nadam state tensor, the average's tensors and its count, by name"""
        torch.cuda.synchronize()
        state = {"G/" + k: v.detach().clone() for k, v in self.G.state_dict().items()}
        state.update({"D/" + k: v.detach().clone() for k, v in self.D.state_dict().items()})
        for tag, net, opt in (("G", self.G, self.step.gen_opt), ("D", self.D, self.step.dis_opt)):
            for name, q in net.named_parameters():
                for k, v in opt.state.get(q, {}).items():
                    if torch.is_tensor(v):
                        state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
        state.update({"A/" + k: v.detach().clone() for k, v in self.average.generator.state_dict().items()})
        state["A/updates"] = torch.tensor([self.average.updates])
        return state


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def differing(a, b):
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))[:6]
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


@functools.lru_cache(maxsize=None)
def uninterrupted(mode):
    """Run A: x1 .. x6 without a snapshot; the states after iterations 1, 3 and 6 and the losses"""
    run = Run(mode, snapshot=False)
    states = {}
    for k in range(1, 7):
        run.iterate(k)
        if k in (1, 3, 6):
            states[k] = run.state()
    return states, [l.clone() for l in run.losses]


def assert_continues_like_the_uninterrupted_run(run, mode, what):
    states, losses = uninterrupted(mode)
    bad = differing(states[3], run.state())
    assert not bad, "%s, %s: after the restore %d of %d tensors differ from the uninterrupted run, first %s" % (what, mode, len(bad), len(states[3]), bad[:4])
    run.losses = []
    run.iterate(4, 5, 6)
    bad = differing(states[6], run.state())
    assert not bad, "%s, %s: three iterations on, %d of %d tensors differ, first %s" % (what, mode, len(bad), len(states[6]), bad[:4])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(losses[3:], run.losses)) and len(run.losses) == 3


@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_a_detour_and_back(mode):
    states, _ = uninterrupted(mode)
    assert any(k.endswith("weight_u") for k in states[3]) and any(k.endswith("/sched") for k in states[3]) and any(k.startswith("A/") for k in states[3])
    assert len(differing(states[3], states[6])) > 50
    run = Run(mode).iterate(1, 2, 3)
    run.snapshot.take(3)
    run.iterate(7, 8)
    moved = differing(states[3], run.state())
    assert len(moved) > 50 and "A/updates" in moved, "the detour did not change the state"
    assert run.snapshot.restore() == 3
    assert run.snapshot.status()["taken"] == 1
    assert_continues_like_the_uninterrupted_run(run, mode, "detour")


def test_a_moment_that_did_not_exist_at_the_take():
    """take(1): D's u / v gain Nadam state only at the second D-step, so the slot holds their fill; restored, it is fresh state"""
    states, losses = uninterrupted("eager")
    run = Run("eager").iterate(1)
    late = [k for k in states[3] if k not in states[1]]
    assert late and all("/opt/" in k and ("weight_u" in k or "weight_v" in k) for k in late), late[:4]
    run.snapshot.take(1)
    run.iterate(2, 3, 7)
    assert run.snapshot.restore() == 1
    now = run.state()
    assert sorted(now) == sorted(states[3])
    bad = [k for k in states[1] if not torch.equal(bits(states[1][k]), bits(now[k]))]
    assert not bad, "after the restore %s differ from the uninterrupted run after iteration 1" % bad[:4]
    for k in late:          # bit for bit what Nadam creates
        want = torch.tensor([0.0, 1.0], dtype=torch.float64, device=DEV) if k.endswith("/sched") else torch.zeros_like(now[k])
        assert torch.equal(bits(now[k]), bits(want)), k
    run.losses = []
    run.iterate(2, 3, 4, 5, 6)
    assert not differing(states[6], run.state())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(losses[1:], run.losses))


@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_a_poisoned_weight_and_back(mode):
    run = Run(mode).iterate(1, 2, 3)
    run.snapshot.take(3)
    name, weight = next((n, p) for n, p in run.D.named_parameters() if p.dim() >= 2 and p.numel() > 16 and "weight_u" not in n and "weight_v" not in n)
    with torch.no_grad():
        weight.view(-1)[5] = float("nan")
    if run.runner is not None:          # a replay reads the panels packed behind the previous step: re-pack them, as the optimizer would
        from locate_amd import ops
        ops.refresh_panels([p for p in run.D.parameters() if "_locate_panels" in p.__dict__])
    run.iterate(7, 8)
    run.snapshot.take(5)
    state = run.snapshot.status()
    assert (state["good"], state["iteration"], state["taken"], state["rejected"], state["last_rejected_iteration"]) == (0, 3, 1, 1, 5)
    assert state["last_rejected_tensor"].startswith("D/") and state["last_rejected_count"] >= 1
    assert run.step.dis_opt.counters()["consecutive_skips"] == 2          # the guard could only skip
    assert run.snapshot.restore() == 3
    assert run.step.dis_opt.counters()["consecutive_skips"] == 0 and run.step.dis_opt.counters()["skipped"] == 2
    assert_continues_like_the_uninterrupted_run(run, mode, "poison")


@pytest.mark.parametrize("mode", ["eager", "graphed"])
def test_a_snapshot_that_never_restores_changes_nothing(mode):
    states, losses = uninterrupted(mode)
    run = Run(mode)
    for k in range(1, 7):
        run.iterate(k)
        if k in (2, 4, 5):
            run.snapshot.take(k)
    assert not differing(states[6], run.state())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(losses, run.losses)) and len(run.losses) == 6
    state = run.snapshot.status()
    assert (state["good"], state["iteration"], state["taken"], state["rejected"]) == (0, 5, 3, 0)


def test_training_snapshot_entries():
    from locate_amd import TrainStep, TrainingSnapshot
    G, D, step, average = build_tiny()
    snap = TrainingSnapshot(step, average)
    g_sd, d_sd = list(G.state_dict()), list(D.state_dict())
    n_g, n_d = len(list(G.parameters())), len(list(D.parameters()))
    assert snap.names[:len(g_sd)] == ["G/" + k for k in g_sd]
    assert len(snap.names) == 2 * len(g_sd) + len(d_sd) + 3 * (n_g + n_d)
    assert snap.names[-len(g_sd):] == ["A/" + k for k in g_sd] and "G/noise" not in snap.names and "A/noise" not in snap.names
    assert snap.slot_bytes % 16 == 0 and snap.slot(0).numel() == snap.slot(1).numel() == snap.slot_bytes
    with pytest.raises(ValueError):
        snap.take(0)
    assert snap.status()["taken"] == 0
    step.reducer_g = object()
    with pytest.raises(ValueError):
        TrainingSnapshot(step)
    assert isinstance(step, TrainStep)


# ---- 7. the trainer, end to end ------------------------------------------------------------------------------------------------------
def make_trainer(out, store, **kw):
    from locate_amd import InputPipeline, RunStatistics, Trainer, TrainingSnapshot
    G, D, step, average = build_tiny()
    pipeline = InputPipeline(store, 32, 8, seed=11)
    t = Trainer(step, pipeline, str(out), epochs=1, max_iterations=12, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                image_interval_function=lambda batch: 1000, print_every_function=lambda batch: 2, average=average, stats=RunStatistics(G, D),
                stats_every=1, snapshot=TrainingSnapshot(step, average), rollback_every=2, **kw)
    assert pipeline.batches_per_epoch == 12
    name, weight = next((n, p) for n, p in D.named_parameters() if p.dim() >= 2 and p.numel() > 16 and "weight_u" not in n and "weight_v" not in n)
    iteration = t._iteration

    def poisoned_iteration():
        out = iteration()
        if t.iterations + 1 == 7:          # behind the seventh iteration
            with torch.no_grad():
                weight.view(-1)[5] = float("nan")
        return out
    t._iteration = poisoned_iteration
    return t, "D/" + name


def test_trainer_rolls_back(tmp_path):
    from locate_amd import DeviceImageStore, NonFiniteError
    store = DeviceImageStore(np.random.default_rng(6).integers(0, 256, size=(96, 78, 64, 3), dtype=np.uint8), DEV)
    out = tmp_path / "on"
    t, poisoned = make_trainer(out, store)
    assert t.run() == 12
    # takes at 2, 4, 6; the poison behind 7 is seen at the progress line of 8; back to 6; on with the batches of 9 ...
    with open(str(out / "error" / "rollbacks.json")) as f:
        records = json.load(f)
    assert len(records) == 1 and (records[0]["iteration"], records[0]["to_iteration"], records[0]["epoch"], records[0]["cause"]) == (7, 6, 1, "nonfinite")
    assert records[0]["tensors"][0][0] == poisoned
    assert not os.path.exists(str(out / "error" / "nonfinite.json"))
    saved = torch.load(str(out / "netD.torch"), map_location="cpu", weights_only=True)
    tensors = [v for v in saved.values() if torch.is_tensor(v)] if isinstance(saved, dict) else []
    assert tensors and all(bool(torch.isfinite(v).all()) for v in tensors if v.is_floating_point())
    assert all(bool(torch.isfinite(p).all()) for p in t.step.dis.parameters()) and all(bool(torch.isfinite(p).all()) for p in t.step.gen.parameters())
    with np.load(str(out / "error" / "1-stats.npz")) as z:          # the bad records stay as evidence
        at = z["iterations"].tolist()
        bad = [it for it, row in zip(at, z["nonfinite"]) if row.sum() > 0]
    assert bad == [7, 8] and at[-1] == 12
    state = torch.load(str(out / "trainer.torch"), map_location="cpu", weights_only=True)
    assert state["rollbacks"] == 1 and state["iterations"] == 12
    assert state["guard"]["D"]["consecutive_skips"] == 0 and state["guard"]["D"]["skipped"] >= 1
    status = t.snapshot.status()
    assert status["good"] >= 0 and status["iteration"] in (10, 12) and status["taken"] >= 4
    # max_rollbacks = 0: the same poison is what it always was
    out = tmp_path / "off"
    t, _ = make_trainer(out, store, max_rollbacks=0)
    with pytest.raises(NonFiniteError) as info:
        t.run()
    assert info.value.iteration == 7
    with open(str(out / "error" / "nonfinite.json")) as f:
        assert json.load(f)["iteration"] == 7
    assert not os.path.exists(str(out / "trainer.torch")) and not os.path.exists(str(out / "error" / "rollbacks.json"))


def test_command_line_flags(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    base = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--epochs", "1", "--minibatches", "1",
            "--images", "16", "--stats-every", "1", "--ema-half-life", "100", "--max-iterations", "4"]
    done = subprocess.run(base + ["--out", out, "--rollback-every", "2", "--max-rollbacks", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    state = torch.load(os.path.join(out, "trainer.torch"), map_location="cpu", weights_only=True)
    assert state["rollbacks"] == 0
    assert not os.path.exists(os.path.join(out, "error", "rollbacks.json")) and not os.path.exists(os.path.join(out, "error", "nonfinite.json"))
    # without the flag: no key
    done = subprocess.run(base + ["--out", out + "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "rollbacks" not in torch.load(os.path.join(out + "2", "trainer.torch"), map_location="cpu", weights_only=True)
