"""The averaged generator on the MI355X: the update kernel through the raw C ABI against the numpy float32 model
(tests/helpers/average_model.py) bit for bit - every size class, misaligned views, the exact copy, guards around every buffer -
and `AveragedGenerator` around a running training: it follows the live weights exactly as the model says, leaves the trajectory
where a run without it would be, gives a generator whose forward sees every update, and survives a save and a resume."""
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
import average_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
GUARD = 32                           # sentinel words on either side of every buffer
SENTINEL = 0x7FC0DEAD                # as int32: a NaN with a payload no arithmetic here produces - any write shows


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 1. - 2. the kernel through the raw ABI ---------------------------------------------------------------------------------------
class Arena:
    """float32 buffers inside ONE allocation, each between sentinel guards, each at a chosen offset (in elements) from a 16-byte
    boundary; the whole allocation is compared afterwards, so a write anywhere outside a buffer is seen"""

    def __init__(self):
        self.words = []          # int32 pieces
        self.spans = []          # (start, n) per buffer
        self.size = 0

    def add(self, values, offset):
        assert self.size % 4 == 0 and 0 <= offset < 4
        values = bits(values)
        start = self.size + GUARD + offset
        total = -(-(GUARD + offset + values.size + GUARD) // 4) * 4          # the next buffer starts on a 16-byte boundary again
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
        return self.dev

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.spans[i][0]


def launch(avg, src, weights, times=1):
    """the tables as AveragedGenerator builds them, then `times` launches"""
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_average_record_bytes() == 32
    chunk = L.locate_average_chunk_elems()
    rec, chunks = bytearray(), []
    for i, w in enumerate(weights):
        n = avg.spans[i][1]
        assert src.spans[i][1] == n
        rec += struct.pack("<QQqf4x", avg.ptr(i), src.ptr(i), n, w)
        chunks.extend((i, c) for c in range(-(-n // chunk)))
    t_dev = torch.frombuffer(rec, dtype=torch.uint8).clone().to(DEV)
    c_dev = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(DEV)
    for _ in range(times):
        check(L.locate_average_update(ctypes.c_void_p(t_dev.data_ptr()), ctypes.c_void_p(c_dev.data_ptr()), len(weights), len(chunks),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_average_update")
    torch.cuda.synchronize()
    return len(chunks)


def mixed_values(rng, n):
    """magnitudes from 1e-6 to 1e6, some zeros, some subnormals of both signs"""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32)
    kind = rng.integers(0, 8, size=n)
    x[kind == 0] = (rng.standard_normal(int((kind == 0).sum())) * 1e-40).astype(np.float32)          # subnormal
    x[kind == 1] = 0.0
    return x


SPECIAL = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF,
                    0x00400000, 0x3F800000], dtype=np.uint32).view(np.int32)       # NaNs with payloads (quiet, signalling), +-Inf, -0.0, subnormals
SIZES = [1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5]
OFFSETS = [(0, 0), (1, 0), (0, 1), (1, 1), (3, 0), (0, 3), (3, 3)]          # (avg, src) elements past a 16-byte boundary


def test_kernel_against_the_model_bit_for_bit():
    from locate_amd import average_weight
    rng = np.random.default_rng(12)
    weights_pool = [average_weight(half_life_images=10000, batch=64)[1], average_weight(half_life_images=64, batch=8)[1], 0.5]
    avg, src, weights, want = Arena(), Arena(), [], []
    for si, n in enumerate(SIZES):
        for oi, (oa, os_) in enumerate(OFFSETS):
            a, s = mixed_values(rng, n), mixed_values(rng, n)
            w = weights_pool[(si + oi) % 3]
            avg.add(a, oa)
            src.add(s, os_)
            weights.append(w)
            for _ in range(8):
                a = M.update32(a, s, w)
            want.append(a)
    # three exact copies: 16-byte path with a tail, the scalar path over two chunks, a tensor shorter than one 16-byte word
    for n, (oa, os_) in ((65, (0, 0)), (4097, (1, 1)), (3, (0, 3))):
        s = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
        s[:min(n, SPECIAL.size)] = SPECIAL[:min(n, SPECIAL.size)]
        avg.add(mixed_values(rng, n), oa)
        src.add(s.view(np.float32), os_)
        weights.append(1.0)
        want.append(s.view(np.float32))
    assert len(weights) == 73
    expected = avg.host().copy()
    for (start, n), w in zip(avg.spans, want):
        expected[start:start + n] = bits(w)
    src_before = src.host().copy()
    avg.upload()
    src.upload()
    n_chunks = launch(avg, src, weights, times=8)
    got = avg.dev.cpu().numpy()
    assert np.array_equal(src.dev.cpu().numpy(), src_before), "a source was written"
    for i, (start, n) in enumerate(avg.spans):
        lo, hi = start - GUARD, start + n + GUARD
        assert np.array_equal(got[start:hi - GUARD], expected[start:hi - GUARD]), \
            "tensor %d (n = %d, weight %r): %d of %d elements differ" % (i, n, weights[i], int((got[start:start + n] != expected[start:start + n]).sum()), n)
        assert (got[lo:start] == SENTINEL).all() and (got[start + n:hi] == SENTINEL).all(), "tensor %d: a guard was written" % i
    assert np.array_equal(got, expected)          # and nothing anywhere else
    copied = got[avg.spans[70][0]:avg.spans[70][0] + SPECIAL.size]
    assert np.array_equal(copied, SPECIAL)          # NaN payloads, Inf, -0.0 and subnormals arrive as they are
    subnormal = [(np.abs(w) > 0) & (np.abs(w) < 1.1754944e-38) for w in want[:70]]
    print("%d tensors, %d chunks, %d subnormal results" % (len(weights), n_chunks, sum(int(m.sum()) for m in subnormal)))
    assert sum(int(m.sum()) for m in subnormal) > 0


@pytest.mark.parametrize("offset", [0, 1])
def test_chunk_boundaries(offset):
    from locate_amd import average_weight
    from locate_amd._lib import lib
    chunk = lib().locate_average_chunk_elems()
    n = 2 * chunk + 1
    w = average_weight(beta=0.999)[1]
    ramp = np.arange(1, n + 1, dtype=np.float32)
    avg, src = Arena(), Arena()
    avg.add(np.zeros(n, np.float32), offset)
    src.add(ramp, offset)
    expected = avg.host().copy()
    expected[avg.spans[0][0]:avg.spans[0][0] + n] = bits(M.update32(np.zeros(n, np.float32), ramp, w))
    avg.upload()
    src.upload()
    assert launch(avg, src, [w]) == 3
    got = avg.dev.cpu().numpy()
    bad = np.nonzero(got != expected)[0]
    assert bad.size == 0, "first differences at words %s (the buffer starts at %d, chunks of %d)" % (bad[:8], avg.spans[0][0], chunk)


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    for args in ((None, p, 1, 1), (p, None, 1, 1), (p, p, 0, 1), (p, p, 1, 0)):
        assert L.locate_average_update(*args, None) == 1
        assert b"locate_average_update" in L.locate_last_error()


# ---- 3. - 5. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) -------------
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


def host_copy(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def is_uv(name):
    return name.endswith(("weight_u", "weight_v"))


def average(G):
    from locate_amd import AveragedGenerator
    return AveragedGenerator(G, half_life_images=64, batch=8)          # beta = 0.917: six updates move the average visibly


@pytest.mark.parametrize("launch_mode", ["eager", "graphed"])
def test_the_average_follows_the_training_and_does_not_touch_it(launch_mode):
    from locate_amd.graph import GraphedTrainStep

    def run(averaged):
        G, D, step, (lat, real, aug) = build_tiny()
        avg = average(G) if averaged else None
        snaps = [host_copy(G)] if averaged else []
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch_mode == "graphed" else None
        for _ in range(6):
            if runner is not None:
                runner.replay()
            else:
                step(lat, real, aug)
            if averaged:
                snaps.append(host_copy(G))
                avg.update()
        return training_state(G, D, step), avg, snaps

    plain, _, _ = run(False)
    followed, avg, snaps = run(True)
    # (a) the training is where it would be without the average
    assert sorted(plain) == sorted(followed)
    bad = [k for k in plain if not torch.equal(plain[k], followed[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch_mode, len(bad), len(plain), bad[:4])
    assert any(is_uv(k) for k in plain)
    # (b) the average is the model applied to the live weights after every iteration; u / v are the live ones
    assert avg.updates == 6 and len(snaps) == 7
    got = host_copy(avg.generator)
    assert sorted(got) == sorted(snaps[0])
    moved = 0
    for k in got:
        want = snaps[0][k]
        for snap in snaps[1:]:
            want = M.update32(want, snap[k], 1.0 if is_uv(k) else avg.one_minus_beta)
        assert np.array_equal(bits(got[k]), bits(want)), "%s %s: %d of %d elements differ" % (launch_mode, k, int((bits(got[k]) != bits(want)).sum()), want.size)
        if is_uv(k):
            assert np.array_equal(bits(got[k]), bits(snaps[-1][k]))
        else:
            moved += int(not np.array_equal(got[k], snaps[-1][k]) and not np.array_equal(got[k], snaps[0][k]))
    assert moved > 10, "the training did not move the weights: nothing was tested"
    assert torch.equal(avg.generator.noise, avg.source.noise) and avg.generator.noise.data_ptr() != avg.source.noise.data_ptr()
    assert not any(q.requires_grad for q in avg.generator.parameters())
    assert not any("_locate_wmax" in q.__dict__ for q in avg.generator.parameters())


def sample(gen, latents):
    """eval mode, no_grad, u / v put back afterwards: the same start for every forward that is compared"""
    from locate_amd import Sampler
    return Sampler(gen, fixed_noise=latents, advance_spectral_norm=False).sample().clone()


def small_metric(seed=4):
    from locate_amd import SlicedWasserstein
    swd = SlicedWasserstein(32, images=16, nhoods_per_image=8, dir_repeats=2, dirs_per_repeat=8, seed=seed, chunk=8, device=DEV)
    return swd.set_reference(torch.randn(16, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV))


def test_the_average_is_usable():
    from locate_amd import Generator
    G, D, step, (lat, real, aug) = build_tiny()
    rng_state = torch.random.get_rng_state()
    avg = average(G)
    assert torch.equal(torch.random.get_rng_state(), rng_state)          # building it draws nothing that a run could notice
    own = avg.generator
    assert own is not G and own.runtime is not G.runtime and own.batched_spectral_norm and own.runtime.precision == G.runtime.precision
    assert own.training == G.training and own.cfg is G.cfg
    live = {k: v.data_ptr() for k, v in G.state_dict(keep_vars=True).items()}
    assert all(v.data_ptr() != live[k] for k, v in own.state_dict(keep_vars=True).items())
    # at updates == 0 it IS the live generator: same mode, same batch, same u / v -> the same bits (its panels are packed here)
    first = sample(own, lat)
    assert avg.updates == 0 and torch.equal(first, sample(G, lat))
    for _ in range(3):
        step(lat, real, aug)
        avg.update()
    out, live_out = sample(own, lat), sample(G, lat)
    assert tuple(out.shape) == (8, 3, 32, 32) and bool(torch.isfinite(out).all())
    assert not torch.equal(out, live_out) and not torch.equal(out, first)
    # the forward saw the update: a generator built from the averaged state now, with nothing cached, gives the same bits
    fresh = Generator(G.cfg)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in own.state_dict().items()}, strict=True)
    fresh.noise = own.noise.detach().cpu().clone()
    fresh = fresh.to(DEV)
    fresh.batched_spectral_norm = True
    assert torch.equal(out, sample(fresh, lat))
    # one more update, forwarded again: still not stale
    step(lat, real, aug)
    avg.update()
    fresh.load_state_dict(own.state_dict(), strict=True)
    assert torch.equal(sample(own, lat), sample(fresh, lat)) and not torch.equal(sample(own, lat), out)
    # the metric takes it like any generator, and leaves it as it was
    swd = small_metric()
    before = {k: v.detach().clone() for k, v in own.state_dict().items()}
    values = [swd.evaluate(own), swd.evaluate(own)]
    assert values[0] == values[1] and len(values[0]["levels"]) == 2 and all(math.isfinite(v) and v > 0 for v in values[0]["levels"])
    after = own.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    # reset(): the live generator again
    assert avg.reset().updates == 0 and torch.equal(sample(own, lat), sample(G, lat))


def test_state_survives_a_round_trip_on_the_device():
    G, _, step, (lat, real, aug) = build_tiny()
    a = average(G)
    step(lat, real, aug)
    a.update()
    state = a.state_dict()
    G2, _, _, _ = build_tiny()
    b = average(G2)
    ptrs = [q.data_ptr() for q in b.generator.parameters()]
    table = b._table()
    b.load_state_dict(state)
    assert b.updates == 1 and [q.data_ptr() for q in b.generator.parameters()] == ptrs and b._table() is table
    assert all(torch.equal(v, a.generator.state_dict()[k]) for k, v in b.generator.state_dict().items())
    from locate_amd import AveragedGenerator
    with pytest.raises(ValueError):
        AveragedGenerator(G2, beta=0.5).load_state_dict(state)


def test_trainer_and_resume(tmp_path):
    from locate_amd import DeviceImageStore, Generator, InputPipeline, SlicedWasserstein, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, averaged=True):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        swd = SlicedWasserstein(32, images=16, nhoods_per_image=8, dir_repeats=2, dirs_per_repeat=8, seed=3, chunk=8, device=DEV)
        swd.reference_from_pipeline(pipeline)
        avg = average(G) if averaged else None
        t = Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                    subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, swd=swd, average=avg)
        return t, avg

    whole, avg_whole = trainer(tmp_path / "whole", 6)
    assert whole.run() == 6 and avg_whole.updates == 6
    rel = [os.path.relpath(f, str(tmp_path / "whole")) for f in whole.written]
    pictures = [f for f in rel if f.endswith(".png") and not f.endswith(".ema.png")]
    assert pictures == ["1/1-2.png", "1/1-4.png", "1/1-END.png", "2/1-2.png"]
    for f in pictures:
        twin = f[:-4] + ".ema.png"
        assert rel.index(twin) == rel.index(f) + 1 and os.path.getsize(str(tmp_path / "whole" / twin)) > 0
    from locate_amd.monitor import read_png
    assert read_png(str(tmp_path / "whole" / "1/1-4.ema.png")).shape == read_png(str(tmp_path / "whole" / "1/1-4.png")).shape
    assert not np.array_equal(read_png(str(tmp_path / "whole" / "1/1-4.ema.png")), read_png(str(tmp_path / "whole" / "1/1-4.png")))
    # netG_ema.torch: the reference's layout
    fresh = Generator(avg_whole.generator.cfg)
    saved = torch.load(str(tmp_path / "whole" / "netG_ema.torch"), map_location="cpu", weights_only=True)
    fresh.load_state_dict(saved, strict=True)
    assert "netG_ema.torch" in rel and all(torch.equal(v.cpu(), saved[k]) for k, v in avg_whole.generator.state_dict().items())
    rec = json.load(open(str(tmp_path / "whole" / "error" / "swd.json")))
    assert len(rec) == 1 and sorted(rec[0]) == ["average", "epoch", "iterations", "levels", "mean"] and sorted(rec[0]["average"]) == ["levels", "mean"]
    assert len(rec[0]["average"]["levels"]) == 2 and all(math.isfinite(v) and v > 0 for v in rec[0]["average"]["levels"] + [rec[0]["average"]["mean"]])
    assert rec[0]["average"]["levels"] != rec[0]["levels"]
    state = torch.load(str(tmp_path / "whole" / "trainer.torch"), map_location="cpu", weights_only=True)
    assert state["average"]["updates"] == 6

    # 3 + save + fresh objects + resume + 3
    head, avg_head = trainer(tmp_path / "parts", 3)
    assert head.run() == 3 and avg_head.updates == 3
    tail, avg_tail = trainer(tmp_path / "parts", 6)
    assert avg_tail.updates == 0
    assert tail.resume().iterations == 3 and avg_tail.updates == 3
    assert all(torch.equal(v, avg_head.generator.state_dict()[k]) for k, v in avg_tail.generator.state_dict().items())
    assert tail.run() == 6 and avg_tail.updates == 6
    a, b = avg_whole.generator.state_dict(), avg_tail.generator.state_dict()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, "%d of %d averaged tensors differ after the resume, first %s" % (len(bad), len(a), bad[:4])
    assert torch.equal(avg_whole.generator.noise, avg_tail.generator.noise)

    # a state without an average: the average starts from the resumed weights
    plain, _ = trainer(tmp_path / "plain", 3, averaged=False)
    assert plain.run() == 3
    rel_plain = [os.path.relpath(f, str(tmp_path / "plain")) for f in plain.written]
    assert not [f for f in rel_plain if "ema" in f] and not os.path.exists(str(tmp_path / "plain" / "netG_ema.torch"))
    assert "average" not in torch.load(str(tmp_path / "plain" / "trainer.torch"), map_location="cpu", weights_only=True)
    assert rel_plain == [f for f in (os.path.relpath(g, str(tmp_path / "parts")) for g in head.written) if "ema" not in f]          # today's files
    late, avg_late = trainer(tmp_path / "plain", 6)
    late.resume()
    assert avg_late.updates == 0
    live = late.gen.state_dict()
    assert all(torch.equal(v, live[k]) for k, v in avg_late.generator.state_dict().items())
    assert all(torch.equal(v, avg_head.source.state_dict()[k]) for k, v in live.items())          # the weights after three iterations


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))

    def files(out, extra):
        cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
               "--minibatches", "1", "--images", "16"] + extra
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
        assert "4 iterations" in done.stdout
        return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)

    with_flag = files(str(tmp_path / "on"), ["--ema-half-life", "64"])
    without = files(str(tmp_path / "off"), [])
    ema = [f for f in with_flag if "ema" in f]
    assert ema == ["1/1-END.ema.png", "netG_ema.torch"]
    assert without == [f for f in with_flag if f not in ema]          # without the flag: the files there were before it existed
    for name in ("0.png", "1.png", "1/1-END.png", "error/1.json", "netD.torch", "netG.extra.torch", "netG.torch", "optD.torch", "optG.torch", "trainer.torch"):
        assert name in without, name
    state = torch.load(os.path.join(str(tmp_path / "on"), "trainer.torch"), map_location="cpu", weights_only=True)
    assert state["average"]["updates"] == 4
    assert state["average"]["one_minus_beta"] == float(np.float32(1.0 - 0.5 ** (8 / 64)))
    assert "average" not in torch.load(os.path.join(str(tmp_path / "off"), "trainer.torch"), map_location="cpu", weights_only=True)
