"""Top-k training beside the training step on the MI355X, on the tiny fixture network of tests/test_gpu_lecam_step.py (32 x 32, base
width 1, batch 8), a few iterations each: with gamma = 1 - k stays the batch size - the run is the run without a TopK, bit for bit,
eager and replayed; with floor = 0.5, gamma = 0.5, every = 1 every iteration follows the numpy definition fed with the recorded logits
and the scheduled k, a replayed run equals the eager one while k moves between replays, and the run is not the plain one; the Trainer
writes error/topk.json and a resumed run continues record, curve and weights."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import topk_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
S, B = 32, 8
ANNEALED = dict(floor=0.5, gamma=0.5, every=1)          # k: 8, 4, 4, ...


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def build_tiny(topk=None):
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=S, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1, topk=topk)
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


def differing(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def make(**kw):
    from locate_amd import TopK
    return TopK(batch=B, device=DEV, **dict(dict(capacity=16), **kw))


def record(out, topk, losses, launches):
    losses += [out["d_error"].clone(), out["g_error"].clone(), out["penalty"].clone()]
    if topk is not None:
        launches.append((out["g_logits"].clone(), out["g_error"].clone(), out["g_error_all"].clone(), topk.state.clone()))
    else:
        assert "g_error_all" not in out and "g_logits" not in out


def run_eager(topk, iterations=4, warmup=2):
    """`warmup` plain calls of the step - what a capture's warm-up runs, with the k the record starts from - then TrainLoop.iteration,
    which moves k itself; (state, losses, (g_logits, g_error, g_error_all, record) of every launch, the warm-up's included)"""
    from locate_amd import TrainLoop
    G, D, step, (lat, real, aug) = build_tiny(topk)
    losses, launches = [], []
    for _ in range(warmup):
        record(step(lat, real, aug), topk, [], launches)
    loop = TrainLoop(step)
    for _ in range(iterations):
        record(loop.iteration(lat, real, aug), topk, losses, launches)
    return training_state(G, D, step), losses, launches


def run_replayed(topk, replays=4):
    """the capture's two warm-up iterations, then replays with advance() before each, as the Trainer does"""
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny(topk)
    runner = GraphedTrainStep(step, lat, real, aug, warmup=2)
    losses, launches = [], []
    for n in range(replays):
        if topk is not None:
            topk.advance(n)
        record(runner.replay(), topk, losses, launches)
    return training_state(G, D, step), losses, launches


def same(one, two):
    assert not differing(one[0], two[0])
    assert len(one[1]) == len(two[1]) and all(torch.equal(a, b) for a, b in zip(one[1], two[1]))


_PLAIN = {}


def plain(replayed):
    """the run without a TopK, made once"""
    if replayed not in _PLAIN:
        _PLAIN[replayed] = run_replayed(None) if replayed else run_eager(None)
    return _PLAIN[replayed]


def words(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).reshape(-1).view(np.uint32)


def follows_the_model(topk, launches, ks, ring_rows=16):
    """every launch's two losses and the record behind it, then the ring and the curve, against the definition fed with the recorded
    logits and the k of that launch; returns the k_used's"""
    state, ring = M.new_state(B), M.new_ring(ring_rows)
    used = []
    for n, ((logits, g_error, g_error_all, rec), k) in enumerate(zip(launches, ks)):
        state[0] = k
        want = M.g_loss(logits.cpu().numpy(), state, ring)[0]
        assert words(g_error)[0] == words(T(want))[0] and words(g_error_all)[0] == words(T(want))[1], (n, g_error, g_error_all, want)
        assert np.array_equal(words(rec), state), (n, words(rec), state)
        used.append(int(state[3]))
    assert np.array_equal(words(topk.state), state) and np.array_equal(words(topk.ring), ring.reshape(-1))
    assert topk.flush() == M.curve(ring, 0, len(launches)) and topk.curve() == M.curve(ring, 0, len(launches))
    return used


@pytest.mark.parametrize("replayed", [False, True])
def test_with_gamma_one_the_run_is_the_run_without_a_topk(replayed):
    topk = make(gamma=1.0, floor=0.5, every=1)
    run = run_replayed(topk) if replayed else run_eager(topk)
    same(plain(replayed), run)
    assert any(k.endswith("weight_u") for k in run[0]) and any("/opt/" in k for k in run[0])
    if not replayed:
        assert follows_the_model(topk, run[2], [B] * 6) == [B] * 6
        assert all(torch.equal(g_error, g_error_all) for _, g_error, g_error_all, _ in run[2])
    else:
        assert topk.status()["launches"] == 6 and topk.status()["k_used"] == B


def test_annealed_the_run_follows_the_definition_and_a_replay_equals_eager():
    eager_topk, replayed_topk = make(**ANNEALED), make(**ANNEALED)
    eager = run_eager(eager_topk)
    ks = [B, B] + [M.topk_k(B, 0.5, 0.5, n) for n in range(4)]          # the warm-up runs with the k the record starts from
    assert ks == [8, 8, 8, 4, 4, 4]
    assert follows_the_model(eager_topk, eager[2], ks) == ks
    print("g_error / g_error_all per launch: %r" % [(float(a), float(b)) for _, a, b, _ in eager[2]])
    # the loss over the better half is not above the loss over all: relu(1 - f) falls with f
    assert all(float(a) <= float(b) for _, a, b, _ in eager[2][3:])
    replayed = run_replayed(replayed_topk)
    same(eager, replayed)
    assert len(replayed[2]) == 4 and all(torch.equal(a, b) for x, y in zip(eager[2][2:], replayed[2]) for a, b in zip(x, y))
    assert torch.equal(eager_topk.state, replayed_topk.state) and torch.equal(eager_topk.ring, replayed_topk.ring)
    assert [row["k"] for row in replayed_topk.flush()] == ks
    # and it is a top-k run: not the plain one of as many iterations
    assert differing(plain(False)[0], eager[0])
    assert any(not torch.equal(a, b) for a, b in zip(plain(False)[1], eager[1]))


def test_trainer_writes_topk_json_and_a_resumed_run_continues_it(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, topk):
        G, D, step, _ = build_tiny(topk)
        pipeline = InputPipeline(store, S, B, seed=11)
        t = Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                    subepoch_function=lambda e: 1, image_interval_function=lambda batch: 100)
        assert t.topk is topk
        return t

    def topk_json(out):
        with open(str(out / "error" / "topk.json")) as f:
            return json.load(f)

    a_whole = make(**ANNEALED)
    whole = trainer(tmp_path / "whole", 3, a_whole)
    assert whole.run() == 3
    rec = topk_json(tmp_path / "whole")
    assert sorted(rec) == ["active", "curve", "k", "k_used", "launches", "mean_all", "mean_kept", "nonfinite", "threshold"]
    assert [sorted(row) for row in rec["curve"]] == [["active", "k", "launch", "mean_all", "mean_kept", "nonfinite", "threshold"]] * 3
    assert [row["launch"] for row in rec["curve"]] == [1, 2, 3] and [row["k"] for row in rec["curve"]] == [8, 4, 4]
    assert rec["launches"] == 3 and rec["k"] == 4 and rec["k_used"] == 4 and rec["nonfinite"] == 0
    assert rec["threshold"] == rec["curve"][-1]["threshold"] and rec["mean_kept"] == rec["curve"][-1]["mean_kept"]
    assert all(row["mean_kept"] >= row["threshold"] and row["mean_kept"] >= row["mean_all"] for row in rec["curve"])
    assert str(tmp_path / "whole" / "error" / "topk.json") in whole.written

    a_head = make(**ANNEALED)
    head = trainer(tmp_path / "parts", 2, a_head)
    assert head.run() == 2
    assert topk_json(tmp_path / "parts")["curve"] == rec["curve"][:2]
    saved = torch.load(str(tmp_path / "parts" / "trainer.torch"), map_location="cpu", weights_only=True)["topk"]
    assert int(saved["record"][1]) == 2 and saved["settings"]["every"] == 1
    a_tail = make(**ANNEALED)
    tail = trainer(tmp_path / "parts", 3, a_tail)
    assert tail.resume().iterations == 2 and a_tail.status() == a_head.status()
    assert tail.run() == 3
    assert topk_json(tmp_path / "parts") == rec
    assert torch.equal(a_tail.state, a_whole.state)
    assert not differing(training_state(whole.gen, whole.dis, whole.step), training_state(tail.gen, tail.dis, tail.step))
    # without a TopK: no topk.json; a state saved with other settings is refused; a state without one starts the curve there
    t = trainer(tmp_path / "none", 1, None)
    assert t.run() == 1 and not os.path.exists(str(tmp_path / "none" / "error" / "topk.json"))
    with pytest.raises(ValueError, match="ran with"):
        trainer(tmp_path / "parts", 4, make(floor=0.5, gamma=0.5, every=2)).resume()
    fresh = make(**ANNEALED)
    assert trainer(tmp_path / "none", 2, fresh).resume().iterations == 1 and fresh.status()["launches"] == 0
