"""The LeCam regulariser beside the training step on the MI355X, on the tiny fixture network of tests/test_gpu_ada_step.py (32 x 32,
base width 1, batch 8), a few iterations each: inactive - weight 0, or a warmup beyond the run - the run is the run without a LeCam,
bit for bit, eager and replayed, with the anchors recorded; active, it follows the numpy definition fed with the recorded logits
and a replayed run equals the eager one; the Trainer writes error/lecam.json and a resumed run continues anchors, curve and
weights."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lecam_model as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
S, B = 32, 8


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def build_tiny(lecam=None):
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
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1, lecam=lecam)
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
    from locate_amd import LeCam
    return LeCam(batch=B, device=DEV, **dict(dict(decay=0.75, capacity=16), **kw))


def record(out, losses, logits):
    losses += [out["d_error"].clone(), out["g_error"].clone(), out["penalty"].clone()]
    logits.append((out["d_true"].clone(), out["d_gen"].clone(), out["lecam"].clone() if "lecam" in out else None))


def run_eager(lecam, iterations=3, unobserved=0):
    """`unobserved` plain calls of the step - what a capture's warm-up runs - then TrainLoop.iteration, which observes itself;
    (state, losses, (d_true, d_gen, R) of every observed iteration)"""
    from locate_amd import TrainLoop
    G, D, step, (lat, real, aug) = build_tiny(lecam)
    for _ in range(unobserved):
        step(lat, real, aug)
    loop = TrainLoop(step)
    losses, logits = [], []
    for _ in range(iterations):
        record(loop.iteration(lat, real, aug), losses, logits)
    return training_state(G, D, step), losses, logits


def run_replayed(lecam, replays=3):
    """the capture's two warm-up iterations, then replays with observe() after each, as the Trainer does"""
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny(lecam)
    runner = GraphedTrainStep(step, lat, real, aug, warmup=2)
    losses, logits = [], []
    for _ in range(replays):
        out = runner.replay()
        if lecam is not None:
            lecam.observe(out["d_true"], out["d_gen"])
        record(out, losses, logits)
    return training_state(G, D, step), losses, logits


def same(one, two):
    assert not differing(one[0], two[0])
    assert len(one[1]) == len(two[1]) and all(torch.equal(a, b) for a, b in zip(one[1], two[1]))


_PLAIN = {}


def plain(replayed):
    """the run without a LeCam, made once"""
    if replayed not in _PLAIN:
        _PLAIN[replayed] = run_replayed(None) if replayed else run_eager(None)
    return _PLAIN[replayed]


def follows_the_model(lecam, logits, weight, one_sided, warmup, ring_rows=16):
    """anchors, ring, status and every iteration's R against the definition fed with the recorded logits; returns the R's"""
    state, ring = L.new_state(), L.new_ring(ring_rows)
    seen = []
    for k, (d_true, d_gen, R) in enumerate(logits, 1):
        t, g = d_true.cpu().numpy(), d_gen.cpu().numpy()
        want = L.d_loss(t, -g, np.zeros(B, np.float32), 100.0, state, weight, one_sided, warmup)[0][3]          # R does not read d_aug
        got = R.cpu().numpy().reshape(1)
        assert np.array_equal(got.view(np.uint32), np.array([want], np.float32).view(np.uint32)), (k, got, want)
        seen.append(float(got[0]))
        L.observe(t, g, k, state, ring, lecam.rate)
    assert np.array_equal(lecam.state.cpu().numpy().view(np.uint32), state)
    assert np.array_equal(lecam.ring.cpu().numpy().view(np.uint32), ring)
    s = L.fields(state)
    assert lecam.status() == {"anchor_real": float(s["alpha_r"]), "anchor_fake": float(s["alpha_f"]), "observations": len(logits),
                              "accepted": len(logits), "nonfinite": 0, "active": L.is_active(state, weight, warmup)}
    assert lecam.flush() == L.curve(ring, 0, len(logits)) and lecam.curve() == L.curve(ring, 0, len(logits))
    return seen


@pytest.mark.parametrize("replayed", [False, True])
@pytest.mark.parametrize("settings", [dict(weight=0.0, warmup=0), dict(weight=0.3, warmup=10 ** 6)])
def test_inactive_the_run_is_the_run_without_a_lecam(settings, replayed):
    lecam = make(**settings)
    run = run_replayed(lecam) if replayed else run_eager(lecam)
    same(plain(replayed), run)
    seen = follows_the_model(lecam, run[2], settings["weight"], True, settings["warmup"])
    assert seen == [0.0, 0.0, 0.0] and not lecam.status()["active"] and lecam.status()["anchor_real"] != lecam.status()["anchor_fake"]
    assert any(k.endswith("weight_u") for k in run[0]) and any("/opt/" in k for k in run[0])


@pytest.mark.parametrize("one_sided", [True, False])
def test_active_the_run_follows_the_definition_and_a_replay_equals_eager(one_sided):
    eager_lecam, replayed_lecam = make(weight=0.3, warmup=0, one_sided=one_sided), make(weight=0.3, warmup=0, one_sided=one_sided)
    eager = run_eager(eager_lecam, iterations=4, unobserved=2)
    seen = follows_the_model(eager_lecam, eager[2], 0.3, one_sided, 0)
    print("R per iteration (one_sided=%s): %r" % (one_sided, seen))
    assert seen[0] == 0.0          # no anchor yet in the first observed iteration
    if one_sided:
        # the clamped form is silent while every D(real) lies below the generated anchor and every D(G(z)) above the real one -
        # what a discriminator that has not yet learned to separate them can show; it is never negative
        assert all(r >= 0.0 for r in seen[1:])
    else:
        assert all(r > 0.0 for r in seen[1:])
    replayed = run_replayed(replayed_lecam, replays=4)
    same(eager, replayed)
    assert all(torch.equal(a, b) for x, y in zip(eager[2], replayed[2]) for a, b in zip(x, y))
    assert torch.equal(eager_lecam.state, replayed_lecam.state) and torch.equal(eager_lecam.ring, replayed_lecam.ring)
    # and wherever the regulariser spoke it is a regularised run: not the plain one of as many iterations
    if "six" not in _PLAIN:
        _PLAIN["six"] = run_eager(None, iterations=4, unobserved=2)
    if any(r > 0.0 for r in seen):
        assert differing(_PLAIN["six"][0], eager[0])


def test_trainer_writes_lecam_json_and_a_resumed_run_continues_it(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, lecam):
        G, D, step, _ = build_tiny(lecam)
        pipeline = InputPipeline(store, S, B, seed=11)
        t = Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                    subepoch_function=lambda e: 1, image_interval_function=lambda batch: 100)
        assert t.lecam is lecam
        return t

    def lecam_json(out):
        with open(str(out / "error" / "lecam.json")) as f:
            return json.load(f)

    a_whole = make(weight=0.3, warmup=1)
    whole = trainer(tmp_path / "whole", 3, a_whole)
    assert whole.run() == 3
    rec = lecam_json(tmp_path / "whole")
    assert sorted(rec) == ["accepted", "active", "anchor_fake", "anchor_real", "curve", "nonfinite", "observations"]
    assert [sorted(row) for row in rec["curve"]] == [["accepted", "anchor_fake", "anchor_real", "iteration", "mean_fake", "mean_real"]] * 3
    assert [row["iteration"] for row in rec["curve"]] == [1, 2, 3] and rec["observations"] == 3 and rec["active"] is True
    assert rec["anchor_real"] == rec["curve"][-1]["anchor_real"] and rec["anchor_fake"] == rec["curve"][-1]["anchor_fake"]
    assert str(tmp_path / "whole" / "error" / "lecam.json") in whole.written

    a_head = make(weight=0.3, warmup=1)
    head = trainer(tmp_path / "parts", 2, a_head)
    assert head.run() == 2
    assert lecam_json(tmp_path / "parts")["curve"] == rec["curve"][:2]
    saved = torch.load(str(tmp_path / "parts" / "trainer.torch"), map_location="cpu", weights_only=True)["lecam"]
    assert saved["observations"] == 2 and saved["settings"]["warmup"] == 1
    a_tail = make(weight=0.3, warmup=1)
    tail = trainer(tmp_path / "parts", 3, a_tail)
    assert tail.resume().iterations == 2 and a_tail.status() == a_head.status()
    assert tail.run() == 3
    assert lecam_json(tmp_path / "parts") == rec
    assert torch.equal(a_tail.state, a_whole.state)
    assert not differing(training_state(whole.gen, whole.dis, whole.step), training_state(tail.gen, tail.dis, tail.step))
    # without a LeCam: no lecam.json; a state saved with other settings is refused; a state without one starts the anchors there
    t = trainer(tmp_path / "none", 1, None)
    assert t.run() == 1 and not os.path.exists(str(tmp_path / "none" / "error" / "lecam.json"))
    with pytest.raises(ValueError, match="ran with"):
        trainer(tmp_path / "parts", 4, make(weight=0.3, warmup=2)).resume()
    fresh = make(weight=0.3, warmup=1)
    assert trainer(tmp_path / "none", 2, fresh).resume().iterations == 1 and fresh.status()["observations"] == 0
