"""The adaptive augmentation beside the training step on the MI355X, on the tiny fixture network of tests/test_gpu_diffaug_step.py
(32 x 32, base width 1, batch 8), a few iterations each: at p = 0 the run is the run without an augment and at p = 1 the plain
DiffAugment run, bit for bit, eager and replayed; a moving p follows the numpy definition fed with the recorded logits; the Trainer
writes error/ada.json and a resumed run continues curve and weights."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ada_model as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
FULL = "color,translation,cutout"
S, B = 32, 8


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def build_tiny(augment=None):
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
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1, augment=augment)
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


def adaptive(seed=5, **kw):
    from locate_amd import AdaptiveDiffAugment
    return AdaptiveDiffAugment(S=S, batch=B, policy=FULL, seed=seed, device=DEV, **kw)


def run_eager(augment, iterations=3):
    """through TrainLoop.iteration, which draws and observes itself; (state, losses, logits of every iteration)"""
    from locate_amd import TrainLoop
    G, D, step, (lat, real, aug) = build_tiny(augment)
    loop = TrainLoop(step)
    losses, logits = [], []
    for _ in range(iterations):
        out = loop.iteration(lat, real, aug)
        losses += [out["d_error"].clone(), out["g_error"].clone(), out["penalty"].clone()]
        logits.append(out["d_true"].clone())
    return training_state(G, D, step), losses, logits


def run_replayed(augment, replays=3):
    """the capture's two warm-up iterations on one draw, then replays with draw() before and observe() after each, as the Trainer does"""
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny(augment)
    if augment is not None:
        augment.draw()
    runner = GraphedTrainStep(step, lat, real, aug, warmup=2)
    losses = []
    for _ in range(replays):
        if augment is not None:
            augment.draw()
        out = runner.replay()
        if hasattr(augment, "observe"):
            augment.observe(out["d_true"])
        losses += [out["d_error"].clone(), out["g_error"].clone(), out["penalty"].clone()]
    return training_state(G, D, step), losses


def same(one, two):
    assert not differing(one[0], two[0])
    assert len(one[1]) == len(two[1]) and all(torch.equal(a, b) for a, b in zip(one[1], two[1]))


def test_at_p_0_the_run_is_the_run_without_an_augment():
    """initial_p = 0 and a target that r_t <= 1 never exceeds: every image's ops are masked, T is a copy"""
    a = adaptive(target=1.0, interval=1, kimg=0.001)
    plain, eager = run_eager(None), run_eager(a)
    same(plain, eager)
    status = a.status()
    assert status["p"] == 0.0 and status["updates"] == 3 and status["ups"] == 0 and a.draws == 3
    assert (a.params[:, 9] == 7.0).all() and (a.params[:, 10:] == 0.0).all()
    b = adaptive(target=1.0, interval=1, kimg=0.001)
    same(run_replayed(None), run_replayed(b))
    assert b.status()["p"] == 0.0 and b.status()["updates"] == 3          # the two warm-up iterations were not observed
    assert any(k.endswith("weight_u") for k in plain[0]) and any("/opt/" in k for k in plain[0])


def test_at_p_1_the_run_is_the_plain_diffaugment_run():
    from locate_amd import DiffAugment
    a = adaptive(seed=9, kimg=float("inf"), initial_p=1.0)
    same(run_eager(DiffAugment(S=S, batch=B, policy=FULL, seed=9, device=DEV)), run_eager(a))
    assert a.status()["p"] == 1.0 and a.observations == 3 and not a.params[:, 9:].any()
    b = adaptive(seed=9, kimg=float("inf"), initial_p=1.0)
    same(run_replayed(DiffAugment(S=S, batch=B, policy=FULL, seed=9, device=DEV)), run_replayed(b))
    # and it is an augmented run: not the run without an augment
    assert differing(run_eager(None)[0], run_eager(adaptive(seed=9, kimg=float("inf"), initial_p=1.0))[0])


def test_a_moving_p_follows_the_definition_fed_with_the_recorded_logits():
    settings = dict(target=0.0, interval=2, kimg=0.064, initial_p=0.5, p_max=0.875)          # step = 8 * 2 / 64 = 0.25
    a = adaptive(seed=2, capacity=2, **settings)
    assert a.step == np.float32(0.25)
    _, _, logits = run_eager(a, iterations=7)
    first = a.flush()          # three windows through a ring of two rows: the oldest is lost
    state, ring = A.new_state(0.5), A.new_ring(8)
    for k, d in enumerate(logits, 1):
        A.observe(d.cpu().numpy(), k, state, ring, 2, 0.0, a.step, 0.875)
    want = A.curve(ring, 0, 3)
    assert first == want[1:] and a.curve() == want[1:]
    assert np.array_equal(a.state.cpu().numpy().view(np.uint32), state)
    assert len({row["p"] for row in want} | {0.5}) > 1          # p did move
    got = a.status()
    f = A.fields(state)
    assert got == {"p": float(f["p"]), "r_t": float(f["r"]), "updates": 3, "ups": f["ups"], "downs": f["downs"], "nonfinite": 0}
    assert a.flush() == []
    # the masks of the last draw are the gate of its raw rows at the p of that moment (p did not move after the sixth observation)
    assert np.array_equal(a.params.cpu().numpy().view(np.uint32), A.gate(a.last_rows, want[-1]["p"], 7).view(np.uint32))


def test_trainer_writes_ada_json_and_a_resumed_run_continues_it(tmp_path):
    from locate_amd import DeviceImageStore, DiffAugment, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, augment):
        G, D, step, _ = build_tiny(augment)
        pipeline = InputPipeline(store, S, B, seed=11)
        t = Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                    subepoch_function=lambda e: 1, image_interval_function=lambda batch: 100)
        assert t.augment is augment and t.adaptive == hasattr(augment, "observe")
        return t

    def make():
        return adaptive(seed=21, target=0.0, interval=1, kimg=0.064, initial_p=0.5)          # step 0.125 per iteration

    def ada_json(out):
        with open(str(out / "error" / "ada.json")) as f:
            return json.load(f)

    a_whole = make()
    whole = trainer(tmp_path / "whole", 3, a_whole)
    assert whole.run() == 3
    record = ada_json(tmp_path / "whole")
    assert sorted(record) == ["curve", "downs", "nonfinite", "p", "r_t", "updates", "ups"]
    assert [sorted(row) for row in record["curve"]] == [["iteration", "p", "r_t"]] * 3
    assert [row["iteration"] for row in record["curve"]] == [1, 2, 3] and record["updates"] == 3 and record["p"] == record["curve"][-1]["p"]
    assert record["p"] != 0.5 and str(tmp_path / "whole" / "error" / "ada.json") in whole.written

    a_head = make()
    head = trainer(tmp_path / "parts", 2, a_head)
    assert head.run() == 2
    assert ada_json(tmp_path / "parts")["curve"] == record["curve"][:2]
    saved = torch.load(str(tmp_path / "parts" / "trainer.torch"), map_location="cpu", weights_only=True)["augment"]
    assert saved["adaptive"] is True and saved["observations"] == 2
    a_tail = make()
    tail = trainer(tmp_path / "parts", 3, a_tail)
    assert tail.resume().iterations == 2 and a_tail.status()["p"] == a_head.status()["p"]
    assert tail.run() == 3 and a_tail.draws == 1
    assert ada_json(tmp_path / "parts") == record
    assert np.array_equal(a_tail.last_rows, a_whole.last_rows)
    assert torch.equal(a_tail.params, a_whole.params) and torch.equal(a_tail.state, a_whole.state)
    assert not differing(training_state(whole.gen, whole.dis, whole.step), training_state(tail.gen, tail.dis, tail.step))
    # a plain augment, and none: no ada.json; a plain run's state is refused by an adaptive one
    for name, augment in (("plain", DiffAugment(S=S, batch=B, policy=FULL, seed=21, device=DEV)), ("none", None)):
        t = trainer(tmp_path / name, 1, augment)
        assert t.run() == 1 and not os.path.exists(str(tmp_path / name / "error" / "ada.json"))
    with pytest.raises(ValueError, match="plain DiffAugment"):
        trainer(tmp_path / "plain", 2, make()).resume()
