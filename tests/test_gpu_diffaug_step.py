"""The differentiable augmentation inside the training step on the MI355X, on the tiny fixture network of the trajectory tests
(tests/test_gpu_average.py: 32 x 32, base width 1, batch 8), compared after at most 3 iterations: a step without an augment is the
step it was; the G-step's gradient reaches the generator through T's adjoint; hipGraph replays equal eager iterations with draw()
between them; a resume continues the parameter stream; the returned images stay un-augmented."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import diffaug_model as M  # noqa: E402

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


def build_tiny(augment=None, pass_keyword=True, **kw):
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=S, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    options = dict(stacked_d=True, minibatches=1)
    options.update(kw)
    if pass_keyword:
        options["augment"] = augment
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), **options)
    inputs = tuple(T(z["step1/" + k]).to(DEV) for k in ("latent", "real", "aug"))
    assert tuple(inputs[1].shape) == (B, 3, S, S)
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


def augment(seed=5, policy=FULL):
    from locate_amd import DiffAugment
    return DiffAugment(S=S, batch=B, policy=policy, seed=seed, device=DEV)


def test_without_an_augment_the_step_is_todays():
    """augment=None - called directly and through TrainLoop.iteration - against the code path that is given no augment argument
    at all: weights, u / v, both optimizers' states and the losses, bit for bit"""
    from locate_amd import TrainLoop
    runs = []
    for how in ("keyword absent", "augment=None", "through TrainLoop"):
        G, D, step, (lat, real, aug) = build_tiny(pass_keyword=how != "keyword absent")
        assert step.augment is None
        loop = TrainLoop(step)
        losses = []
        for _ in range(3):
            out = loop.iteration(lat, real, aug) if how == "through TrainLoop" else step(lat, real, aug)
            losses += [out["d_error"].clone(), out["g_error"].clone(), out["penalty"].clone()]
        runs.append((training_state(G, D, step), losses))
    for state, losses in runs[1:]:
        assert not differing(runs[0][0], state)
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], losses))
    assert any(k.endswith("weight_u") for k in runs[0][0]) and any("/opt/" in k for k in runs[0][0])
    # and an augment does change the run: the comparison above is not vacuous
    a = augment()
    G, D, step, (lat, real, aug) = build_tiny(a)
    loop = TrainLoop(step)
    for _ in range(3):
        loop.iteration(lat, real, aug)
    assert a.draws == 3 and len(differing(runs[0][0], training_state(G, D, step))) > 10


@pytest.mark.parametrize("phase", ["g_forward_backward", "g_forward + g_backward"])
def test_gradient_reaches_the_generator_through_the_adjoint(phase):
    """One G-step's .grad on the generator against a composition of the project's own pieces: diff_augment by hand on rows
    3B .. 4B, the existing D forward and backward for D's input gradient gy, an adjoint of T applied to it, and the result pushed
    through the generator.

    (a) With the backward KERNEL as the adjoint the composition runs the launches the step runs: every gradient of the generator,
        bit for bit.
    (b) With the float64 definition's adjoint, rounded to fp32, pushed by torch.autograd.backward: the gradient of the generator's
        final layer (out_conv's last weight).  What enters the generator differs from the step's by delta, |delta| <= beta
        element-wise, beta = BACKWARD_BOUND (tests/test_gpu_diffaug.py, check 3) + u |gx| for the definition's own rounding to
        fp32.  The generator's backward is linear in what enters it, dW = L gx, so the two gradients differ by L delta.  L itself
        is not at hand element by element, but it can be applied: the tolerance is the size of L (sigma * beta) for one fixed
        pattern of random signs sigma, pushed through the same reference path - the size L delta has for errors of independent
        sign, which rounding errors are - times 16 for the spread between sign patterns (the sum over the 3 B S^2 = 24576
        elements behind one weight is then a random walk: 16 is four standard deviations of its largest of a few hundred
        components, with a factor 4 to spare).  It is NOT the bound for errors that all line up with a row of L (that one is
        sqrt(24576) = 157 times larger); nothing in the tolerance comes from the step's own result.  Relative to the gradient's
        largest element it is a few 1e-6; the figures are printed."""
    from locate_amd import TrainLoop, diff_augment, diff_augment_backward
    from locate_amd.train import g_loss
    a = augment()
    G, D, step, (lat, real, aug) = build_tiny(a)
    TrainLoop(step).iteration(lat, real, aug)          # one whole iteration first: u / v trainable, lazily made state exists
    rows = a.draw()
    sd = {"G": {k: v.detach().clone() for k, v in G.state_dict().items()}, "D": {k: v.detach().clone() for k, v in D.state_dict().items()}}

    def grads():
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in G.named_parameters() if p.grad is not None}

    # the step's own G-step
    out = step.g_forward_backward(lat) if phase == "g_forward_backward" else step.g_backward(step.g_forward(lat))
    got = grads()
    assert len(got) > 10

    def generator_pass():
        G.load_state_dict(sd["G"])          # the same weights and u / v as the step's pass started from
        G.zero_grad()
        return G(lat)

    # D's input gradient, from the same weights and u / v
    D.load_state_dict(sd["D"])
    D.requires_grad_(False)
    try:
        fake = generator_pass()
        assert torch.equal(fake.detach(), out["fake"])          # the returned images are the un-augmented ones
        g_rows = a.params[3 * B:4 * B]
        seen = diff_augment(fake.detach(), g_rows, FULL).requires_grad_()
        d_out = D(seen)
        loss, g = g_loss(d_out)
        assert torch.equal(loss[0], out["g_error"])
        step._backward([d_out], [g.view_as(d_out)])
        gy = seen.grad.detach().contiguous()
    finally:
        D.requires_grad_(True)
    # (a) the kernel's adjoint, through the step's own backward driver
    step._backward([fake], [diff_augment_backward(gy, g_rows, FULL)])
    by_hand = grads()
    assert sorted(by_hand) == sorted(got)
    bad = [n for n in got if not torch.equal(got[n], by_hand[n])]
    assert not bad, "%d of %d generator gradients differ, first %s" % (len(bad), len(got), bad[:4])
    # (b) the float64 definition's adjoint
    gy_host = gy.cpu().numpy()
    want_gx = M.backward(gy_host, rows[3 * B:], M.FULL)
    beta = M.backward_bound(gy_host, rows[3 * B:], M.FULL) + np.abs(want_gx) * M.U32
    last = [n for n, p in G.named_parameters() if n.startswith("out_conv") and p.dim() == 4][-1]
    torch.autograd.backward([generator_pass()], [torch.from_numpy(want_gx.astype(np.float32)).to(DEV)])
    want = grads()[last]
    sigma = np.random.default_rng(17).choice([-1.0, 1.0], size=beta.shape)
    torch.autograd.backward([generator_pass()], [torch.from_numpy((sigma * beta).astype(np.float32)).to(DEV)])
    tol = 16.0 * float(grads()[last].abs().max())
    err = float((got[last] - want).abs().max())
    top = float(want.abs().max())
    print("%s: %s: largest difference %.3e, tolerance %.3e (%.3e and %.3e of the gradient's largest element %.3e)"
          % (phase, last, err, tol, err / top, tol / top, top))
    assert top > 0 and 0 < tol < 1e-4 * top
    assert err <= tol


@pytest.mark.parametrize("mode", ["stacked", "three-streams", "unstacked"])
def test_replays_equal_eager_iterations_with_draws_between_them(mode):
    from locate_amd.graph import GraphedTrainStep
    kw = {"stacked": dict(stacked_d=True), "three-streams": dict(concurrent_d=True, stacked_d=False), "unstacked": dict(stacked_d=False)}[mode]
    a1, a2 = augment(9), augment(9)
    G1, D1, step1, (lat, real, aug) = build_tiny(a1, **kw)
    G2, D2, step2, _ = build_tiny(a2, **kw)
    # the warm-up iterations of the capture run on ONE draw; the eager run does the same
    a1.draw()
    a2.draw()
    runner = GraphedTrainStep(step2, lat, real, aug, warmup=2)
    for _ in range(2):
        step1(lat, real, aug)
    for _ in range(3):
        r1, r2 = a1.draw(), a2.draw()
        assert np.array_equal(r1, r2)
        out1 = step1(lat, real, aug)
        out2 = runner.replay()
    torch.cuda.synchronize()
    for k in ("d_error", "g_error", "penalty", "fake", "generated"):
        assert torch.equal(out2[k], out1[k]), k
    assert not differing(training_state(G1, D1, step1), training_state(G2, D2, step2))
    # the replays did read the new rows: with the first draw kept, the run ends elsewhere
    a3 = augment(9)
    G3, D3, step3, _ = build_tiny(a3, **kw)
    a3.draw()
    for _ in range(5):
        step3(lat, real, aug)
    assert differing(training_state(G1, D1, step1), training_state(G3, D3, step3))


def test_returned_images_are_not_augmented():
    a = augment()
    G, D, step, (lat, real, aug) = build_tiny(a)
    from locate_amd import diff_augment
    a.draw()
    _, _, plain_step, _ = build_tiny()
    plain = plain_step(lat, real, aug)          # the D-step's generator pass runs before anything an augment could change
    out = step(lat, real, aug)
    torch.cuda.synchronize()
    assert torch.equal(out["generated"], plain["generated"])
    assert not torch.equal(out["d_error"], plain["d_error"])          # while the discriminator did see something else
    # the G-step's images (test_gradient_reaches_the_generator... holds them to the generator's own forward, bit for bit)
    assert tuple(out["fake"].shape) == (B, 3, S, S) and not out["fake"].requires_grad
    assert not torch.equal(out["fake"], diff_augment(out["fake"], a.params[3 * B:], FULL))
    assert float(out["fake"].abs().max()) <= 1.0 + 1e-6 and float(out["generated"].abs().max()) <= 1.0 + 1e-6          # tanh's range: no brightness offset, and
    assert float((out["fake"] == 0).float().mean()) < 0.01          # no cut, no border


def test_trainer_resume_continues_the_parameter_stream(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, max_iterations, augmented=True):
        a = augment(21) if augmented else None
        G, D, step, _ = build_tiny(a)
        pipeline = InputPipeline(store, S, B, seed=11)
        t = Trainer(step, pipeline, str(out), epochs=2, max_iterations=max_iterations, images=13, seed=3, miniter_function=lambda e: 1,
                    subepoch_function=lambda e: 1, image_interval_function=lambda batch: 100)
        assert t.augment is a
        return t, a

    whole, a_whole = trainer(tmp_path / "whole", 3)
    assert whole.run() == 3 and a_whole.draws == 3
    head, a_head = trainer(tmp_path / "parts", 2)
    assert head.run() == 2
    saved = torch.load(str(tmp_path / "parts" / "trainer.torch"), map_location="cpu", weights_only=True)
    assert saved["augment"]["policy"] == FULL and torch.equal(saved["augment"]["generator_state"], a_head.generator.get_state())
    tail, a_tail = trainer(tmp_path / "parts", 3)
    assert tail.resume().iterations == 2
    assert torch.equal(a_tail.generator.get_state(), a_head.generator.get_state())
    assert tail.run() == 3 and a_tail.draws == 1
    assert np.array_equal(a_tail.last_rows, a_whole.last_rows)
    assert not differing(training_state(whole.gen, whole.dis, whole.step), training_state(tail.gen, tail.dis, tail.step))
    # off: trainer.torch has no such key
    plain, _ = trainer(tmp_path / "plain", 1, augmented=False)
    assert plain.run() == 1
    assert "augment" not in torch.load(str(tmp_path / "plain" / "trainer.torch"), map_location="cpu", weights_only=True)
