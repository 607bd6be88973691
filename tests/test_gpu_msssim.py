"""The multi-scale SSIM on the MI355X: the ten level numbers of every pair (csrc/msssim.hip) against the float64 model
(tests/helpers/msssim_model.py) inside the model's DERIVED bound, the exact cases, the bits' independence of the call, a NaN image,
the combination in locate_amd/msssim.py against the model's, the metric bit for bit against its parts, what it is for - a collapsed
set shows -, and its behaviour around a running training: an evaluation between two iterations, eager or replayed, leaves the
trajectory where a run without it would be."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import msssim_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
PAIRS = {32: 5, 64: 3, 128: 2, 256: 2}
KEYS = ["clamped", "levels", "mean", "nonfinite", "pairs", "real", "std"]
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    _CACHE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def images(u):
    """bytes 0 .. 255 [n, 3, S, S] -> the fp32 device images that encode to them"""
    return torch.from_numpy(M.decode(u)).to(DEV)


def encoded(u):
    from locate_amd import encode_images
    triple = encode_images(images(u))
    want = torch.from_numpy((np.asarray(u) - 128).astype(np.int8).reshape(len(u), -1)).to(DEV)
    assert torch.equal(triple[0][:, :want.shape[1]], want) and int(triple[2].sum()) == 0          # the codes are the bytes minus 128
    return triple


def case(S):
    """(a, b, names): P pairs each of uniform bytes, low-pass images and the bright near-flat texture, the constants and the
    anticorrelated pair; (want [n, 2, 5]) from the model, made once per size"""
    if S not in _CACHE:
        P = PAIRS[S]
        anti = M.anticorrelated(S)
        zero, white = np.zeros((1, 3, S, S)), np.full((1, 3, S, S), 255.0)
        a = np.concatenate([M.uniform_bytes(P, S, S), M.low_pass(P, S, S + 1), M.bright_texture(P, S, S + 2), zero, white, white, anti[0][None]])
        b = np.concatenate([M.uniform_bytes(P, S, S + 3), M.low_pass(P, S, S + 4), M.bright_texture(P, S, S + 5), zero, white, zero, anti[1][None]])
        names = ["uniform"] * P + ["low-pass"] * P + ["bright"] * P + ["0 | 0", "255 | 255", "255 | 0", "anticorrelated"]
        want = np.stack([M.levels(x, y) for x, y in zip(a, b)])
        _CACHE[S] = (a, b, names, want)
    return _CACHE[S]


# ---- 1. inside the bound -------------------------------------------------------------------------------------------------------------------
# 32: windows 11, 11, 8, 4, 2 and three 1 x 1 outputs, one launch; 64: the ring of row sums wraps at the two upper levels, one launch
# above 64 KB of LDS; 128: one tiled launch (6 x 4 tiles, the last band and strip short) and the launch from planes; 256: two tiled
# launches (12 x 8 tiles), the second from fp32 planes
@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_levels_stay_inside_the_derived_bound(S):
    from locate_amd import ms_ssim_levels
    a, b, names, want = case(S)
    got = ms_ssim_levels(encoded(a), encoded(b))
    assert tuple(got.shape) == (len(a), 2, 5) and got.dtype == torch.float64 and got.device.type == "cuda"
    got = got.cpu().numpy()
    share = np.abs(got - want) / M.LEVEL_BOUND
    for kind in sorted(set(names)):
        rows = [i for i, n in enumerate(names) if n == kind]
        print("S = %d, %-14s: worst |got - want| / LEVEL_BOUND %.5f (ssim %.5f, cs %.5f)"
              % (S, kind, share[rows].max(), share[rows][:, 0].max(), share[rows][:, 1].max()))
    print("S = %d: worst share of the bound used %.5f (LEVEL_BOUND %.3e)" % (S, share.max(), M.LEVEL_BOUND))
    assert np.isfinite(got).all() and (np.abs(got - want) <= M.LEVEL_BOUND).all()
    assert (want[names.index("anticorrelated"), 1, :4] < -0.85).all()


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_exact_cases(S):
    from locate_amd import ms_ssim_levels
    a, b, names, _ = case(S)
    ta, tb = encoded(a), encoded(b)
    same = ms_ssim_levels(ta, ta)
    assert bool((same == 1.0).all()), "an image against itself: %s" % same[(same != 1.0).any(dim=2).any(dim=1)]
    assert bool((ms_ssim_levels(tb, tb) == 1.0).all())
    assert torch.equal(ms_ssim_levels(ta, tb), ms_ssim_levels(tb, ta))


# ---- 3. the bits do not depend on the call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_same_bits_whatever_the_call(S):
    from locate_amd import ms_ssim_levels
    a, b, names, _ = case(S)
    ta, tb = encoded(a[:7]), encoded(b[:7])
    first = ms_ssim_levels(ta, tb)
    assert torch.equal(ms_ssim_levels(ta, tb), first)          # a second call
    alone = ms_ssim_levels(tuple(t[6:7] for t in ta), tuple(t[6:7] for t in tb))          # the last of 7, alone
    assert torch.equal(alone, first[6:7])
    assert torch.equal(ms_ssim_levels(tuple(t[2:4] for t in ta), tuple(t[2:4] for t in tb)), first[2:4])
    row = ta[0].shape[1]

    def shifted(t):          # the same rows 16 bytes into a larger buffer
        buf = torch.zeros(7 * row + 64, dtype=torch.int8, device=DEV)
        view = buf[16:16 + 7 * row].view(7, row)
        view.copy_(t[0])
        assert view.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + 16
        return (view, t[1], t[2])
    assert torch.equal(ms_ssim_levels(shifted(ta), shifted(tb)), first)
    assert torch.equal(ms_ssim_levels((ta[0], ta[1], None), (tb[0], tb[1], None)), first)          # no flags


# ---- 4. a NaN image ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 128])
def test_a_nan_image_is_counted_and_left_out(S):
    from locate_amd import MultiScaleSSIM, encode_images, ms_ssim_levels, ms_ssim_value
    a, b, names, _ = case(S)
    x, y = images(a[:6]), images(b[:6])
    clean = ms_ssim_levels(encode_images(x), encode_images(y))
    bad_x, bad_y = x.clone(), y.clone()
    bad_x[1, 2, 5, 7] = float("nan")
    bad_y[4, 0, 0, 0] = float("inf")
    got = ms_ssim_levels(encode_images(bad_x), encode_images(bad_y))
    ok = torch.tensor([True, False, True, True, False, True], device=DEV)
    assert torch.equal(got[ok], clean[ok]) and bool(torch.isnan(got[~ok]).all())
    value, clamped = ms_ssim_value(got)
    clean_value, clean_clamped = ms_ssim_value(clean)
    assert bool(torch.isnan(value[~ok]).all()) and torch.equal(value[ok], clean_value[ok]) and torch.equal(clamped[ok], clean_clamped[ok])
    assert not bool(clamped[~ok].any())
    rec = MultiScaleSSIM(S, pairs=6, chunk=2, device=DEV).between(bad_x, bad_y)
    kept = clean_value[ok].cpu().numpy()
    lv = clean[ok].cpu().numpy()
    assert rec["pairs"] == 6 and rec["nonfinite"] == 2 and rec["clamped"] == int(clean_clamped[ok].sum())
    assert rec["mean"] == pytest.approx(kept.mean(), rel=1e-12) and rec["std"] == pytest.approx(kept.std(), rel=1e-9, abs=1e-12)
    assert np.allclose(rec["levels"]["ssim"], lv[:, 0].mean(axis=0), rtol=1e-12, atol=0) and np.allclose(rec["levels"]["cs"], lv[:, 1].mean(axis=0), rtol=1e-12, atol=0)


# ---- 5. the combination --------------------------------------------------------------------------------------------------------------------
def test_value_against_the_models_combination():
    """over the device's own levels: five pow calls and four products at a few ulp each, about 1e-15; a wrong weight or a dropped
    level is off by 1e-2"""
    from locate_amd import ms_ssim_levels, ms_ssim_value
    a, b, names, _ = case(32)
    levels = ms_ssim_levels(encoded(a), encoded(b))
    levels = torch.cat([levels, torch.full((1, 2, 5), float("nan"), dtype=torch.float64, device=DEV)])
    value, clamped = ms_ssim_value(levels)
    assert value.dtype == torch.float64 and clamped.dtype == torch.bool and tuple(value.shape) == (len(a) + 1,)
    want, want_clamped = M.value(levels.cpu().numpy())
    got = value.cpu().numpy()
    assert np.isnan(got[-1]) and np.isnan(want[-1]) and (np.abs(got[:-1] - want[:-1]) <= 1e-12 * np.abs(want[:-1])).all()
    assert clamped.cpu().numpy().tolist() == want_clamped.tolist()
    assert want_clamped[names.index("anticorrelated")] and got[names.index("anticorrelated")] == 0.0 and not want_clamped[-1]
    assert got[names.index("255 | 255")] == 1.0


# ---- 6. the metric is its parts ------------------------------------------------------------------------------------------------------------
def record_of(levels):
    """what a record must hold, from per-pair levels on the device (float64 numpy on the host)"""
    from locate_amd import ms_ssim_value
    value, clamped = ms_ssim_value(levels)
    return value.cpu().numpy(), clamped.cpu().numpy(), levels.cpu().numpy()


def check_record(rec, value, clamped, lv):
    assert sorted(rec) == KEYS and rec["pairs"] == len(value) and rec["nonfinite"] == 0 and rec["clamped"] == int(clamped.sum())
    assert rec["mean"] == pytest.approx(value.mean(), rel=1e-12) and rec["std"] == pytest.approx(value.std(), rel=1e-9, abs=1e-12)
    assert np.allclose(rec["levels"]["ssim"], lv[:, 0].mean(axis=0), rtol=1e-12, atol=0) and np.allclose(rec["levels"]["cs"], lv[:, 1].mean(axis=0), rtol=1e-12, atol=0)


def test_between_and_among_are_their_parts():
    from locate_amd import MultiScaleSSIM, encode_images, ms_ssim, ms_ssim_levels, ms_ssim_value
    a, b, names, _ = case(32)
    x, y = images(a[:12]), images(b[:12])
    m = MultiScaleSSIM(32, pairs=12, chunk=4, device=DEV)
    levels = ms_ssim_levels(encode_images(x), encode_images(y))
    rec = m.between(x, y)
    check_record(rec, *record_of(levels))
    assert rec["real"] is None and m.between(x, y) == rec
    v, c, lv = ms_ssim(x, y)
    assert torch.equal(lv, levels) and torch.equal(v, ms_ssim_value(levels)[0]) and torch.equal(c, ms_ssim_value(levels)[1])
    ca, cb = encode_images(x[0::2]), encode_images(x[1::2])          # among: image 2 j against 2 j + 1
    pairwise = ms_ssim_levels(ca, cb)
    check_record(m.among(x), *record_of(pairwise))
    for j in range(6):
        assert torch.equal(ms_ssim_levels(encode_images(x[2 * j:2 * j + 1]), encode_images(x[2 * j + 1:2 * j + 2])), pairwise[j:j + 1])
    one = m.among(x[:2])
    assert one["pairs"] == 1 and one["std"] == 0.0 and one["mean"] == float(ms_ssim_value(pairwise[:1])[0][0])          # bit for bit
    with pytest.raises(ValueError):
        m.among(x[:3])
    with pytest.raises(ValueError):
        m.between(x, y[:5])


# ---- 7. what it is for ---------------------------------------------------------------------------------------------------------------------
def test_collapse_shows():
    """64 images that are one low-pass image plus noise of 2 bytes against 64 independent low-pass images.  The model on the CPU, same
    seeds: mean 0.9994 (no pair clamped) against 0.039 (21 of 32 clamped) - the thresholds 0.9 and half of the first clear with room"""
    from locate_amd import MultiScaleSSIM
    S = 32
    base = M.low_pass(1, S, 70)[0]
    near = np.clip(base[None] + np.random.default_rng(71).integers(-2, 3, size=(64, 3, S, S)), 0, 255).astype(np.float64)
    far = M.low_pass(64, S, 72)
    m = MultiScaleSSIM(S, pairs=32, device=DEV)
    collapsed, diverse = m.among(images(near)), m.among(images(far))
    print("collapsed: mean %.5f clamped %d cs %s\ndiverse: mean %.5f clamped %d cs %s"
          % (collapsed["mean"], collapsed["clamped"], collapsed["levels"]["cs"], diverse["mean"], diverse["clamped"], diverse["levels"]["cs"]))
    assert collapsed["mean"] > 0.9 and collapsed["clamped"] == 0 and collapsed["pairs"] == 32
    assert diverse["mean"] < 0.5 * collapsed["mean"]


# ---- 8. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) ---------------------
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


STORE = np.random.default_rng(26).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_an_evaluation_between_iterations_has_no_side_effect(launch):
    from locate_amd import MultiScaleSSIM
    from locate_amd.graph import GraphedTrainStep

    def run(measure):
        G, D, step, (lat, real, aug) = build_tiny()
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
        values, losses = [], []
        for i in range(6):
            out = runner.replay() if runner is not None else step(lat, real, aug)
            losses.append((out["d_error"].detach().clone(), out["g_error"].detach().clone()))
            if measure and i == 2:
                m = MultiScaleSSIM(32, pairs=8, seed=4, chunk=8, device=DEV)
                values = [m.evaluate(G), m.evaluate(G), m.evaluate_against(G, G)]
                assert G.training
                assert tuple(m.latents(G.g_in).shape) == (16, G.g_in)
        return training_state(G, D, step), losses, values

    plain, plain_losses, _ = run(False)
    watched, losses, values = run(True)
    assert sorted(plain) == sorted(watched)
    bad = [k for k in plain if not torch.equal(plain[k], watched[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain_losses, losses))
    assert values[0] == values[1] and values[0]["pairs"] == 8 and values[0]["nonfinite"] == 0 and values[0]["real"] is None
    assert math.isfinite(values[0]["mean"]) and len(values[0]["levels"]["cs"]) == 5
    # a generator against itself: all 16 images, each against the same latent's image one power iteration of u / v on
    assert values[2]["pairs"] == 16 and math.isfinite(values[2]["mean"]) and "real" not in values[2]


def test_evaluate_is_the_parts_and_restores_the_mode():
    from locate_amd import MultiScaleSSIM, encode_images, ms_ssim_levels
    G, _, _, _ = build_tiny()
    m = MultiScaleSSIM(32, pairs=8, seed=4, chunk=8, device=DEV)
    G.eval()
    first = m.evaluate(G)
    assert not G.training
    G.train()
    assert m.evaluate(G) == first and G.training
    rng = torch.Generator(device=DEV)
    rng.manual_seed(4 + 9)
    latents = torch.randn(16, G.g_in, device=DEV, generator=rng)
    assert torch.equal(m.latents(G.g_in), latents)
    for other in (1, 2, 3, 5, 6, 7, 8):          # the offsets the other metrics and the trainer draw from
        rng.manual_seed(4 + other)
        assert not torch.equal(torch.randn(16, G.g_in, device=DEV, generator=rng), latents)
    G.eval()
    with torch.no_grad():
        chunks = [G(latents[:8]), G(latents[8:])]
    levels = torch.cat([ms_ssim_levels(encode_images(c[0::2]), encode_images(c[1::2])) for c in chunks])
    check_record(first, *record_of(levels))


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, files in os.walk(str(root)) for f in files)


def test_trainer_records_the_metric(tmp_path):
    from locate_amd import AveragedGenerator, DeviceImageStore, InputPipeline, MultiScaleSSIM, Trainer
    store = DeviceImageStore(STORE, DEV)

    def trainer(out, with_metric, average=False):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        m = None
        if with_metric:
            m = MultiScaleSSIM(32, pairs=8, seed=3, chunk=8, device=DEV).reference_from_pipeline(pipeline)
            assert (pipeline.epoch, pipeline.pos) == (0, 0)          # the training pipeline's shuffle is not advanced
            assert sorted(m.real) == [k for k in KEYS if k != "real"] and m.real["pairs"] == 8 and m.real["nonfinite"] == 0
        t = Trainer(step, pipeline, str(out), epochs=1, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                    image_interval_function=lambda batch: 2, msssim=m, average=AveragedGenerator(G, half_life_images=64, batch=8) if average else None)
        return t, G, D, step, m

    path = os.path.join(str(tmp_path / "with"), "error", "msssim.json")
    first, G0, D0, step0, m0 = trainer(tmp_path / "with", True)
    assert first.run() == 4 and path in first.written
    rec = json.load(open(path))
    assert len(rec) == 1 and rec[0] == dict(m0.evaluate(G0), epoch=1, iterations=4) and "average" not in rec[0]          # the weights are the saved ones
    assert sorted(rec[0]) == sorted(KEYS + ["epoch", "iterations"]) and rec[0]["real"] == m0.real and rec[0]["pairs"] == 8
    assert not os.path.exists(path + ".tmp")

    plain, G2, D2, step2, _ = trainer(tmp_path / "without", False)
    assert plain.run() == 4
    assert listing(tmp_path / "without") == [f for f in listing(tmp_path / "with") if f != os.path.join("error", "msssim.json")]
    a, b = training_state(G0, D0, step0), training_state(G2, D2, step2)
    assert sorted(a) == sorted(b) and not [k for k in a if not torch.equal(a[k], b[k])]

    third, G3, _, _, m3 = trainer(tmp_path / "average", True, average=True)
    assert third.run() == 4
    rec = json.load(open(os.path.join(str(tmp_path / "average"), "error", "msssim.json")))
    assert len(rec) == 1 and sorted(rec[0]) == sorted(KEYS + ["epoch", "iterations", "average", "average_to_live"])
    assert rec[0]["average"] == {k: v for k, v in m3.evaluate(third.average.generator).items() if k != "real"}
    assert rec[0]["average_to_live"] == m3.evaluate_against(G3, third.average.generator) and "real" not in rec[0]["average_to_live"]
    assert {k: v for k, v in rec[0].items() if k not in ("average", "average_to_live")} == dict(m3.evaluate(G3), epoch=1, iterations=4)


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, STORE)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--msssim-pairs", "8"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    rec = json.load(open(os.path.join(out, "error", "msssim.json")))
    assert len(rec) == 1 and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["pairs"], rec[0]["nonfinite"]) == (1, 4, 8, 0)
    assert sorted(rec[0]) == sorted(KEYS + ["epoch", "iterations"]) and rec[0]["real"]["pairs"] == 8 and math.isfinite(rec[0]["mean"])
    assert len(rec[0]["levels"]["ssim"]) == 5 and all(math.isfinite(v) for v in rec[0]["levels"]["cs"] + rec[0]["real"]["levels"]["cs"])
    assert not [f for f in listing(out) if "swd" in f or "manifold" in f or "spectrum" in f]
