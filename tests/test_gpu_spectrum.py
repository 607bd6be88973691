"""The radial power spectrum on the MI355X: per-plane spectra (csrc/spectrum.hip) against the float64 model
(tests/helpers/spectrum_model.py) inside the model's DERIVED bound - every plane, every bin -, the exact cases, the bits' independence
of the call, the set summary against float64 numpy, the composition in locate_amd/spectrum.py bit for bit against its parts, and the
metric's behaviour around a running training: an evaluation between two iterations, eager or replayed, leaves the trajectory where a
run without it would be."""
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
import spectrum_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
BINS = {32: 24, 64: 46, 128: 92, 256: 182}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    _CACHE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def tables(S, name="none"):
    """the package's tables (the ones the kernel reads), as the model's argument"""
    from locate_amd.spectrum import dft_tables
    if (S, name) not in _CACHE:
        _CACHE[(S, name)] = dft_tables(S, name)
    return _CACHE[(S, name)]


def planes(n, S, seed, shift=0.0):
    return (np.tanh(np.random.default_rng(seed).standard_normal((n, S, S))) + shift).astype(np.float32)


def spectra_of(x, name="none"):
    from locate_amd import radial_spectrum
    return radial_spectrum(dev(x), window=name).cpu().numpy()


# ---- 1. per-plane spectra against the model ------------------------------------------------------------------------------------------
# (3, 32): one tile per wave; (7, 32): an odd number of planes; (6, 64): the flagship size, several tiles per wave; (2, 128) and
# (1, 256): the three-launch form through the workspace; + 50: a DC term 10^4 times the rest of the spectrum
@pytest.mark.parametrize("n,S,name,shift", [(3, 32, "none", 0.0), (3, 32, "hann", 0.0), (7, 32, "none", 0.0), (7, 32, "hann", 0.0),
                                            (6, 64, "none", 0.0), (6, 64, "hann", 0.0), (2, 128, "none", 0.0), (1, 256, "none", 0.0),
                                            (6, 64, "none", 50.0)])
def test_spectra_stay_inside_the_derived_bound(n, S, name, shift):
    x = planes(n, S, 1000 * n + S, shift)
    tabs = tables(S, name)
    want, bound = M.spectrum(x, tabs), M.spectrum_bound(x, tabs)
    got = spectra_of(x, name)
    assert got.shape == (n, BINS[S]) and got.dtype == np.float64 and np.isfinite(got).all()
    ratio = np.abs(got - want) / bound
    print("%d x %d x %d %s shift %g: worst |got - want| / bound %.4f; bound / value: median %.1e, max %.1e"
          % (n, S, S, name, shift, ratio.max(), np.median(bound / want), (bound / want).max()))
    assert (np.abs(got - want) <= bound).all()
    if shift == 0.0:
        assert (bound <= 0.05 * want).all(), "a bound that large would hide a structural mistake"


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128])
def test_exact_cases(S):
    """The checkerboard 0.5 (-1)^(x + y): every product of both stages is +-0.5 or +-1 times an exact table entry at (H, H): 0.25 there,
    exactly.  The last bin holds (H, H) alone at 32 and 128: ==.  At 64 the definition's rounded radius puts (H, H - 1) and
    (H - 1, H) (radius 44.55) into the last bin as well, whose rounding noise is added to the 0.25: within the bound there.
    The constant 0.25: 0.0625 in bin 0, which is (0, 0) alone: ==.  A cosine at (fy, kx) = (4, 3): radius 5."""
    yy, xx = np.mgrid[:S, :S]
    x = np.stack([0.5 * (-1.0) ** (yy + xx), np.full((S, S), 0.25), np.cos(2 * np.pi * (3 * xx + 4 * yy) / S)]).astype(np.float32)
    tabs = tables(S)
    got, want, bound = spectra_of(x), M.spectrum(x, tabs), M.spectrum_bound(x, tabs)
    alone = int(M.multiplicity(S)[-1]) == 1
    print("S = %d: checkerboard's last bin %.17g (%s), constant's bin 0 %.17g, cosine's bin 5 %.9g; largest other bin %.2e / %.2e / %.2e"
          % (S, got[0, -1], "alone" if alone else "shared", got[1, 0], got[2, 5], got[0, :-1].max(), got[1, 1:].max(), np.delete(got[2], 5).max()))
    assert want[0, -1] == 0.25 and want[1, 0] == 0.0625
    if alone:
        assert got[0, -1] == 0.25
    assert abs(got[0, -1] - 0.25) <= bound[0, -1]
    assert (got[0, :-1] <= bound[0, :-1]).all()
    assert got[1, 0] == 0.0625 and (got[1, 1:] <= bound[1, 1:]).all()
    # the cosine's samples are rounded to fp32, relative 2^-24 each: its mean square is 0.5 within ((1 + 2^-24)^2 - 1) / 2
    assert abs(got[2, 5] - want[2, 5]) <= bound[2, 5] and abs(got[2, 5] - 0.5) <= bound[2, 5] + 2.0 ** -24 and bound[2, 5] <= 0.01
    assert (np.abs(np.delete(got[2] - want[2], 5)) <= np.delete(bound[2], 5)).all()


# ---- 3. the bits do not depend on the call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128])
def test_same_bits_whatever_the_call(S):
    from locate_amd import radial_spectrum
    n = 5 if S <= 64 else 3
    x = dev(planes(n * 3, S, 7 + S).reshape(n, 3, S, S))
    first = radial_spectrum(x)
    assert tuple(first.shape) == (n, 3, BINS[S]) and first.dtype == torch.float64 and first.device == x.device
    assert torch.equal(radial_spectrum(x), first)          # a second call
    buf = torch.zeros(x.numel() + 1, device=DEV)          # the same values one float into an allocation: no 16-byte loads of the plane
    off = buf[1:].view(n, 3, S, S)
    off.copy_(x)
    assert off.data_ptr() % 16 == 4 and torch.equal(radial_spectrum(off), first)
    assert torch.equal(radial_spectrum(x[1:n - 1]), first[1:n - 1]) and torch.equal(radial_spectrum(x[n - 1:]), first[n - 1:])
    assert torch.equal(radial_spectrum(x[0, 1]), first[0, 1])          # a single plane
    if S == 32:          # beside another window's tables
        hann = radial_spectrum(x, window="hann")
        assert not torch.equal(hann, first) and torch.equal(radial_spectrum(x), first) and torch.equal(radial_spectrum(x, "hann"), hann)


def test_a_nan_plane_is_counted_and_left_out():
    from locate_amd import radial_spectrum, spectrum_summary
    from locate_amd.spectrum import summary_means
    S, n = 32, 6
    x = dev(planes(n * 3, S, 21).reshape(n, 3, S, S))
    clean = radial_spectrum(x)
    bad = x.clone()
    bad[2, 1, 5, 7] = float("nan")
    bad[4, 0, 0, 0] = float("inf")
    got = radial_spectrum(bad)
    ok = torch.ones(n, 3, dtype=torch.bool)
    ok[2, 1] = ok[4, 0] = False
    assert torch.equal(got[ok.to(DEV)], clean[ok.to(DEV)])          # no other plane's bits change
    assert not torch.isfinite(got[2, 1]).any() and not torch.isfinite(got[4, 0]).any()
    summary = spectrum_summary(got)
    assert summary["nonfinite"].cpu().tolist() == [1, 1, 0] and summary["planes"] == n
    assert torch.isfinite(summary["sum"]).all() and torch.isfinite(summary["sumsq"]).all()
    s, q, count = M.summary(got.cpu().numpy(), S)
    assert np.allclose(summary["sum"].cpu().numpy(), s, rtol=1e-12, atol=0) and np.allclose(summary["sumsq"].cpu().numpy(), q, rtol=1e-12, atol=0)
    means, nonfinite = summary_means(summary)
    sums = summary["sum"].cpu().numpy()
    assert nonfinite == 2 and means[0] == (sums[0] / 5).tolist() and means[1] == (sums[1] / 5).tolist() and means[2] == (sums[2] / 6).tolist()
    one = got.clone()          # one bin of one plane is enough to leave the whole plane out
    one[0, 2] = clean[0, 2]
    one[0, 2, 3] = float("inf")
    assert spectrum_summary(one)["nonfinite"].cpu().tolist() == [1, 1, 1]


# ---- 4. the set summary ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", [(1, 32), (37, 32), (300, 64)])
def test_summary_against_float64_numpy(n, S):
    """over the device's own per-plane spectra: the inputs are fp64 and the order is fixed - 1e-12 relative (n 2^-53 would do)"""
    from locate_amd import radial_spectrum, spectrum_summary
    x = dev(planes(3, S, n + S).reshape(1, 3, S, S)).repeat(n, 1, 1, 1) * torch.linspace(0.5, 1.5, n, device=DEV)[:, None, None, None]
    spectra = radial_spectrum(x)
    summary = spectrum_summary(spectra)
    s, q, bad = M.summary(spectra.cpu().numpy(), S)
    got_s, got_q = summary["sum"].cpu().numpy(), summary["sumsq"].cpu().numpy()
    print("%d x 3 x %d: sum %.2e, sumsq %.2e relative" % (n, BINS[S], (np.abs(got_s - s) / s).max(), (np.abs(got_q - q) / q).max()))
    assert got_s.shape == (3, BINS[S]) and (np.abs(got_s - s) <= 1e-12 * s).all() and (np.abs(got_q - q) <= 1e-12 * q).all()
    assert summary["nonfinite"].cpu().tolist() == [0, 0, 0] and bad.tolist() == [0, 0, 0]
    again = spectrum_summary(spectra)
    assert torch.equal(again["sum"], summary["sum"]) and torch.equal(again["sumsq"], summary["sumsq"])


# ---- 5. the composition ------------------------------------------------------------------------------------------------------------------
def test_between_is_its_parts_bit_for_bit():
    from locate_amd import RadialSpectrum, radial_spectrum, spectrum_summary
    from locate_amd.spectrum import gap_record, summary_means
    S, n = 32, 12
    a = dev(planes(n * 3, S, 31).reshape(n, 3, S, S))
    b = dev((planes(n * 3, S, 32) * np.linspace(0.5, 1.0, S)[None, None, :]).astype(np.float32).reshape(n, 3, S, S))
    for name in ("none", "hann"):
        rs = RadialSpectrum(S, images=n, seed=4, chunk=4, window=name, device=DEV)
        got = rs.between(a, b)
        real, _ = summary_means(spectrum_summary(radial_spectrum(a, name)))
        fake, bad = summary_means(spectrum_summary(radial_spectrum(b, name)))
        want = dict({"bins": 24, "images": n, "window": name}, **gap_record(real, fake, S))
        want.update(nonfinite=bad, baseline=None)
        assert got == want and not rs.has_reference
        assert sorted(got) == ["baseline", "bins", "fake", "gap_db", "high_gap_db", "images", "max_abs_gap_db", "nonfinite", "real", "window"]
        assert rs.set_reference(a).distance(b) == got and rs.has_reference
        assert rs.set_reference([a[:5], a[5:]]).distance(iter([b[:7], b[7:]])) == got          # batches summing to N
        with pytest.raises(ValueError):
            rs.distance(b[:7])
        assert got["gap_db"][0][3] == 10.0 * math.log10(got["fake"][0][3] / got["real"][0][3])
        assert got["high_gap_db"][1] == sum(got["gap_db"][1][8:]) / 16 and got["max_abs_gap_db"] == max(abs(v) for row in got["gap_db"] for v in row)
        same = rs.between(a, a)
        assert same["max_abs_gap_db"] == 0.0 and same["high_gap_db"] == [0.0, 0.0, 0.0]
        based = rs.set_reference(a, baseline=b)
        assert based.baseline == dict(gap_record(real, fake, S), nonfinite=0) and based.distance(a)["baseline"] == based.baseline


def test_a_checkerboard_shows_in_the_last_bin():
    """what the metric is for: a faint checkerboard, invisible to a pixel distance, is the largest gap of the record"""
    from locate_amd import RadialSpectrum
    S, n = 64, 16
    a = planes(n * 3, S, 41).reshape(n, 3, S, S)
    a = (a[..., :, :] + np.roll(a, 1, axis=-1) + np.roll(a, 1, axis=-2) + np.roll(np.roll(a, 1, axis=-1), 1, axis=-2)) / 4          # smooth: little energy at the top
    yy, xx = np.mgrid[:S, :S]
    b = a + 0.01 * (-1.0) ** (yy + xx)
    rec = RadialSpectrum(S, images=n, device=DEV).between(dev(a), dev(b))
    top = [row[-1] for row in rec["gap_db"]]
    print("gap of the last bin: %s dB; the largest elsewhere %.3f dB" % (top, max(abs(v) for row in rec["gap_db"] for v in row[:-1])))
    # a 2 x 2 box filter has no response at (H, H): the real set's last bin is all but empty, the checkerboard's 10^-4 lifts it by tens
    # of dB; every other frequency is untouched
    assert all(v > 3.0 for v in top) and rec["max_abs_gap_db"] == max(top) and max(abs(v) for row in rec["gap_db"] for v in row[:-1]) < 0.01


# ---- 6. around a training run: the tiny fixture network of tests/test_gpu_swd.py (32 x 32, base width 1, batch 8) ---------------------
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


def small_metric(seed=4):
    from locate_amd import RadialSpectrum
    rs = RadialSpectrum(32, images=16, seed=seed, chunk=8, device=DEV)
    return rs.set_reference(torch.randn(16, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV))


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_an_evaluation_between_iterations_has_no_side_effect(launch):
    from locate_amd.graph import GraphedTrainStep

    def run(measure):
        G, D, step, (lat, real, aug) = build_tiny()
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
        values, losses = [], []
        for i in range(6):
            out = runner.replay() if runner is not None else step(lat, real, aug)
            losses.append((out["d_error"].detach().clone(), out["g_error"].detach().clone()))
            if measure and i == 2:
                rs = small_metric()
                values = [rs.evaluate(G), rs.evaluate(G)]
                assert G.training
                assert tuple(rs.latents(G.g_in).shape) == (16, G.g_in)
        return training_state(G, D, step), losses, values

    plain, plain_losses, _ = run(False)
    watched, losses, values = run(True)
    assert sorted(plain) == sorted(watched)
    bad = [k for k in plain if not torch.equal(plain[k], watched[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(plain_losses, losses))
    assert values[0] == values[1] and values[0]["images"] == 16 and values[0]["nonfinite"] == 0
    assert all(math.isfinite(v) for row in values[0]["gap_db"] for v in row) and len(values[0]["fake"][0]) == 24


def test_evaluate_is_the_parts_and_restores_the_mode():
    from locate_amd import radial_spectrum, spectrum_summary
    from locate_amd.spectrum import summary_means
    G, _, _, _ = build_tiny()
    rs = small_metric()
    G.eval()
    first = rs.evaluate(G)
    assert not G.training
    G.train()
    assert rs.evaluate(G) == first and G.training
    rng = torch.Generator(device=DEV)
    rng.manual_seed(4 + 3)
    latents = torch.randn(16, G.g_in, device=DEV, generator=rng)
    assert torch.equal(rs.latents(G.g_in), latents)
    G.eval()
    with torch.no_grad():
        images = torch.cat([G(latents[:8]), G(latents[8:])])
    assert first["fake"] == summary_means(spectrum_summary(radial_spectrum(images)))[0]


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, files in os.walk(str(root)) for f in files)


def test_trainer_records_the_metric(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, RadialSpectrum, Trainer
    store = DeviceImageStore(STORE, DEV)

    def trainer(out, epochs, with_metric):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        rs = None
        if with_metric:
            rs = RadialSpectrum(32, images=16, seed=3, chunk=8, device=DEV).reference_from_pipeline(pipeline)
            assert (pipeline.epoch, pipeline.pos) == (0, 0)          # the training pipeline's shuffle is not advanced
            assert rs.baseline is not None and rs.baseline["nonfinite"] == 0          # 32 images in the store: a second, disjoint 16
        t = Trainer(step, pipeline, str(out), epochs=epochs, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                    image_interval_function=lambda batch: 2, spectrum=rs)
        return t, G, D, step, rs

    path = os.path.join(str(tmp_path / "with"), "error", "spectrum.json")
    first, G0, _, _, rs0 = trainer(tmp_path / "with", 1, True)
    assert first.run() == 4 and path in first.written
    rec = json.load(open(path))
    assert len(rec) == 1 and rec[0] == dict(rs0.evaluate(G0), epoch=1, iterations=4) and "average" not in rec[0]          # the weights are the saved ones
    assert sorted(rec[0]) == ["baseline", "bins", "epoch", "fake", "gap_db", "high_gap_db", "images", "iterations", "max_abs_gap_db", "nonfinite",
                              "real", "window"]
    assert sorted(rec[0]["baseline"]) == ["fake", "gap_db", "high_gap_db", "max_abs_gap_db", "nonfinite", "real"] and rec[0]["baseline"]["real"] == rec[0]["real"]
    assert not os.path.exists(path + ".tmp")
    rest, G1, D1, step1, _ = trainer(tmp_path / "with", 2, True)          # a resumed run appends
    assert rest.resume().epoch == 1 and rest.run() == 8
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 8) and rec2[1]["real"] == rec[0]["real"]

    plain, G2, D2, step2, _ = trainer(tmp_path / "without", 2, False)
    assert plain.run() == 8
    extra = [os.path.join("error", "spectrum.json")]
    assert listing(tmp_path / "without") == [f for f in listing(tmp_path / "with") if f not in extra]
    strip = lambda files, root: [os.path.relpath(f, str(root)) for f in files if not f.endswith("spectrum.json")]      # noqa: E731
    assert strip(plain.written, tmp_path / "without") == strip(first.written + rest.written, tmp_path / "with")
    for name in ("error/1.json", "error/2.json"):          # the loss curves: the same numbers
        assert json.load(open(os.path.join(str(tmp_path / "with"), name))) == json.load(open(os.path.join(str(tmp_path / "without"), name))), name
    a, b = training_state(G1, D1, step1), training_state(G2, D2, step2)
    assert sorted(a) == sorted(b) and not [k for k in a if not torch.equal(a[k], b[k])]


def test_trainer_records_the_average_too(tmp_path):
    from locate_amd import AveragedGenerator, DeviceImageStore, InputPipeline, RadialSpectrum, Trainer
    store = DeviceImageStore(STORE, DEV)
    G3, _, step, _ = build_tiny()
    pipeline = InputPipeline(store, 32, 8, seed=11)
    rs = RadialSpectrum(32, images=8, seed=3, chunk=8, window="hann", device=DEV).reference_from_pipeline(pipeline)
    t3 = Trainer(step, pipeline, str(tmp_path / "average"), epochs=1, images=13, seed=3, miniter_function=lambda e: 1,
                 subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, spectrum=rs,
                 average=AveragedGenerator(G3, half_life_images=64, batch=8))
    assert t3.run() == 4
    rec = json.load(open(os.path.join(str(tmp_path / "average"), "error", "spectrum.json")))
    ema = rs.evaluate(t3.average.generator)
    assert len(rec) == 1 and rec[0]["average"] == {k: v for k, v in ema.items() if k != "baseline"} and rec[0]["window"] == "hann"
    assert {k: v for k, v in rec[0].items() if k != "average"} == dict(rs.evaluate(G3), epoch=1, iterations=4)


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, STORE)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--spectrum-images", "16", "--spectrum-window", "hann"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    rec = json.load(open(os.path.join(out, "error", "spectrum.json")))
    assert len(rec) == 1 and (rec[0]["epoch"], rec[0]["iterations"], rec[0]["images"], rec[0]["bins"], rec[0]["window"]) == (1, 4, 16, 24, "hann")
    assert rec[0]["baseline"] is not None and rec[0]["nonfinite"] == 0 and len(rec[0]["gap_db"]) == 3 and len(rec[0]["gap_db"][0]) == 24
    assert all(math.isfinite(v) for row in rec[0]["gap_db"] for v in row) and math.isfinite(rec[0]["max_abs_gap_db"])
    assert not [f for f in listing(out) if "swd" in f or "manifold" in f]
