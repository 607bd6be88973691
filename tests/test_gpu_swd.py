"""The sliced Wasserstein metric on the MI355X: every entry point of csrc/swd.hip through the raw C ABI against the float64 model
(tests/helpers/swd_model.py) within bounds worked out from the number formats, the composition in locate_amd/metric.py bit for
bit against its parts, the definition's exact invariances, and the metric's behaviour around a running training: an evaluation
between two iterations, eager or replayed, leaves the trajectory where a run without it would be."""
import ctypes
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
import swd_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    _CACHE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def sentinel(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def garbage(nbytes):
    assert 0 < nbytes <= 1 << 20
    return torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)


# ---- 1. the pyramid --------------------------------------------------------------------------------------------------------------
def spiked(rng, planes, S, where):
    """normal data with one value of 100 in every plane at `where` = (row, column) in {0: first, 1: middle, 2: last}"""
    x = rng.standard_normal((planes, S, S)).astype(np.float32)
    at = [(0, S // 2, S - 1)[w] for w in where]
    x[:, at[0], at[1]] = 100.0
    return x


PLACES = [(r, c) for r in range(3) for c in range(3)]          # four corners, four edge middles, the centre


def abi_down(x):
    from locate_amd._lib import check, lib
    planes, S = x.shape[0], x.shape[-1]
    xd, out = dev(x), sentinel(planes, S // 2, S // 2)
    check(lib().locate_pyr_down(p(xd), planes, S, p(out), stream()), "locate_pyr_down")
    return out.cpu().numpy()


def abi_residual(x, coarse, alias=False):
    from locate_amd._lib import check, lib
    planes, S = x.shape[0], x.shape[-1]
    xd, cd = dev(x), dev(coarse)
    out = xd if alias else sentinel(planes, S, S)
    check(lib().locate_pyr_residual(p(xd), p(cd), planes, S, p(out), stream()), "locate_pyr_residual")
    return out.cpu().numpy()


# (3, 8): every output touches a mirrored tap; (2, 12) and (2, 20): sizes that are no multiple of 8 take the kernels' scalar form
@pytest.mark.parametrize("planes,S", [(3, 8), (6, 16), (5, 32), (3, 64), (2, 12), (2, 20)])
def test_pyramid_entry_points_against_the_model(planes, S):
    rng = np.random.default_rng(100 * planes + S)
    worst_d = worst_r = 0.0
    for where in PLACES:
        x, coarse = spiked(rng, planes, S, where), spiked(rng, planes, S // 2, where)
        got = abi_down(x)
        err = float(np.abs(got - M.down(x)).max())
        assert err <= M.pyr_bound(x), ("down", where, err)
        worst_d = max(worst_d, err)
        got = abi_residual(x, coarse)
        err = float(np.abs(got - (x.astype(np.float64) - M.up(coarse))).max())
        assert err <= M.pyr_bound(x), ("residual", where, err)          # max|x| = max|coarse| = 100
        worst_r = max(worst_r, err)
        assert np.array_equal(abi_residual(x, coarse, alias=True), got), "out aliasing x gives other bits"
    print("%d x %d x %d: down %.2e, residual %.2e, bound %.2e" % (planes, S, S, worst_d, worst_r, 1e-3))


def test_pyramid_on_a_misaligned_buffer():
    """a view that starts 4 bytes into an allocation: the 16-byte loads and stores are not taken"""
    from locate_amd._lib import check, lib
    rng = np.random.default_rng(9)
    x, coarse = rng.standard_normal((2, 16, 16)).astype(np.float32), rng.standard_normal((2, 8, 8)).astype(np.float32)
    buf = torch.zeros(2 * 16 * 16 + 1, device=DEV)
    xd = buf[1:]
    xd.copy_(dev(x).reshape(-1))
    out = sentinel(2 * 8 * 8 + 1)
    check(lib().locate_pyr_down(p(xd), 2, 16, p(out[1:]), stream()), "locate_pyr_down")
    assert np.array_equal(out[1:].cpu().numpy().reshape(2, 8, 8), abi_down(x)) and math.isnan(float(out[0]))
    cd = dev(coarse)
    check(lib().locate_pyr_residual(p(xd), p(cd), 2, 16, p(xd), stream()), "locate_pyr_residual")
    assert np.array_equal(xd.cpu().numpy().reshape(2, 16, 16), abi_residual(x, coarse)) and float(buf[0]) == 0.0


@pytest.mark.parametrize("S", [32, 64])
def test_laplacian_pyramid_against_the_model(S):
    from locate_amd import laplacian_pyramid
    rng = np.random.default_rng(S)
    x = np.stack([spiked(rng, 3, S, (i % 3, 2 - i % 3)) for i in range(2)])
    got = laplacian_pyramid(dev(x))
    want = M.laplacian_pyramid(x)
    assert [tuple(g.shape) for g in got] == [w.shape for w in want] and len(got) == (2 if S == 32 else 3)
    for l, (g, w) in enumerate(zip(got, want)):
        err = float(np.abs(g.cpu().numpy() - w).max())
        print("S = %d level %d: %.2e (bound %.2e)" % (S, l, err, M.pyr_bound(x)))
        assert err <= M.pyr_bound(x)
    assert torch.equal(laplacian_pyramid(dev(x), levels=1)[0], dev(x))


# ---- 2. - 3. descriptors -----------------------------------------------------------------------------------------------------------
def positions(rng, N, S, P):
    """random corners in [0, S - 7]; the first descriptors sit at both extremes of both axes"""
    pos = rng.integers(0, S - 6, size=(N * P, 2)).astype(np.int32)
    pos[0], pos[1], pos[2], pos[3] = (0, 0), (S - 7, S - 7), (0, S - 7), (S - 7, 0)
    return pos


def abi_stats(level, pos, P):
    from locate_amd._lib import check, lib
    L = lib()
    N, S = level.shape[0], level.shape[-1]
    ld, pd, stats, ws = dev(level), dev(pos, np.int32), sentinel(6), garbage(L.locate_swd_stats_workspace_bytes())
    check(L.locate_swd_stats(p(ld), N, S, p(pd), P, p(stats), p(ws), stream()), "locate_swd_stats")
    return stats.cpu().numpy()


@pytest.mark.parametrize("N,S,P,shift", [(3, 16, 5, 0.0), (2, 32, 128, 0.0), (2, 32, 128, 50.0)])
def test_descriptor_stats(N, S, P, shift):
    rng = np.random.default_rng(N * 100 + S + P)
    level = (rng.standard_normal((N, 3, S, S)) * [[[[1.0]], [[0.5]], [[3.0]]]] + shift).astype(np.float32)
    pos = positions(rng, N, S, P)
    got = abi_stats(level, pos, P)
    mu, sigma = M.stats64(M.descriptors(level, pos, P))
    print("mu", got[:3], mu, "r", got[3:], 1 / sigma)
    assert got.dtype == np.float32
    assert (np.abs(got[:3] - mu) <= 1e-6 * (np.abs(mu) + sigma)).all()          # one fp32 rounding; the fp64 sums give ~1e-13
    assert (np.abs(got[3:].astype(np.float64) * sigma - 1) <= 1e-6).all()
    assert np.array_equal(abi_stats(level, pos, P), got)


def abi_project(level, pos, P, dirs, stats):
    from locate_amd._lib import check, lib
    N, S, D = level.shape[0], level.shape[-1], dirs.shape[1]
    ld, pd, dd, sd, proj = dev(level), dev(pos, np.int32), dev(dirs), dev(stats), sentinel(D, N * P)
    check(lib().locate_swd_project(p(ld), N, S, p(pd), P, p(dd), D, p(sd), p(proj), stream()), "locate_swd_project")
    return proj.cpu().numpy()


def unit_dirs(rng, D):
    d = rng.standard_normal((M.K, D))
    return (d / np.sqrt((d * d).sum(0, keepdims=True))).astype(np.float32)


# (3, 16, 5, 3): both tile edges ragged, K = 147 odd against the k-step of 2; (2, 32, 128, 128): one full tile per image;
# (5, 16, 128, 130): several row tiles and a ragged column tile; shift 50: |mu| = 50 sigma, which a mean folded into a
# per-direction constant does not survive (1.55 of the bound in fp32 on the host, 0.10 in the specified order)
@pytest.mark.parametrize("N,S,P,D,shift", [(3, 16, 5, 3, 0.0), (2, 32, 128, 128, 0.0), (5, 16, 128, 130, 0.0), (2, 32, 128, 128, 50.0)])
def test_projection_within_the_dot_product_bound(N, S, P, D, shift):
    rng = np.random.default_rng(N + S + P + D)
    level = (rng.standard_normal((N, 3, S, S)) + shift).astype(np.float32)
    pos, dirs = positions(rng, N, S, P), unit_dirs(rng, D)
    desc = M.descriptors(level, pos, P)
    st = M.stats(desc)
    got = abi_project(level, pos, P, dirs, st)
    want, bound = M.project(desc, dirs, st), M.proj_bound(desc, dirs, st)
    ratio = np.abs(got - want) / bound
    print("N %d S %d P %d D %d shift %g: worst error / bound %.3f" % (N, S, P, D, shift, ratio.max()))
    assert got.shape == (D, N * P) and np.isfinite(got).all()
    assert (np.abs(got - want) <= bound).all()
    assert np.array_equal(abi_project(level, pos, P, dirs, st), got)
    # an image of NaN: its descriptors' projections, and no others, are not finite
    bad = N // 2
    level[bad] = np.nan
    finite = np.isfinite(abi_project(level, pos, P, dirs, st))
    owner = np.arange(N * P) // P
    assert (finite == (owner != bad)[None, :]).all()


# ---- 4. the distance ---------------------------------------------------------------------------------------------------------------
def abi_distance(a, b):
    from locate_amd._lib import check, lib
    L = lib()
    out, ws = sentinel(1), garbage(L.locate_swd_distance_workspace_bytes())
    check(L.locate_swd_distance(p(a), p(b), a.numel(), p(out), p(ws), stream()), "locate_swd_distance")
    return float(out)


@pytest.mark.parametrize("count", [1, 7 * 13, 128 * 4099])
def test_distance_against_float64(count):
    g = torch.Generator().manual_seed(count)
    base_a, base_b = torch.randn(count + 1, generator=g).to(DEV), torch.randn(count + 1, generator=g).to(DEV)
    for off in (0, 1):          # off = 1: not 16-byte aligned
        a, b = base_a[off:off + count], base_b[off:off + count]
        want = float((a.double() - b.double()).abs().mean())
        got = abi_distance(a, b)
        print("count %d offset %d: %.9g against %.9g" % (count, off, got, want))
        assert abs(got - want) <= 1e-6 * want
        assert abi_distance(a, a) == 0.0 and abi_distance(a, b) == got


# ---- 5. - 7. the composition -------------------------------------------------------------------------------------------------------
SHAPE = dict(images=8, nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8)
_CACHE = {}


def case():
    """a: normal noise; b: smooth (noise through the 5 x 5 filter, times 6) and quantised to multiples of 2^-12, so that 4 b and
    2 b + 3 are exact in fp32; the metric object; the model's values and bounds for (a, b) - computed once"""
    if "case" not in _CACHE:
        from locate_amd import SlicedWasserstein
        rng = np.random.default_rng(5)
        a = rng.standard_normal((8, 3, 32, 32)).astype(np.float32)
        b = (np.round(6.0 * M.blur(rng.standard_normal((8, 3, 32, 32))) * 4096) / 4096).astype(np.float32)
        swd = SlicedWasserstein(32, seed=21, device=DEV, **SHAPE)
        pos = {k: [t.numpy() for t in v] for k, v in swd.positions.items()}
        model = M.swd(a, b, pos["reference"], pos["candidate"], 16, swd.directions.numpy(), 2, with_bound=True)
        _CACHE["case"] = (a, b, swd, model)
    return _CACHE["case"]


def by_hand(swd, a, b):
    from locate_amd import descriptor_stats, laplacian_pyramid, project_descriptors, sorted_distance
    R, Dr, P = swd.dir_repeats, swd.dirs_per_repeat, swd.nhoods_per_image
    la, lb = laplacian_pyramid(a), laplacian_pyramid(b)
    levels = []
    for l in range(len(la)):
        pa, pb = swd.positions["reference"][l].to(DEV), swd.positions["candidate"][l].to(DEV)
        sa, sb = descriptor_stats(la[l], pa, P), descriptor_stats(lb[l], pb, P)
        vals = []
        for r in range(R):
            dirs = swd.directions[:, r * Dr:(r + 1) * Dr].contiguous().to(DEV)
            xa = torch.sort(project_descriptors(la[l], pa, P, dirs, sa), dim=1).values
            xb = torch.sort(project_descriptors(lb[l], pb, P, dirs, sb), dim=1).values
            vals.append(float(sorted_distance(xa, xb)))
        levels.append(sum(vals) / R)
    return {"levels": levels, "mean": sum(levels) / len(levels)}


def test_between_is_its_parts_bit_for_bit():
    a, b, swd, _ = case()
    ad, bd = dev(a), dev(b)
    got = swd.between(ad, bd)
    assert got == by_hand(swd, ad, bd) and len(got["levels"]) == 2
    assert not swd.has_reference
    assert swd.set_reference(ad).distance(bd) == got and swd.has_reference
    assert swd.set_reference([ad[:3], ad[3:]]).distance(iter([bd[:5], bd[5:]])) == got          # batches summing to N
    with pytest.raises(ValueError):
        swd.distance(bd[:7])
    swd._reference = None


def test_end_to_end_against_the_model():
    a, b, swd, model = case()
    got = swd.between(dev(a), dev(b))
    for l, (g, w, bound) in enumerate(zip(got["levels"], model["levels"], model["bound"])):
        print("level %d: %.9g against %.9g, difference %.2e, bound %.2e = %.2f %% of the value" % (l, g, w, abs(g - w), bound, 100 * bound / w))
        assert bound <= 0.05 * w, "inputs with a larger value are needed"
        assert abs(g - w) <= bound
    assert abs(got["mean"] - model["mean"]) <= max(model["bound"])


def test_exact_properties():
    a, b, swd, model = case()
    ad, bd = dev(a), dev(b)
    same = swd.between(ad, ad, same_positions=True)
    assert same["levels"] == [0.0, 0.0] and same["mean"] == 0.0
    assert all(v > 0 for v in swd.between(ad, ad)["levels"])
    got = swd.between(ad, bd)
    assert swd.between(ad, 4 * bd) == got          # every step is equivariant under a power of four
    moved = swd.between(ad, 2 * bd + 3)            # exact in fp32 for this b
    assert np.array_equal((2 * bd + 3).cpu().numpy().astype(np.float64), 2 * b.astype(np.float64) + 3)
    for l in range(2):
        print("level %d: 2 b + 3 moves the value by %.2e (bound %.2e)" % (l, abs(moved["levels"][l] - got["levels"][l]), model["bound"][l]))
        assert abs(moved["levels"][l] - got["levels"][l]) <= model["bound"][l]


# ---- 8. - 9. around a training run: the tiny fixture network of tests/test_gpu_monitor.py (32 x 32, base width 1, batch 8) ------------
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


def small_metric(seed=4):
    from locate_amd import SlicedWasserstein
    swd = SlicedWasserstein(32, images=16, nhoods_per_image=8, dir_repeats=2, dirs_per_repeat=8, seed=seed, chunk=8, device=DEV)
    return swd.set_reference(torch.randn(16, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(DEV))


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_an_evaluation_between_iterations_has_no_side_effect(launch):
    from locate_amd.graph import GraphedTrainStep

    def run(measure):
        G, D, step, (lat, real, aug) = build_tiny()
        runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
        values = []
        for i in range(6):
            if runner is not None:
                runner.replay()
            else:
                step(lat, real, aug)
            if measure and i == 2:
                swd = small_metric()
                values = [swd.evaluate(G), swd.evaluate(G)]
                assert G.training
                assert tuple(swd.latents(G.g_in).shape) == (16, G.g_in)
        return training_state(G, D, step), values

    plain, _ = run(False)
    watched, values = run(True)
    assert sorted(plain) == sorted(watched)
    bad = [k for k in plain if not torch.equal(plain[k], watched[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (launch, len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain)
    assert values[0] == values[1] and len(values[0]["levels"]) == 2
    assert all(math.isfinite(v) and v > 0 for v in values[0]["levels"]) and math.isfinite(values[0]["mean"])


def test_evaluate_restores_eval_mode_too():
    G, _, _, _ = build_tiny()
    swd = small_metric()
    G.eval()
    first = swd.evaluate(G)
    assert not G.training
    G.train()
    assert swd.evaluate(G) == first and G.training


def test_trainer_records_the_metric(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, SlicedWasserstein, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, epochs, with_metric):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        swd = None
        if with_metric:
            swd = SlicedWasserstein(32, images=16, nhoods_per_image=8, dir_repeats=2, dirs_per_repeat=8, seed=3, chunk=8, device=DEV)
            swd.reference_from_pipeline(pipeline)
            assert (pipeline.epoch, pipeline.pos) == (0, 0)          # the training pipeline's shuffle is not advanced
        t = Trainer(step, pipeline, str(out), epochs=epochs, images=13, seed=3, miniter_function=lambda e: 1, subepoch_function=lambda e: 1,
                    image_interval_function=lambda batch: 2, swd=swd)
        return t, G, D, step

    path = os.path.join(str(tmp_path / "with"), "error", "swd.json")
    first, _, _, _ = trainer(tmp_path / "with", 1, True)
    assert first.run() == 4 and path in first.written
    rec = json.load(open(path))
    assert len(rec) == 1 and sorted(rec[0]) == ["epoch", "iterations", "levels", "mean"] and (rec[0]["epoch"], rec[0]["iterations"]) == (1, 4)
    assert len(rec[0]["levels"]) == 2 and all(math.isfinite(v) for v in rec[0]["levels"] + [rec[0]["mean"]])
    assert not os.path.exists(path + ".tmp")
    rest, G1, D1, step1 = trainer(tmp_path / "with", 2, True)          # a resumed run appends
    assert rest.resume().epoch == 1 and rest.run() == 8
    rec2 = json.load(open(path))
    assert len(rec2) == 2 and rec2[0] == rec[0] and (rec2[1]["epoch"], rec2[1]["iterations"]) == (2, 8)

    plain, G2, D2, step2 = trainer(tmp_path / "without", 2, False)
    assert plain.run() == 8
    assert not os.path.exists(os.path.join(str(tmp_path / "without"), "error", "swd.json"))
    # the same files as with the metric, its own aside, in the same order: two epochs' worth against the second epoch's
    strip = lambda files, root: [os.path.relpath(f, str(root)) for f in files if not f.endswith("swd.json")]      # noqa: E731
    assert strip(plain.written, tmp_path / "without") == strip(first.written + rest.written, tmp_path / "with")
    for name in ("1/1-2.png", "1/1-END.png", "error/1.json", "2/1-4.png", "error/2.json", "trainer.torch", "netG.torch"):
        assert name in strip(plain.written, tmp_path / "without"), name
    # and the same trajectory
    a, b = training_state(G1, D1, step1), training_state(G2, D2, step2)
    assert sorted(a) == sorted(b) and not [k for k in a if not torch.equal(a[k], b[k])]


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--swd-images", "16"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "4 iterations" in done.stdout
    rec = json.load(open(os.path.join(out, "error", "swd.json")))
    assert len(rec) == 1 and rec[0]["epoch"] == 1 and rec[0]["iterations"] == 4
    assert len(rec[0]["levels"]) == 2 and all(math.isfinite(v) and v > 0 for v in rec[0]["levels"]) and math.isfinite(rec[0]["mean"])
