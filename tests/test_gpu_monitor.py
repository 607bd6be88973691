"""The training monitor on the MI355X: the grid kernels (csrc/grid.hip) through the raw C ABI against the recorded output of the
reference's chain (tests/golden/g23_sample_grid.npz) and against the numpy model where a case is too big to store - equality,
never a tolerance - and the behaviour of Sampler, LossHistory and Trainer around a running training: a sampling pass between
iterations, eager or replayed, must leave the trajectory exactly where the reference's loop (or, with
advance_spectral_norm=False, a run without any monitoring) would."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
FIXTURE_CASES = ["tanh13", "randn16", "tiny5", "const4", "nrow5", "range6"]


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """The render tests hold several hundred MB of sentinel-filled buffers (the 64 x 3 x 256 x 256 case alone 250 MB); hand the
    cached blocks back when the module is done instead of leaving them to whatever runs next in the process."""
    yield
    _RUNS.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def abi_grid(x_np, nrow, padding, value_range=None, pad_value=0.0):
    """locate_image_range + locate_image_grid with every argument built here: (range, grid_f32, grid_u8) on the host.
    The outputs are pre-filled with sentinels (NaN; bytes 0x5A, which no alpha byte may keep), the workspace with garbage."""
    from locate_amd._lib import check, lib
    L = lib()
    x = torch.from_numpy(np.ascontiguousarray(x_np, dtype=np.float32)).to(DEV)
    n, S = int(x.shape[0]), int(x.shape[2])
    _, _, GH, GW = M.geometry(n, S, nrow, padding)
    f32 = torch.full((3, GH, GW), float("nan"), device=DEV)
    u8 = torch.full((GH, GW, 4), 0x5A, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if value_range is None:
        rng = torch.full((2,), float("nan"), device=DEV)
        nbytes = L.locate_image_range_workspace_bytes()
        assert 0 < nbytes <= 1 << 20
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        check(L.locate_image_range(p(x), x.numel(), p(rng), p(ws), stream), "locate_image_range")
        divisor = 0.0
    else:
        rng = torch.tensor(value_range, dtype=torch.float32).to(DEV)
        divisor = float(np.float32(max(float(value_range[1]) - float(value_range[0]), 1e-5)))
    check(L.locate_image_grid(p(x), n, S, nrow, padding, pad_value, p(rng), divisor, p(f32), p(u8), stream), "locate_image_grid")
    torch.cuda.synchronize()
    return rng.cpu().numpy(), f32.cpu().numpy(), u8.cpu().numpy()


def report(name, got, want):
    diff = int((got != want).sum())
    print("%s: %d of %d values differ" % (name, diff, want.size))
    return diff


def fixture_case(z, name):
    nrow, padding = (int(v) for v in z["args_" + name])
    vr = tuple(float(v) for v in z["range_" + name]) or None
    return z["x_" + name], nrow, padding, vr


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_kernels_reproduce_the_recorded_chain(name):
    z = load_golden("g23_sample_grid")
    x, nrow, padding, vr = fixture_case(z, name)
    rng, f32, u8 = abi_grid(x, nrow, padding, vr)
    # the recorded fp32 grid where the fixture holds it; the model (which the fixture tool held equal to it) elsewhere
    want_f32 = z["grid_" + name] if "grid_" + name in z.files else M.model(x, nrow, padding, vr)[0]
    if vr is None:
        assert rng[0] == x.min() and rng[1] == x.max(), (rng, x.min(), x.max())
    bad = report(name + " bytes", u8, z["rgba_" + name]) + report(name + " fp32 grid", f32, want_f32)
    assert bad == 0
    assert u8.shape == z["rgba_" + name].shape and f32.dtype == np.float32


@pytest.mark.parametrize("n,S,nrow,padding,pad_value", [(64, 64, 8, 8, 0.0), (64, 256, 8, 8, 0.0), (1, 7, 8, 2, 0.0), (7, 5, 3, 0, 0.0),
                                                        (256, 32, 8, 2, 0.5), (10, 33, 16, 1, 1.0)])
def test_kernels_equal_the_model(n, S, nrow, padding, pad_value):
    rng_np = np.random.default_rng(n * 1000 + S)
    x = np.tanh(1.5 * rng_np.standard_normal((n, 3, S, S), dtype=np.float32)).astype(np.float32)
    rng, f32, u8 = abi_grid(x, nrow, padding, None, pad_value)
    want_f32, want_u8 = M.model(x, nrow, padding, None, pad_value)
    assert rng[0] == x.min() and rng[1] == x.max()
    tag = "%d x 3 x %d x %d" % (n, S, S)
    assert report(tag + " bytes", u8, want_u8) + report(tag + " fp32 grid", f32, want_f32) == 0


def test_range_over_odd_sizes_and_a_nan():
    from locate_amd._lib import check, lib
    L = lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ws = torch.empty(L.locate_image_range_workspace_bytes(), dtype=torch.uint8, device=DEV)
    base = torch.randn(1 << 20, generator=torch.Generator().manual_seed(4)).to(DEV)
    for off, count in ((0, 1), (1, 3), (0, 1023), (3, 70001), (0, 1 << 20), (1, (1 << 20) - 1)):
        x = base[off:off + count]                     # off != 0: not 16-byte aligned
        rng = torch.full((2,), float("nan"), device=DEV)
        check(L.locate_image_range(p(x), count, p(rng), p(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_image_range")
        assert torch.equal(rng, torch.stack([x.min(), x.max()])), (off, count)
    x = base[:5000].clone()
    x[4321] = float("nan")
    rng = torch.zeros(2, device=DEV)
    check(L.locate_image_range(p(x), 5000, p(rng), p(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_image_range")
    assert torch.isnan(rng).all()                     # the caller can see a non-finite batch, as with torch's min() / max()


def test_image_grid_python_layer():
    from locate_amd import image_grid
    from locate_amd._lib import LocateError
    z = load_golden("g23_sample_grid")
    for name in ("nrow5", "range6", "tanh13"):
        x, nrow, padding, vr = fixture_case(z, name)
        xd = T(x).to(DEV)
        rgba = image_grid(xd, nrow=nrow, padding=padding, value_range=vr)
        assert rgba.dtype == torch.uint8 and rgba.is_cuda and np.array_equal(rgba.cpu().numpy(), z["rgba_" + name])
        want = z["grid_" + name] if "grid_" + name in z.files else M.model(x, nrow, padding, vr)[0]
        assert np.array_equal(image_grid(xd, nrow=nrow, padding=padding, value_range=vr, as_float=True).cpu().numpy(), want)
        out = torch.zeros_like(rgba)
        assert image_grid(xd, nrow=nrow, padding=padding, value_range=vr, out=out) is out and torch.equal(out, rgba)
    # a range whose width is not the same in fp32 and in double: the divisor comes from the doubles
    x = z["x_range6"]
    vr = (-0.3, 0.7000001)
    assert np.array_equal(image_grid(T(x).to(DEV), value_range=vr).cpu().numpy(), M.model(x, 8, 2, vr)[1])
    with pytest.raises(ValueError):
        image_grid(torch.zeros(2, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        image_grid(torch.zeros(2, 3, 8, 8, device=DEV), out=torch.zeros(3, 3, 4, dtype=torch.uint8, device=DEV))
    from locate_amd._lib import check, lib
    with pytest.raises(LocateError):                 # the library refuses a call without an output
        r = torch.zeros(2, device=DEV)
        check(lib().locate_image_grid(ctypes.c_void_p(r.data_ptr()), 1, 1, 1, 0, 0.0, ctypes.c_void_p(r.data_ptr()), 0.0, None, None, None), "x")


# ---- around a training run: the tiny fixture network (32 x 32, base width 1, batch 8) --------------------------------------------
def build_tiny(minibatches=1):
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
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=minibatches)
    inputs = tuple(T(z["step1/" + k]).to(DEV) for k in ("latent", "real", "aug"))
    return G, D, step, inputs


def training_state(G, D, step):
    """every parameter (u and v included) and every Nadam state tensor, by name"""
    torch.cuda.synchronize()
    state = {"G/" + k: v.detach().clone() for k, v in G.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in D.state_dict().items()})
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        for name, p in net.named_parameters():
            for k, v in opt.state.get(p, {}).items():
                if torch.is_tensor(v):
                    state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
    return state


def assert_same_state(a, b, what):
    assert sorted(a) == sorted(b), what
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, "%s: %d of %d tensors differ, first %s" % (what, len(bad), len(a), bad[:4])


K = 4
_RUNS = {}


def fixed_latents(G):
    return torch.randn(13, G.g_in, generator=torch.Generator().manual_seed(13)).to(DEV)


def run(launch, monitor):
    """K iterations of the fixture step, `launch` = eager | graphed, with after every iteration: nothing (`none`), a
    Sampler(images=13) that keeps u / v (`keep`) or advances them (`advance`), or the reference's sampling lines spelled out here
    (`manual`, main.py:195-202).  13 images != batch 8: a second batch size goes through the generator between the iterations."""
    if (launch, monitor) in _RUNS:
        return _RUNS[(launch, monitor)]
    from locate_amd import Sampler
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny()
    noise = fixed_latents(G)
    sampler = Sampler(G, fixed_noise=noise, advance_spectral_norm=(monitor == "advance")) if monitor in ("keep", "advance") else None
    runner = GraphedTrainStep(step, lat, real, aug, warmup=2) if launch == "graphed" else None
    pictures = []
    for _ in range(K):
        if runner is not None:
            runner.replay()
        else:
            step(lat, real, aug)
        if sampler is not None:
            pictures.append(sampler.render().clone())
            assert G.training
        elif monitor == "manual":
            G.eval()
            with torch.no_grad():
                G(noise)
            G.train()
    _RUNS[(launch, monitor)] = (training_state(G, D, step), pictures)
    return _RUNS[(launch, monitor)]


def test_sampler_renders_the_generator_output(tmp_path):
    from locate_amd import Sampler, image_grid
    from locate_amd.monitor import read_png
    G1, _, _, _ = build_tiny()
    G2, _, _, _ = build_tiny()
    sampler = Sampler(G1, images=13, seed=5)
    assert sampler.fixed_noise.shape == (13, G1.g_in) and sampler.padding == 8 and sampler.advance_spectral_norm
    assert torch.equal(Sampler(G1, images=13, seed=5).fixed_noise, sampler.fixed_noise)
    picture = sampler.render().clone()
    assert G1.training
    G2.eval()
    with torch.no_grad():
        fake = G2(sampler.fixed_noise)
    G2.train()
    assert torch.equal(picture, image_grid(fake, nrow=8, padding=8))
    assert tuple(picture.shape) == (2 * 40 + 8, 8 * 40 + 8, 4)
    assert np.array_equal(picture.cpu().numpy(), M.model(fake.cpu().numpy(), 8, 8)[1])
    # save(): with u / v kept, the file holds the bytes render() returns
    keeper = Sampler(G1, fixed_noise=sampler.fixed_noise, advance_spectral_norm=False)
    before = [p.detach().clone() for p in keeper._uv]
    shown = keeper.render().clone()
    path = keeper.save(str(tmp_path / "sample.png"))
    assert np.array_equal(read_png(path), shown.cpu().numpy())
    assert before and all(torch.equal(a, b) for a, b in zip(before, keeper._uv))
    try:
        from PIL import Image
    except ImportError:
        pass
    else:
        with Image.open(path) as im:
            assert np.array_equal(np.asarray(im), shown.cpu().numpy())
    # preview: plot_images' form of a real batch
    real = T(load_golden("g8_tiny_e2e")["step1/real"]).to(DEV)
    keeper.preview(real, str(tmp_path / "real.png"))
    assert np.array_equal(read_png(str(tmp_path / "real.png")), M.model(real.cpu().numpy(), 8, 2)[1])


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_sampling_that_keeps_u_and_v_has_no_side_effect(launch):
    """Every parameter, u, v and Nadam moment after K iterations with a picture after each equals the run without monitoring."""
    plain, _ = run(launch, "none")
    watched, pictures = run(launch, "keep")
    assert_same_state(watched, plain, launch)
    assert len(pictures) == K and not torch.equal(pictures[0], pictures[-1])


@pytest.mark.parametrize("launch", ["eager", "graphed"])
def test_sampling_that_advances_u_and_v_is_the_reference_loop(launch):
    watched, pictures = run(launch, "advance")
    manual, _ = run(launch, "manual")
    assert_same_state(watched, manual, launch)
    plain, _ = run(launch, "none")
    moved = [k for k in plain if k.startswith("G/") and k.endswith(("weight_u", "weight_v")) and not torch.equal(plain[k], watched[k])]
    assert moved, "the sampling pass advances the generator's u / v"
    _, kept_pictures = run(launch, "keep")
    assert torch.equal(kept_pictures[0], pictures[0])          # the first picture is taken before any pass has moved anything


def test_loss_history_under_replay():
    from locate_amd import LossHistory
    from locate_amd.graph import GraphedTrainStep
    G, D, step, (lat, real, aug) = build_tiny()
    runner = GraphedTrainStep(step, lat, real, aug, warmup=2)
    whole, small = LossHistory(), LossHistory(capacity=2)
    want = []
    for _ in range(5):
        out = runner.replay()
        assert whole.record(out) and small.record(out)
        want.append((float(out["d_error"]) / 2, float(out["g_error"])))
    assert whole.flush() == want and whole.flush() == []
    small.flush()
    assert list(zip(small.d, small.g)) == want and list(zip(whole.d, whole.g)) == want
    assert len({w for w in want}) == 5


def test_trainer_writes_its_files_and_resumes(tmp_path):
    from locate_amd import DeviceImageStore, InputPipeline, Trainer
    from locate_amd.monitor import read_png
    images = np.random.default_rng(6).integers(0, 256, size=(64, 78, 64, 3), dtype=np.uint8)

    def trainer(out, max_iterations, lines=None):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(DeviceImageStore(images, DEV), 32, 8, seed=11)
        t = Trainer(step, pipeline, str(out), epochs=1, max_iterations=max_iterations, images=13, seed=3,
                    image_interval_function=lambda batch: 2, print_every_function=lambda batch: 2,
                    log=None if lines is None else lines.append)
        return t, G, D, step

    lines = []
    whole, G1, D1, step1 = trainer(tmp_path / "whole", 6, lines)
    assert whole.schedule(0) == {"miniter": 1, "subepochs": 1, "print_every": 2, "image_interval": 2}
    assert whole.run() == 6
    state_whole = training_state(G1, D1, step1)
    out = str(tmp_path / "whole")
    for name in ("1/1-2.png", "1/1-4.png", "1/1-6.png", "netG.torch", "netD.torch", "netG.extra.torch", "optG.torch", "optD.torch", "trainer.torch"):
        assert os.path.exists(os.path.join(out, name)), name
    assert not os.path.exists(os.path.join(out, "1/1-END.png")) and not os.path.exists(os.path.join(out, "1/1-3.png"))
    assert read_png(os.path.join(out, "1/1-4.png")).shape == (2 * 40 + 8, 8 * 40 + 8, 4)
    assert len(lines) == 3 and lines[0].startswith("[1][1/1][2/8] | Rate: ") and "| D:" in lines[0] and lines[-1].startswith("[1][1/1][6/8]")

    first, _, _, _ = trainer(tmp_path / "parts", 3)
    assert first.run() == 3
    rest, G2, D2, step2 = trainer(tmp_path / "parts", 6)
    assert rest.resume().iterations == 3 and (rest.epoch, rest.sub, rest.i) == (0, 0, 3)
    assert rest.run() == 6
    assert_same_state(training_state(G2, D2, step2), state_whole, "3 + 3 iterations against 6")
    assert torch.equal(rest.sampler.fixed_noise, whole.sampler.fixed_noise)
    assert np.array_equal(read_png(os.path.join(out, "1/1-6.png")), read_png(str(tmp_path / "parts" / "1" / "1-6.png")))

    # the uninterrupted run goes on to the end of its only epoch: the END picture, the loss curves, the state of epoch 2
    whole.max_iterations = None
    assert whole.run() == 8
    for name in ("1/1-8.png", "1/1-END.png", "error/1.json"):
        assert os.path.exists(os.path.join(out, name)), name
    rec = json.load(open(os.path.join(out, "error", "1.json")))
    assert len(rec["d"]) == 8 and len(rec["g"]) == 8 and rec["mean_window"] == 16 and rec["d_moving_average"] == []
    saved = torch.load(os.path.join(out, "trainer.torch"), weights_only=True)
    assert (saved["epoch"], saved["sub"], saved["i"], saved["iterations"]) == (1, 0, 0, 8)
    assert saved["pipeline"]["epoch"] == 0 and saved["pipeline"]["pos"] == 8


def test_graphed_trainer_equals_replays_by_hand(tmp_path):
    """Trainer(graphed=True) against the same schedule spelled out: GraphedTrainStep on the first batch (its two eager
    iterations included), a replay per iteration fed from a twin pipeline and a twin latent generator, the advancing sampling pass
    after iterations 2 and 4."""
    from locate_amd import DeviceImageStore, InputPipeline, Sampler, Trainer
    from locate_amd.graph import GraphedTrainStep
    from locate_amd.monitor import read_png
    images = np.random.default_rng(7).integers(0, 256, size=(64, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)
    G1, D1, step1, _ = build_tiny()
    t = Trainer(step1, InputPipeline(store, 32, 8, seed=11), str(tmp_path), epochs=1, max_iterations=5, images=13, seed=3, graphed=True,
                image_interval_function=lambda batch: 2)
    assert t.run() == 5
    want_files = ["1/1-2.png", "1/1-4.png", "trainer.torch", "netG.torch"]
    assert all(os.path.exists(os.path.join(str(tmp_path), f)) for f in want_files)

    G2, D2, step2, _ = build_tiny()
    pipe = InputPipeline(store, 32, 8, seed=11)
    latents = torch.Generator(device=DEV)
    latents.manual_seed(3 + 1)
    sampler = Sampler(G2, images=13, seed=3)
    runner, picture = None, None
    for i in range(1, 6):
        lat = torch.randn((8, G2.g_in), device=DEV, generator=latents)
        real, aug = pipe.next_batch()
        if runner is None:
            runner = GraphedTrainStep(step2, lat, real, aug)
            runner.replay()
        else:
            runner.replay(lat, real, aug)
        if i % 2 == 0:
            picture = sampler.render().clone()
    assert_same_state(training_state(G1, D1, step1), training_state(G2, D2, step2), "graphed trainer")
    assert np.array_equal(read_png(os.path.join(str(tmp_path), "1", "1-4.png")), picture.cpu().numpy())


def test_command_line(tmp_path):
    """python -m locate_amd.run end to end at 32 x 32 (full width), stopped after 3 iterations and resumed to 4, then replayed as graphs."""
    from locate_amd.monitor import read_png
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(48, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    base = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
            "--minibatches", "1", "--images", "16"]

    def call(*extra):
        done = subprocess.run(base + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
        return done.stdout

    assert "3 iterations" in call("--max-iterations", "3")
    for name in ("0.png", "1.png", "trainer.torch", "netG.torch", "optD.torch"):
        assert os.path.exists(os.path.join(out, name)), name
    assert read_png(os.path.join(out, "0.png")).shape == (6 * 34 + 2, 8 * 34 + 2, 4)          # plot_images of 48 real images
    assert "4 iterations" in call("--max-iterations", "4", "--resume", "--keep-spectral-norm")
    text = call("--resume")                                    # to the end of the epoch: 6 batches of 8 from 48 images
    assert "6 iterations" in text and "[1][1/1][" not in text  # print_every = 16 > 6 batches: no progress line
    assert read_png(os.path.join(out, "1", "1-END.png")).shape == (2 * 40 + 8, 8 * 40 + 8, 4)
    assert os.path.exists(os.path.join(out, "error", "1.json"))
    graphed = str(tmp_path / "graphed")
    base[base.index(out)] = graphed
    assert "2 iterations" in call("--max-iterations", "2", "--graph")
    assert os.path.exists(os.path.join(graphed, "trainer.torch"))
