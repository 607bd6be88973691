"""The device-side input pipeline on the MI355X (csrc/input.hip through the C ABI, locate_amd/data.py on top): the kernels'
output against Pillow's own bytes (tests/golden/g22_input_pipeline.npz) and against the integer model where the image does not
fit LDS whole - equality, not a tolerance - and the pipeline's behaviour around it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import input_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def abi_transform(sources, idx, params, n_first, S, side_lo):
    """One locate_input_transform call, every argument built here: returns (out_first, out_rest)."""
    from locate_amd import data
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_input_param_record_bytes() == data.PARAM_DTYPE.itemsize
    N, H, W = sources.shape[:3]
    n = len(idx)
    data.validate(idx, params, N, H, W, side_lo, min(H, W))
    table, ktaps = data.resize_table(side_lo, min(H, W), S)
    store = torch.from_numpy(sources).to(DEV)
    d_idx = torch.from_numpy(np.asarray(idx, dtype=np.int32)).to(DEV)
    d_par = torch.from_numpy(params.view(np.uint8).copy()).to(DEV)
    d_coef, d_lut = torch.from_numpy(table).to(DEV), data.output_lut().to(DEV)
    ws = torch.empty(max(L.locate_input_workspace_bytes(n, H, W), 16), dtype=torch.uint8, device=DEV)
    assert L.locate_input_workspace_bytes(n, H, W) == 4 * n * L.locate_input_mean_blocks(H, W)
    out_a = torch.full((n_first, 3, S, S), float("nan"), device=DEV)
    out_b = torch.full((n - n_first, 3, S, S), float("nan"), device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    check(L.locate_input_transform(p(store), N, H, W, p(d_idx), p(d_par), n, n_first, p(d_coef), side_lo, min(H, W), ktaps, p(d_lut),
                                   S, p(out_a), p(out_b), p(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "locate_input_transform")
    torch.cuda.synchronize()
    return out_a.cpu(), out_b.cpu()


def make_records(rows):
    """rows of (flip, order list, factors, top, left, side) as PARAM_DTYPE records"""
    from locate_amd import data
    rec = np.zeros(len(rows), dtype=data.PARAM_DTYPE)
    for i, (flip, order, f, top, left, side) in enumerate(rows):
        rec[i] = (flip, data.pack_order(order), f[0], f[1], f[2], top, left, side)
    return rec


def report(name, got, want):
    diff = int((got != want).sum())
    print("%s: %d of %d values differ" % (name, diff, want.numel()))
    return diff


@pytest.mark.parametrize("name", ["large", "small"])
def test_kernels_reproduce_pillow(name):
    z = load_golden("g22_input_pipeline")
    src, S = z["src_" + name], int(z["rec_%s_size" % name][0])
    orders = z["rec_%s_order" % name]
    plain = [i for i in range(len(orders)) if (orders[i] == M.HUE).all()]
    jit = [i for i in range(len(orders)) if i not in plain]
    assert plain and jit
    sel = plain + jit                                               # the plain batch and the augmented batch of ONE launch
    crop = z["rec_%s_crop" % name]
    rec = make_records([(int(z["rec_%s_flip" % name][i]), [int(o) for o in orders[i]], z["rec_%s_factors" % name][i],
                         int(crop[i][0]), int(crop[i][1]), int(crop[i][2])) for i in sel])
    idx = z["rec_%s_source" % name][sel]
    out_plain, out_jit = abi_transform(src, idx, rec, len(plain), S, side_lo=S)
    want = torch.stack([torch.from_numpy(M.to_float(z["out_" + name][i])) for i in sel])
    want_direct = (torch.from_numpy(z["out_" + name][sel]).permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5
    assert torch.equal(want, want_direct)
    got = torch.cat([out_plain, out_jit])
    for k, i in enumerate(sel):
        report("%s record %d" % (name, i), got[k], want[k])
    assert torch.equal(got, want)


def big_sources():
    H, W = 314, 256
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = np.stack([127.5 + 127.0 * np.sin(0.05 * (c + 1) * xx + c) * np.cos(0.031 * (3 - c) * yy) + 15 * np.sin(0.8 * xx + yy)
                       for c in range(3)], axis=2)
    return np.stack([np.clip(np.rint(smooth), 0, 255).astype(np.uint8), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8),
                     rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)])


def test_band_path_matches_the_model_at_128():
    """S = 128 from 314 x 256: a crop of up to 256 x 256 pixels does not fit LDS, blocks work on bands of output rows.
    The LAST image of the store is used too: its final 16-byte group is where the store ends."""
    src, S = big_sources(), 128
    rows = [(0, [3, 3, 3, 3], (1, 1, 1), 0, 0, 256), (0, [3, 3, 3, 3], (1, 1, 1), 58, 0, 256), (0, [3, 3, 3, 3], (1, 1, 1), 186, 128, 128),
            (1, [1, 0, 2, 3], (1.2, 0.8, 1.2), 58, 0, 256), (0, [0, 2, 3, 1], (0.8, 1.2, 0.8), 0, 0, 128),
            (1, [2, 3, 1, 0], (1.1, 1.15, 0.85), 71, 13, 243), (0, [3, 0, 1, 2], (1.2, 1.2, 1.2), 93, 35, 221),
            (1, [2, 1, 0, 3], (0.93, 1.07, 1.2), 100, 50, 201)]
    idx = np.array([0, 2, 1, 2, 1, 0, 2, 1], dtype=np.int32)
    out_plain, out_jit = abi_transform(src, idx, make_records(rows), 3, S, side_lo=128)
    got = torch.cat([out_plain, out_jit])
    bad = 0
    for k, (flip, order, f, top, left, side) in enumerate(rows):
        want = torch.from_numpy(M.to_float(M.transform_u8(src[idx[k]], S, flip, order, f, top, left, side)))
        bad += report("314 x 256 record %d" % k, got[k], want)
    assert bad == 0


def test_bad_arguments_are_refused_by_the_library():
    from locate_amd._lib import LocateError
    src = big_sources()[:1]
    rec = make_records([(0, [3, 3, 3, 3], (1, 1, 1), 0, 0, 256)])
    with pytest.raises(LocateError):
        abi_transform(src, np.array([0], dtype=np.int32), rec, 1, 126, side_lo=128)          # S not a multiple of 4


def small_store(n=40, seed=9):
    from locate_amd import DeviceImageStore
    rng = np.random.default_rng(seed)
    return DeviceImageStore(rng.integers(0, 256, size=(n, 78, 64, 3), dtype=np.uint8), DEV)


def test_pipeline_matches_the_model_and_writes_in_place():
    from locate_amd import InputPipeline
    store, S, B = small_store(), 32, 8
    pipe = InputPipeline(store, S, B, seed=3)
    twin = InputPipeline(store, S, B, seed=3)
    idx, params = twin._draw()                                       # the host draws the first batch pair would use
    real, aug = pipe.next_batch()
    torch.cuda.synchronize()
    src = store.data.cpu().numpy()
    for k in range(2 * B):
        r = params[k]
        order = [(int(r["order"]) >> (4 * j)) & 15 for j in range(4)]
        want = M.to_float(M.transform_u8(src[idx[k]], S, int(r["flip"]), order, (r["brightness"], r["contrast"], r["saturation"]),
                                         int(r["top"]), int(r["left"]), int(r["side"])))
        got = (real[k] if k < B else aug[k - B]).cpu()
        assert torch.equal(got, torch.from_numpy(want)), k
    # same seed, outputs passed in: written in place, equal to the returned form
    again = InputPipeline(store, S, B, seed=3)
    out_real, out_aug = torch.zeros_like(real), torch.zeros_like(aug)
    r2, a2 = again.next_batch(out_real=out_real, out_aug=out_aug)
    assert r2 is out_real and a2 is out_aug
    assert torch.equal(out_real, real) and torch.equal(out_aug, aug)
    # and the sequence goes on identically, across an epoch boundary (5 batches per epoch)
    for _ in range(7):
        p, q = pipe.next_batch(), again.next_batch()
        assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])
    assert not torch.equal(p[0], real)


def test_side_stream_equals_default_stream():
    from locate_amd import InputPipeline
    store, S, B = small_store(), 32, 8
    a = InputPipeline(store, S, B, seed=21)
    want = [tuple(t.clone() for t in a.next_batch()) for _ in range(3)]
    b = InputPipeline(store, S, B, seed=21)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [tuple(t.clone() for t in b.next_batch()) for _ in range(3)]
    side.synchronize()
    torch.cuda.synchronize()
    for (r, g), (r2, g2) in zip(want, got):
        assert torch.equal(r, r2) and torch.equal(g, g2)


def test_overfit_repeats_on_the_device():
    from locate_amd import InputPipeline
    pipe = InputPipeline(small_store(), 32, 8, seed=2, overfit=True)
    first = [t.clone() for t in pipe.next_batch()]
    for _ in range(2):
        r, a = pipe.next_batch()
        assert torch.equal(r, first[0]) and torch.equal(a, first[1])


def test_store_from_a_file(tmp_path):
    from locate_amd import DeviceImageStore
    arr = np.random.default_rng(1).integers(0, 256, size=(11, 78, 64, 3), dtype=np.uint8)
    path = str(tmp_path / "store.npy")
    np.save(path, arr)
    store = DeviceImageStore(path, DEV, chunk_bytes=3 * 78 * 64 * 3)          # four chunks
    assert (store.N, store.H, store.W) == (11, 78, 64) and np.array_equal(store.data.cpu().numpy(), arr)
    with pytest.raises(ValueError):
        DeviceImageStore(arr.astype(np.float32), DEV)


def test_train_loop_iteration_fed_by_the_pipeline():
    from locate_amd import Discriminator, Generator, InputPipeline, Nadam, NetConfig, TrainLoop, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    torch.manual_seed(cfg.seed)
    G, D = Generator(cfg).to(DEV), Discriminator(cfg).to(DEV)
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)))
    loop = TrainLoop(step)
    latent = torch.randn(z["step1/latent"].shape).to(DEV)
    pipe = InputPipeline(small_store(), 32, latent.shape[0], seed=0)
    for _ in range(2):
        real, aug = pipe.next_batch()
        assert float(real.min()) >= -1 and float(real.max()) <= 1
        out = loop.iteration(latent, real, aug)
        torch.cuda.synchronize()
        for k in ("d_error", "g_error"):
            assert k in out and torch.isfinite(out[k].detach().float()).all(), (k, out[k])
