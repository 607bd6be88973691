"""Times one `SlicedWasserstein.set_reference` + `evaluate` at 64 x 64, N = 4096 (locate_amd/metric.py, csrc/swd.hip) with HIP
events, split by stage - generator passes, pyramid, statistics, projection, sort, distance - and prints the projection kernel's
TFLOP/s against the 157 TF fp32-MFMA peak, the stencils' TB/s of algorithmic traffic, and, with --train-iters K, the share
of an epoch of the reference's schedule that one evaluation per epoch costs (the training step is timed in the same call).
One JSON line at the end.  Usage (GPU box): python tools/bench_swd.py [--tiny] [--images 4096] [--reps 3] [--train-iters 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import (Discriminator, Generator, NetConfig, SlicedWasserstein, TrainStep, descriptor_stats, get_model,  # noqa: E402
                        laplacian_pyramid, project_descriptors, sorted_distance)
from locate_amd import metric  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402

MFMA_PEAK = 157.3e12


def timed(fn, reps, warmup=1):
    """seconds per call: warm-up, then `reps` calls between two HIP events"""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 generator instead of the full one")
    ap.add_argument("--train-iters", type=int, default=0, help="also time this many training iterations (batch 64) for the epoch share")
    ap.add_argument("--dataset", type=int, default=202599, help="images per pass of the data for the epoch share (CelebA)")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    S, N = args.image_size, args.images
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    gen.batched_spectral_norm = True
    swd = SlicedWasserstein(S, images=N, chunk=args.chunk, device=dev)
    P, R, Dr = swd.nhoods_per_image, swd.dir_repeats, swd.dirs_per_repeat
    n = N * P
    real = torch.randn(N, 3, S, S, device=dev).clamp(-1, 1)
    out = {"image_size": S, "images": N, "generator": "tiny" if args.tiny else "full", "levels": swd.sizes, "descriptors": n}

    # ---- the whole calls ----
    out["set_reference_ms"] = 1e3 * timed(lambda: swd.set_reference(real), args.reps)
    out["evaluate_ms"] = 1e3 * timed(lambda: swd.evaluate(gen), args.reps)

    # ---- by stage: the same launches, one stage at a time over pre-built inputs ----
    latents = swd.latents(gen.g_in)

    def generate():
        gen.eval()
        with torch.no_grad():
            for at in range(0, N, args.chunk):
                gen(latents[at:at + args.chunk])
        gen.train()
    out["generator_ms"] = 1e3 * timed(generate, args.reps)

    def pyramid():
        for at in range(0, N, args.chunk):
            laplacian_pyramid(real[at:at + args.chunk], len(swd.sizes))
    out["pyramid_ms"] = 1e3 * timed(pyramid, args.reps)
    levels = swd._levels(real)
    tables = swd._device_tables()
    stats = [descriptor_stats(lv, tables["candidate"][l], P) for l, lv in enumerate(levels)]
    out["stats_ms"] = 1e3 * timed(lambda: [descriptor_stats(lv, tables["candidate"][l], P) for l, lv in enumerate(levels)], args.reps)

    def project(l):
        return [project_descriptors(levels[l], tables["candidate"][l], P, d, stats[l]) for d in tables["dirs"]]
    per_level = [timed(lambda l=l: project(l), args.reps) for l in range(len(levels))]
    out["projection_ms"] = 1e3 * sum(per_level)
    flop = 2.0 * n * Dr * R * metric.K
    out["projection_tflops_per_level"] = [flop / t / 1e12 for t in per_level]
    out["projection_of_mfma_peak"] = [flop / t / MFMA_PEAK for t in per_level]
    proj = project(0)[0]
    t_sort = timed(lambda: torch.sort(proj, dim=1), args.reps)
    out["sort_ms"] = 1e3 * t_sort * R * len(levels)
    out["sort_gkeys_per_s"] = proj.numel() / t_sort / 1e9
    a, b = torch.sort(proj, dim=1).values, torch.sort(project(0)[1], dim=1).values
    t_dist = timed(lambda: sorted_distance(a, b), args.reps)
    out["distance_ms"] = 1e3 * t_dist * R * len(levels)
    out["distance_tb_per_s"] = 2 * 4 * a.numel() / t_dist / 1e12
    del a, b, proj

    # ---- the stencils alone on the whole set (805 MB of level-0 traffic at the defaults: HBM, not the 256 MB Infinity Cache) ----
    coarse = metric.pyr_down(real)
    t_down = timed(lambda: metric.pyr_down(real), args.reps)
    res = torch.empty_like(real)
    t_res = timed(lambda: metric.pyr_residual(real, coarse, out=res), args.reps)
    out["pyr_down_tb_per_s"] = 4 * (real.numel() + coarse.numel()) / t_down / 1e12
    out["pyr_residual_tb_per_s"] = 4 * (2 * real.numel() + coarse.numel()) / t_res / 1e12
    out["pyr_down_ms"], out["pyr_residual_ms"] = 1e3 * t_down, 1e3 * t_res
    del coarse, res, levels

    # ---- the share of an epoch: the reference's schedule has (e + 1)^2 passes over the data in epoch e ----
    if args.train_iters > 0:
        B = 64
        dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
        dis.batched_spectral_norm = True
        step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)
        lat, x, y = torch.randn(B, gen.g_in, device=dev), real[:B].clone(), real[B:2 * B].clone()
        from locate_amd.graph import GraphedTrainStep
        runner = GraphedTrainStep(step, lat, x, y, warmup=2)          # replayed as hipGraphs, as bench.py measures the step
        t_step = timed(runner.replay, args.train_iters, warmup=3)
        out["train_iteration_ms"] = 1e3 * t_step
        for e in (0, 1, 2):
            epoch = (e + 1) ** 2 * (args.dataset // B) * t_step
            out["share_of_epoch_%d" % (e + 1)] = out["evaluate_ms"] * 1e-3 / (epoch + out["evaluate_ms"] * 1e-3)
    for k in sorted(out):
        print("%-32s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
