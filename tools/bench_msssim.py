"""Times the multi-scale SSIM (locate_amd/msssim.py, csrc/msssim.hip) in one session: `ms_ssim_levels` for 4096 pairs at 64 x 64 (one
launch) and 256 pairs at 256 x 256 (two tiled launches and the launch for side 64), each call behind a fill of 512 MiB that empties
L2 and the 256 MiB Infinity Cache, against the ATen yardstick on the same bytes - float64 depthwise `F.conv2d` with the 2-D window,
`avg_pool2d`, the same formulas - and the largest difference between the two results.  Per shape: ms, and the achieved float64
FLOP/s from the fma count the separable definition needs (5 moments, n taps, rows and columns) as a share of the 78.6 TFLOP/s
float64 vector peak; these are shares of a CALL's time, not of a kernel's.  Then a whole `MultiScaleSSIM.evaluate` of a generator
at 64 x 64 (wall clock, synchronised) beside the same forwards alone: the generator's share.  HIP events around single calls;
`rounds` rounds with all settings alternating; a figure is the median of the round values, beside it their range.  One JSON line at
the end.
Usage (GPU box): python tools/bench_msssim.py [--rounds 7] [--small 4096] [--large 256] [--eval-pairs 512]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from locate_amd import MultiScaleSSIM, encode_images, ms_ssim_levels, window_taps  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
C1, C2 = (0.01 * 255.0) * (0.01 * 255.0), (0.03 * 255.0) * (0.03 * 255.0)


def timed(fn, flush):
    """seconds of one call, behind a cache-clearing fill"""
    flush.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def aten_levels(a, b, taps):
    """the yardstick: int8 codes [P, 3 S^2] -> float64 [P, 2, 5] with depthwise conv2d and avg_pool2d in float64"""
    P = a.shape[0]
    S = int(round((a.shape[1] // 3) ** 0.5))
    x = a.view(P, 3, S, S).double() + 128.0
    y = b.view(P, 3, S, S).double() + 128.0
    out = torch.empty(P, 2, 5, dtype=torch.float64, device=a.device)
    for l in range(5):
        n = min(11, S >> l)
        g = taps[l, :n]
        w = (g[:, None] * g[None, :]).expand(3, 1, n, n).contiguous()
        f = lambda p: F.conv2d(p, w, groups=3)          # noqa: E731
        mx, my, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
        v1, v2 = 2.0 * sxy + C2, sxx + syy + C2
        out[:, 1, l] = (v1 / v2).mean(dim=(1, 2, 3))
        out[:, 0, l] = (((2.0 * mx * my + C1) * v1) / ((mx * mx + my * my + C1) * v2)).mean(dim=(1, 2, 3))
        if l < 4:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return out


def fma_count(S):
    """float64 fma per pair: per level and channel 5 n (s o + o o) in the two passes (s the side, o the outputs per side)"""
    total = 0
    for l in range(5):
        s = S >> l
        n = min(11, s)
        o = s - n + 1
        total += 3 * 5 * n * (s * o + o * o)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small", type=int, default=4096, help="pairs at 64 x 64")
    ap.add_argument("--large", type=int, default=256, help="pairs at 256 x 256")
    ap.add_argument("--eval-pairs", type=int, default=512, help="pairs of the timed evaluate() at 64 x 64")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings = {}, {}
    for S, n in ((64, args.small), (256, args.large)):
        rng = torch.Generator(device=dev).manual_seed(S)
        smooth = F.avg_pool2d(torch.randn(2 * n, 3, S + 8, S + 8, device=dev, generator=rng), 9, stride=1)          # low-pass images
        smooth = torch.tanh(3.0 * smooth)
        ta, tb = encode_images(smooth[:n].contiguous()), encode_images(smooth[n:].contiguous())
        taps = torch.from_numpy(window_taps(S)).to(dev)
        tag = "%dx3x%dx%d" % (n, S, S)
        settings["msssim_" + tag] = lambda ta=ta, tb=tb: ms_ssim_levels(ta, tb)
        step = 256 if S == 64 else 16          # the yardstick's float64 intermediates, a slice at a time

        def aten(ta=ta, tb=tb, taps=taps, step=step, n=n):
            return torch.cat([aten_levels(ta[0][at:at + step], tb[0][at:at + step], taps) for at in range(0, n, step)])
        settings["aten_" + tag] = aten
        out["aten_minus_kernel_max_" + tag] = float((aten() - ms_ssim_levels(ta, tb)).abs().max())
    for fn in settings.values():          # every shape once before anything is timed
        fn()
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, flush))
    for name, values in rounds.items():
        out[name + "_ms"] = 1e3 * statistics.median(values)
        out[name + "_ms_range"] = [1e3 * min(values), 1e3 * max(values)]
    for S, n in ((64, args.small), (256, args.large)):
        tag = "%dx3x%dx%d" % (n, S, S)
        seconds = out["msssim_%s_ms" % tag] * 1e-3
        out["fp64_tflops_" + tag] = 2.0 * n * fma_count(S) / seconds / 1e12
        out["fp64_vector_share_" + tag] = 2.0 * n * fma_count(S) / seconds / FP64_VECTOR_PEAK
        out["aten_over_kernel_" + tag] = out["aten_%s_ms" % tag] / out["msssim_%s_ms" % tag]

    # a whole evaluate() of the flagship generator at 64 x 64, beside its forwards alone
    from locate_amd import Generator, NetConfig, get_model
    cfg = NetConfig(image_size=64)
    torch.manual_seed(cfg.seed)
    gen, _ = get_model(Generator(cfg), cfg.glr, dev, cfg)
    metric = MultiScaleSSIM(64, pairs=args.eval_pairs, chunk=64, device=dev)
    latents = metric.latents(gen.g_in)

    def forwards():
        gen.eval()
        with torch.no_grad():
            for at in range(0, latents.shape[0], 64):
                gen(latents[at:at + 64])
        gen.train()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    metric.evaluate(gen)
    forwards()
    whole = [wall(lambda: metric.evaluate(gen)) for _ in range(args.rounds)]
    alone = [wall(forwards) for _ in range(args.rounds)]
    out["evaluate_%d_pairs_64_ms" % args.eval_pairs] = 1e3 * statistics.median(whole)
    out["evaluate_%d_pairs_64_ms_range" % args.eval_pairs] = [1e3 * min(whole), 1e3 * max(whole)]
    out["generator_forwards_alone_ms"] = 1e3 * statistics.median(alone)
    out["generator_forwards_alone_ms_range"] = [1e3 * min(alone), 1e3 * max(alone)]
    out["generator_share_of_evaluate"] = statistics.median(alone) / statistics.median(whole)
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
