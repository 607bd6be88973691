"""Times the differentiable augmentation (locate_amd/augment.py, csrc/diffaug.hip) in one session, every call behind a fill of 512 MiB
that empties L2 and the 256 MiB Infinity Cache:
  * forward and backward at 192 x 3 x 64 x 64 (the D-step's stacked batch at the benchmark's size: one launch, the image in LDS) and
    at 48 x 3 x 256 x 256 (two launches through the workspace), full policy;
  * a plain device-to-device copy of the same bytes - the kernels read and write the batch once, so the copy is the floor - and the
    ratio to it;
  * the ATen yardstick: the paper's sequence restated with ATen calls (brightness, saturation, contrast, a padded gather, a mask),
    forward alone and forward + autograd backward;
  * one replayed training iteration (hipGraphs, the benchmark's networks at 64 x 64, batch 64) with the full policy, draw() included,
    against the same step without an augment - which launches exactly what it launched before the augmentation existed.
HIP events around single calls, `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it
their range.  One JSON line at the end.
Usage (GPU box): python tools/bench_diffaug.py [--rounds 9] [--steps 30]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from locate_amd import DiffAugment, diff_augment, diff_augment_backward, draw_parameters  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402

FULL = "color,translation,cutout"


def timed(fn, flush):
    """seconds of one call, behind a cache-clearing fill"""
    flush.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def aten_forward(x, p, D):
    """the yardstick: the paper's three colour steps, the shift as a gather from a zero-padded copy, the cut as a multiplication"""
    n, _, S, _ = x.shape
    b, s, c = (p[:, k].view(n, 1, 1, 1) for k in range(3))
    x = x + b
    mu = x.mean(dim=1, keepdim=True)
    x = (x - mu) * s + mu
    M = x.mean(dim=(1, 2, 3), keepdim=True)
    x = (x - M) * c + M
    ar = torch.arange(S, device=x.device)
    ty, tx = p[:, 3].long().view(n, 1, 1), p[:, 4].long().view(n, 1, 1)
    rows = (ar.view(1, S, 1) - ty + D).expand(n, S, S)
    cols = (ar.view(1, 1, S) - tx + D).expand(n, S, S)
    padded = F.pad(x, (D, D, D, D))
    w = padded[torch.arange(n, device=x.device).view(n, 1, 1), :, rows, cols].permute(0, 3, 1, 2)
    inside = ((ar.view(1, S, 1) >= p[:, 5].view(n, 1, 1)) & (ar.view(1, S, 1) < p[:, 6].view(n, 1, 1))
              & (ar.view(1, 1, S) >= p[:, 7].view(n, 1, 1)) & (ar.view(1, 1, S) < p[:, 8].view(n, 1, 1)))
    return w * (1.0 - inside.float()).unsqueeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=30, help="replayed iterations per timed window of the step comparison")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings = {}, {}
    shapes = ((192, 64), (48, 256))
    for n, S in shapes:
        gen = torch.Generator(device=dev).manual_seed(S)
        x = torch.rand(n, 3, S, S, device=dev, generator=gen) * 2.0 - 1.0
        g = torch.rand(n, 3, S, S, device=dev, generator=gen) * 2.0 - 1.0
        p = torch.from_numpy(draw_parameters(n, S, torch.Generator().manual_seed(S), FULL)).to(dev)
        dst = torch.empty_like(x)
        tag = "%dx3x%dx%d" % (n, S, S)
        D = S // 8
        settings["fwd_" + tag] = lambda x=x, p=p: diff_augment(x, p, FULL)
        settings["bwd_" + tag] = lambda g=g, p=p: diff_augment_backward(g, p, FULL)
        settings["copy_" + tag] = lambda x=x, dst=dst: dst.copy_(x)
        settings["aten_fwd_" + tag] = lambda x=x, p=p, D=D: aten_forward(x, p, D)

        def aten_both(x=x, g=g, p=p, D=D):
            leaf = x.detach().requires_grad_()
            aten_forward(leaf, p, D).backward(g)
            return leaf.grad
        settings["aten_fwd_bwd_" + tag] = aten_both
        out["aten_minus_kernel_max_fwd_" + tag] = float((aten_forward(x, p, D) - diff_augment(x, p, FULL)).abs().max())
        out["aten_minus_kernel_max_bwd_" + tag] = float((aten_both() - diff_augment_backward(g, p, FULL)).abs().max())
        out["bytes_" + tag] = 2 * x.numel() * 4
    for fn in settings.values():          # every shape once before anything is timed
        fn()
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, flush))
    for name, values in rounds.items():
        out[name + "_us"] = 1e6 * statistics.median(values)
        out[name + "_us_range"] = [1e6 * min(values), 1e6 * max(values)]
    for n, S in shapes:
        tag = "%dx3x%dx%d" % (n, S, S)
        for d in ("fwd", "bwd"):
            out["%s_over_copy_%s" % (d, tag)] = out["%s_%s_us" % (d, tag)] / out["copy_%s_us" % tag]
            out["%s_tb_per_s_%s" % (d, tag)] = out["bytes_" + tag] / (out["%s_%s_us" % (d, tag)] * 1e-6) / 1e12
        out["copy_tb_per_s_" + tag] = out["bytes_" + tag] / (out["copy_%s_us" % tag] * 1e-6) / 1e12
        out["aten_fwd_over_kernel_" + tag] = out["aten_fwd_%s_us" % tag] / out["fwd_%s_us" % tag]
        out["aten_fwd_bwd_over_kernels_" + tag] = out["aten_fwd_bwd_%s_us" % tag] / (out["fwd_%s_us" % tag] + out["bwd_%s_us" % tag])

    if not args.no_step:
        # one replayed iteration at the benchmark's size, with and without the augmentation, windows alternating
        from locate_amd import Discriminator, Generator, NetConfig, TrainStep, get_model
        from locate_amd.graph import GraphedTrainStep
        S, B = 64, 64
        runners = {}
        for name in ("plain", "augmented"):
            cfg = NetConfig(image_size=S)
            torch.manual_seed(cfg.seed)
            G, GO = get_model(Generator(cfg), cfg.glr, dev)
            Dn, DO = get_model(Discriminator(cfg), cfg.dlr, dev)
            G.batched_spectral_norm = Dn.batched_spectral_norm = True
            aug = DiffAugment(S=S, batch=B, policy=FULL, seed=1, device=dev) if name == "augmented" else None
            step = TrainStep(G, Dn, GO, DO, augment=aug)
            gen = torch.Generator(device="cpu").manual_seed(1234)
            latent = torch.randn(B, S, generator=gen).to(dev)
            real = torch.randn(B, 3, S, S, generator=gen).clamp(-1, 1).to(dev)
            fake = torch.randn(B, 3, S, S, generator=gen).clamp(-1, 1).to(dev)
            if aug is not None:
                aug.draw()
            runners[name] = (GraphedTrainStep(step, latent, real, fake, warmup=2), aug)

        def window(name):
            runner, aug = runners[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if aug is not None:
                    aug.draw()
                runner.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps
        for name in runners:
            window(name)
        windows = {name: [] for name in runners}
        for _ in range(args.rounds):
            for name in runners:
                windows[name].append(window(name))
        for name, values in windows.items():
            out["step_%s_ms" % name] = 1e3 * statistics.median(values)
            out["step_%s_ms_range" % name] = [1e3 * min(values), 1e3 * max(values)]
        out["step_augmented_minus_plain_ms"] = out["step_augmented_ms"] - out["step_plain_ms"]
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
