"""Times `AveragedGenerator.update()` (locate_amd/average.py, csrc/average.hip) on the benchmark generator (64 x 64, full width)
with HIP events around every single launch: back to back - both operands then sit in the 256 MiB Infinity Cache - and with a
cache-evicting fill of --evict-mib (default 1280) between two launches, which is what the training loop sees.  Prints the bytes
moved (12 per averaged element, 8 per copied one), the GB/s, and the same update through ATen on the same tensor lists
(`torch._foreach_lerp_` for the averaged tensors + `torch._foreach_copy_` for u / v) as the yardstick, `--rounds` times alternating
with the kernel so that the yardstick's own spread from round to round is known; with --train-iters K the training step (batch 64,
replayed as hipGraphs as bench.py measures it) is timed in the same call for the update's share of it.  One JSON line at the end.
Usage (GPU box): python tools/bench_average.py [--reps 30] [--rounds 5] [--train-iters 20] [--step-ms MS]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import AveragedGenerator, Discriminator, Generator, NetConfig, TrainStep, get_model  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402


def each_launch_ms(fn, reps, warmup=3, between=None):
    """milliseconds of every one of `reps` calls, each between two HIP events of its own; `between` runs outside the events"""
    for _ in range(warmup):
        if between is not None:
            between()
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        if between is not None:
            between()
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in pairs]


def loop_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 generator (a rehearsal: measures overheads only)")
    ap.add_argument("--reps", type=int, default=30, help="timed launches per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=5, help="kernel / yardstick rounds, alternating")
    ap.add_argument("--evict-mib", type=int, default=1280, help="size of the fill between two launches (at least 1024)")
    ap.add_argument("--train-iters", type=int, default=0, help="also time this many training iterations (batch 64)")
    ap.add_argument("--step-ms", type=float, default=0.0, help="the step time bench.py reported, for the share (else --train-iters)")
    args = ap.parse_args()
    if args.reps < 20 or args.evict_mib < 1024 or args.rounds < 2:
        ap.error("--reps >= 20, --evict-mib >= 1024 and --rounds >= 2")
    require_gpu()
    dev = torch.device("cuda:0")
    S = args.image_size
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    gen.batched_spectral_norm = True
    avg = AveragedGenerator(gen, half_life_images=10000, batch=64)
    with torch.no_grad():
        for p in gen.parameters():          # the live weights have moved away from the average, as in a run
            p.add_(1e-3 * torch.randn_like(p))
    w = avg.one_minus_beta
    averaged = [(a, s) for a, s, wt in avg._pairs if wt != 1.0]
    copied = [(a, s) for a, s, wt in avg._pairs if wt == 1.0]
    n_avg, n_copy = sum(a.numel() for a, _ in averaged), sum(a.numel() for a, _ in copied)
    nbytes = 12 * n_avg + 8 * n_copy
    out = {"image_size": S, "generator": "tiny" if args.tiny else "full", "tensors": len(avg._pairs), "chunks": avg._table()[3],
           "averaged_elements": n_avg, "copied_elements": n_copy, "bytes_moved": nbytes, "one_minus_beta": w, "reps": args.reps,
           "rounds": args.rounds, "evict_mib": args.evict_mib}

    lerp_dst, lerp_src = [a for a, _ in averaged], [s.detach() for _, s in averaged]
    copy_dst, copy_src = [a for a, _ in copied], [s.detach() for _, s in copied]

    @torch.no_grad()
    def aten():
        torch._foreach_lerp_(lerp_dst, lerp_src, w)
        if copy_dst:
            torch._foreach_copy_(copy_dst, copy_src)

    junk = torch.empty(args.evict_mib << 18, dtype=torch.float32, device=dev)
    tick = [0]

    def evict():
        tick[0] += 1
        junk.fill_(float(tick[0]))

    med = statistics.median
    rounds = {"kernel_hot": [], "aten_hot": [], "kernel_evicted": [], "aten_evicted": []}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits both alike
        rounds["kernel_evicted"].append(med(each_launch_ms(avg.update, args.reps, between=evict)))
        rounds["aten_evicted"].append(med(each_launch_ms(aten, args.reps, between=evict)))
        rounds["kernel_hot"].append(med(each_launch_ms(avg.update, args.reps)))
        rounds["aten_hot"].append(med(each_launch_ms(aten, args.reps)))
    for k, v in rounds.items():
        out[k + "_us_rounds"] = [1e3 * x for x in v]
        out[k + "_us"] = 1e3 * med(v)
        out[k + "_gb_per_s"] = nbytes / (med(v) * 1e-3) / 1e9
    out["aten_evicted_spread_us"] = 1e3 * (max(rounds["aten_evicted"]) - min(rounds["aten_evicted"]))
    out["kernel_evicted_spread_us"] = 1e3 * (max(rounds["kernel_evicted"]) - min(rounds["kernel_evicted"]))
    out["bar_met"] = bool(out["kernel_evicted_us"] <= out["aten_evicted_us"] + out["aten_evicted_spread_us"])

    step_ms = args.step_ms
    if args.train_iters > 0:
        B = 64
        dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
        dis.batched_spectral_norm = True
        step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)
        lat, x, y = (torch.randn(B, gen.g_in, device=dev), torch.randn(B, 3, S, S, device=dev).clamp(-1, 1),
                     torch.randn(B, 3, S, S, device=dev).clamp(-1, 1))
        from locate_amd.graph import GraphedTrainStep
        runner = GraphedTrainStep(step, lat, x, y, warmup=2)

        def both():
            runner.replay()
            avg.update()
        plain, followed = [], []
        for _ in range(3):
            plain.append(loop_ms(runner.replay, args.train_iters))
            followed.append(loop_ms(both, args.train_iters))
        out["train_iteration_ms_rounds"] = plain
        out["train_iteration_with_update_ms_rounds"] = followed
        out["train_iteration_ms"] = med(plain)
        out["train_iteration_with_update_ms"] = med(followed)
        if step_ms <= 0:
            step_ms = med(plain)
    if step_ms > 0:
        out["step_ms_for_share"] = step_ms
        out["share_of_step_evicted"] = out["kernel_evicted_us"] * 1e-3 / step_ms
        out["share_of_step_hot"] = out["kernel_hot_us"] * 1e-3 / step_ms
    for k in sorted(out):
        print("%-40s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
