"""Times `RunStatistics.record()` (locate_amd/stats.py, csrc/stats.hip) on the benchmark networks (64 x 64, full width, batch 64)
with HIP events around every single record: directly behind a replayed training iteration - what a run sees: the weights and
gradients come from HBM, the iteration's 1.5 GB of other traffic lie in between - with a cache-evicting fill of --evict-mib
(default 1280) between two records, and back to back, where the operands sit in the 256 MiB Infinity Cache.  Prints the bytes read
(4 per element), the GB/s, and the same statistics through ATen on the same tensor list as the comparison: two
`torch._foreach_norm` launches (ord 2 and inf: the norm and the largest magnitude; they do not leave non-finite elements out)
plus a count of `~isfinite` per tensor, and the two multi-tensor launches alone; `--rounds` times alternating with the kernel.
The training step (replayed as hipGraphs, as bench.py measures it) is timed in the same call, alone and with a record after
every iteration and after every 16th, for the record's share of it.  One JSON line at the end.
Usage (GPU box): python tools/bench_stats.py [--reps 30] [--rounds 5] [--train-iters 32] [--step-ms MS]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import Discriminator, Generator, NetConfig, RunStatistics, TrainStep, get_model  # noqa: E402
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
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 networks (a rehearsal: measures overheads only)")
    ap.add_argument("--reps", type=int, default=30, help="timed records per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=5, help="kernel / comparison rounds, alternating")
    ap.add_argument("--evict-mib", type=int, default=1280, help="size of the fill between two records (at least 1024)")
    ap.add_argument("--train-iters", type=int, default=32, help="training iterations per timed loop (a multiple of 16)")
    ap.add_argument("--step-ms", type=float, default=0.0, help="the step time bench.py reported, for the share (else this call's)")
    args = ap.parse_args()
    if args.reps < 20 or args.evict_mib < 1024 or args.rounds < 2 or args.train_iters < 16 or args.train_iters % 16:
        ap.error("--reps >= 20, --evict-mib >= 1024, --rounds >= 2 and --train-iters a positive multiple of 16")
    require_gpu()
    dev = torch.device("cuda:0")
    S, B = args.image_size, 64
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
    gen.batched_spectral_norm = dis.batched_spectral_norm = True
    step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)
    lat, x, y = (torch.randn(B, gen.g_in, device=dev), torch.randn(B, 3, S, S, device=dev).clamp(-1, 1),
                 torch.randn(B, 3, S, S, device=dev).clamp(-1, 1))
    from locate_amd.graph import GraphedTrainStep
    runner = GraphedTrainStep(step, lat, x, y, warmup=2)          # the gradients now sit in the graphs' fixed buffers
    runner.replay()

    stats = RunStatistics(gen, dis, capacity=4096)
    stats.record(0)
    (row,) = stats.flush()
    tensors = [t for _, t in stats._entries()]
    elements = sum(t.numel() for t in tensors)
    nbytes = 4 * elements
    out = {"image_size": S, "networks": "tiny" if args.tiny else "full", "entries": len(tensors), "chunks": stats._tab[3],
           "gradient_entries": sum(1 for n in row["names"] if n.endswith(".grad")), "elements": elements, "bytes_read": nbytes,
           "nonfinite_in_the_record": row["total"], "reps": args.reps, "rounds": args.rounds, "evict_mib": args.evict_mib}
    tick = [0]

    def record():
        tick[0] += 1
        stats.record(tick[0])

    # record() finds its table by reading ~2 addresses per parameter on the host first; behind an iteration the host runs ahead
    # of the device and the events see the two launches alone, but back to back they would see the host.  The kernel figures
    # therefore come from the launch itself, on the table record() cached, into a row of the ring.
    from locate_amd.stats import _launch
    table, scratch_row = stats._tab, stats._ring[stats.capacity - 1]

    def kernel():
        _launch(table, scratch_row)
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        record()
    out["record_host_us"] = 1e6 * (time.perf_counter() - t0) / 50
    torch.cuda.synchronize()
    stats.flush()
    stats.clear()

    try:
        torch._foreach_norm(tensors[:2], float("inf"))
        largest = lambda: torch._foreach_norm(tensors, float("inf"))          # noqa: E731
        out["aten_largest_magnitude"] = "_foreach_norm(inf)"
    except Exception:          # an ATen without the multi-tensor form: one launch per tensor
        largest = lambda: [t.abs().amax() for t in tensors]          # noqa: E731
        out["aten_largest_magnitude"] = "abs().amax() per tensor"

    @torch.no_grad()
    def aten_norms():
        return torch._foreach_norm(tensors, 2), largest()

    @torch.no_grad()
    def aten():
        return aten_norms(), [torch.isfinite(t).logical_not_().sum() for t in tensors]

    junk = torch.empty(args.evict_mib << 18, dtype=torch.float32, device=dev)
    fills = [0]

    def evict():
        fills[0] += 1
        junk.fill_(float(fills[0]))

    med = statistics.median
    names = ("record_behind_iteration", "kernel_behind_iteration", "kernel_evicted", "kernel_hot", "aten_behind_iteration", "aten_evicted", "aten_hot",
             "aten_norms_only_evicted", "aten_norms_only_hot")
    rounds = {k: [] for k in names}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits both alike
        rounds["record_behind_iteration"].append(med(each_launch_ms(record, args.reps, between=runner.replay)))
        rounds["kernel_behind_iteration"].append(med(each_launch_ms(kernel, args.reps, between=runner.replay)))
        rounds["aten_behind_iteration"].append(med(each_launch_ms(aten, args.reps, between=runner.replay)))
        rounds["kernel_evicted"].append(med(each_launch_ms(kernel, args.reps, between=evict)))
        rounds["aten_evicted"].append(med(each_launch_ms(aten, args.reps, between=evict)))
        rounds["aten_norms_only_evicted"].append(med(each_launch_ms(aten_norms, args.reps, between=evict)))
        rounds["kernel_hot"].append(med(each_launch_ms(kernel, args.reps)))
        rounds["aten_hot"].append(med(each_launch_ms(aten, args.reps)))
        rounds["aten_norms_only_hot"].append(med(each_launch_ms(aten_norms, args.reps)))
        stats.flush()          # outside every timed region: the ring never fills inside one
        stats.clear()
    for k, v in rounds.items():
        out[k + "_us_rounds"] = [1e3 * t for t in v]
        out[k + "_us"] = 1e3 * med(v)
        out[k + "_gb_per_s"] = nbytes / (med(v) * 1e-3) / 1e9

    def every(k):
        count = [0]

        def fn():
            runner.replay()
            count[0] += 1
            if count[0] % k == 0:
                record()
        return fn
    plain, each, sixteenth = [], [], []
    for _ in range(3):
        plain.append(loop_ms(runner.replay, args.train_iters))
        each.append(loop_ms(every(1), args.train_iters))
        sixteenth.append(loop_ms(every(16), args.train_iters, warmup=0))
        stats.flush()
        stats.clear()
    out["train_iteration_ms_rounds"], out["train_iteration_ms"] = plain, med(plain)
    out["train_iteration_record_every_1_ms_rounds"], out["train_iteration_record_every_1_ms"] = each, med(each)
    out["train_iteration_record_every_16_ms_rounds"], out["train_iteration_record_every_16_ms"] = sixteenth, med(sixteenth)
    step_ms = args.step_ms if args.step_ms > 0 else med(plain)
    out["step_ms_for_share"] = step_ms
    out["share_of_step_every_1"] = out["record_behind_iteration_us"] * 1e-3 / step_ms
    out["share_of_step_every_16"] = out["record_behind_iteration_us"] * 1e-3 / 16 / step_ms
    for k in sorted(out):
        print("%-44s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
