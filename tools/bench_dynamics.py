"""Times `RunDynamics` (locate_amd/dynamics.py, csrc/dynamics.hip) on the benchmark networks (64 x 64, full width, batch 64) with HIP
events around every single call: `mark()` (the REBASE pass), the delta part of `record()` (the RECORD pass, and both in one pass),
the sigma part (the u / v copy, `power_iterations` + `sigma_rounds` batched power iterations, the copy of the sigmas) and the
whole `record()` - each directly behind a replayed training iteration, what a run sees, and back to back, where the operands sit
in the Infinity Cache.  Prints the bytes each moves and the TB/s.  Yardsticks in the same process, alternating with the kernels:
the statistics' two launches over the same weights (`RunStatistics`' table without the gradients), and ATen's
`_foreach_sub` + `_foreach_norm` + `_foreach_copy_` on the same lists.  The training step (replayed as hipGraphs, as bench.py
measures it) is timed alone and with mark() / record() around every iteration and around every 16th, for the share of the step.
One JSON line at the end.
Usage (GPU box): python tools/bench_dynamics.py [--reps 30] [--rounds 5] [--train-iters 32] [--sigma-rounds 4] [--step-ms MS]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import Discriminator, Generator, NetConfig, RunDynamics, TrainStep, get_model  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=30, help="timed calls per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=5, help="kernel / yardstick rounds, alternating")
    ap.add_argument("--train-iters", type=int, default=32, help="training iterations per timed loop (a multiple of 16)")
    ap.add_argument("--sigma-rounds", type=int, default=4)
    ap.add_argument("--step-ms", type=float, default=0.0, help="the step time bench.py reported, for the share (else this call's)")
    args = ap.parse_args()
    if args.reps < 20 or args.rounds < 2 or args.train_iters < 16 or args.train_iters % 16 or args.sigma_rounds < 1:
        ap.error("--reps >= 20, --rounds >= 2, --sigma-rounds >= 1 and --train-iters a positive multiple of 16")
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
    runner = GraphedTrainStep(step, lat, x, y, warmup=2)
    runner.replay()

    dyn = RunDynamics(gen, dis, capacity=4096, sigma_rounds=args.sigma_rounds)
    dyn.mark()
    runner.replay()
    dyn.record(0)
    (row,) = dyn.flush()
    ratios = dyn.ratios()[0]
    weights = [p.detach() for _, p in dyn._parameters()]
    elements = sum(t.numel() for t in weights)
    geometry = [(int(m.module.weight_bar.shape[0]), int(m.module.weight_bar.numel() // m.module.weight_bar.shape[0])) for _, m in dyn._sn_layers()]
    sn_elements = sum(h * wd for h, wd in geometry)
    rounds_per_record = dyn._sn["rounds"] + args.sigma_rounds
    out = {"image_size": S, "networks": "tiny" if args.tiny else "full", "entries": len(weights), "chunks": dyn._tab[3], "layers": len(geometry),
           "elements": elements, "weight_bytes": 4 * elements, "spectral_norm_weight_bytes": 4 * sn_elements, "sigma_rounds": args.sigma_rounds,
           "power_iteration_rounds_per_record": rounds_per_record, "reps": args.reps, "rounds": args.rounds,
           "first_record": {"G/update": ratios["G/update"], "D/update": ratios["D/update"], "lipschitz_min": float(ratios["lipschitz"].min()),
                            "lipschitz_median": float(statistics.median(ratios["lipschitz"].tolist())), "lipschitz_max": float(ratios["lipschitz"].max()),
                            "nonfinite": int(row["nonfinite"].sum())}}
    # bytes each part moves: mode 1 reads weights and base, mode 2 reads the weights and writes the base, mode 3 reads both and writes
    # one; a power-iteration round reads every spectral-norm weight twice (column sums, row dots)
    moved = {"mark": 8 * elements, "delta": 8 * elements, "delta_rebase": 12 * elements, "sigma": 8 * sn_elements * rounds_per_record,
             "stats_weights": 4 * elements, "aten": 24 * elements}
    moved["record"] = moved["delta"] + moved["sigma"]
    tick = [0]

    def record():
        tick[0] += 1
        dyn.record(tick[0])

    from locate_amd.dynamics import REBASE, RECORD, _launch
    table, scratch_row = dyn._tab, dyn._ring[dyn.capacity - 1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        record()
    out["record_host_us"] = 1e6 * (time.perf_counter() - t0) / 50
    torch.cuda.synchronize()
    dyn.flush()
    dyn.clear()

    # the statistics' kernel over the same weights (no gradients): the bandwidth yardstick of this session
    from locate_amd.stats import _device_table as stats_table, _launch as stats_launch
    s_table = stats_table(weights)
    s_row = torch.zeros(1 + len(weights), 2, dtype=torch.int64, device=dev)
    bases = [b.view_as(t) for b, t in zip(dyn._slots, weights)]
    deltas = [torch.empty_like(t) for t in weights]

    @torch.no_grad()
    def aten():          # the same three things through ATen: d = w - base, |d| per tensor, base <- w
        torch._foreach_copy_(deltas, weights)
        torch._foreach_sub_(deltas, bases)
        norms = torch._foreach_norm(deltas, 2)
        torch._foreach_copy_(bases, weights)
        return norms
    try:
        aten()
        out["aten"] = "_foreach_copy_ + _foreach_sub_ + _foreach_norm(2) + _foreach_copy_"
    except Exception as err:          # an ATen without one of the multi-tensor forms
        out["aten"] = "unavailable: %s" % err
        aten = None

    parts = {"mark": dyn.mark, "delta": lambda: _launch(table, RECORD, scratch_row), "delta_rebase": lambda: _launch(table, RECORD | REBASE, scratch_row),
             "sigma": lambda: dyn._sigmas(scratch_row), "record": record, "stats_weights": lambda: stats_launch(s_table, s_row)}
    if aten is not None:
        parts["aten"] = aten
    med = statistics.median
    rounds = {"%s_%s" % (k, where): [] for k in parts for where in ("behind_iteration", "hot")}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits all alike
        for k, fn in parts.items():
            rounds[k + "_behind_iteration"].append(med(each_launch_ms(fn, args.reps, between=runner.replay)))
        for k, fn in parts.items():
            rounds[k + "_hot"].append(med(each_launch_ms(fn, args.reps)))
        dyn.flush()          # outside every timed region: the ring never fills inside one
        dyn.clear()
    for k, v in rounds.items():
        out[k + "_us_rounds"] = [1e3 * t for t in v]
        out[k + "_us"] = 1e3 * med(v)
        out[k + "_tb_per_s"] = moved[k.rsplit("_behind_iteration", 1)[0].rsplit("_hot", 1)[0]] / (med(v) * 1e-3) / 1e12
    out["bytes_moved"] = moved
    out["sigma_us_per_round_behind_iteration"] = out["sigma_behind_iteration_us"] / rounds_per_record
    out["delta_over_stats_bandwidth_behind_iteration"] = out["delta_behind_iteration_tb_per_s"] / out["stats_weights_behind_iteration_tb_per_s"]

    def every(k):
        count = [0]

        def fn():
            count[0] += 1
            if count[0] % k == 0:
                dyn.mark()
            runner.replay()
            if count[0] % k == 0:
                record()
        return fn
    plain, each, sixteenth = [], [], []
    for _ in range(3):
        plain.append(loop_ms(runner.replay, args.train_iters))
        each.append(loop_ms(every(1), args.train_iters))
        sixteenth.append(loop_ms(every(16), args.train_iters, warmup=0))
        dyn.flush()
        dyn.clear()
    out["train_iteration_ms_rounds"], out["train_iteration_ms"] = plain, med(plain)
    out["train_iteration_dynamics_every_1_ms_rounds"], out["train_iteration_dynamics_every_1_ms"] = each, med(each)
    out["train_iteration_dynamics_every_16_ms_rounds"], out["train_iteration_dynamics_every_16_ms"] = sixteenth, med(sixteenth)
    step_ms = args.step_ms if args.step_ms > 0 else med(plain)
    out["step_ms_for_share"] = step_ms
    cost_us = out["mark_behind_iteration_us"] + out["record_behind_iteration_us"]
    out["mark_plus_record_us"] = cost_us
    out["share_of_step_every_1"] = cost_us * 1e-3 / step_ms
    out["share_of_step_every_16"] = cost_us * 1e-3 / 16 / step_ms
    for k in sorted(out):
        print("%-52s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
