"""Times `GuardedNadam.step()` (locate_amd/guard.py, csrc/guard.hip) against `Nadam.step()` on the benchmark networks' tensors
(64 x 64, full width, batch 64), both optimizers of the training step (discriminator, then generator) per measurement, with HIP
events around every single pair of steps: directly behind a replayed training iteration - what a run sees: parameters, moments and
gradients come from HBM, the iteration's other traffic lies in between - with a cache-evicting fill of --evict-mib (default 1280)
in between, and back to back, where the operands sit in the 256 MiB Infinity Cache.  The optimizers under test are extra ones
over the replayed step's parameters and gradient buffers, with moments of their own.  Prints the bytes a Nadam step moves (28 per
element) and the guard's extra read (4 per element), GB/s, the launches per iteration, and - in the same call - the training
iteration replayed as hipGraphs with `Nadam` and with an idle `GuardedNadam`, for the guard's share of the step.  One JSON line at
the end.
Usage (GPU box): python tools/bench_guard.py [--reps 30] [--rounds 5] [--train-iters 32]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import Discriminator, Generator, GuardedNadam, Nadam, NetConfig, TrainStep, get_model  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402
from tools.bench_stats import each_launch_ms, loop_ms  # noqa: E402


def build(cfg, dev, guarded):
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
    if guarded:
        gen_opt = GuardedNadam(gen.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2))
        dis_opt = GuardedNadam(dis.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2))
    gen.batched_spectral_norm = dis.batched_spectral_norm = True
    return gen, dis, TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 networks (a rehearsal: measures overheads only)")
    ap.add_argument("--reps", type=int, default=30, help="timed steps per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=5, help="Nadam / GuardedNadam rounds, alternating")
    ap.add_argument("--evict-mib", type=int, default=1280, help="size of the fill between two steps (at least 1024)")
    ap.add_argument("--train-iters", type=int, default=32, help="training iterations per timed loop")
    args = ap.parse_args()
    if args.reps < 20 or args.evict_mib < 1024 or args.rounds < 2 or args.train_iters < 16:
        ap.error("--reps >= 20, --evict-mib >= 1024, --rounds >= 2 and --train-iters >= 16")
    require_gpu()
    dev = torch.device("cuda:0")
    S, B = args.image_size, 64
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    from locate_amd.graph import GraphedTrainStep
    real, aug = (torch.randn(B, 3, S, S, device=dev).clamp(-1, 1) for _ in range(2))
    runners = {}
    for name, guarded in (("nadam", False), ("guarded", True)):
        gen, dis, step = build(cfg, dev, guarded)
        lat = torch.randn(B, gen.g_in, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        runners[name] = (GraphedTrainStep(step, lat, real, aug, warmup=2), gen, dis, step)
        runners[name][0].replay()
    runner, gen, dis, step = runners["nadam"]          # the gradients sit in the graphs' fixed buffers

    # extra optimizers over the replayed step's parameters: moments of their own, the same gradient buffers
    pairs = {"nadam": [Nadam(net.parameters(), lr=1e-5) for net in (dis, gen)],
             "guarded": [GuardedNadam(net.parameters(), lr=1e-5) for net in (dis, gen)],
             "guarded_clipping": [GuardedNadam(net.parameters(), lr=1e-5, max_norm=1e-3) for net in (dis, gen)]}

    def stepper(name):
        def fn():
            for opt in pairs[name]:
                opt.step()
        return fn
    steps = {name: stepper(name) for name in pairs}
    elements = sum(p.numel() for net in (dis, gen) for p in net.parameters() if p.grad is not None)
    tensors = sum(1 for net in (dis, gen) for p in net.parameters() if p.grad is not None)
    out = {"image_size": S, "networks": "tiny" if args.tiny else "full", "tensors": tensors, "elements": elements,
           "nadam_bytes": 28 * elements, "guard_extra_bytes": 4 * elements, "reps": args.reps, "rounds": args.rounds,
           "evict_mib": args.evict_mib, "launches_per_iteration_nadam": 4, "launches_per_iteration_guarded": 8}
    import time
    for name, fn in steps.items():          # the host's part of a step: table look-ups by address, one ctypes call per group
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        out[name + "_host_us"] = 1e6 * (time.perf_counter() - t0) / 20
        torch.cuda.synchronize()

    junk = torch.empty(args.evict_mib << 18, dtype=torch.float32, device=dev)
    fills = [0]

    def evict():
        fills[0] += 1
        junk.fill_(float(fills[0]))

    med = statistics.median
    rounds = {}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits all alike
        for name, fn in steps.items():
            rounds.setdefault(name + "_behind_iteration", []).append(med(each_launch_ms(fn, args.reps, between=runner.replay)))
            rounds.setdefault(name + "_evicted", []).append(med(each_launch_ms(fn, args.reps, between=evict)))
            rounds.setdefault(name + "_hot", []).append(med(each_launch_ms(fn, args.reps)))
    for k, v in rounds.items():
        out[k + "_us_rounds"] = [1e3 * t for t in v]
        out[k + "_us"] = 1e3 * med(v)
    for where in ("behind_iteration", "evicted", "hot"):
        out["nadam_%s_gb_per_s" % where] = 28 * elements / (out["nadam_%s_us" % where] * 1e-6) / 1e9
        out["guarded_%s_gb_per_s" % where] = 32 * elements / (out["guarded_%s_us" % where] * 1e-6) / 1e9
        extra = out["guarded_%s_us" % where] - out["nadam_%s_us" % where]
        out["guard_extra_%s_us" % where] = extra
        out["guard_extra_%s_gb_per_s" % where] = 4 * elements / (extra * 1e-6) / 1e9 if extra > 0 else None
    counters = [opt.counters() for opt in pairs["guarded"] + pairs["guarded_clipping"]]
    out["counters_idle"], out["counters_clipping"] = counters[:2], counters[2:]

    plain, guarded = [], []
    for _ in range(3):
        plain.append(loop_ms(runners["nadam"][0].replay, args.train_iters))
        guarded.append(loop_ms(runners["guarded"][0].replay, args.train_iters))
    out["train_iteration_ms_rounds"], out["train_iteration_ms"] = plain, med(plain)
    out["train_iteration_guarded_ms_rounds"], out["train_iteration_guarded_ms"] = guarded, med(guarded)
    out["share_of_step"] = out["guard_extra_behind_iteration_us"] * 1e-3 / med(plain)
    out["counters_guarded_run"] = {"G": runners["guarded"][3].gen_opt.counters(), "D": runners["guarded"][3].dis_opt.counters()}
    for k in sorted(out):
        print("%-44s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
