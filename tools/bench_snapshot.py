"""Times `TrainingSnapshot.take()` and `.restore()` (locate_amd/snapshot.py, csrc/snapshot.hip) on the benchmark networks (64 x 64,
full width, batch 64, with an averaged generator), HIP events around every single call:
  * a take BEHIND a real training iteration (replayed as hipGraphs, as bench.py measures it) - its operands then come from HBM,
    which is what a run sees - and a take back to back;
  * the iteration that FOLLOWS a take against an iteration that follows none - a take pushes a slot's worth of stores through the
    Infinity Cache the next iteration's weights sit in - for ordinary and for nontemporal stores (the debug variant of the library
    reads LOCATE_SNAPSHOT_NT at every call; the product library has one form compiled in, see csrc/snapshot.hip);
  * restore() with its `refresh_panels`, host read included;
  * the bytes moved (8 per 4-byte word: read once, written once) and the TB/s;
  * as the yardstick, what ATen can do for the same tensor list: `torch._foreach_copy_` into preallocated clones, alone and with a
    finiteness verdict from `torch._foreach_norm` (kept on the device), `--rounds` times alternating with the kernel so that the
    yardstick's own spread from round to round is the margin.
One JSON line at the end.  Usage (GPU box): python tools/bench_snapshot.py [--reps 20] [--rounds 3] [--tiny]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("LOCATE_HIP_DEBUG_LIBRARY", "1")          # the variant that can switch the store form per call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import AveragedGenerator, Discriminator, Generator, NetConfig, TrainStep, TrainingSnapshot, get_model  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402
from locate_amd.graph import GraphedTrainStep  # noqa: E402


def each_call_ms(fn, reps, warmup=2, between=None):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 networks (a rehearsal: measures overheads only)")
    ap.add_argument("--reps", type=int, default=20, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3, help="kernel / yardstick rounds, alternating")
    ap.add_argument("--rollback-every", type=int, default=256, help="for the cost per iteration")
    args = ap.parse_args()
    if args.reps < 5 or args.rounds < 2:
        ap.error("--reps >= 5 and --rounds >= 2")
    require_gpu()
    dev = torch.device("cuda:0")
    S, B = args.image_size, args.batch
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
    gen.batched_spectral_norm = dis.batched_spectral_norm = True
    step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)
    avg = AveragedGenerator(gen, half_life_images=10000, batch=B)
    lat, x, y = (torch.randn(B, gen.g_in, device=dev), torch.randn(B, 3, S, S, device=dev).clamp(-1, 1),
                 torch.randn(B, 3, S, S, device=dev).clamp(-1, 1))
    runner = GraphedTrainStep(step, lat, x, y, warmup=2)          # the optimizer states exist from here on
    snap = TrainingSnapshot(step, avg)
    count = [0]

    def iteration():
        runner.replay()
        avg.update()

    def take():
        count[0] += 1
        snap.take(count[0])

    def stores(nontemporal):
        os.environ["LOCATE_SNAPSHOT_NT"] = "1" if nontemporal else "0"

    live = [t for t in snap._live() if t is not None and t.numel()]
    words = sum(t.numel() * t.element_size() // 4 for t in live)
    nbytes = 8 * words
    out = {"image_size": S, "batch": B, "networks": "tiny" if args.tiny else "full", "entries": len(snap.names), "live_tensors": len(live),
           "slot_bytes": snap.slot_bytes, "bytes_moved_per_take": nbytes, "reps": args.reps, "rounds": args.rounds,
           "debug_library": os.environ.get("LOCATE_HIP_DEBUG_LIBRARY") == "1"}

    # the yardstick: the same tensors through ATen, into clones made once
    clones = [torch.empty_like(t) for t in live]
    by_dtype = {}
    for t in live:
        by_dtype.setdefault(t.dtype, []).append(t)
    verdict = torch.zeros((), dtype=torch.bool, device=dev)

    @torch.no_grad()
    def aten_copy():
        torch._foreach_copy_(clones, live)

    @torch.no_grad()
    def aten_copy_and_verdict():
        torch._foreach_copy_(clones, live)
        ok = [torch.stack(torch._foreach_norm(ts)).isfinite().all() for ts in by_dtype.values()]
        verdict.copy_(torch.stack(ok).all())

    med = statistics.median
    keys = ("take_plain_behind", "take_nt_behind", "take_plain_hot", "take_nt_hot", "aten_copy_behind", "aten_pair_behind",
            "iteration_alone", "iteration_after_plain", "iteration_after_nt")
    rounds = {k: [] for k in keys}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits all alike
        for nt, tag in ((False, "plain"), (True, "nt")):
            stores(nt)
            rounds["take_%s_behind" % tag].append(med(each_call_ms(take, args.reps, between=iteration)))
            rounds["take_%s_hot" % tag].append(med(each_call_ms(take, args.reps)))
            rounds["iteration_after_%s" % tag].append(med(each_call_ms(iteration, args.reps, between=take)))
        rounds["iteration_alone"].append(med(each_call_ms(iteration, args.reps)))
        rounds["aten_copy_behind"].append(med(each_call_ms(aten_copy, args.reps, between=iteration)))
        rounds["aten_pair_behind"].append(med(each_call_ms(aten_copy_and_verdict, args.reps, between=iteration)))
    for k, v in rounds.items():
        out[k + "_ms_rounds"] = v
        out[k + "_ms"] = med(v)
        out[k + "_spread_ms"] = max(v) - min(v)
    for k in ("take_plain_behind", "take_nt_behind", "take_plain_hot", "take_nt_hot", "aten_copy_behind"):
        out[k + "_tb_per_s"] = nbytes / (out[k + "_ms"] * 1e-3) / 1e12
    for tag in ("plain", "nt"):          # what a take costs a run: itself plus what it does to the iteration behind it
        out["take_plus_following_%s_ms" % tag] = out["take_%s_behind_ms" % tag] + out["iteration_after_%s_ms" % tag] - out["iteration_alone_ms"]
        out["share_of_run_%s" % tag] = out["take_plus_following_%s_ms" % tag] / (args.rollback_every * out["iteration_alone_ms"])
    margin = out["aten_copy_behind_spread_ms"]
    best = min(out["take_plain_behind_ms"], out["take_nt_behind_ms"])
    out["faster_than_foreach_copy_alone"] = bool(best + margin < out["aten_copy_behind_ms"])
    out["faster_than_the_aten_pair"] = bool(best + out["aten_pair_behind_spread_ms"] < out["aten_pair_behind_ms"])

    # the host's part of a take (the getters, the table look-up by address, two launches): what the back-to-back events see
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        take()
    out["take_host_ms"] = (time.perf_counter() - t0) * 1e3 / args.reps
    torch.cuda.synchronize()

    # restore with its re-pack, host read included (the product store form is irrelevant here)
    stores(False)
    take()
    assert snap.status()["good"] >= 0, snap.status()
    restore = each_call_ms(snap.restore, args.reps, between=iteration)
    out["restore_ms"] = med(restore)
    out["restore_ms_max"] = max(restore)
    out["status"] = snap.status()
    for k in sorted(out):
        print("%-40s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
