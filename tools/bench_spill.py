"""Times the snapshot's spill to disk (locate_amd/spill.py, csrc/digest.hip) on the benchmark networks (64 x 64, full width, batch
64, with an averaged generator), in one session, interleaved rounds, spreads reported:
  * the two digest launches over a slot, BEHIND a real training iteration (replayed as hipGraphs, as bench.py measures it) and
    back to back, HIP events around every single call, with the implied TB/s (4 bytes per word); as the yardstick the snapshot's
    take in the same rounds, which moves twice the bytes;
  * the main thread's wall time of `spill.begin()`, the device idle, so that the 64-byte status read waits for nothing;
  * the iterations that overlap the device-to-host copy against iterations with no copy in flight;
  * begin() to the rename, with the writer's share split into event wait, host digest and file write;
  * as the yardstick for the whole feature, the wall time of `Trainer.save_state()` on the same state: what a mid-epoch save costs.
One JSON line at the end.  Usage (GPU box): python tools/bench_spill.py [--reps 20] [--rounds 3] [--spills 4] [--tiny] [--out DIR]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import (AveragedGenerator, Discriminator, Generator, NetConfig, SnapshotSpill, Trainer, TrainStep, TrainingSnapshot,  # noqa: E402
                        get_model)
from locate_amd._lib import require_gpu  # noqa: E402
from locate_amd.graph import GraphedTrainStep  # noqa: E402
from locate_amd.spill import _launch_digest  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spills", type=int, default=4, help="whole spills per round (each waits for its file)")
    ap.add_argument("--overlap", type=int, default=2, help="iterations timed behind every begin()")
    ap.add_argument("--out", default=None, help="folder for the files (default: a temporary one, removed at the end)")
    args = ap.parse_args()
    if args.reps < 5 or args.rounds < 2 or args.spills < 2:
        ap.error("--reps >= 5, --rounds >= 2, --spills >= 2")
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
    folder = args.out or tempfile.mkdtemp(prefix="bench_spill_")
    spill = SnapshotSpill(snap, os.path.join(folder, "spill"))
    count = [0]

    def iteration():
        runner.replay()
        avg.update()

    def take():
        count[0] += 1
        spill.take(count[0], {"iterations": count[0]})

    def take_alone():          # the snapshot's own take, as tools/bench_snapshot.py times it
        count[0] += 1
        snap.take(count[0])

    def digest():
        _launch_digest(spill._tables[0], torch.cuda.current_stream())

    words = sum(spill._counts)
    out = {"image_size": S, "batch": B, "networks": "tiny" if args.tiny else "full", "entries": len(snap.names), "slot_bytes": snap.slot_bytes,
           "words": words, "reps": args.reps, "rounds": args.rounds, "spills_per_round": args.spills}
    med = statistics.median
    take()
    torch.cuda.synchronize()
    keys = ("digest_behind", "digest_hot", "take_behind", "take_hot", "iteration_alone", "iteration_during_copy", "begin_host", "latency",
            "writer_event", "writer_digest", "writer_write")
    rounds = {k: [] for k in keys}
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits all alike
        rounds["digest_behind"].append(med(each_call_ms(digest, args.reps, between=iteration)))
        rounds["take_behind"].append(med(each_call_ms(take_alone, args.reps, between=iteration)))
        rounds["digest_hot"].append(med(each_call_ms(digest, args.reps)))
        rounds["take_hot"].append(med(each_call_ms(take_alone, args.reps)))
        during, alone, begin, latency, shares = [], [], [], [], {"event": [], "digest": [], "write": []}
        for _ in range(args.spills):
            take()
            alone += each_call_ms(iteration, args.overlap, warmup=1)          # no copy in flight; ends with the device idle
            t0 = time.perf_counter()
            began = spill.begin()
            begin.append((time.perf_counter() - t0) * 1e3)
            assert began, spill.status()
            during += each_call_ms(iteration, args.overlap, warmup=0)          # issued at once: they run beside the copy
            spill.wait()
            latency.append(spill.status()["last_seconds"] * 1e3)
            for k in shares:
                shares[k].append(spill.timing[k] * 1e3)
        rounds["iteration_alone"].append(statistics.mean(alone))
        rounds["iteration_during_copy"].append(statistics.mean(during))
        rounds["begin_host"].append(med(begin))
        rounds["latency"].append(med(latency))
        for k in shares:
            rounds["writer_" + k].append(med(shares[k]))
    for k, v in rounds.items():
        out[k + "_ms_rounds"] = v
        out[k + "_ms"] = med(v)
        out[k + "_spread_ms"] = max(v) - min(v)
    for k in ("digest_behind", "digest_hot"):
        out[k + "_tb_per_s"] = 4 * words / (out[k + "_ms"] * 1e-3) / 1e12
    for k in ("take_behind", "take_hot"):
        out[k + "_tb_per_s"] = 8 * words / (out[k + "_ms"] * 1e-3) / 1e12
    out["digest_clearly_under_take"] = bool(out["digest_behind_ms"] + out["digest_behind_spread_ms"] + out["take_behind_spread_ms"] < out["take_behind_ms"])
    out["slowdown_during_copy_ms"] = out["iteration_during_copy_ms"] - out["iteration_alone_ms"]
    out["host_digest_mwords_per_s"] = words / (out["writer_digest_ms"] * 1e-3) / 1e6
    out["file_write_gb_per_s"] = snap.slot_bytes / (out["writer_write_ms"] * 1e-3) / 1e9
    out["spill_status"] = spill.status()
    spill.close()

    # the yardstick: what a mid-epoch save costs today, on the same state
    pipeline = types.SimpleNamespace(batch=B, batches_per_epoch=1000, state_dict=lambda: {"epoch": 0, "pos": 0})
    trainer = Trainer(step, pipeline, os.path.join(folder, "save"), average=avg)
    trainer.sampler          # made outside the timing
    saves = []
    for _ in range(args.rounds):
        iteration()
        t0 = time.perf_counter()
        trainer.save_state()
        saves.append((time.perf_counter() - t0) * 1e3)
    out["save_state_ms_rounds"] = saves
    out["save_state_ms"] = med(saves)
    out["save_state_spread_ms"] = max(saves) - min(saves)
    out["save_state_over_begin"] = out["save_state_ms"] / out["begin_host_ms"]
    if args.out is None:
        shutil.rmtree(folder, ignore_errors=True)
    for k in sorted(out):
        print("%-40s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
