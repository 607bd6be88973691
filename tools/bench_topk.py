"""Times what top-k training of the generator (locate_amd/topk.py TopK, csrc/topk.hip) adds, in one session, every single call behind a
fill of 512 MiB that empties L2 and the 256 MiB Infinity Cache:
  * locate_g_loss_topk at B = 64 (the benchmark's batch) with k = B and k = B / 2, and at B = 4096, against locate_g_loss of this tree
    and - with --parent-lib - of a library built from the PARENT commit, loaded beside this tree's, alternating in the same rounds.
    All are one single-block launch; the yardstick for a difference is the parent's own spread from round to round;
  * both selection forms (rank count, bitonic sort) at B = 64, 256, 512, 1024, 2048 and 4096 with k = B / 2: where the library's
    choice by size (TOPK_SORT_FROM, csrc/topk.hip) comes from;
  * one replayed training iteration (hipGraphs, the benchmark's networks at 64 x 64, batch 64) without a TopK and with one whose k
    keeps moving (advance() included), windows alternating.  A step that is never timed is built FIRST, and --step-order
    swaps the two: the position of a step in the process has measured 0.6 ms (profiles/notes_lecam.md).
It also checks that locate_g_loss of this tree, and locate_g_loss_topk with k = B in both forms, write the parent's locate_g_loss bits
for B in 1, 8, 64, 257, 1000, 4096.
HIP events around single calls, `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it
their range.  One JSON line at the end.
Usage (GPU box): python tools/bench_topk.py [--parent-lib PATH/liblocate_hip.so] [--rounds 9] [--steps 30] [--no-step]
                                         [--step-order none,topk]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import TopK  # noqa: E402
from locate_amd._lib import PROTOTYPES, check, lib, require_gpu  # noqa: E402

FORMS = {"rank": 1, "sort": 2}


def timed(fn, flush):
    """seconds of one call, behind a cache-clearing fill"""
    flush.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def bind(handle):
    fn = handle.locate_g_loss
    fn.restype, fn.argtypes = PROTOTYPES["locate_g_loss"]
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblocate_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=30, help="replayed iterations per timed window of the step comparison")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--step-order", default="none,topk", help="the order in which the two timed steps are built and timed")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    libs = {"new": lib()}
    if args.parent_lib:
        libs["parent"] = bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings = {"parent_lib": bool(args.parent_lib)}, {}
    ring = torch.zeros(64, 8, dtype=torch.int32, device=dev)

    def plain(which, f, loss, g):
        check(libs[which].locate_g_loss(f.data_ptr(), f.numel(), loss.data_ptr(), g.data_ptr(), stream), "locate_g_loss")

    def selected(record, f, losses, g, form):
        check(lib().locate_g_loss_topk(f.data_ptr(), f.numel(), record.data_ptr(), ring.data_ptr(), 64, form, losses.data_ptr(), g.data_ptr(),
                                       stream), "locate_g_loss_topk")

    def record_of(k):
        record = torch.zeros(16, dtype=torch.int32, device=dev)
        record[0] = k
        return record

    gen = torch.Generator(device="cpu").manual_seed(64)
    same = True
    for B in (1, 8, 64, 257, 1000, 4096):
        f = torch.randn(B, generator=gen).to(dev) * 1.5
        got = {}
        for which in list(libs) + list(FORMS):
            losses, g = torch.full((2,), -1.0, device=dev), torch.full((B,), -1.0, device=dev)
            if which in FORMS:
                selected(record_of(B), f, losses, g, FORMS[which])
            else:
                plain(which, f, losses, g)
            got[which] = torch.cat([losses[:1], g]).view(torch.int32).clone()
        same = same and all(torch.equal(got["new"], v) for v in got.values())
    out["plain_and_k_equal_B_write_the_parents_bits" if args.parent_lib else "k_equal_B_writes_locate_g_loss_bits"] = bool(same)

    data = {B: torch.randn(B, generator=gen).to(dev) * 1.5 for B in (64, 256, 512, 1024, 2048, 4096)}
    bufs = {B: (torch.empty(2, device=dev), torch.empty(B, device=dev)) for B in data}
    for B in (64, 4096):
        for which in libs:
            settings["g_loss_%s_B%d" % (which, B)] = lambda which=which, B=B: plain(which, data[B], *bufs[B])
    for B, k in ((64, 64), (64, 32), (4096, 4096), (4096, 2048)):
        settings["g_loss_topk_B%d_k%d" % (B, k)] = lambda B=B, r=record_of(k): selected(r, data[B], *bufs[B], 0)
    for B in data:
        for name, form in FORMS.items():
            settings["form_%s_B%d" % (name, B)] = lambda B=B, r=record_of(B // 2), form=form: selected(r, data[B], *bufs[B], form)
    for fn in settings.values():          # everything once before anything is timed
        fn()
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, flush))
    for name, values in rounds.items():
        out[name + "_us"] = 1e6 * statistics.median(values)
        out[name + "_us_range"] = [1e6 * min(values), 1e6 * max(values)]
    base = "parent" if "parent" in libs else "new"
    for B in (64, 4096):
        lo, hi = out["g_loss_%s_B%d_us_range" % (base, B)]
        out["g_loss_%s_B%d_spread_us" % (base, B)] = hi - lo
    for B, k in ((64, 64), (64, 32), (4096, 4096), (4096, 2048)):
        out["g_loss_topk_B%d_k%d_minus_%s_us" % (B, k, base)] = out["g_loss_topk_B%d_k%d_us" % (B, k)] - out["g_loss_%s_B%d_us" % (base, B)]

    if not args.no_step:
        from locate_amd import Discriminator, Generator, NetConfig, TrainStep, get_model
        from locate_amd.graph import GraphedTrainStep
        S, B = 64, 64
        runners = {}
        names = ("none", "topk")
        chosen = args.step_order.split(",")
        if sorted(chosen) != sorted(names):
            ap.error("--step-order is a permutation of " + ",".join(names))
        out["step_order"] = chosen
        for name in ["first_built_untimed"] + chosen:
            cfg = NetConfig(image_size=S)
            torch.manual_seed(cfg.seed)
            G, GO = get_model(Generator(cfg), cfg.glr, dev)
            Dn, DO = get_model(Discriminator(cfg), cfg.dlr, dev)
            G.batched_spectral_norm = Dn.batched_spectral_norm = True
            # k falls from B to B / 2 in about 45 iterations: most of those replays are preceded by a copy into the record
            topk = TopK(batch=B, gamma=1.0 - 1.0 / B, floor=0.5, every=1, device=dev) if name == "topk" else None
            step = TrainStep(G, Dn, GO, DO, topk=topk)
            sgen = torch.Generator(device="cpu").manual_seed(1234)
            latent = torch.randn(B, S, generator=sgen).to(dev)
            real = torch.randn(B, 3, S, S, generator=sgen).clamp(-1, 1).to(dev)
            fake = torch.randn(B, 3, S, S, generator=sgen).clamp(-1, 1).to(dev)
            runner = GraphedTrainStep(step, latent, real, fake, warmup=2)
            if name == "first_built_untimed":
                runner.replay()
                torch.cuda.synchronize()
                del runner, step, G, Dn, GO, DO
                continue
            runners[name] = (runner, topk)
        done = {name: 0 for name in runners}

        def window(name):
            runner, topk = runners[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if topk is not None:
                    topk.advance(done[name] % (2 * B))          # k keeps moving through the whole measurement
                done[name] += 1
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
        out["step_topk_minus_none_ms"] = out["step_topk_ms"] - out["step_none_ms"]
        out["topk_status"] = runners["topk"][1].status()
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
