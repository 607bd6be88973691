"""Times what the LeCam regulariser (locate_amd/lecam.py LeCam, csrc/lecam.hip) adds, in one session, every single call behind a fill
of 512 MiB that empties L2 and the 256 MiB Infinity Cache, at the benchmark's batch of 64 logits:
  * locate_d_loss_lecam, active and inactive, against locate_d_loss of this tree and - with --parent-lib - of a library built from
    the PARENT commit, loaded beside this tree's, alternating in the same rounds.  All are one single-block launch; the yardstick
    for a difference is the parent's own spread from round to round;
  * the observe launch alone;
  * one replayed training iteration (hipGraphs, the benchmark's networks at 64 x 64, batch 64) without a LeCam, with an inactive
    one (weight 0.3, a warmup beyond the run) and with an active one (weight 0.3, warmup 0), observe() included, windows
    alternating.  A step that is never timed is built FIRST: the first step a process builds has measured 0.55 ms slower than the
    others (profiles/notes_ada.md).
It also checks that locate_d_loss of this tree, and the inactive locate_d_loss_lecam, write the parent's locate_d_loss bits for
B in 1, 8, 64, 257, 1000.
HIP events around single calls, `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it
their range.  One JSON line at the end.
Usage (GPU box): python tools/bench_lecam.py [--parent-lib PATH/liblocate_hip.so] [--rounds 9] [--steps 30] [--no-step]
                                          [--step-order none,inactive,active]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import LeCam  # noqa: E402
from locate_amd._lib import PROTOTYPES, check, lib, require_gpu  # noqa: E402

GAMMA = 100.0


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
    fn = handle.locate_d_loss
    fn.restype, fn.argtypes = PROTOTYPES["locate_d_loss"]
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblocate_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=30, help="replayed iterations per timed window of the step comparison")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--step-order", default="none,inactive,active", help="the order in which the three timed steps are built and timed")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    libs = {"new": lib()}
    if args.parent_lib:
        libs["parent"] = bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings = {"parent_lib": bool(args.parent_lib)}, {}

    def plain(which, t, f, a, losses, g):
        B = t.numel()
        check(libs[which].locate_d_loss(t.data_ptr(), f.data_ptr(), a.data_ptr(), B, GAMMA, losses.data_ptr(), g[0].data_ptr(),
                                        g[1].data_ptr(), g[2].data_ptr(), stream), "locate_d_loss")

    def regularised(state, t, f, a, losses, g, warmup):
        B = t.numel()
        check(lib().locate_d_loss_lecam(t.data_ptr(), f.data_ptr(), a.data_ptr(), B, GAMMA, state.data_ptr(), 0.3, 1, warmup,
                                        losses.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), stream), "locate_d_loss_lecam")

    # a record with anchors and five accepted observations: active at warmup 5, inactive at warmup 6
    record = torch.zeros(16, dtype=torch.int32, device=dev)
    record[:2] = torch.tensor([0.3125, -0.4375], device=dev).view(torch.int32)
    record[2] = 5
    gen = torch.Generator(device="cpu").manual_seed(64)
    same = True
    for B in (1, 8, 64, 257, 1000):
        t, f, a = (torch.randn(B, generator=gen).to(dev) * 1.5 for _ in range(3))
        got = {}
        for which in list(libs) + ["inactive"]:
            losses, g = torch.full((4,), -1.0, device=dev), torch.full((3, B), -1.0, device=dev)
            if which == "inactive":
                regularised(record, t, f, a, losses, g, 6)
            else:
                plain(which, t, f, a, losses, g)
            got[which] = torch.cat([losses[:3], g.reshape(-1)]).view(torch.int32).clone()
        same = same and all(torch.equal(got["new"], v) for v in got.values())
    out["plain_and_inactive_write_the_parents_bits" if args.parent_lib else "inactive_writes_locate_d_loss_bits"] = bool(same)

    B = 64
    t, f, a = (torch.randn(B, generator=gen).to(dev) * 1.5 for _ in range(3))
    losses, g = torch.empty(4, device=dev), torch.empty(3, B, device=dev)
    for which in libs:
        settings["d_loss_" + which] = lambda which=which: plain(which, t, f, a, losses, g)
    settings["d_loss_lecam_inactive"] = lambda: regularised(record, t, f, a, losses, g, 6)
    settings["d_loss_lecam_active"] = lambda: regularised(record, t, f, a, losses, g, 5)
    observer = LeCam(batch=B, device=dev)
    settings["observe_64_logits"] = lambda: observer.observe(t, f)
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
    lo, hi = out["d_loss_%s_us_range" % base]
    out["d_loss_%s_spread_us" % base] = hi - lo
    for name in ("d_loss_lecam_inactive", "d_loss_lecam_active") + (("d_loss_new",) if base == "parent" else ()):
        out["%s_minus_%s_us" % (name, base)] = out[name + "_us"] - out["d_loss_%s_us" % base]

    if not args.no_step:
        from locate_amd import Discriminator, Generator, NetConfig, TrainStep, get_model
        from locate_amd.graph import GraphedTrainStep
        S = 64
        runners = {}
        names = ("none", "inactive", "active")
        chosen = args.step_order.split(",")
        if sorted(chosen) != sorted(names):
            ap.error("--step-order is a permutation of " + ",".join(names))
        order = ["first_built_untimed"] + chosen
        out["step_order"] = order[1:]
        for name in order:
            cfg = NetConfig(image_size=S)
            torch.manual_seed(cfg.seed)
            G, GO = get_model(Generator(cfg), cfg.glr, dev)
            Dn, DO = get_model(Discriminator(cfg), cfg.dlr, dev)
            G.batched_spectral_norm = Dn.batched_spectral_norm = True
            lecam = None
            if name in ("inactive", "active"):
                lecam = LeCam(batch=B, weight=0.3, warmup=10 ** 9 if name == "inactive" else 0, device=dev)
            step = TrainStep(G, Dn, GO, DO, lecam=lecam)
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
            runners[name] = (runner, lecam)

        def window(name):
            runner, lecam = runners[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                got = runner.replay()
                if lecam is not None:
                    lecam.observe(got["d_true"], got["d_gen"])
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
        out["step_inactive_minus_none_ms"] = out["step_inactive_ms"] - out["step_none_ms"]
        out["step_active_minus_none_ms"] = out["step_active_ms"] - out["step_none_ms"]
        out["lecam_status"] = {name: runners[name][1].status() for name in ("inactive", "active")}
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
