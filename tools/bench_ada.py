"""Times what the adaptive augmentation (locate_amd/augment.py AdaptiveDiffAugment, csrc/ada.hip, the per-image op mask of
csrc/diffaug.hip) adds, in one session, every single call behind a fill of 512 MiB that empties L2 and the 256 MiB Infinity Cache,
at 192 x 3 x 64 x 64 (the D-step's stacked batch at the benchmark's size: one launch) and 48 x 3 x 256 x 256 (two launches):
  * diffaug forward and backward, full policy, every mask 0 - and the same two calls through a library built from the PARENT commit
    (--parent-lib, loaded beside this tree's), alternating in the same rounds: what the mask branch costs an unmasked batch.  The
    yardstick for the difference is the parent's own spread from round to round;
  * the same kernels with every op masked (the copy path) against a device-to-device copy of the same bytes;
  * the gate launch (4 x 64 rows) and the observe launch (64 logits) alone;
  * one replayed training iteration (hipGraphs, the benchmark's networks at 64 x 64, batch 64) with AdaptiveDiffAugment at p = 1
    (kimg = inf: the plain run's work plus staging copy, gate and observe) and at p = 0, against plain DiffAugment, windows alternating.
It also checks that this tree's kernels at mask 0 write the parent's bytes, and that the parent ignores the mask word.
HIP events around single calls, `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it
their range.  One JSON line at the end.
Usage (GPU box): python tools/bench_ada.py [--parent-lib PATH/liblocate_hip.so] [--rounds 9] [--steps 30] [--no-step] [--reverse-steps]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import AdaptiveDiffAugment, DiffAugment, draw_parameters  # noqa: E402
from locate_amd._lib import PROTOTYPES, check, lib, require_gpu  # noqa: E402

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


def bind(handle):
    for name in ("locate_diffaug_fwd", "locate_diffaug_bwd", "locate_diffaug_workspace_bytes"):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblocate_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=30, help="replayed iterations per timed window of the step comparison")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--reverse-steps", action="store_true", help="build and time the three steps in the opposite order")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    libs = {"new": lib()}
    if args.parent_lib:
        libs["parent"] = bind(ctypes.CDLL(os.path.abspath(args.parent_lib)))
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings = {"parent_lib": bool(args.parent_lib)}, {}
    shapes = ((192, 64), (48, 256))
    for n, S in shapes:
        gen = torch.Generator(device=dev).manual_seed(S)
        x = torch.rand(n, 3, S, S, device=dev, generator=gen) * 2.0 - 1.0
        rows = draw_parameters(n, S, torch.Generator().manual_seed(S), FULL)
        p0 = torch.from_numpy(rows).to(dev)
        rows[:, 9] = 7.0
        p7 = torch.from_numpy(rows).to(dev)
        dst = torch.empty_like(x)
        ws = torch.empty(max(int(lib().locate_diffaug_workspace_bytes(n, S)), 16), dtype=torch.uint8, device=dev)
        tag = "%dx3x%dx%d" % (n, S, S)

        def call(which, entry, p, x=x, dst=dst, ws=ws, n=n, S=S):
            check(getattr(libs[which], entry)(x.data_ptr(), p.data_ptr(), dst.data_ptr(), n, S, 7, ws.data_ptr(), stream), entry)
        results = {}
        for which in libs:
            for d in ("fwd", "bwd"):
                settings["%s_%s_%s" % (d, which, tag)] = lambda which=which, d=d, p0=p0, call=call: call(which, "locate_diffaug_" + d, p0)
                call(which, "locate_diffaug_" + d, p0)
                results[(which, d, 0)] = dst.clone()
                call(which, "locate_diffaug_" + d, p7)
                results[(which, d, 7)] = dst.clone()
        for d in ("fwd", "bwd"):
            settings["%s_masked_%s" % (d, tag)] = lambda d=d, p7=p7, call=call: call("new", "locate_diffaug_" + d, p7)
            assert torch.equal(results[("new", d, 7)], x), "a fully masked batch is not a copy"
            if "parent" in libs:
                out["mask0_equals_parent_%s_%s" % (d, tag)] = bool(torch.equal(results[("new", d, 0)].view(torch.int32),
                                                                               results[("parent", d, 0)].view(torch.int32)))
                out["parent_ignores_mask_%s_%s" % (d, tag)] = bool(torch.equal(results[("parent", d, 7)].view(torch.int32),
                                                                               results[("parent", d, 0)].view(torch.int32)))
        settings["copy_" + tag] = lambda x=x, dst=dst: dst.copy_(x)
        out["bytes_" + tag] = 2 * x.numel() * 4
    # the two launches beside the step, at the benchmark's batch
    a = AdaptiveDiffAugment(S=64, batch=64, policy=FULL, seed=1, device=dev, initial_p=0.5)
    a.draw()
    logits = torch.randn(64, device=dev)
    settings["gate_256_rows"] = lambda: check(lib().locate_ada_gate(a._raw.data_ptr(), a.state.data_ptr(), a.params.data_ptr(), 256, 7, stream),
                                              "locate_ada_gate")
    settings["observe_64_logits"] = lambda: a.observe(logits)
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
            out["%s_masked_over_copy_%s" % (d, tag)] = out["%s_masked_%s_us" % (d, tag)] / out["copy_%s_us" % tag]
            if "parent" in libs:
                out["%s_new_minus_parent_us_%s" % (d, tag)] = out["%s_new_%s_us" % (d, tag)] - out["%s_parent_%s_us" % (d, tag)]
                lo, hi = out["%s_parent_%s_us_range" % (d, tag)]
                out["%s_parent_spread_us_%s" % (d, tag)] = hi - lo

    if not args.no_step:
        from locate_amd import Discriminator, Generator, NetConfig, TrainStep, get_model
        from locate_amd.graph import GraphedTrainStep
        S, B = 64, 64
        runners = {}
        names = ("plain", "adaptive_p1", "adaptive_p0")
        out["step_order"] = list(names[::-1] if args.reverse_steps else names)
        for name in out["step_order"]:
            cfg = NetConfig(image_size=S)
            torch.manual_seed(cfg.seed)
            G, GO = get_model(Generator(cfg), cfg.glr, dev)
            Dn, DO = get_model(Discriminator(cfg), cfg.dlr, dev)
            G.batched_spectral_norm = Dn.batched_spectral_norm = True
            if name == "plain":
                aug = DiffAugment(S=S, batch=B, policy=FULL, seed=1, device=dev)
            else:
                aug = AdaptiveDiffAugment(S=S, batch=B, policy=FULL, seed=1, device=dev, kimg=float("inf"),
                                          initial_p=1.0 if name == "adaptive_p1" else 0.0)
            step = TrainStep(G, Dn, GO, DO, augment=aug)
            gen = torch.Generator(device="cpu").manual_seed(1234)
            latent = torch.randn(B, S, generator=gen).to(dev)
            real = torch.randn(B, 3, S, S, generator=gen).clamp(-1, 1).to(dev)
            fake = torch.randn(B, 3, S, S, generator=gen).clamp(-1, 1).to(dev)
            aug.draw()
            runners[name] = (GraphedTrainStep(step, latent, real, fake, warmup=2), aug)

        def window(name):
            runner, aug = runners[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                aug.draw()
                got = runner.replay()
                if hasattr(aug, "observe"):
                    aug.observe(got["d_true"])
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
        out["step_adaptive_p1_minus_plain_ms"] = out["step_adaptive_p1_ms"] - out["step_plain_ms"]
        out["step_adaptive_p0_minus_plain_ms"] = out["step_adaptive_p0_ms"] - out["step_plain_ms"]
        out["adaptive_status"] = {name: runners[name][1].status() for name in ("adaptive_p1", "adaptive_p0")}
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
