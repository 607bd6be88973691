"""Cost of the training monitor (locate_amd/monitor.py, csrc/grid.hip) at the reference's sample size - 64 images - for one image
size per call (S = 64 is the benchmark's; S = 256 the largest picture).

  render        image_grid on a resident batch: the range launches and the compose launch, HIP events over --reps calls;
  Sampler.save  split into the generator's eval pass (events), the render (events), the copy of the picture to pinned host
                memory (host clock around a synchronise) and the PNG encoder (host clock; zlib levels 1 and 6);
  record        LossHistory.record per call: host time to enqueue its two launches and their device time (events);
  flush         LossHistory.flush of 16 records on an idle device (host clock: one device-to-host copy and its synchronise).

With --step-ms (the training step's time from bench.py, same session) it prints the monitor's amortised share at the reference's
cadence for batch 64: one sample per 16 * 1024 // 64 = 256 iterations, one record per iteration, one flush per 16:
    (generator pass + render) / 256 + record + flush / 16      - the PNG encoder runs on the host and is reported, not charged.
One JSON line.  Usage (GPU machine): python tools/bench_monitor.py --image-size 64 [--step-ms 8.9] [--reps 200]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import Generator, LossHistory, NetConfig, Sampler, get_model, image_grid  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402
from locate_amd.monitor import write_png  # noqa: E402


def events_ms(fn, reps, warmup=10):
    """(device ms per call, host ms per call to enqueue)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps * 1e3
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, host


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pass-reps", type=int, default=20, help="timed generator passes")
    ap.add_argument("--step-ms", type=float, default=None)
    args = ap.parse_args()
    arch, cus, _ = require_gpu()
    dev = torch.device("cuda:0")
    S, n = args.image_size, args.images
    rec = {"device": arch, "cus": cus, "image_size": S, "images": n, "reps": args.reps}

    x = torch.tanh(1.5 * torch.randn(n, 3, S, S, device=dev))
    picture = image_grid(x, padding=8)
    rec["picture"] = list(picture.shape)
    rec["render_ms"], rec["render_host_ms"] = events_ms(lambda: image_grid(x, padding=8, out=picture), args.reps)
    rec["render_fixed_range_ms"], _ = events_ms(lambda: image_grid(x, padding=8, value_range=(-1.0, 1.0), out=picture), args.reps)
    rec["render_bytes"] = 2 * x.numel() * 4 + picture.numel()          # the batch read twice (range, compose), the picture written once

    cfg = NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, _ = get_model(Generator(cfg), cfg.glr, dev, cfg)
    gen.batched_spectral_norm = True
    for keep in (False, True):
        sampler = Sampler(gen, images=n, seed=1, advance_spectral_norm=not keep)
        ms, _ = events_ms(sampler.sample, args.pass_reps, warmup=3)
        rec["generator_pass_keep_uv_ms" if keep else "generator_pass_ms"] = ms
    sampler = Sampler(gen, images=n, seed=1)
    shown = sampler.render()
    rec["copy_to_host_ms"] = host_ms(lambda: sampler._to_host(shown), 20)
    host = sampler._to_host(shown).copy()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "p.png")
        for level in (1, 6):
            rec["png_encode_level%d_ms" % level] = host_ms(lambda: write_png(path, host, level=level), 3)
            rec["png_level%d_bytes" % level] = os.path.getsize(path)
        rec["save_end_to_end_ms"] = host_ms(lambda: sampler.save(path), 5)

    out = {"d_error": torch.rand((), device=dev), "g_error": torch.rand((), device=dev)}
    history = LossHistory(capacity=1 << 16)
    rec["record_ms"], rec["record_host_ms"] = events_ms(lambda: history.record(out), 2000, warmup=50)
    history.flush()

    def flush16():
        for _ in range(16):
            history.record(out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        history.flush()
        return time.perf_counter() - t0
    for _ in range(5):
        flush16()
    rec["flush_ms"] = sum(flush16() for _ in range(50)) / 50 * 1e3

    sample_gpu = rec["generator_pass_ms"] + rec["render_ms"]
    rec["amortised_device_ms"] = sample_gpu / 256 + rec["record_ms"] + rec["flush_ms"] / 16
    rec["amortised_host_bound_ms"] = sample_gpu / 256 + max(rec["record_ms"], rec["record_host_ms"]) + rec["flush_ms"] / 16
    if args.step_ms:
        rec["step_ms"] = args.step_ms
        rec["amortised_share_of_step"] = rec["amortised_device_ms"] / args.step_ms
        rec["amortised_host_bound_share_of_step"] = rec["amortised_host_bound_ms"] / args.step_ms
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
