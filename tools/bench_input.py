"""Cost of the device-side input pipeline (locate_amd/data.py, csrc/input.hip): one batch PAIR (plain + augmented) at the step's
two sizes - B = 64 at S = 64 from 157 x 128 sources, B = 32 at S = 128 from 314 x 256 - on a synthetic store of random bytes.

Two numbers per shape, both by HIP events on the current stream after a warm-up:
  kernels    the library call alone (contrast pass + transform pass), records already on the device, a different batch each call;
  pipeline   InputPipeline.next_batch(): host draws, the pinned copy of the records and the two launches, as a training loop
             calls it (the host's own share is printed as wall time per call; it overlaps the step in a real loop).
Bytes are ALGORITHMIC: every crop pixel read once, every augmented sample's whole source image read once more for its
contrast mean, every output written once; the rate is that over the kernel time, against the 8 TB/s HBM peak.
One JSON line per shape.  Usage (GPU machine): python tools/bench_input.py [--reps 200] [--images 2048]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from locate_amd import data  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402

PEAK = 8.0e12


def events_ms(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps * 1e3            # enqueue side only: no synchronise inside
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, host


def bench_shape(B, S, H, W, images, reps, seed=0):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    store = data.DeviceImageStore(rng.integers(0, 256, size=(images, H, W, 3), dtype=np.uint8), dev)
    pipe = data.InputPipeline(store, S, B, seed=seed)
    real, aug = pipe.next_batch()
    d = pipe._ensure_device()
    n = 2 * B

    # kernels alone: `sets` different batch pairs uploaded beforehand, visited in turn
    sets, uploaded, nbytes = 16, [], 0
    for _ in range(sets):
        idx, params = pipe._draw()
        data.validate(idx, params, store.N, H, W, d["plan"].side_lo, d["plan"].side_hi)
        side = params["side"].astype(np.int64)
        nbytes += int((side * side * 3).sum()) + B * H * W * 3 + n * 3 * S * S * 4
        uploaded.append((torch.from_numpy(idx).to(dev), torch.from_numpy(params.view(np.uint8).copy()).to(dev)))
    nbytes /= sets
    k = [0]

    def kernels():
        i, p = uploaded[k[0] % sets]
        k[0] += 1
        data.transform(store, i, p, n, B, d["plan"], S, real, aug, d["workspace"])

    kern_ms, _ = events_ms(kernels, reps)
    pipe_ms, host_ms = events_ms(lambda: pipe.next_batch(real, aug), reps)
    return {"metric": "input_pipeline_batch_pair", "batch": B, "image_size": S, "source": [H, W], "store_images": images,
            "kernels_ms_per_pair": round(kern_ms, 5), "kernels_images_per_s": round(n / kern_ms * 1e3, 1),
            "algorithmic_bytes_per_pair": int(nbytes), "kernels_bytes_per_s": round(nbytes / kern_ms * 1e3, 1),
            "share_of_hbm_peak": round(nbytes / kern_ms * 1e3 / PEAK, 4),
            "pipeline_ms_per_pair": round(pipe_ms, 5), "pipeline_images_per_s": round(n / pipe_ms * 1e3, 1),
            "pipeline_host_ms_per_call": round(host_ms, 5), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--images", type=int, default=2048, help="images in the synthetic store at S = 64 (a quarter of it at S = 128)")
    args = ap.parse_args()
    require_gpu()
    for B, S, H, W, images in ((64, 64, 157, 128, args.images), (32, 128, 314, 256, max(args.images // 4, 64))):
        print(json.dumps(bench_shape(B, S, H, W, images, args.reps)), flush=True)


if __name__ == "__main__":
    main()
