"""Times the manifold metrics (locate_amd/manifold.py, the within kernels of csrc/neighbours.hip) in one session on a synthetic store
at S = 64: `within` (with `covered`) at 4096 x 4096 and 4096 x 65536 in ms and P int-op/s, two yardsticks on the same shapes and
data - `nearest` with k = 1, the same K loop with a heavier epilogue, and ATen: the references dequantised to fp32 in chunks, the
matmul form of the squared distance, compare, sum - and a whole `ManifoldMetrics.evaluate` at the defaults with the generator's share.
The radii are, per reference, the median of its exact distances to 64 of the queries: about half of the pairs count, and pairs sit
on the <= boundary.  How many of the 4096 `hits` the fp32 yardstick gets wrong is counted.  HIP events around `reps` calls after a
warm-up; `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it their range.  One JSON
line at the end.  Usage (GPU box): python tools/bench_manifold.py [--images 65536] [--reps 5] [--rounds 5] [--tiny]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from locate_amd import DeviceImageStore, Generator, ManifoldMetrics, NearestNeighbours, NetConfig, encode_images, get_model, nearest, within  # noqa: E402
from locate_amd import neighbours  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402


def timed(fn, reps, warmup=1):
    """seconds per call: warm-up, then `reps` calls between two HIP events"""
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def aten_within(q, r, radius2, elems, chunk=8192):
    """the yardstick: fp32 copies of `chunk` reference rows at a time, |q|^2 + |r|^2 - 2 q r^T <= radius2, summed both ways"""
    qf = q[0][:, :elems].float()
    qn = q[1].float()[:, None]
    hits = torch.zeros(q[0].shape[0], dtype=torch.int32, device=qf.device)
    covered = []
    for a in range(0, r[0].shape[0], chunk):
        rf = r[0][a:a + chunk, :elems].float()
        inside = qn + r[1][a:a + chunk].float()[None, :] - 2.0 * (qf @ rf.t()) <= radius2[a:a + chunk].float()[None, :]
        hits += inside.sum(1, dtype=torch.int32)
        covered.append(inside.sum(0, dtype=torch.int32))
    return hits, torch.cat(covered)


def median_radii(q, r, elems, sample=64, chunk=8192):
    """int64 [N]: per reference the median (the lower one: an element) of its exact distances to the first `sample` queries - the
    dot products in float64, exact below 2^53"""
    qd = q[0][:sample, :elems].double()
    out = []
    for a in range(0, r[0].shape[0], chunk):
        d = q[1][:sample, None] + r[1][None, a:a + chunk] - 2 * (qd @ r[0][a:a + chunk, :elems].double().t()).round().long()
        out.append(d.sort(dim=0).values[(sample - 1) // 2])
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--images", type=int, default=65536, help="rows of the large reference set")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 generator instead of the full one")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    S, N = args.image_size, args.images
    rb, elems = neighbours.row_bytes(S), 3 * S * S
    Q = 4096
    out = {"image_size": S, "queries": Q, "reference_rows": [Q, N], "row_bytes": rb}

    # ---- a synthetic store at 2 S x 2 S: 4096 random images, repeated with another byte mask per copy ----
    base = np.random.default_rng(0).integers(0, 256, size=(min(N, 4096), 2 * S, 2 * S, 3), dtype=np.uint8)
    images = np.concatenate([base[:min(4096, N - a)] ^ np.uint8((a // 4096) & 255) for a in range(0, N, 4096)])
    store = DeviceImageStore(images, dev)
    del images
    bank = NearestNeighbours(S=S, k=1, images=64, seed=999, device=dev).reference_from_store(store).bank
    x = torch.rand(Q, 3, S, S, device=dev) * 2 - 1
    q = encode_images(x)
    refs = {Q: tuple(t[:Q].contiguous() for t in bank), N: bank}
    radii = {n: median_radii(q, refs[n], elems) for n in refs}

    mm = ManifoldMetrics(S=S, device=dev)          # the defaults: k = 3, 4096 images, 64 latents per forward
    torch.cuda.synchronize()
    t0 = time.time()
    mm.reference_from_store(store)
    torch.cuda.synchronize()
    out["reference_from_store_s"] = time.time() - t0
    out["baseline"] = mm.baseline
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, _ = get_model(Generator(cfg), cfg.glr, dev, cfg)
    gen.batched_spectral_norm = True
    latents = mm.latents(gen.g_in)

    settings = {}
    for n in refs:
        settings["within_n%d" % n] = lambda n=n: within(q, refs[n], radii[n])
        settings["within_hits_only_n%d" % n] = lambda n=n: within(q, refs[n], radii[n], covered=False)
        settings["search_k1_n%d" % n] = lambda n=n: nearest(q, refs[n], k=1)
        settings["aten_n%d" % n] = lambda n=n: aten_within(q, refs[n], radii[n], elems)
    settings["evaluate"] = lambda: mm.evaluate(gen)
    settings["generate"] = lambda: mm._generate(gen, latents)
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, 1 if name in ("aten_n%d" % N, "evaluate", "generate") else args.reps))
    for name, values in rounds.items():
        out[name + "_ms"] = 1e3 * statistics.median(values)
        out[name + "_ms_range"] = [1e3 * min(values), 1e3 * max(values)]
    for n in refs:
        out["within_n%d_peta_ops" % n] = 2.0 * Q * n * rb / (out["within_n%d_ms" % n] * 1e-3) / 1e15
        out["within_over_search_n%d" % n] = out["within_n%d_ms" % n] / out["search_k1_n%d_ms" % n]
        out["aten_over_within_n%d" % n] = out["aten_n%d_ms" % n] / out["within_n%d_ms" % n]
        mine, theirs = within(q, refs[n], radii[n]), aten_within(q, refs[n], radii[n], elems)
        out["share_of_pairs_counted_n%d" % n] = float(mine[0].sum().item()) / (Q * n)
        out["aten_wrong_hits_of_4096_n%d" % n] = int((mine[0] != theirs[0]).sum())
        out["aten_wrong_covered_n%d" % n] = int((mine[1] != theirs[1]).sum())
    out["generate_share_of_evaluate"] = out["generate_ms"] / out["evaluate_ms"]
    out["record"] = mm.evaluate(gen)
    for name in sorted(out):
        print("%-36s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
