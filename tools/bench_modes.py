"""Times the binned mode coverage (locate_amd/modes.py, csrc/modes.hip) in one session at S = 64, K = 128:
  * the centroid update - `locate_nn_group_sums` + `locate_nn_centroids` on a prepared grouping - at M = 4096, 16384 and 65536 rows in
    microseconds and TB/s over M row_bytes, beside two yardsticks on the same rows: a plain device-to-device copy of them (the stream
    ceiling, counting the bytes read) and ATen - `index_add_` into an int32 [K, row_bytes] from the rows cast to int32 in chunks;
    also `group_sums` + `centroids` as Python calls them, with the sort of the labels and the allocations;
  * one full Lloyd round, split into assignment (`nearest`, k = 1) and update;
  * a whole `BinnedModes.evaluate` at the defaults with the generator's share, and `reference_from_store`.
The rows are smooth prototypes plus noise, their cluster sizes skewed (a geometric law: the largest holds about a third); the labels
are a real assignment of them to the first K prototypes, so the groups are as unequal as the clusters and some are empty.  Every
timed call runs behind a fill of a buffer larger than the Infinity Cache; HIP events around the call; `rounds` rounds with all
settings alternating; a figure is the median of the round values, beside it their range.  One JSON line at the end.  Usage (GPU box): python tools/bench_modes.py [--reps 5] [--rounds 5] [--tiny] [--no-evaluate]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from locate_amd import BinnedModes, DeviceImageStore, Generator, NetConfig, centroids, get_model, group_sums, nearest  # noqa: E402
from locate_amd import neighbours  # noqa: E402
from locate_amd._lib import check, lib, require_gpu  # noqa: E402

FILL_BYTES = 512 << 20          # twice the Infinity Cache


def timed(fn, reps, fill):
    """seconds per call: a warm-up, then `reps` calls, each behind a cache-clearing fill and between two HIP events of its own"""
    fn()
    total = 0.0
    for i in range(reps):
        fill.fill_(i & 127)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1)
    return total / reps * 1e-3


def skewed_rows(M, rb, elems, dev, seed):
    """(codes int8 [M, rb], their norms, the prototypes' codes int8 [256, rb]) on the device: 256 smooth prototypes plus noise of
    +-6, prototype c drawn with probability ~ 0.67^c"""
    rng = torch.Generator(device=dev)
    rng.manual_seed(seed)
    t = torch.linspace(0, 1, elems, device=dev)
    freq = 1 + torch.arange(256, device=dev, dtype=torch.float32)[:, None]
    proto = (90 * torch.sin(6.2831853 * freq * t[None, :] / 16 + freq)).round()
    which = torch.empty(M, device=dev).exponential_(0.4, generator=rng).long().clamp_(max=255)
    codes = torch.zeros(M, rb, dtype=torch.int8, device=dev)
    for a in range(0, M, 8192):
        part = proto[which[a:a + 8192]] + torch.randint(-6, 7, (min(8192, M - a), elems), device=dev, generator=rng)
        codes[a:a + 8192, :elems] = part.clamp_(-128, 127).to(torch.int8)
    clean = torch.zeros(256, rb, dtype=torch.int8, device=dev)
    clean[:, :elems] = proto.to(torch.int8)
    return codes, square_norms(codes), clean


def square_norms(codes):
    return torch.cat([(codes[a:a + 8192].to(torch.int32) ** 2).sum(1, dtype=torch.int64) for a in range(0, codes.shape[0], 8192)])


def aten_sums(codes, labels, K, chunk=4096):
    """the yardstick: index_add_ of int32 copies of `chunk` rows at a time (every label is >= 0 here)"""
    out = torch.zeros(K, codes.shape[1], dtype=torch.int32, device=codes.device)
    for a in range(0, codes.shape[0], chunk):
        out.index_add_(0, labels[a:a + chunk], codes[a:a + chunk].to(torch.int32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 generator instead of the full one")
    ap.add_argument("--no-evaluate", action="store_true", help="the kernels only: no store, no generator")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    L = lib()
    S, K = args.image_size, args.bins
    rb, elems = neighbours.row_bytes(S), 3 * S * S
    sizes = (4096, 16384, 65536)
    out = {"image_size": S, "bins": K, "row_bytes": rb, "rows": list(sizes)}
    fill = torch.empty(FILL_BYTES, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731

    settings, keep = {}, {}
    for M in sizes:
        codes, norms, clean = skewed_rows(M, rb, elems, dev, seed=M)
        x = (codes, norms, torch.zeros(M, dtype=torch.int32, device=dev))
        centres = (clean[:K].contiguous(), square_norms(clean[:K]), torch.zeros(K, dtype=torch.int32, device=dev))
        labels = nearest(x, centres, k=1)[1][:, 0].contiguous()
        ranked, order = torch.sort(labels, stable=True)
        starts = torch.searchsorted(ranked, torch.arange(K + 1, dtype=torch.int32, device=dev)).to(torch.int32)
        order = order.to(torch.int32)
        counts = (starts[1:] - starts[:-1]).cpu()
        out["largest_group_share_m%d" % M] = float(counts.max()) / M
        out["median_group_m%d" % M] = int(counts.median())
        out["empty_groups_m%d" % M] = int((counts == 0).sum())
        sums = torch.empty(K, rb, dtype=torch.int32, device=dev)
        ws = torch.empty(L.locate_nn_group_sums_workspace_bytes(M, K, rb) // 4, dtype=torch.int32, device=dev)
        new, nn, moved = torch.empty_like(centres[0]), torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
        copy = torch.empty_like(codes)
        long_labels = labels.long()
        keep[M] = (codes, x, centres, labels, order, starts, sums, ws, new, nn, moved, copy, long_labels)

        def kernels(M=M, codes=codes, order=order, starts=starts, sums=sums, ws=ws, centres=centres, new=new, nn=nn, moved=moved):
            check(L.locate_nn_group_sums(ptr(codes), M, rb, ptr(order), M, ptr(starts), K, ptr(sums), ptr(ws), stream), "locate_nn_group_sums")
            check(L.locate_nn_centroids(ptr(sums), ptr(starts), K, M, rb, ptr(centres[0]), ptr(new), ptr(nn), ptr(moved), stream), "locate_nn_centroids")

        def sums_only(M=M, codes=codes, order=order, starts=starts, sums=sums, ws=ws):
            check(L.locate_nn_group_sums(ptr(codes), M, rb, ptr(order), M, ptr(starts), K, ptr(sums), ptr(ws), stream), "locate_nn_group_sums")

        def update(codes=codes, labels=labels, centres=centres, M=M):
            s, _, st = group_sums(codes, labels, K)
            return centroids(s, st, M, centres[0])

        settings["update_kernels_m%d" % M] = kernels
        settings["group_sums_m%d" % M] = sums_only
        settings["update_python_m%d" % M] = update
        settings["copy_m%d" % M] = lambda codes=codes, copy=copy: copy.copy_(codes)
        settings["aten_index_add_m%d" % M] = lambda codes=codes, long_labels=long_labels: aten_sums(codes, long_labels, K)
        settings["assignment_m%d" % M] = lambda x=x, centres=centres: nearest(x, centres, k=1)
        # the kernels against the yardstick, once
        kernels()
        assert torch.equal(sums, aten_sums(codes, long_labels, K)), "group sums differ from index_add_"
        n = (starts[1:] - starts[:-1]).long()[:, None]
        mean = torch.div(2 * sums.long() + n, 2 * n.clamp(min=1), rounding_mode="floor")
        filled = n[:, 0] > 0
        assert torch.equal(new[filled].long(), mean[filled]), "centroids differ from the floor division"

    if not args.no_evaluate:
        # ---- a store of prototypes plus noise at S x S, enough for the defaults' baseline ----
        rng = np.random.default_rng(0)
        n = 16384 + 4096
        y, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        proto = np.stack([np.stack([128 + 80 * np.cos((1 + k % 8) * np.pi * y / S + k) * np.cos((1 + k // 8) * np.pi * xx / S + c) for c in range(3)], axis=2)
                          for k in range(64)])
        which = np.minimum(rng.geometric(0.08, size=n) - 1, 63)
        images = np.empty((n, S, S, 3), dtype=np.uint8)
        for a in range(0, n, 2048):
            images[a:a + 2048] = np.clip(proto[which[a:a + 2048]] + rng.integers(-12, 13, size=(min(2048, n - a), S, S, 3)), 0, 255)
        store = DeviceImageStore(images, dev)
        del images
        bm = BinnedModes(S=S, bins=K, device=dev)          # the defaults: 16384 images, 4096 samples, 10 rounds
        torch.cuda.synchronize()
        t0 = time.time()
        bm.reference_from_store(store)
        torch.cuda.synchronize()
        out["reference_from_store_s"] = time.time() - t0
        out["converged_at"] = bm.converged_at
        out["baseline"] = {k: v for k, v in bm.baseline.items() if k != "fake_counts"}
        cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
        torch.manual_seed(cfg.seed)
        gen, _ = get_model(Generator(cfg), cfg.glr, dev, cfg)
        gen.batched_spectral_norm = True
        latents = bm.latents(gen.g_in)
        settings["evaluate"] = lambda: bm.evaluate(gen)
        settings["generate"] = lambda: bm._generate(gen, latents)

    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, 1 if name in ("evaluate", "generate") or name.startswith("aten") else args.reps, fill))
    for name, values in rounds.items():
        out[name + "_us"] = 1e6 * statistics.median(values)
        out[name + "_us_range"] = [1e6 * min(values), 1e6 * max(values)]
    for M in sizes:
        size = float(M) * rb
        for name in ("update_kernels", "group_sums", "update_python", "copy", "aten_index_add"):
            out["%s_m%d_tb_per_s" % (name, M)] = size / (out["%s_m%d_us" % (name, M)] * 1e-6) / 1e12
        out["update_over_copy_rate_m%d" % M] = out["copy_m%d_us" % M] / out["update_kernels_m%d_us" % M]
        out["aten_over_update_m%d" % M] = out["aten_index_add_m%d_us" % M] / out["update_kernels_m%d_us" % M]
        out["lloyd_round_m%d_us" % M] = out["assignment_m%d_us" % M] + out["update_python_m%d_us" % M]
    if not args.no_evaluate:
        out["generate_share_of_evaluate"] = out["generate_us"] / out["evaluate_us"]
        record = bm.evaluate(gen)
        out["record"] = {k: record[k] for k in ("bins", "images", "samples", "ndb", "ndb_over_k", "js", "missing", "nonfinite")}
    for name in sorted(out):
        print("%-36s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
