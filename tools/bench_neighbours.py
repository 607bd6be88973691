"""Times the exact nearest-neighbour search (locate_amd/neighbours.py, csrc/neighbours.hip) in one session on a synthetic store whose
bank is well past the 256 MiB Infinity Cache (S = 64, N = 65536: 805 MB of codes): the encoder, the bank build, `nearest` at Q = 64
and Q = 4096 in ms and as TB/s of bank read, the whole `evaluate`, and the ATen yardstick on the same data - the bank dequantised to
fp32 in chunks, the matmul form of the squared distance, `topk` per chunk and over the chunks' winners.  HIP events around `reps`
calls after a warm-up; `rounds` rounds with all settings alternating; a figure is the median of the round values, beside it their
range.  One JSON line at the end.  Usage (GPU box): python tools/bench_neighbours.py [--images 65536] [--reps 5] [--rounds 5] [--tiny]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from locate_amd import DeviceImageStore, Generator, NearestNeighbours, NetConfig, encode_images, get_model, nearest  # noqa: E402
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


def aten_nearest(q, bank, k, elems, chunk=8192):
    """the yardstick: fp32 copies of `chunk` bank rows at a time, |q|^2 + |r|^2 - 2 q r^T, topk per chunk, topk of the winners"""
    qf = q[0][:, :elems].float()
    qn = q[1].float()[:, None]
    best_d, best_i = [], []
    for a in range(0, bank[0].shape[0], chunk):
        rf = bank[0][a:a + chunk, :elems].float()
        d = qn + bank[1][a:a + chunk].float()[None, :] - 2.0 * (qf @ rf.t())
        v, i = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        best_d.append(v)
        best_i.append(i + a)
    d, i = torch.cat(best_d, dim=1), torch.cat(best_i, dim=1)
    v, j = torch.topk(d, k, dim=1, largest=False)
    return v, torch.gather(i, 1, j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--images", type=int, default=65536, help="bank rows")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 generator instead of the full one")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    S, N, k = args.image_size, args.images, args.k
    rb, elems = neighbours.row_bytes(S), 3 * S * S
    out = {"image_size": S, "bank_rows": N, "k": k, "row_bytes": rb, "bank_bytes": N * rb}

    # ---- a synthetic store at 2 S x 2 S: 4096 random images, repeated with another byte mask per copy ----
    base = np.random.default_rng(0).integers(0, 256, size=(min(N, 4096), 2 * S, 2 * S, 3), dtype=np.uint8)
    images = np.concatenate([base[:min(4096, N - a)] ^ np.uint8((a // 4096) & 255) for a in range(0, N, 4096)])
    store = DeviceImageStore(images, dev)
    del images
    nn = NearestNeighbours(S=S, k=k, images=64, seed=999, device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    nn.reference_from_store(store)
    torch.cuda.synchronize()
    out["reference_from_store_s"] = time.time() - t0          # first call: includes the tap table and the two baselines
    t0 = time.time()
    nn.reference_from_store(store)
    torch.cuda.synchronize()
    out["reference_from_store_again_s"] = time.time() - t0
    out["bank_build_us_per_image"] = 1e6 * out["reference_from_store_again_s"] / N

    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, _ = get_model(Generator(cfg), cfg.glr, dev, cfg)
    gen.batched_spectral_norm = True

    x = torch.rand(4096, 3, S, S, device=dev) * 2 - 1
    codes = torch.empty(4096, rb, dtype=torch.int8, device=dev)
    norms, flags = torch.empty(4096, dtype=torch.int64, device=dev), torch.empty(4096, dtype=torch.int32, device=dev)
    q = {64: encode_images(x[:64]), 4096: encode_images(x)}
    settings = {
        "encode_4096": lambda: neighbours._encode_into(x, codes, norms, flags),
        "encode_64": lambda: neighbours._encode_into(x[:64], codes[:64], norms[:64], flags[:64]),
        "search_q64": lambda: nearest(q[64], nn.bank, k=k),
        "search_q4096": lambda: nearest(q[4096], nn.bank, k=k),
        "aten_q64": lambda: aten_nearest(q[64], nn.bank, k, elems),
        "aten_q4096": lambda: aten_nearest(q[4096], nn.bank, k, elems),
        "evaluate": lambda: nn.evaluate(gen),
        "generate": lambda: nn.generate(gen),
    }
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, 1 if name == "aten_q4096" else args.reps))
    for name, values in rounds.items():
        out[name + "_ms"] = 1e3 * statistics.median(values)
        out[name + "_ms_range"] = [1e3 * min(values), 1e3 * max(values)]
    out["encode_4096_tb_per_s"] = 4096 * (4 * elems + rb) / (out["encode_4096_ms"] * 1e-3) / 1e12          # fp32 read + codes written
    for Q in (64, 4096):
        out["search_q%d_bank_tb_per_s" % Q] = N * rb / (out["search_q%d_ms" % Q] * 1e-3) / 1e12
        out["search_q%d_tera_ops" % Q] = 2.0 * Q * N * rb / (out["search_q%d_ms" % Q] * 1e-3) / 1e12
        out["aten_over_search_q%d" % Q] = out["aten_q%d_ms" % Q] / out["search_q%d_ms" % Q]
    # how often the fp32 yardstick names another nearest row (its sums pass 2^24)
    _, mine = nearest(q[4096], nn.bank, k=1)
    _, theirs = aten_nearest(q[4096], nn.bank, 1, elems)
    out["aten_top1_disagreements_of_4096"] = int((mine.long() != theirs).sum())
    for name in sorted(out):
        print("%-36s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
