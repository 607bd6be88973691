"""Times the format audit (locate_amd/formats.py, csrc/formats.hip) on the benchmark networks (64 x 64, full width, batch 64):
  (a) the audit of ALL weights as one list (eight views per call), with HIP events around the whole list, against the statistics'
      two launches (`locate_stats_reduce`) over the same tensors - the bandwidth yardstick, at one read of every element where the
      audit takes two and a few hundred operations per element where the statistics take three;
  (b) an audited EAGER iteration (`with audit.iteration(i)`) against the plain eager iteration, wall clock around a synchronised loop;
  (c) from (b), what `formats_every=256` adds to an eager iteration on average.
Then one audited iteration's table: `snr_db` and the flushed fraction per format for the generator's widest stage and the
discriminator's 5 x 5 layers.  One JSON line at the end.
Usage (GPU box): python tools/bench_formats.py [--reps 20] [--rounds 3] [--train-iters 6] [--tiny]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from locate_amd import Discriminator, FormatAudit, Generator, NetConfig, TrainStep, get_model  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402


def each_launch_ms(fn, reps, warmup=3):
    """milliseconds of every one of `reps` calls, each between two HIP events of its own"""
    for _ in range(warmup):
        fn()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in pairs]


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--tiny", action="store_true", help="the base-width-1 networks (a rehearsal: measures overheads only)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="audit / yardstick rounds, alternating")
    ap.add_argument("--train-iters", type=int, default=6, help="eager iterations per timed loop")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    S, B = args.image_size, 64
    cfg = NetConfig(image_size=S, base_feature_factor=1) if args.tiny else NetConfig(image_size=S)
    torch.manual_seed(cfg.seed)
    gen, gen_opt = get_model(Generator(cfg), cfg.glr, dev, cfg)
    dis, dis_opt = get_model(Discriminator(cfg), cfg.dlr, dev, cfg)
    gen.batched_spectral_norm = dis.batched_spectral_norm = True
    step = TrainStep(gen, dis, gen_opt, dis_opt, minibatches=1)
    lat, x, y = (torch.randn(B, gen.g_in, device=dev), torch.randn(B, 3, S, S, device=dev).clamp(-1, 1),
                 torch.randn(B, 3, S, S, device=dev).clamp(-1, 1))
    for _ in range(3):
        step(lat, x, y)
    audit = FormatAudit(gen, dis, capacity=4)
    out = {"image_size": S, "networks": "tiny" if args.tiny else "full", "layers": len(audit.layers), "entries": len(audit.entries()),
           "reps": args.reps, "rounds": args.rounds}
    med = statistics.median

    # (a) all weights as one list
    from locate_amd.formats import MAX_VIEWS, SLOT_WORDS, _Workspaces, _audit, _view
    from locate_amd.stats import _device_table as stats_table, _launch as stats_launch
    weights = [w.detach() for _, w in audit.layers]
    elements = sum(w.numel() for w in weights)
    views = [_view(w.view(w.shape[0], -1), 2) + (2,) for w in weights]
    rows = torch.zeros(len(views), SLOT_WORDS, dtype=torch.int64, device=dev)
    spaces = _Workspaces()

    def audit_weights():
        for at in range(0, len(views), MAX_VIEWS):
            part = views[at:at + MAX_VIEWS]
            _audit(part, list(range(at, at + len(part))), rows, spaces)
    s_table = stats_table(weights)
    s_row = torch.zeros(1 + len(weights), 2, dtype=torch.int64, device=dev)
    a_rounds, s_rounds = [], []
    for _ in range(args.rounds):          # alternating, so that a drift of the machine hits both alike
        a_rounds.append(med(each_launch_ms(audit_weights, args.reps)))
        s_rounds.append(med(each_launch_ms(lambda: stats_launch(s_table, s_row), args.reps)))
    t0 = time.perf_counter()
    for _ in range(10):
        audit_weights()
    out["weights_audit_host_us"] = 1e5 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    out.update(weight_elements=elements, weight_bytes=4 * elements, weights_audit_calls=-(-len(views) // MAX_VIEWS),
               weights_audit_us_rounds=[1e3 * t for t in a_rounds], weights_audit_us=1e3 * med(a_rounds),
               weights_stats_us_rounds=[1e3 * t for t in s_rounds], weights_stats_us=1e3 * med(s_rounds),
               weights_audit_over_stats=med(a_rounds) / med(s_rounds),
               weights_audit_tb_per_s=8 * elements / (med(a_rounds) * 1e-3) / 1e12, weights_stats_tb_per_s=4 * elements / (med(s_rounds) * 1e-3) / 1e12)

    # (b) an audited eager iteration against the plain one
    def plain(i):
        step(lat, x, y)

    def audited(i):
        with audit.iteration(i):
            step(lat, x, y)
    plain_ms, audited_ms = [], []
    for _ in range(args.rounds):
        plain_ms.append(wall_ms(plain, args.train_iters))
        audited_ms.append(wall_ms(audited, min(args.train_iters, audit.capacity)))
        audit.flush()
        audit.clear()
    out.update(eager_iteration_ms_rounds=plain_ms, eager_iteration_ms=med(plain_ms), audited_iteration_ms_rounds=audited_ms,
               audited_iteration_ms=med(audited_ms), audited_over_plain=med(audited_ms) / med(plain_ms))
    # (c) every 256th iteration audited
    extra = med(audited_ms) - med(plain_ms)
    out["formats_every_256_extra_ms_per_iteration"] = extra / 256
    out["formats_every_256_share_of_eager_iteration"] = extra / 256 / med(plain_ms)

    # the table: one audited iteration
    with audit.iteration(0):
        step(lat, x, y)
    (row,) = audit.flush()
    report = audit.report()[-1]
    out["unmatched"] = audit.unmatched
    out["audit_calls_per_iteration"] = int(row["calls"].sum()) // 2
    by_weight = {"%s/%s" % (tag, n): m for tag, net in (("G", gen), ("D", dis)) for n, m in
                 ((name + ".weight_bar", mod) for name, mod in net.named_modules() if hasattr(mod, "weight_bar"))}
    convs = [(n, by_weight[n]) for n, _ in audit.layers if n in by_weight and isinstance(by_weight[n], (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    widest = max((n for n, m in convs if n.startswith("G/") and m.kernel_size != (1, 1)), key=lambda n: by_weight[n].weight_bar.shape[0] * by_weight[n].weight_bar.shape[1])
    picked = [widest] + [n for n, m in convs if n.startswith("D/") and tuple(m.kernel_size) == (5, 5)]
    table = []
    print("%-58s %-9s %10s | %s" % ("layer", "role", "elements", "  ".join("%-22s" % f for f in report["formats"])))
    for name in picked:
        for role in ("fwd.x", "fwd.w", "dgrad.gy", "wgrad.gy"):
            s = audit.slot(name, role)
            if not row["calls"][s]:
                continue
            cells = [(float(report["snr_db"][s, f]), float(report["flushed"][s, f])) for f in range(5)]
            table.append({"layer": name, "role": role, "shape": list(by_weight[name].weight_bar.shape), "calls": int(row["calls"][s]),
                          "elements": int(row["n"][s]), "snr_db": [c[0] for c in cells], "flushed": [c[1] for c in cells]})
            print("%-58s %-9s %10d | %s" % (name, role, int(row["n"][s]), "  ".join("%6.1f dB %9.2e fl." % c for c in cells)))
    out["table"] = table
    active = row["calls"] > 0
    out["median_snr_db_by_role"] = {role: [float(np.nanmedian(report["snr_db"][active & np.array([r == role for _, r in audit.entries()])][:, f]))
                                           for f in range(5)] for role in ("fwd.x", "fwd.w", "dgrad.gy", "dgrad.w", "wgrad.x", "wgrad.gy")}
    for k in sorted(out):
        if k != "table":
            print("%-48s %s" % (k, out[k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
