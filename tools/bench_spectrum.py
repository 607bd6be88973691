"""Times the radial power spectrum (locate_amd/spectrum.py, csrc/spectrum.hip) in one session: `radial_spectrum` at 4096 x 3 x 64 x 64
(the fused kernel) and at 256 x 3 x 256 x 256 (the three-launch form), each call behind a fill of 512 MiB that empties L2 and the
256 MiB Infinity Cache, against the ATen yardstick on the same data - `torch.fft.rfft2`, the squared magnitude, `index_add_` into the
bins, in float64 from the squares on, as the kernel does - and the set summary.  Per shape: ms, the achieved fp32 FLOP/s from the
6 S^3 operations per plane the definition needs (2 S^3 in stage 1, 4 S^3 in stage 2) as a share of the 157.3 TFLOP/s fp32 matrix
peak, and the achieved bytes/s from one read of the planes and one write of the spectra as a share of the 8 TB/s HBM peak; these are
shares of a CALL's time (its launches and the gaps between them), not of a kernel's.  How far the yardstick is from the kernel's
result, relative to the bin values, is reported too.  HIP events around single calls; `rounds` rounds with all settings alternating; a
figure is the median of the round values, beside it their range.  One JSON line at the end.
Usage (GPU box): python tools/bench_spectrum.py [--rounds 7] [--small 4096] [--large 256]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from locate_amd import radial_bins, radial_spectrum, spectrum_summary  # noqa: E402
from locate_amd._lib import require_gpu  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
HBM_PEAK = 8.0e12


def timed(fn, flush):
    """seconds of one call, behind a cache-clearing fill"""
    flush.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def aten_spectrum(x, bins, weight, R):
    """the yardstick: rfft2 (complex64), squares and everything after them in float64, index_add_ into the bins"""
    S = x.shape[-1]
    F = torch.fft.rfft2(x)
    p = (F.real.double().square() + F.imag.double().square()) * weight / float(S) ** 4
    out = torch.zeros(x.shape[:-2] + (R,), dtype=torch.float64, device=x.device)
    return out.index_add_(-1, bins, p.flatten(-2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small", type=int, default=4096, help="images at 64 x 64")
    ap.add_argument("--large", type=int, default=256, help="images at 256 x 256")
    args = ap.parse_args()
    require_gpu()
    dev = torch.device("cuda:0")
    flush = torch.empty(512 << 18, device=dev)          # 512 MiB of fp32
    out, settings, data = {}, {}, {}
    for S, n in ((64, args.small), (256, args.large)):
        x = torch.tanh(torch.randn(n, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(S)))
        table, mult = radial_bins(S)
        H = S // 2
        k = torch.arange(H + 1)
        weight = torch.where((k == 0) | (k == H), 1.0, 2.0).double()[None, :].repeat(S, 1).to(dev)
        bins, R = torch.from_numpy(table).long().flatten().to(dev), int(mult.size)
        data[S] = (x, bins, weight, R)
        tag = "%dx3x%dx%d" % (n, S, S)
        settings["spectrum_" + tag] = lambda x=x: radial_spectrum(x)
        settings["aten_" + tag] = lambda x=x, bins=bins, weight=weight, R=R: aten_spectrum(x, bins, weight, R)
        spectra = radial_spectrum(x)
        settings["summary_" + tag] = lambda spectra=spectra: spectrum_summary(spectra)
        theirs = aten_spectrum(x, bins, weight, R)
        out["aten_minus_kernel_relative_max_" + tag] = float(((theirs - spectra).abs() / spectra).max())
    for fn in settings.values():          # every shape once before anything is timed
        fn()
    rounds = {name: [] for name in settings}
    for _ in range(args.rounds):
        for name, fn in settings.items():
            rounds[name].append(timed(fn, flush))
    for name, values in rounds.items():
        out[name + "_ms"] = 1e3 * statistics.median(values)
        out[name + "_ms_range"] = [1e3 * min(values), 1e3 * max(values)]
    for S, n in ((64, args.small), (256, args.large)):
        tag = "%dx3x%dx%d" % (n, S, S)
        seconds = out["spectrum_%s_ms" % tag] * 1e-3
        flops, nbytes = 3.0 * n * 6 * S ** 3, 3.0 * n * (4 * S * S + 8 * data[S][3])
        out["fp32_matrix_tflops_" + tag] = flops / seconds / 1e12
        out["fp32_matrix_share_" + tag] = flops / seconds / FP32_MATRIX_PEAK
        out["hbm_tb_per_s_" + tag] = nbytes / seconds / 1e12
        out["hbm_share_" + tag] = nbytes / seconds / HBM_PEAK
        out["bound_by_" + tag] = "fp32 matrix rate" if flops / FP32_MATRIX_PEAK > nbytes / HBM_PEAK else "HBM"
        out["aten_over_kernel_" + tag] = out["aten_%s_ms" % tag] / out["spectrum_%s_ms" % tag]
    for name in sorted(out):
        print("%-52s %s" % (name, out[name]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
