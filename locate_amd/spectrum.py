"""Measuring a run: the radial (azimuthally averaged) power spectrum of generated images against real ones - the instrument for
the spectral artefacts of up-convolutions (Durall et al. 2020, "Watch your Up-Convolution"; Odena et al. 2016): an excess at the
high end of the spectrum and a checkerboard at (Nyquist, Nyquist).  The reference has no metric at all; this is an addition.

Per plane x fp32 [S, S], S in {32, 64, 128, 256}, H = S / 2 (csrc/spectrum.hip through the C ABI, include/locate_hip.h):
  1. the real-input DFT in two fp32 matrix products against the tables of `dft_tables` (a window, if any, folded in):
     Y[a][k], a = 0 .. S - 1, k = 0 .. H;
  2. the power (Yr^2 + Yi^2) m[k] / S^4 in float64, m = 2 for the columns whose Hermitian twin is not computed: the powers of a
     plane add up to the mean of its (windowed) squares, and a constant plane c has c^2 at frequency 0;
  3. the SUM of the powers per radial bin of `radial_bins`: float64 [R], the same bits from call to call.  The corners beyond the
     axis Nyquist are kept - the checkerboard lives in the last bin, which holds (H, H) alone.
A set's summary (`spectrum_summary`) is per channel and bin the sum and the sum of squares of spectrum / multiplicity - the
azimuthal average - over the planes whose spectrum is finite, and the number of those that are not.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import math

import numpy as np
import torch

from .sampling import FixedLatents, _gpu, _ptr, _stream, batches, plain_batches

SIZES = (32, 64, 128, 256)
WINDOWS = ("none", "hann")
_WORKSPACE_BYTES = 256 << 20          # planes of 128 and 256 go through the kernels this much workspace at a time


def _size(S):
    if isinstance(S, bool) or int(S) != S or int(S) not in SIZES:
        raise ValueError("the spectrum takes S in %s, got %r" % (SIZES, S))
    return int(S)


def radial_bins(S):
    """(bins int32 [S, S/2 + 1], multiplicity int64 [R]).  Frequency (a, k) has fy = a for a <= S/2, else a - S; its bin is the
    smallest r with 4 (fy^2 + k^2) < (2 r + 1)^2 - the rounded radius, in integers.  multiplicity[r] counts the frequencies of
    the FULL S x S spectrum in bin r (columns 1 .. S/2 - 1 stand for two); they add up to S^2."""
    S = _size(S)
    H = S // 2
    a = np.arange(S, dtype=np.int64)
    fy = np.where(a <= H, a, a - S)
    k = np.arange(H + 1, dtype=np.int64)
    d = 4 * (fy[:, None] ** 2 + k[None, :] ** 2)
    r = ((np.sqrt(d.astype(np.float64)) + 1) // 2).astype(np.int64)
    for _ in range(2):          # the float square root may be one off; settle it in integers
        r = np.where((r > 0) & ((2 * r - 1) ** 2 > d), r - 1, r)
        r = np.where((2 * r + 1) ** 2 <= d, r + 1, r)
    assert ((d < (2 * r + 1) ** 2) & ((r == 0) | ((2 * r - 1) ** 2 <= d))).all()
    weight = np.where((k == 0) | (k == H), 1, 2)[None, :].repeat(S, 0)
    mult = np.bincount(r.ravel(), weights=weight.ravel(), minlength=int(r.max()) + 1).astype(np.int64)
    return r.astype(np.int32), mult


def bin_slots(bins):
    """The bin table in the form the kernels read: (slot int32 [S, S/2 + 1], start int32 [R + 1]).  slot[a][k] is the place of
    (a, k) in the list of all frequencies ordered by (bin, a, k); bin r is list[start[r] : start[r + 1]]."""
    bins = np.asarray(bins)
    order = np.argsort(bins.ravel(), kind="stable")
    slot = np.empty(order.size, dtype=np.int32)
    slot[order] = np.arange(order.size, dtype=np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(bins.ravel()))]).astype(np.int32)
    return slot.reshape(bins.shape), start


def window_weights(S, window="none"):
    """float64 [S]: ones, or the periodic Hann window scaled to sum w^2 = S (white noise keeps its level)."""
    S = _size(S)
    if window not in WINDOWS:
        raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
    if window == "none":
        return np.ones(S)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(S) / S)
    return w * np.sqrt(S / (w * w).sum())


def dft_tables(S, window="none"):
    """(C, Sn) fp32 [S, S]: cos and sin of 2 pi ((k j) mod S) / S times w[j], made in float64 and rounded once.  Where (k j) mod S
    is a multiple of S / 4 the factor is the exact 0 or +-1."""
    S = _size(S)
    w = window_weights(S, window)
    j = np.arange(S, dtype=np.int64)
    kj = np.outer(j, j) % S
    q = S // 4
    ang = 2 * np.pi * kj / S
    c, s = np.cos(ang), np.sin(ang)
    exact = kj % q == 0
    quarter = (kj[exact] // q) % 4
    c[exact] = np.array([1.0, 0.0, -1.0, 0.0])[quarter]
    s[exact] = np.array([0.0, 1.0, 0.0, -1.0])[quarter]
    return (c * w[None, :]).astype(np.float32), (s * w[None, :]).astype(np.float32)


_TABLES = {}
_SIZES_BY_BINS = {}


def _sizes_by_bins():
    """{R: S}: 24, 46, 92, 182 bins tell the four sizes apart (made once)"""
    if not _SIZES_BY_BINS:
        _SIZES_BY_BINS.update({int(radial_bins(S)[1].size): S for S in SIZES})
    return _SIZES_BY_BINS


def device_tables(S, window, device):
    """{"cos", "sin", "slot", "start", "count", "R"} on `device`, made once per (S, window, device)."""
    key = (_size(S), window, str(device))
    if key not in _TABLES:
        c, s = dft_tables(S, window)
        bins, mult = radial_bins(S)
        slot, start = bin_slots(bins)
        _TABLES[key] = {"cos": torch.from_numpy(c).to(device), "sin": torch.from_numpy(s).to(device), "slot": torch.from_numpy(slot).to(device),
                        "start": torch.from_numpy(start).to(device), "count": torch.from_numpy(mult.astype(np.float64)).to(device), "R": int(mult.size)}
    return _TABLES[key]


def radial_spectrum(x, window="none"):
    """x: fp32 [n, 3, S, S] on the GPU (any [..., S, S]) -> float64 [n, 3, R] on the device: per plane the power sum of every
    radial bin.  No host read.  A plane's result depends on its values alone: not on the other planes of the call, nor on the
    buffer's alignment."""
    from ._lib import check, lib
    if window not in WINDOWS:
        raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
    x = _gpu(x, "x")
    if x.dim() < 2 or x.shape[-1] != x.shape[-2] or x.numel() == 0:
        raise ValueError("x must be [..., S, S], got %s" % (tuple(x.shape),))
    S = _size(x.shape[-1])
    L = lib()
    t = device_tables(S, window, x.device)
    planes = x.numel() // (S * S)
    out = torch.empty(tuple(x.shape[:-2]) + (t["R"],), dtype=torch.float64, device=x.device)
    flat, rows = x.reshape(planes, S, S), out.reshape(planes, t["R"])
    per_plane = L.locate_spectrum_workspace_bytes(1, S)
    step = planes if per_plane == 0 else max(1, _WORKSPACE_BYTES // per_plane)
    if per_plane and x.data_ptr() % 16:
        flat = flat.clone()          # the staged kernels load 16 bytes per lane; a fresh allocation is aligned
    ws = None
    for at in range(0, planes, step):
        m = min(step, planes - at)
        if per_plane and ws is None:
            ws = torch.empty(L.locate_spectrum_workspace_bytes(m, S) // 8, dtype=torch.float64, device=x.device)
        check(L.locate_spectrum_planes(_ptr(flat[at:at + m]), m, S, _ptr(t["cos"]), _ptr(t["sin"]), _ptr(t["slot"]), _ptr(t["start"]), t["R"],
                                       _ptr(rows[at:at + m]), _ptr(ws) if ws is not None else None, _stream()), "locate_spectrum_planes")
    return out


def spectrum_summary(spectra):
    """spectra: float64 [n, C, R] on the GPU (R tells the size: 24, 46, 92, 182 bins at 32, 64, 128, 256).  Per channel and bin, over the planes in ascending order and with
    one fixed summation order: {"sum", "sumsq"}: float64 [C, R] of spectrum / multiplicity over the planes whose spectrum is
    finite; "nonfinite": int32 [C], the planes that hold a NaN or an Inf; "planes": n.  Device tensors; nothing is read here."""
    from ._lib import check, lib
    spectra = _gpu(spectra, "spectra", torch.float64)
    sizes = _sizes_by_bins()
    if spectra.dim() != 3 or spectra.shape[2] not in sizes or spectra.shape[0] < 1 or spectra.shape[1] < 1:
        raise ValueError("spectra must be [n, C, R] with R in %s, got %s" % (sorted(sizes), tuple(spectra.shape)))
    R = int(spectra.shape[2])
    S = sizes[R]
    L = lib()
    n, C = int(spectra.shape[0]), int(spectra.shape[1])
    sums = torch.empty(2, C, R, dtype=torch.float64, device=spectra.device)
    bad = torch.empty(C, dtype=torch.int32, device=spectra.device)
    ws = torch.empty(L.locate_spectrum_summary_workspace_bytes(n * C) // 4, dtype=torch.int32, device=spectra.device)
    check(L.locate_spectrum_summary(_ptr(spectra), n, C, R, _ptr(device_tables(S, "none", spectra.device)["count"]), _ptr(sums), _ptr(bad), _ptr(ws),
                                    _stream()), "locate_spectrum_summary")
    return {"sum": sums[0], "sumsq": sums[1], "nonfinite": bad, "planes": n}


def summary_means(summary):
    """The host side of a summary: ([C][R] means over the finite planes, the number of planes that are not finite)."""
    bad = summary["nonfinite"].cpu().tolist()
    sums = summary["sum"].cpu().tolist()          # small: C R doubles
    return [[v / (summary["planes"] - b) if summary["planes"] > b else float("nan") for v in row] for row, b in zip(sums, bad)], int(sum(bad))


def gap_record(real, fake, S):
    """From two sets' [C][R] means: {"real", "fake", "gap_db" = 10 log10(fake / real) [C][R], "high_gap_db" [C]: the mean of gap_db
    over the bins r >= S / 4 (the upper half of the axis band and the corners), "max_abs_gap_db"}.  A bin that is zero or not
    finite in either set gives a gap that is not finite; it is not guarded."""
    def gap(f, r):
        if not (math.isfinite(f) and math.isfinite(r)) or f < 0 or r < 0 or (f == 0 and r == 0):
            return float("nan")
        if r == 0:
            return float("inf")
        if f == 0:
            return float("-inf")
        return 10.0 * math.log10(f / r)
    gaps = [[gap(f, r) for f, r in zip(frow, rrow)] for frow, rrow in zip(fake, real)]
    first = int(S) // 4
    return {"real": [list(row) for row in real], "fake": [list(row) for row in fake], "gap_db": gaps,
            "high_gap_db": [sum(row[first:]) / len(row[first:]) for row in gaps], "max_abs_gap_db": max(abs(v) for row in gaps for v in row)}


class RadialSpectrum(FixedLatents):
    """The radial power spectrum of a candidate image set against a cached real set, both of `images` fp32 [3, S, S] images.

    A record (`between`, `distance`, `evaluate`):
      "bins": R; "images": the candidate's images; "window";
      "real", "fake": [3][R], per channel the mean azimuthal average (bin sum / multiplicity) over the set's finite planes;
      "gap_db": 10 log10(fake / real) [3][R]; "high_gap_db": [3], its mean over the bins r >= S / 4; "max_abs_gap_db";
      "nonfinite": the candidate's planes that hold a NaN or an Inf (left out of the means);
      "baseline": the same gap keys for a second, disjoint real set against the first, or None - what two samples of the SAME
      distribution give at this sample size: a gap counts where it clearly exceeds the baseline's.

    `latents` [N, g_in] is drawn on the device on first use, from a generator seeded `seed + 3`.  `chunk` is part of the metric's
    definition as it is of `SlicedWasserstein`'s: InPlaceNorm takes its statistics over the batch it sees.  Construction needs no
    GPU.  Under data parallelism only rank 0 should evaluate."""

    latent_seed = 3

    def __init__(self, S, images=4096, seed=999, chunk=64, window="none", device="cuda"):
        self.S = _size(S)
        if window not in WINDOWS:
            raise ValueError("window must be one of %s, got %r" % (WINDOWS, window))
        self.images, self.seed, self.chunk, self.window = int(images), int(seed), int(chunk), window
        if min(self.images, self.chunk) < 1:
            raise ValueError("images and chunk must be >= 1")
        FixedLatents.__init__(self, device)
        self.bins = int(radial_bins(self.S)[1].size)
        self.baseline = None
        self._reference = None

    def spectra(self, batches, expect=None):
        """float64 [n, 3, R]: the per-plane spectra of one [n, 3, S, S] tensor or an iterable of such batches."""
        if torch.is_tensor(batches):
            batches = (batches,)
        parts = []
        for x in batches:
            x = _gpu(x, "images")
            if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.S, self.S):
                raise ValueError("images must be [n, 3, %d, %d], got %s" % (self.S, self.S, tuple(x.shape)))
            parts.append(radial_spectrum(x, self.window))
        n = sum(p.shape[0] for p in parts)
        if n < 1 or (expect is not None and n != expect):
            raise ValueError("%d images given, this metric was built for %d" % (n, self.images if expect is None else expect))
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def _means(self, batches, expect=None):
        return summary_means(spectrum_summary(self.spectra(batches, expect)))

    def _record(self, real, fake, images, nonfinite):
        value = {"bins": self.bins, "images": int(images), "window": self.window}
        value.update(gap_record(real, fake, self.S))
        value["nonfinite"] = int(nonfinite)
        value["baseline"] = None if self.baseline is None else dict(self.baseline)
        return value

    def set_reference(self, batches, baseline=None):
        """batches: one [N, 3, S, S] tensor or an iterable of batches summing to N - the real set, whose means are kept.
        baseline: a second such set, or None."""
        self._reference = self._means(batches, self.images)[0]
        self.baseline = None
        if baseline is not None:
            means, bad = self._means(baseline, self.images)
            self.baseline = dict(gap_record(self._reference, means, self.S), nonfinite=bad)
        return self

    @property
    def has_reference(self):
        return self._reference is not None

    def _need_reference(self):
        if self._reference is None:
            raise RuntimeError("set_reference() first")

    def between(self, a, b):
        """The record of b (as "fake") against a (as "real"), nothing cached: radial_spectrum, spectrum_summary, gap_record."""
        real, _ = self._means(a)
        spectra = self.spectra(b)
        fake, bad = summary_means(spectrum_summary(spectra))
        return self._record(real, fake, spectra.shape[0], bad)

    def distance(self, batches):
        """The record of the candidate set (N images) against the cached real set."""
        self._need_reference()
        fake, bad = self._means(batches, self.images)
        return self._record(self._reference, fake, self.images, bad)

    def reference_from_pipeline(self, pipeline):
        """set_reference() with N images of the plain chain: the first output of `InputPipeline.next_batch()`, from a pipeline of
        this metric's own over the same store, seeded seed + 2 - the training pipeline's shuffle is not advanced.  The N images that
        follow in the same pass - so disjoint from the first - become the baseline when the store holds at least 2 N images and the
        pass that many in whole batches; else the baseline is None."""
        batch = min(pipeline.batch, self.images)
        second = len(pipeline.store) >= 2 * self.images and -(-2 * self.images // batch) <= len(pipeline.store) // batch
        sets, held = [[], []], 0
        for real in plain_batches(pipeline, self.S, self.images, self.seed, (2 if second else 1) * self.images):
            cut = max(0, min(real.shape[0], self.images - held))          # the part that still belongs to the first set
            if cut:
                sets[0].append(radial_spectrum(real[:cut], self.window))
            if cut < real.shape[0]:
                sets[1].append(radial_spectrum(real[cut:], self.window))
            held += real.shape[0]
        means = [summary_means(spectrum_summary(torch.cat(s))) for s in sets if s]
        self._reference = means[0][0]
        self.baseline = dict(gap_record(self._reference, means[1][0], self.S), nonfinite=means[1][1]) if second else None
        return self

    def evaluate(self, gen):
        """distance() of the generator's images of the fixed latents: eval mode, no_grad, `chunk` latents per forward.  Every
        spectral-norm u / v is snapshotted before and copied back in place after, and the training mode restored: no side effect
        on the training, eager or replayed.  Call it between two iterations, never inside one."""
        self._need_reference()
        with self._sampling(gen):
            spectra = self.spectra(batches(gen, self.latents(gen.g_in), self.chunk), self.images)
        fake, bad = summary_means(spectrum_summary(spectra))
        return self._record(self._reference, fake, self.images, bad)
