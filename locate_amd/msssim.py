"""Measuring a run: the multi-scale structural similarity (MS-SSIM, Wang et al. 2003) between pairs of images - the diversity
number beside the sliced Wasserstein distance in Karras et al. 2018, table 1 (after Odena et al. 2017): how alike two samples of one
generator are, luminance apart from contrast and structure, scale by scale.  The same pair kernel compares the SAME latents under
two settings (live against averaged generator, fp8 against fp32).  The reference has no metric at all; this is an addition.

The definition is stated once, in float64 numpy, in tests/helpers/msssim_model.py.  In short (csrc/msssim.hip through the C ABI,
include/locate_hip.h): images in the 8-bit domain of `neighbours.encode_images` (value = code + 128, L = 255), S in {32, 64, 128, 256},
five levels of side S >> l, each the 2 x 2 mean of the one above; per level a Gaussian window of n = min(11, side) taps with
sigma = 1.5 n / 11 (`window_taps`), "valid" filtering, the SSIM and contrast-structure (cs) maps with C1 = (0.01 L)^2,
C2 = (0.03 L)^2, their means over all three channels' outputs: ten numbers a pair (`ms_ssim_levels`), float64 throughout.  A pair's
value (`ms_ssim_value`) is prod_{l < 4} max(cs_l, 0)^w_l max(ssim_4, 0)^w_4 with `WEIGHTS`; a pair where one of those five numbers is
negative is `clamped` - unrelated images do go negative at the fine levels - so a record carries the clamped count and the raw
per-level means beside the value.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import numpy as np
import torch

from .neighbours import _triple, encode_images
from .sampling import FixedLatents, _ptr, _stream, batches, plain_batches

SIZES = (32, 64, 128, 256)
LEVELS = 5
TAPS = 11
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_WORKSPACE_BYTES = 256 << 20          # pairs of 128 and 256 go through the kernels this much workspace at a time


def _size(S):
    if isinstance(S, bool) or int(S) != S or int(S) not in SIZES:
        raise ValueError("MS-SSIM takes S in %s, got %r" % (SIZES, S))
    return int(S)


def window_taps(S):
    """float64 [5, 11], zero padded: row l holds the n = min(11, S >> l) taps exp(-t^2 / (2 sigma^2)), t = j - (n - 1) / 2,
    sigma = 1.5 n / 11, divided by their sum.  An even window is centred between pixels."""
    S = _size(S)
    taps = np.zeros((LEVELS, TAPS), dtype=np.float64)
    for l in range(LEVELS):
        n = min(TAPS, S >> l)
        t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        g = np.exp(-(t * t) / (2.0 * (1.5 * n / TAPS) ** 2))
        taps[l, :n] = g / g.sum()
    return taps


_TAPS = {}
_SIZE_BY_ROW = {3 * S * S: S for S in SIZES}          # row_bytes(S) == 3 S^2 at the four sizes


def _device_taps(S, device):
    key = (S, str(device))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(window_taps(S)).to(device)
    return _TAPS[key]


def ms_ssim_levels(a, b):
    """a, b: (codes, norms, flags) triples as `encode_images` returns them, of equal shape (flags may be None: none flagged; the norms
    are not read).  Pair i is row i of a against row i of b.  Returns float64 [P, 2, 5] on the device: [:, 0] the levels' ssim means,
    [:, 1] their cs means; ten NaNs for a pair with a flagged member.  No host read.  A pair's numbers depend on its two rows alone:
    (a, b) gives the bits of (b, a), and a row against itself 1.0 ten times."""
    from ._lib import check, lib
    ac, _, af = _triple(a, "a", flags_optional=True)
    bc, _, bf = _triple(b, "b", flags_optional=True)
    if tuple(ac.shape) != tuple(bc.shape) or ac.device != bc.device:
        raise ValueError("a and b must be of equal shape on one device, got %s and %s" % (tuple(ac.shape), tuple(bc.shape)))
    if int(ac.shape[1]) not in _SIZE_BY_ROW:
        raise ValueError("code rows of %d bytes: MS-SSIM takes the sizes %s" % (ac.shape[1], SIZES))
    S, P, row = _SIZE_BY_ROW[int(ac.shape[1])], int(ac.shape[0]), int(ac.shape[1])
    L = lib()
    taps = _device_taps(S, ac.device)
    out = torch.empty(P, 2, LEVELS, dtype=torch.float64, device=ac.device)
    per_pair = L.locate_msssim_workspace_bytes(1, S)
    step = P if per_pair == 0 else max(1, min(65535, _WORKSPACE_BYTES // per_pair))
    ws = None
    for at in range(0, P, step):
        m = min(step, P - at)
        if per_pair and ws is None:
            ws = torch.empty(L.locate_msssim_workspace_bytes(m, S) // 8, dtype=torch.float64, device=ac.device)
        check(L.locate_msssim_pairs(_ptr(ac[at:at + m]), _ptr(None if af is None else af[at:at + m]), _ptr(bc[at:at + m]),
                                    _ptr(None if bf is None else bf[at:at + m]), m, row, S, _ptr(taps), _ptr(out[at:at + m]), _ptr(ws), _stream()),
              "locate_msssim_pairs")
    return out


def ms_ssim_value(levels):
    """levels: float64 [P, 2, 5] on the GPU -> (value float64 [P], clamped bool [P]): prod_{l < 4} max(cs_l, 0)^w_l max(ssim_4, 0)^w_4
    and whether one of those five numbers was negative (the clamp is `tf.image.ssim_multiscale`'s; without it a negative mean gives
    NaN).  A NaN row stays NaN and is not clamped.  A few torch operations on the device; nothing is read."""
    if not torch.is_tensor(levels) or not levels.is_cuda:
        raise TypeError("levels must be a GPU tensor (there is no CPU path); got %s" % (levels.device if torch.is_tensor(levels) else type(levels).__name__))
    if levels.dtype != torch.float64 or levels.dim() != 3 or tuple(levels.shape[1:]) != (2, LEVELS):
        raise ValueError("levels must be float64 [P, 2, 5], got %s %s" % (levels.dtype, tuple(levels.shape)))
    terms = torch.cat([levels[:, 1, :LEVELS - 1], levels[:, 0, LEVELS - 1:]], dim=1)
    clamped = (terms < 0).any(dim=1)
    # clamp(min=0) keeps a NaN; pow and prod carry it on
    value = terms.clamp(min=0.0).pow(torch.tensor(WEIGHTS, dtype=torch.float64, device=levels.device)).prod(dim=1)
    return value, clamped


def _images(x, name, S=None):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise TypeError("%s must be a GPU tensor (there is no CPU path); got %s" % (name, x.device if torch.is_tensor(x) else type(x).__name__))
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or int(x.shape[2]) not in SIZES or (S is not None and x.shape[2] != S):
        raise ValueError("%s must be fp32 [P, 3, S, S] with S %s, got %s" % (name, "in %s" % (SIZES,) if S is None else "= %d" % S, tuple(x.shape)))
    return x


def ms_ssim(x, y):
    """x, y: fp32 [P, 3, S, S] on the GPU -> (value float64 [P], clamped bool [P], levels float64 [P, 2, 5]) of x[i] against y[i]:
    `encode_images`, `ms_ssim_levels`, `ms_ssim_value`."""
    x, y = _images(x, "x"), _images(y, "y")
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError("x and y must be of equal shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    levels = ms_ssim_levels(encode_images(x), encode_images(y))
    return ms_ssim_value(levels) + (levels,)


KEYS = ("pairs", "mean", "std", "clamped", "nonfinite", "levels")


class _Sums:
    """What a record is made of, added chunk by chunk on the device: per-pair values and levels are reduced with torch float64
    operations; one small host copy at the end."""

    def __init__(self):
        self.parts = []

    def add(self, levels):
        value, clamped = ms_ssim_value(levels)
        ok = ~torch.isnan(value)
        v = torch.where(ok, value, torch.zeros_like(value))
        lv = torch.where(ok[:, None, None], levels, torch.zeros_like(levels))
        self.parts.append(torch.cat([torch.stack([ok.sum().double(), v.sum(), (v * v).sum(), (clamped & ok).sum().double(), (~ok).sum().double()]),
                                     lv.sum(dim=0).reshape(-1)]))
        return value

    def record(self):
        host = torch.stack(self.parts).sum(dim=0).cpu().tolist()          # the one host copy: 15 doubles
        n, s, q, clamped, bad = host[:5]
        nan = float("nan")
        mean = s / n if n else nan
        return {"pairs": int(n + bad), "mean": mean, "std": max(q / n - mean * mean, 0.0) ** 0.5 if n else nan, "clamped": int(clamped), "nonfinite": int(bad),
                "levels": {"ssim": [v / n if n else nan for v in host[5:5 + LEVELS]], "cs": [v / n if n else nan for v in host[5 + LEVELS:]]}}


class MultiScaleSSIM(FixedLatents):
    """MS-SSIM of `pairs` image pairs of size S.

    A record (`between`, `among`, `evaluate`, `evaluate_against`):
      "pairs"; "mean", "std": of the pairs' values (the population standard deviation) over the pairs that are not NaN;
      "clamped": how many of those had a negative level number clamped to 0 - their value is 0;
      "nonfinite": the pairs with a member that holds a NaN or an Inf (left out of everything else);
      "levels": {"ssim": [5], "cs": [5]}: the means of the raw, unclamped level numbers over the same pairs;
      "real": the same keys for pairs of real images (`reference_from_pipeline`), or None.
    Read "mean" and "levels" against "real", never against 1: samples more alike than real images are alike have lost variation, and
    the levels say at which scale.  Where "clamped" is a large share of the pairs the mean is mostly zeros: read levels["cs"].

    `latents` [2 pairs, g_in] is drawn on the device on first use, from a generator seeded `seed + 9`.  `chunk` (even) latents go
    through the generator per forward, and the pairs are formed inside a chunk - image 2 j with 2 j + 1 -: it is part of the
    metric's definition as it is of `SlicedWasserstein`'s, InPlaceNorm takes its statistics over the batch it sees.  Compare runs
    only at equal pairs, chunk and size.  Construction needs no GPU.  Under data parallelism only rank 0 should evaluate."""

    latent_seed = 9

    def __init__(self, S, pairs=4096, seed=999, chunk=64, device="cuda"):
        self.S = _size(S)
        self.pairs, self.seed, self.chunk = int(pairs), int(seed), int(chunk)
        if self.pairs < 1:
            raise ValueError("pairs must be >= 1, got %d" % self.pairs)
        if self.chunk < 2 or self.chunk % 2:
            raise ValueError("chunk must be even and >= 2 (the pairs are formed inside a chunk), got %d" % self.chunk)
        FixedLatents.__init__(self, device)
        self.real = None

    def _latent_count(self):
        return 2 * self.pairs

    def _record(self, sums):
        value = sums.record()
        value["real"] = None if self.real is None else dict(self.real)
        return value

    def between(self, x, y):
        """The record of x[i] against y[i]: fp32 [P, 3, S, S] each."""
        x, y = _images(x, "x", self.S), _images(y, "y", self.S)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError("x and y must be of equal shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        sums = _Sums()
        sums.add(ms_ssim_levels(encode_images(x), encode_images(y)))
        return self._record(sums)

    @staticmethod
    def _among(images, sums):
        codes, norms, flags = encode_images(images)
        return sums.add(ms_ssim_levels((codes[0::2], norms[0::2], flags[0::2]), (codes[1::2], norms[1::2], flags[1::2])))

    def among(self, images):
        """The record of image 2 j against image 2 j + 1: fp32 [2 P, 3, S, S]."""
        images = _images(images, "images", self.S)
        if images.shape[0] % 2:
            raise ValueError("an even number of images makes the pairs, got %d" % images.shape[0])
        sums = _Sums()
        self._among(images, sums)
        return self._record(sums)

    def reference_from_pipeline(self, pipeline):
        """`among` of the first 2 pairs images of the plain chain - the first output of `InputPipeline.next_batch()`, from a pipeline of
        this metric's own over the same store, seeded seed + 2: the training pipeline's shuffle is not advanced -, kept as the
        record's "real".  The images are taken `chunk` at a time, as evaluate() takes the generator's."""
        self._need_gpu()
        sums, rest = _Sums(), None
        for real in plain_batches(pipeline, self.S, 2 * self.pairs, self.seed, 2 * self.pairs):
            real = real if rest is None else torch.cat([rest, real])
            whole = real.shape[0] - real.shape[0] % 2
            for at in range(0, whole, self.chunk):
                self._among(real[at:min(at + self.chunk, whole)], sums)
            rest = real[whole:]
        self.real = {k: v for k, v in sums.record().items() if k in KEYS}
        return self

    def evaluate(self, gen):
        """The record of the generator's images of the fixed latents, image 2 j against 2 j + 1 inside every chunk: eval mode, no_grad,
        `chunk` latents per forward, the levels computed per chunk - never more than a chunk of images is held.  Every spectral-norm
        u / v is snapshotted before and copied back in place after, and the training mode restored: no side effect on the training,
        eager or replayed.  Call it between two iterations, never inside one."""
        sums = _Sums()
        with self._sampling(gen):
            for images in batches(gen, self.latents(gen.g_in), self.chunk):
                self._among(images, sums)
        return self._record(sums)

    def evaluate_against(self, gen_a, gen_b):
        """The record of the SAME fixed latents through two generators, image i of one against image i of the other - live against
        averaged, fp8 against fp32: 2 pairs pairs.  The same care as evaluate() for both; no "real" entry (pairs of real images
        answer another question)."""
        if gen_a.g_in != gen_b.g_in:
            raise ValueError("the generators take latents of %d and %d" % (gen_a.g_in, gen_b.g_in))
        sums = _Sums()
        with self._sampling(gen_a, gen_b):
            for a, b in batches([gen_a, gen_b], self.latents(gen_a.g_in), self.chunk):
                sums.add(ms_ssim_levels(encode_images(a), encode_images(b)))
        return sums.record()
