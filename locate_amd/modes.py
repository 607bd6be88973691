"""Which modes are missing: the Number of statistically Different Bins (NDB; Richardson & Weiss, "On GANs and GMMs", 2018), exact.
`ManifoldMetrics` says with one number that modes are lost; this names them.  The reference has nothing of the kind; this is an
addition.

  1. the real images are clustered into K Voronoi cells ("bins") by k-means;
  2. the generated samples are assigned to the same cells;
  3. per cell a two-sample proportion test says whether the samples' share differs from the real images'.
NDB is the number of cells that differ, beside it the Jensen-Shannon divergence of the two histograms, the cells ordered from the
most under-represented, and each cell's centre as a picture.  The paper defines all this in pixel space, which is this project's
domain: no pretrained network.

Everything is in the 8-bit code domain of `locate_amd.neighbours`, where Lloyd's algorithm is integer arithmetic:
  * assignment: `nearest(x, centres, k=1)` - exact squared distances on the int8 matrix instruction, ties to the lower index, a
    flagged image (NaN / Inf) gets -1 and belongs to no cell;
  * update (csrc/modes.hip): the int32 sum of the code rows of every cell, one read of the bank at stream rate, and per coordinate
    floor((2 sum + n) / (2 n)) - the mean rounded to the nearest integer, a half upwards: the best INTEGER centre coordinate by
    coordinate.  An empty cell keeps its centre.
A numpy model reproduces every word with `==` (tests/helpers/modes_model.py).

Memory: the real set is `images` row_bytes(S) bytes (16384 at 64 x 64: 201 MB), the sums 4 K row_bytes(S), the update's workspace
4 (ceil(images / 64) + K + 1) (row_bytes(S) + 1) + 8 (K + 1) bytes.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import math
from statistics import NormalDist

import torch

from .neighbours import CanonicalViews, _sample_args, _triple, encode_images, nearest
from .sampling import FixedLatents, _gpu, _ptr, _stream

K_MAX = 65535
M_MAX = (1 << 24) - 1


def _group_args(codes, K):
    codes = _gpu(codes, "codes", torch.int8)
    if codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] < 64 or codes.shape[1] % 64:
        raise ValueError("codes must be int8 [n, row_bytes] with row_bytes a multiple of 64, got %s" % (tuple(codes.shape),))
    K = int(K)
    if not 1 <= K <= K_MAX:
        raise ValueError("K must be 1 .. %d, got %d" % (K_MAX, K))
    return codes, K


def group_sums(codes, labels, K):
    """codes: int8 [N, row_bytes] on the GPU; labels: int32 [N] on the GPU, -1 .. K - 1 (-1: in no group).  Returns
    (sums int32 [K, row_bytes], counts int32 [K], starts int32 [K + 1]): the sum of the code rows of each label, the number of
    them, and the groups' first places in the stable sort of the labels (the -1 rows sort in front of starts[0]).  The grouping is
    a `torch.sort` and a `searchsorted`, the sums one call of csrc/modes.hip.  Nothing is read on the host."""
    from ._lib import check, lib
    codes, K = _group_args(codes, K)
    labels = _gpu(labels, "labels", torch.int32)
    N, rb = int(codes.shape[0]), int(codes.shape[1])
    if tuple(labels.shape) != (N,) or labels.device != codes.device:
        raise ValueError("labels must be int32 [%d] on the codes' device, got %s" % (N, tuple(labels.shape)))
    if N > M_MAX:
        raise ValueError("at most %d rows, got %d" % (M_MAX, N))
    dev = codes.device
    ranked, order = torch.sort(labels, stable=True)
    starts = torch.searchsorted(ranked, torch.arange(K + 1, dtype=torch.int32, device=dev)).to(torch.int32)
    order = order.to(torch.int32)
    L = lib()
    sums = torch.empty(K, rb, dtype=torch.int32, device=dev)
    ws = torch.empty(L.locate_nn_group_sums_workspace_bytes(N, K, rb) // 4, dtype=torch.int32, device=dev)
    check(L.locate_nn_group_sums(_ptr(codes), N, rb, _ptr(order), N, _ptr(starts), K, _ptr(sums), _ptr(ws), _stream()), "locate_nn_group_sums")
    return sums, starts[1:] - starts[:-1], starts


def centroids(sums, starts, M, previous, out=None):
    """sums int32 [K, row_bytes] and starts int32 [K + 1] as group_sums returns them, M the number of grouped rows, previous int8
    [K, row_bytes]: the centres before.  Returns ((codes, norms, flags), moved): row k of codes is the rounded mean of group k,
    floor((2 sum + n) / (2 n)) per byte, or previous[k] for an empty group; norms its squared length; flags all zero; moved int32
    [K] the bytes that differ from previous[k].  out: where to write the codes (`previous` itself: in place), else a new tensor."""
    from ._lib import check, lib
    sums, starts = _gpu(sums, "sums", torch.int32), _gpu(starts, "starts", torch.int32)
    previous = _gpu(previous, "previous", torch.int8)
    if sums.dim() != 2 or sums.shape[0] < 1 or sums.shape[1] < 64 or sums.shape[1] % 64:
        raise ValueError("sums must be int32 [K, row_bytes] with row_bytes a multiple of 64, got %s" % (tuple(sums.shape),))
    K, rb = int(sums.shape[0]), int(sums.shape[1])
    if tuple(starts.shape) != (K + 1,) or tuple(previous.shape) != (K, rb):
        raise ValueError("starts must be [%d] and previous [%d, %d], got %s and %s" % (K + 1, K, rb, tuple(starts.shape), tuple(previous.shape)))
    dev = sums.device
    if out is None:
        out = torch.empty(K, rb, dtype=torch.int8, device=dev)
    elif not torch.is_tensor(out) or out.dtype != torch.int8 or tuple(out.shape) != (K, rb) or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous int8 [%d, %d] on %s" % (K, rb, dev))
    norms = torch.empty(K, dtype=torch.int64, device=dev)
    moved = torch.empty(K, dtype=torch.int32, device=dev)
    check(lib().locate_nn_centroids(_ptr(sums), _ptr(starts), K, int(M), rb, _ptr(previous), _ptr(out), _ptr(norms), _ptr(moved), _stream()),
          "locate_nn_centroids")
    return (out, norms, torch.zeros(K, dtype=torch.int32, device=dev)), moved


def initial_rows(flags, K, seed):
    """The K distinct unflagged rows k-means starts from: place `randperm(unflagged, seed)[:K]` in the list of unflagged rows.
    flags: a host sequence or CPU tensor.  int64 [K] on the host."""
    ok = torch.nonzero(torch.as_tensor(flags).reshape(-1) == 0).reshape(-1)
    K = int(K)
    if not 1 <= K <= int(ok.numel()):
        raise ValueError("K = %d centres from %d rows that are not flagged" % (K, int(ok.numel())))
    return ok[torch.randperm(int(ok.numel()), generator=torch.Generator().manual_seed(int(seed)))[:K]]


def kmeans_codes(x, K, iterations=10, seed=999):
    """Lloyd's algorithm on the (codes, norms, flags) triple x, exact.  The centres start as the codes of `initial_rows(flags, K,
    seed)` (the flags are read once, here); then `iterations` rounds of nearest(x, C, k=1), group_sums and centroids in place, with
    no host read, and a last assignment to the final centres.  Returns
      centres: a (codes int8 [K, row_bytes], norms, flags) triple; labels int32 [N] (-1: flagged); counts int32 [K];
      inertia int64 [iterations + 1]: the sum of the unflagged rows' squared distance at each assignment - it never increases;
      moved int32 [iterations, K]: the bytes of each centre that a round changed.  All on the device."""
    codes, norms, flags = _triple(x, "x")
    _, K = _group_args(codes, K)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0, got %d" % iterations)
    dev = codes.device
    at = initial_rows(flags.cpu(), K, seed).to(dev)
    centres = (codes[at].contiguous(), norms[at].contiguous(), torch.zeros(K, dtype=torch.int32, device=dev))
    inertia = torch.empty(iterations + 1, dtype=torch.int64, device=dev)
    moved = torch.empty(iterations, K, dtype=torch.int32, device=dev)
    x = (codes, norms, flags)
    for i in range(iterations + 1):
        d2, index = nearest(x, centres, k=1)
        labels = index[:, 0].contiguous()
        inertia[i] = torch.where(d2 >= 0, d2, torch.zeros_like(d2)).sum()
        if i == iterations:
            break
        sums, _, starts = group_sums(codes, labels, K)
        centres, moved[i] = centroids(sums, starts, codes.shape[0], centres[0], out=centres[0])
    counts = torch.bincount(labels.long() + 1, minlength=K + 1)[1:].to(torch.int32)
    return centres, labels, counts, inertia, moved


def ndb_statistics(real_counts, fake_counts, alpha=0.05):
    """The two-sample proportion test per bin, in Python float64 on integers; no GPU.  With n = sum real, m = sum fake, p = r / n,
    q = f / m and the pooled P = (r + f) / (n + m): se = sqrt(P (1 - P) (1 / n + 1 / m)), z = (q - p) / se (negative: the samples
    under-represent the bin; 0.0 where se == 0), different = |z| > NormalDist().inv_cdf(1 - alpha / 2).  Returns "ndb" (the number
    of different bins), "ndb_over_k", "js" (the Jensen-Shannon divergence of p and q, natural logarithms, at most ln 2), "missing"
    (different bins with f == 0), "z" [K], "different" [K] and "order" [K]: the bins by ascending z, ties by index.  With n or m
    zero the four metrics, z and different are None and the order is that of the indices."""
    r, f = [int(v) for v in real_counts], [int(v) for v in fake_counts]
    K = len(r)
    if K < 1 or len(f) != K or min(r) < 0 or min(f) < 0:
        raise ValueError("two lists of K >= 1 counts that are not negative")
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1), got %r" % (alpha,))
    n, m = sum(r), sum(f)
    if n == 0 or m == 0:
        return {"ndb": None, "ndb_over_k": None, "js": None, "missing": None, "z": None, "different": None, "order": list(range(K))}
    critical = NormalDist().inv_cdf(1.0 - alpha / 2.0)
    z, js = [], 0.0
    for rk, fk in zip(r, f):
        p, q, pooled = rk / n, fk / m, (rk + fk) / (n + m)
        se = math.sqrt(pooled * (1.0 - pooled) * (1.0 / n + 1.0 / m))
        z.append((q - p) / se if se > 0.0 else 0.0)
        mid = 0.5 * (p + q)
        if p > 0.0:
            js += 0.5 * p * math.log(p / mid)
        if q > 0.0:
            js += 0.5 * q * math.log(q / mid)
    different = [abs(v) > critical for v in z]
    ndb = sum(different)
    return {"ndb": ndb, "ndb_over_k": ndb / K, "js": js, "missing": sum(1 for d, fk in zip(different, f) if d and fk == 0),
            "z": z, "different": different, "order": sorted(range(K), key=lambda k: (z[k], k))}


BASELINE_KEYS = ("ndb", "ndb_over_k", "js", "missing", "fake_counts")


class BinnedModes(FixedLatents):
    """NDB of `samples` generated samples of size S against `bins` k-means cells of `images` real images.

    `reference_from_store(store)` takes the canonical views (as `NearestNeighbours` defines them) of min(images, N) distinct store
    images, in the order of a CPU `randperm` seeded `seed + 10`, encodes them and runs `kmeans_codes` on them (`iterations` rounds,
    start seeded `seed + 12`); it keeps the centres, `real_counts`, `inertia` and `converged_at` - the first round, counted from 1,
    that moved no centre, or None.  If the store holds at least images + samples images, the next `samples` images of that order
    are binned too: `baseline`, what a perfect generator would score - about alpha K different bins by chance.

    Reading a record: always against `baseline`, never against 0.  `order` lists the bins from the most under-represented;
    `missing` counts the different bins that got no sample at all; `save_picture` shows the centres in that order.  Compare runs
    only at equal bins, images, samples, chunk, seed and size.

    `chunk` latents go through the generator per forward in evaluate() (InPlaceNorm takes its statistics over the batch it sees).
    The fixed latents [samples, g_in] are drawn on the device on first use from a generator seeded `seed + 11`.  Construction needs
    no GPU.  Under data parallelism only rank 0 should evaluate."""

    latent_seed = 11

    def __init__(self, S, bins=128, images=16384, samples=4096, iterations=10, alpha=0.05, seed=999, chunk=64, device="cuda"):
        self.S, self.samples, self.seed, self.chunk = int(S), int(samples), int(seed), int(chunk)
        self._canonical = _sample_args(self.S, 1, self.samples, self.chunk)
        self.bins, self.images, self.iterations, self.alpha = int(bins), int(images), int(iterations), float(alpha)
        if not 1 <= self.bins <= self.images:
            raise ValueError("bins must be 1 .. images, got %d bins for %d images" % (self.bins, self.images))
        if self.bins > K_MAX or self.images > M_MAX:
            raise ValueError("at most %d bins and %d images" % (K_MAX, M_MAX))
        if self.iterations < 0:
            raise ValueError("iterations must be >= 0, got %d" % self.iterations)
        if not 0.0 < self.alpha < 1.0:
            raise ValueError("alpha must lie in (0, 1), got %r" % (alpha,))
        FixedLatents.__init__(self, device)
        self.centres = None
        self.real_index = None
        self.real_counts = None
        self.inertia = None
        self.converged_at = None
        self.baseline = None

    def _latent_count(self):
        return self.samples

    @property
    def has_reference(self):
        return self.centres is not None

    def reference_from_store(self, store):
        """The real set, its bins and - if the store is large enough - the baseline (two small device-to-host copies: the flags at
        the start of k-means, the counts at its end)."""
        self._need_gpu()
        N = len(store)
        n = min(self.images, N)
        if n < self.bins:
            raise ValueError("%d bins from a store of %d images" % (self.bins, N))
        self._canonical = CanonicalViews(self.S, store)
        order = torch.randperm(N, generator=torch.Generator().manual_seed(self.seed + 10)).tolist()
        self.real_index = order[:n]
        real = self._canonical.encode(self.real_index)
        self.centres, _, counts, inertia, moved = kmeans_codes(real, self.bins, iterations=self.iterations, seed=self.seed + 12)
        still = (moved == 0).all(dim=1).to(torch.int64)
        host = torch.cat([counts.to(torch.int64), inertia, still]).cpu().tolist()          # the one host copy
        K = self.bins
        self.real_counts, self.inertia = host[:K], host[K:K + self.iterations + 1]
        self.converged_at = next((i + 1 for i, s in enumerate(host[K + self.iterations + 1:]) if s), None)
        self.baseline = None
        if N >= self.images + self.samples:
            value = self.between(self._canonical.views(order[n:n + self.samples]))
            self.baseline = {key: value[key] for key in BASELINE_KEYS}
        return self

    def between(self, fake):
        """fake: any fp32 [m, 3, S, S] device batch.  The record documented on evaluate(): one `encode_images`, one `nearest` against
        the centres, a bin count and ONE device-to-host copy."""
        if self.centres is None:
            raise RuntimeError("reference_from_store() first")
        if torch.is_tensor(fake) and fake.is_cuda and (fake.dim() != 4 or tuple(fake.shape[1:]) != (3, self.S, self.S)):
            raise ValueError("fake must be [m, 3, %d, %d], got %s" % (self.S, self.S, tuple(fake.shape)))
        g = encode_images(fake)
        _, index = nearest(g, self.centres, k=1)
        host = torch.bincount(index[:, 0].long() + 1, minlength=self.bins + 1).cpu().tolist()          # the one host copy; [0]: flagged
        fake_counts = host[1:]
        value = {"bins": self.bins, "images": sum(self.real_counts), "samples": int(g[0].shape[0]), "alpha": self.alpha}
        stats = ndb_statistics(self.real_counts, fake_counts, self.alpha)
        value.update({key: stats[key] for key in ("ndb", "ndb_over_k", "js", "missing")})
        value["real_counts"], value["fake_counts"] = list(self.real_counts), fake_counts
        value.update({key: stats[key] for key in ("z", "different", "order")})
        value["nonfinite"] = host[0]
        value["kmeans"] = {"iterations": self.iterations, "converged_at": self.converged_at, "inertia": list(self.inertia)}
        value["baseline"] = None if self.baseline is None else dict(self.baseline, fake_counts=list(self.baseline["fake_counts"]))
        return value

    def evaluate(self, gen, latents=None):
        """between() of the generator's images of `latents` (default: the fixed ones) - `sampling.sampling`: eval mode,
        no_grad, `chunk` latents per forward, every spectral-norm u / v copied back afterwards.  Returns
          "bins" K, "images" (the real images that are in a bin), "samples" (the batch, flagged ones included), "alpha";
          "ndb", "ndb_over_k", "js", "missing" (`ndb_statistics`; None if no sample is finite);
          "real_counts" [K], "fake_counts" [K], "z" [K], "different" [K], "order" [K];
          "nonfinite": the samples that hold a NaN or an Inf - they fall into no bin and are left out of the test's m;
          "kmeans": {"iterations", "converged_at", "inertia" [iterations + 1]} of the reference;
          "baseline": {"ndb", "ndb_over_k", "js", "missing", "fake_counts"} of a second real set in the same bins, or None."""
        if self.centres is None:
            raise RuntimeError("reference_from_store() first")
        return self.between(self._generate(gen, latents))

    def centre_images(self):
        """fp32 [K, 3, S, S]: the centres as pictures, (code + 128) / 127.5 - 1."""
        if self.centres is None:
            raise RuntimeError("reference_from_store() first")
        codes = self.centres[0][:, :3 * self.S * self.S].to(torch.float32)
        return ((codes + 128.0) / 127.5 - 1.0).reshape(self.bins, 3, self.S, self.S)

    def save_picture(self, path, record):
        """A PNG of the K centres, sixteen to a row, in the record's `order`: the bins the samples miss most come first."""
        from .monitor import image_grid, write_png
        images = self.centre_images()
        order = torch.tensor([int(k) for k in record["order"]], dtype=torch.int64, device=images.device)
        rgba = image_grid(images[order].contiguous(), nrow=16, value_range=(-1, 1))
        return write_png(path, rgba.cpu())
