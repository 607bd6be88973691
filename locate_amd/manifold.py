"""Precision, recall, density and coverage of generated samples, exact: the k-nearest-neighbour manifold metrics that tell lost
QUALITY from lost MODES.  `NearestNeighbours` finds copies and total collapse; its medians stay healthy when a generator covers a
third of the data well and never draws the rest.  The reference has nothing of the kind; this is an addition.

  precision / recall : Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative Models", 2019;
  density / coverage : Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", 2020.

With reals R (n rows), fakes G (m rows) and k, everything in the 8-bit code domain of `locate_amd.neighbours` - a squared distance
is an integer, so `d2(a, b) <= radius2[b]` has no rounding and the four metrics are ratios of integer counts:
  rad_R = kth_radius(R, k), rad_G = kth_radius(G, k)      each row's squared distance to its k-th nearest OTHER row (-1: no ball)
  hits_g, cov_r = within(G, R, rad_R)                      per fake the real balls it lies in, per real the fakes in its ball
  hits_r, _ = within(R, G, rad_G, covered=False)
  precision = #(hits_g > 0) / m     recall = #(hits_r > 0) / n     density = sum(hits_g) / (k m)     coverage = #(cov_r > 0) / n
A sample that holds a NaN or an Inf is flagged: it has no hits and no ball, is never counted and stays in the denominators.

The papers measure in the feature space of a pretrained network; this project uses none, the domain is the pixel codes.  Pixel-space
values far below 1 are normal even for real data, so the record carries `baseline`: a second, disjoint real set against the first.

Memory: the real set is `images` row_bytes(S) bytes (4096 at 64 x 64: 50 MB), a `within` call's workspace
4 (query_chunk ceil(N / 128) + N ceil(query_chunk / 64)) bytes.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import torch

from .neighbours import CanonicalViews, _sample_args, _triple, encode_images, nearest
from .sampling import FixedLatents, _gpu, _ptr, _stream

COUNTS = ("precise", "recalled", "hit_sum", "covered")


def within(q, r, radius2, skip=None, covered=True, query_chunk=4096):
    """q, r: (codes, norms, flags) triples as encode_images returns them (r's flags may be None: none flagged), rows of equal length;
    radius2: int64 [N] on the device, negative: that reference has no ball.  The pair (i, j) counts iff neither row is flagged,
    radius2[j] >= 0, j != skip[i] (skip: int32 [Q] on the device or None; -1: none) and d2(i, j) <= radius2[j].
    Returns (hits int32 [Q], covered int32 [N] or None): the counting pairs of each query and of each reference.  The queries go
    through the entry point `query_chunk` at a time, `covered` is added up over the chunks on the device.  Nothing is read on the
    host."""
    from ._lib import check, lib
    qc, qn, qf = _triple(q, "q")
    rc, rn, rf = _triple(r, "r", flags_optional=True)
    if qc.shape[1] != rc.shape[1] or qc.device != rc.device:
        raise ValueError("q and r must have rows of equal length on one device, got %s and %s" % (tuple(qc.shape), tuple(rc.shape)))
    Q, N = int(qc.shape[0]), int(rc.shape[0])
    radius2 = _gpu(radius2, "radius2", torch.int64)
    if tuple(radius2.shape) != (N,):
        raise ValueError("radius2 must be int64 [%d], got %s" % (N, tuple(radius2.shape)))
    if skip is not None:
        skip = _gpu(skip, "skip", torch.int32)
        if tuple(skip.shape) != (Q,):
            raise ValueError("skip must be int32 [%d], got %s" % (Q, tuple(skip.shape)))
    chunk = int(query_chunk)
    if chunk < 1:
        raise ValueError("query_chunk must be >= 1, got %d" % chunk)
    chunk = min(chunk, Q)
    L = lib()
    dev = qc.device
    hits = torch.empty(Q, dtype=torch.int32, device=dev)
    total = torch.empty(N, dtype=torch.int32, device=dev) if covered else None
    part = torch.empty(N, dtype=torch.int32, device=dev) if covered and chunk < Q else None
    ws = torch.empty(max(L.locate_nn_within_workspace_bytes(chunk, N, 1 if covered else 0) // 4, 1), dtype=torch.int32, device=dev)
    for a in range(0, Q, chunk):
        b = min(a + chunk, Q)
        out = total if a == 0 else part
        check(L.locate_nn_within(_ptr(qc[a:b]), _ptr(qn[a:b]), _ptr(qf[a:b]), b - a, _ptr(rc), _ptr(rn), _ptr(rf), N, int(qc.shape[1]),
                                 _ptr(radius2), None if skip is None else _ptr(skip[a:b]), _ptr(hits[a:b]), _ptr(out), _ptr(ws), _stream()),
              "locate_nn_within")
        if covered and a > 0:
            total += part
    return hits, total


def kth_radius(x, k):
    """int64 [n]: the squared distance of each row of the triple x to its k-th nearest OTHER row; -1 for a flagged row or when fewer
    than k others exist - "no ball"."""
    n = int(_triple(x, "x")[0].shape[0])
    d2, _ = nearest(x, x, k=k, skip=torch.arange(n, dtype=torch.int32, device=x[0].device))
    return d2[:, int(k) - 1].contiguous()


def metrics(counts, m, n, k):
    """The four metrics of the integer counts: Python true divisions."""
    return {"precision": counts["precise"] / m, "recall": counts["recalled"] / n, "density": counts["hit_sum"] / (k * m),
            "coverage": counts["covered"] / n}


class ManifoldMetrics(FixedLatents):
    """Precision, recall, density and coverage of `images` generated samples of size S against `images` real ones, k (1 .. 8).

    `reference_from_store(store)` draws `images` distinct store indices from a CPU generator seeded `seed + 7`, encodes those
    images' canonical views (as `NearestNeighbours` defines them) and caches their k-th-neighbour radii; if the store holds at
    least 2 `images`, the next `images` indices of the same permutation - a disjoint real set - are measured against the first:
    `baseline`, what a perfect generator would score here.  Otherwise `baseline` is None.

    Reading a record against `baseline`: precision / density below it with recall / coverage at it is lost quality; recall /
    coverage below it with precision at it is lost modes; all four low is both.

    `chunk` latents go through the generator per forward in evaluate(): InPlaceNorm takes its statistics over the batch it sees,
    so compare values only between runs with the same chunk.  The fixed latents [images, g_in] are drawn on the device on first
    use from a generator seeded `seed + 8`.  Construction needs no GPU.  Under data parallelism only rank 0 should evaluate."""

    latent_seed = 8

    def __init__(self, S, k=3, images=4096, seed=999, chunk=64, device="cuda"):
        self.S, self.k, self.images, self.seed, self.chunk = int(S), int(k), int(images), int(seed), int(chunk)
        self._canonical = _sample_args(self.S, self.k, self.images, self.chunk)
        FixedLatents.__init__(self, device)
        self.real = None
        self.real_radius = None
        self.real_index = None
        self.baseline = None

    @property
    def has_reference(self):
        return self.real is not None

    def reference_from_store(self, store):
        """The real set, its radii and - if the store is large enough - the baseline (one small device-to-host copy)."""
        self._need_gpu()
        N = len(store)
        n = min(self.images, N)
        if n < 1:
            raise ValueError("an empty store")
        self._canonical = CanonicalViews(self.S, store)
        order = torch.randperm(N, generator=torch.Generator().manual_seed(self.seed + 7)).tolist()
        self.real_index = order[:n]
        self.real = self._canonical.encode(self.real_index)
        self.real_radius = kth_radius(self.real, self.k)
        self.baseline = None
        if N >= 2 * self.images:
            value = self.between(self._canonical.views(order[n:2 * n]))
            self.baseline = {key: value[key] for key in ("precision", "recall", "density", "coverage", "counts")}
        return self

    def between(self, fake, real=None):
        """fake: any fp32 [m, 3, S, S] device batch; real: another such batch, or None for the cached real set.  The record documented
        on evaluate(): two `nearest` and two `within` calls (one of each when the cached set's radii serve) and ONE device-to-host
        copy."""
        if torch.is_tensor(fake) and fake.is_cuda and (fake.dim() != 4 or tuple(fake.shape[1:]) != (3, self.S, self.S)):
            raise ValueError("fake must be [m, 3, %d, %d], got %s" % (self.S, self.S, tuple(fake.shape)))
        g = encode_images(fake)
        if real is None:
            if self.real is None:
                raise RuntimeError("reference_from_store() first, or pass `real`")
            r, rad_r = self.real, self.real_radius
        else:
            r = encode_images(real)
            rad_r = kth_radius(r, self.k)
        rad_g = kth_radius(g, self.k)
        hits_g, cov_r = within(g, r, rad_r)
        hits_r, _ = within(r, g, rad_g, covered=False)
        counts = torch.stack([(hits_g > 0).sum(), (hits_r > 0).sum(), hits_g.sum(), (cov_r > 0).sum(), (g[2] != 0).sum()]).cpu().tolist()          # the one host copy
        m, n = int(g[0].shape[0]), int(r[0].shape[0])
        value = {"images": m, "real_images": n, "k": self.k}
        value["counts"] = dict(zip(COUNTS, counts[:4]))
        value.update(metrics(value["counts"], m, n, self.k))
        value["nonfinite"] = counts[4]
        value["baseline"] = None if self.baseline is None else dict(self.baseline, counts=dict(self.baseline["counts"]))
        return value

    def evaluate(self, gen, latents=None):
        """between() of the generator's images of `latents` (default: the fixed ones) - `sampling.sampling`: eval mode,
        no_grad, `chunk` latents per forward, every spectral-norm u / v copied back afterwards.  Returns
          "images" m, "real_images" n, "k"; "precision", "recall", "density", "coverage"; "counts": {"precise", "recalled",
          "hit_sum", "covered"}, the integers they are ratios of; "nonfinite": the number of samples that hold a NaN or an Inf;
          "baseline": the four metrics and "counts" of a second real set against the first, or None."""
        if self.real is None:
            raise RuntimeError("reference_from_store() first")
        return self.between(self._generate(gen, latents))
