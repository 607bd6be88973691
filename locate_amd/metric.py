"""Measuring a run: the sliced Wasserstein distance (SWD) between Laplacian-pyramid patch descriptors of real and generated
images (Karras et al., "Progressive Growing of GANs", section 5) - the standard quality metric that needs no pretrained network.
The reference has no metric at all; this is an addition.

Per set of N images [N, 3, S, S] (csrc/swd.hip through the C ABI, include/locate_hip.h):
  1. a Laplacian pyramid with levels at S, S/2, ..., 16 (filter outer([1,4,6,4,1], [1,4,6,4,1]) / 256, mirrored borders);
  2. per level and image, P patches of 7 x 7 x 3 at random positions: n = N P descriptors of K = 147 values;
  3. per level and channel the mean and the population deviation over all gathered values, each descriptor normalised with them;
  4. projections on unit directions, `dirs_per_repeat` at a time;
  5. per direction both sets' projections sorted (`torch.sort`: a radix sort moves keys and computes nothing) and the mean
     absolute difference taken; a level's value is the mean over the repeats, the result the levels' values and their mean.
Karras et al. print the values times 10^3.  Their pipeline quantises the candidates to uint8 first; here the fp32 images are
measured as they are - the normalisation makes the value free of scale and offset.

A channel that is constant over all gathered values has deviation 0: the result is then not finite.  It is not guarded.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import torch

from .sampling import FixedLatents, _gpu, _ptr, _stream, batches, plain_batches

PATCH = 7
K = 3 * PATCH * PATCH


def pyramid_levels(S, min_size=16):
    """The level sizes [S, S/2, ..., min_size]: log2(S) - 3 levels for min_size = 16 (3 at 64, 5 at 256)."""
    S, min_size = int(S), int(min_size)
    if S < min_size or S & (S - 1) or min_size < 8 or min_size & (min_size - 1):
        raise ValueError("the pyramid takes a power-of-two size of at least %d, got %d" % (min_size, S))
    sizes = [S]
    while sizes[-1] > min_size:
        sizes.append(sizes[-1] // 2)
    return sizes


def _planes(x, name):
    x = _gpu(x, name)
    if x.dim() < 2 or x.shape[-1] != x.shape[-2] or x.numel() == 0:
        raise ValueError("%s must be [..., S, S], got %s" % (name, tuple(x.shape)))
    return x, x.numel() // (x.shape[-1] * x.shape[-1]), int(x.shape[-1])


def pyr_down(x):
    """[..., S, S] -> [..., S/2, S/2]: the binomial 5 x 5 filter at every second position (S even, >= 8)."""
    from ._lib import check, lib
    x, planes, S = _planes(x, "x")
    out = torch.empty(tuple(x.shape[:-2]) + (S // 2, S // 2), dtype=torch.float32, device=x.device)
    check(lib().locate_pyr_down(_ptr(x), planes, S, _ptr(out), _stream()), "locate_pyr_down")
    return out


def pyr_residual(x, coarse, out=None):
    """x - up(coarse) for x [..., S, S] and coarse [..., S/2, S/2]; `out` may be x."""
    from ._lib import check, lib
    x, planes, S = _planes(x, "x")
    coarse = _gpu(coarse, "coarse")
    if tuple(coarse.shape) != tuple(x.shape[:-2]) + (S // 2, S // 2):
        raise ValueError("coarse must be %s, got %s" % (tuple(x.shape[:-2]) + (S // 2, S // 2), tuple(coarse.shape)))
    if out is None:
        out = torch.empty_like(x)
    elif not torch.is_tensor(out) or tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous fp32 %s tensor on %s" % (tuple(x.shape), x.device))
    check(lib().locate_pyr_residual(_ptr(x), _ptr(coarse), planes, S, _ptr(out), _stream()), "locate_pyr_residual")
    return out


def laplacian_pyramid(x, levels=None):
    """x: fp32 [n, 3, S, S] on the GPU.  Returns `levels` tensors [n, 3, S_l, S_l] (default: every level of pyramid_levels(S)):
    G_l - up(G_{l+1}) for all but the last, G_{L-1} for the last."""
    x = _gpu(x, "x")
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError("laplacian_pyramid takes [n, c, S, S], got %s" % (tuple(x.shape),))
    count = len(pyramid_levels(x.shape[2])) if levels is None else int(levels)
    if count < 1 or any((x.shape[2] >> i) < 8 or (x.shape[2] >> i) % 2 for i in range(count - 1)):          # every size that is halved
        raise ValueError("%d levels from a size of %d" % (count, x.shape[2]))
    out, g = [], x
    for _ in range(count - 1):
        coarse = pyr_down(g)
        out.append(pyr_residual(g, coarse, out=None if g is x else g))          # a map of our own: in place
        g = coarse
    out.append(g.clone() if g is x else g)
    return out


def _descriptor_args(level, pos, P):
    level = _gpu(level, "level")
    pos = _gpu(pos, "pos", torch.int32)
    if level.dim() != 4 or level.shape[1] != 3 or level.shape[2] != level.shape[3] or level.shape[2] < PATCH:
        raise ValueError("level must be [N, 3, S, S] with S >= %d, got %s" % (PATCH, tuple(level.shape)))
    N, S, P = int(level.shape[0]), int(level.shape[2]), int(P)
    if P < 1 or tuple(pos.shape) != (N * P, 2):
        raise ValueError("pos must be int32 [N * P, 2] = [%d, 2], got %s" % (N * P, tuple(pos.shape)))
    return level, pos, N, S, P


def descriptor_stats(level, pos, P):
    """fp32 [6] on the device: (mu_0, mu_1, mu_2, 1/sigma_0, 1/sigma_1, 1/sigma_2) over every value of the N P descriptors of
    `level` [N, 3, S, S] at `pos` int32 [N P, 2] = (y, x) in [0, S - 7].  fp64 sums in a fixed order."""
    from ._lib import check, lib
    L = lib()
    level, pos, N, S, P = _descriptor_args(level, pos, P)
    stats = torch.empty(6, dtype=torch.float32, device=level.device)
    ws = torch.empty(L.locate_swd_stats_workspace_bytes() // 8, dtype=torch.float64, device=level.device)
    check(L.locate_swd_stats(_ptr(level), N, S, _ptr(pos), P, _ptr(stats), _ptr(ws), _stream()), "locate_swd_stats")
    return stats


def project_descriptors(level, pos, P, dirs, stats):
    """fp32 [D, N P], direction-major: proj[d, j] = sum_k dirs[k, d] (v_jk - mu_c) r_c for dirs fp32 [147, D]."""
    from ._lib import check, lib
    level, pos, N, S, P = _descriptor_args(level, pos, P)
    dirs, stats = _gpu(dirs, "dirs"), _gpu(stats, "stats")
    if dirs.dim() != 2 or dirs.shape[0] != K or dirs.shape[1] < 1 or tuple(stats.shape) != (6,):
        raise ValueError("dirs must be [%d, D] and stats [6], got %s and %s" % (K, tuple(dirs.shape), tuple(stats.shape)))
    D = int(dirs.shape[1])
    proj = torch.empty(D, N * P, dtype=torch.float32, device=level.device)
    check(lib().locate_swd_project(_ptr(level), N, S, _ptr(pos), P, _ptr(dirs), D, _ptr(stats), _ptr(proj), _stream()), "locate_swd_project")
    return proj


def sorted_distance(a, b, out=None):
    """mean |a - b| over all elements of two equally shaped fp32 tensors (two sorted projection sets), as a one-element device
    tensor (`out` when given: a contiguous fp32 tensor of one element).  Nothing is read on the host here."""
    from ._lib import check, lib
    L = lib()
    a, b = _gpu(a, "a"), _gpu(b, "b")
    if a.shape != b.shape or a.numel() == 0:
        raise ValueError("sorted_distance takes two equally shaped, non-empty tensors, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=a.device)
    elif not torch.is_tensor(out) or out.numel() != 1 or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a one-element fp32 tensor on %s" % a.device)
    ws = torch.empty(L.locate_swd_distance_workspace_bytes() // 8, dtype=torch.float64, device=a.device)
    check(L.locate_swd_distance(_ptr(a), _ptr(b), a.numel(), _ptr(out), _ptr(ws), _stream()), "locate_swd_distance")
    return out


class SlicedWasserstein(FixedLatents):
    """SWD of a candidate image set against a cached reference set, both of `images` fp32 [3, S, S] images.

    All randomness is drawn at construction from ONE CPU `torch.Generator` seeded `seed`, in this order: `directions` (float64
    normal [147, R D_r], columns normalised, cast to fp32), then per level `positions["reference"][l]` and
    `positions["candidate"][l]` (two independent int32 [N P, 2] tables of (y, x) in [0, S_l - 7]).  `latents` [N, g_in] is drawn
    on the device on first use, from a generator seeded `seed + 3`.  All are public attributes; nothing needs saving for a resume,
    the seed reproduces them.

    Memory: the cached reference is the sorted projections, N P R D_r 4 bytes PER LEVEL - 1 GiB per level at the defaults
    (4096 128 4 128 4), 3 GiB at 64 x 64 - beside the level buffers of the set being measured (N 3 S^2 4 bytes 4/3).  One repeat
    ([D_r, N P]) is sorted at a time, so the sort's temporaries (values and int64 indices) stay below 1 GiB at the defaults.
    Karras et al. use N = 16384.

    `chunk` is part of the metric's definition: evaluate() sends the latents through the generator `chunk` at a time, and
    InPlaceNorm takes its statistics over the batch it sees.  Compare values only between runs with the same chunk.

    Under data parallelism only rank 0 should evaluate (as with `Sampler`): the metric runs on one device."""

    latent_seed = 3

    def __init__(self, S, images=4096, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=999, chunk=64, device="cuda"):
        self.sizes = pyramid_levels(S)
        self.S, self.images, self.nhoods_per_image = int(S), int(images), int(nhoods_per_image)
        self.dir_repeats, self.dirs_per_repeat, self.seed, self.chunk = int(dir_repeats), int(dirs_per_repeat), int(seed), int(chunk)
        if min(self.images, self.nhoods_per_image, self.dir_repeats, self.dirs_per_repeat, self.chunk) < 1:
            raise ValueError("images, nhoods_per_image, dir_repeats, dirs_per_repeat and chunk must be >= 1")
        FixedLatents.__init__(self, device)
        rng = torch.Generator().manual_seed(self.seed)
        d = torch.randn(K, self.dir_repeats * self.dirs_per_repeat, dtype=torch.float64, generator=rng)
        self.directions = (d / d.square().sum(0, keepdim=True).sqrt()).to(torch.float32)
        n = self.images * self.nhoods_per_image
        self.positions = {"reference": [], "candidate": []}
        for s in self.sizes:
            for which in ("reference", "candidate"):
                self.positions[which].append(torch.randint(0, s - PATCH + 1, (n, 2), generator=rng, dtype=torch.int32))
        self._dev = None
        self._reference = None

    # ---- device copies, made on first use (construction needs no GPU) ----
    def _device_tables(self):
        if self._dev is None:
            self._need_gpu()
            R, Dr = self.dir_repeats, self.dirs_per_repeat
            self._dev = {"dirs": [self.directions[:, r * Dr:(r + 1) * Dr].contiguous().to(self.device) for r in range(R)],
                         "reference": [p.to(self.device) for p in self.positions["reference"]],
                         "candidate": [p.to(self.device) for p in self.positions["candidate"]]}
        return self._dev

    # ---- the two halves ----
    def _levels(self, batches):
        """The level buffers [N, 3, S_l, S_l] of a whole set, filled batch by batch."""
        if torch.is_tensor(batches):
            batches = (batches,)
        buffers, at = None, 0
        for x in batches:
            x = _gpu(x, "images")
            if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.S, self.S):
                raise ValueError("images must be [n, 3, %d, %d], got %s" % (self.S, self.S, tuple(x.shape)))
            if at + x.shape[0] > self.images:
                raise ValueError("more than the %d images this metric was built for" % self.images)
            if buffers is None:
                buffers = [torch.empty(self.images, 3, s, s, dtype=torch.float32, device=x.device) for s in self.sizes]
            for buf, level in zip(buffers, laplacian_pyramid(x, len(self.sizes))):
                buf[at:at + x.shape[0]].copy_(level)
            at += x.shape[0]
        if at != self.images:
            raise ValueError("%d images given, this metric was built for %d" % (at, self.images))
        return buffers

    def _sorted_projections(self, levels, which):
        """per level and repeat: stats -> project -> sort.  [L][R] tensors [D_r, N P], every row ascending."""
        dev = self._device_tables()
        out = []
        for l, level in enumerate(levels):
            pos = dev[which][l]
            stats = descriptor_stats(level, pos, self.nhoods_per_image)
            out.append([torch.sort(project_descriptors(level, pos, self.nhoods_per_image, dirs, stats), dim=1).values for dirs in dev["dirs"]])
        return out

    def _compare(self, ref, cand):
        R = self.dir_repeats
        values = torch.empty(len(self.sizes) * R, dtype=torch.float32, device=ref[0][0].device)
        for l in range(len(self.sizes)):
            for r in range(R):
                sorted_distance(ref[l][r], cand[l][r], out=values[l * R + r:l * R + r + 1])
        host = values.cpu().tolist()          # the one host copy: L R floats
        levels = [sum(host[l * R:(l + 1) * R]) / R for l in range(len(self.sizes))]
        return {"levels": levels, "mean": sum(levels) / len(levels)}

    def set_reference(self, batches):
        """batches: one [N, 3, S, S] tensor or an iterable of batches summing to N.  Keeps the sorted projections."""
        self._reference = self._sorted_projections(self._levels(batches), "reference")
        return self

    @property
    def has_reference(self):
        return self._reference is not None

    def distance(self, batches):
        """{"levels": [per level], "mean": float} of the candidate set against the cached reference."""
        self._need_reference()
        return self._against_reference(self._levels(batches))

    def _need_reference(self):
        if self._reference is None:
            raise RuntimeError("set_reference() first")

    def _against_reference(self, levels):
        return self._compare(self._reference, self._sorted_projections(levels, "candidate"))

    def between(self, a, b, same_positions=False):
        """Both halves without caching: a takes the reference's positions, b the candidate's (or, with same_positions, a's)."""
        ref = self._sorted_projections(self._levels(a), "reference")
        return self._compare(ref, self._sorted_projections(self._levels(b), "reference" if same_positions else "candidate"))

    def reference_from_pipeline(self, pipeline):
        """set_reference() with N images of the plain chain: the first output of `InputPipeline.next_batch()`, from a pipeline of
        this metric's own over the same store, seeded seed + 2 - the training pipeline's shuffle is not advanced."""
        return self.set_reference(plain_batches(pipeline, self.S, self.images, self.seed, self.images))

    def evaluate(self, gen):
        """distance() of the generator's images of the fixed latents: eval mode, no_grad, `chunk` latents per forward.  Every
        spectral-norm u / v is snapshotted before and copied back in place after, and the training mode restored: no side effect
        on the training, eager or replayed.  Call it between two iterations, never inside one."""
        self._need_reference()
        with self._sampling(gen):
            levels = self._levels(batches(gen, self.latents(gen.g_in), self.chunk))
        return self._against_reference(levels)
