"""Nearest training images of generated samples, exact: the figure "sample | its nearest training images" and the distances
behind it.  The sliced Wasserstein distance compares patch statistics of two sets; it cannot tell whether the samples are copies
of training images (memorisation) or all the same picture (collapse).  The reference has nothing of the kind; this is an addition.

Everything is computed in the 8-bit domain (csrc/neighbours.hip through the C ABI, include/locate_hip.h):
  * the code of an image is, per element, the byte its value quantises to - rint((x + 1) 127.5) clamped to [0, 255] - minus 128, as
    int8, in rows of `row_bytes(S)` bytes.  `data.output_lut()` inverts exactly (rint((lut[u] + 1) 127.5) == u for all 256 bytes),
    so the code of a store image's view is its Pillow byte minus 128;
  * the squared distance of two codes is an integer, |q|^2 + |r|^2 - 2 q.r with the dot product on the int8 matrix instruction:
    exact, where `torch.cdist` over dequantised fp32 copies loses the case that matters - a distance near 0 - to cancellation;
  * the search returns, per query, the k references with the smallest (d2, index): ties resolve to the lower index.

Memory: the bank is N row_bytes(S) bytes (CelebA at 64 x 64: 2.4 GB), the search's workspace Q ceil(N / 128) k 8 bytes.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import numpy as np
import torch

from .sampling import FixedLatents, _gpu, _ptr, _stream

K_MAX = 8
BANK_CHUNK = 1024          # images per transform call while the bank is built (the entry point takes at most 65535)


def row_bytes(S):
    """Bytes of one code row: 3 S^2 rounded up to a multiple of 64."""
    return (3 * int(S) * int(S) + 63) // 64 * 64


def _encode_into(x, codes, norms, flags):
    from ._lib import check, lib
    n, S = int(x.shape[0]), int(x.shape[2])
    check(lib().locate_nn_encode(_ptr(x), n, S, _ptr(codes), _ptr(norms), _ptr(flags), _stream()), "locate_nn_encode")


def encode_images(x):
    """x: fp32 [n, 3, S, S] on the GPU -> (codes int8 [n, row_bytes(S)], norms int64 [n], nonfinite int32 [n]).  One pass; an image
    whose count of NaN / Inf elements is not 0 is flagged: the search gives it no neighbours and never returns it."""
    x = _gpu(x, "x", torch.float32)
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or not 1 <= x.shape[2] <= 4096:
        raise ValueError("encode_images takes fp32 [n, 3, S, S], got %s" % (tuple(x.shape),))
    n, S = int(x.shape[0]), int(x.shape[2])
    codes = torch.empty(n, row_bytes(S), dtype=torch.int8, device=x.device)
    norms = torch.empty(n, dtype=torch.int64, device=x.device)
    flags = torch.empty(n, dtype=torch.int32, device=x.device)
    _encode_into(x, codes, norms, flags)
    return codes, norms, flags


def _triple(t, name, flags_optional=False):
    if not isinstance(t, (tuple, list)) or len(t) != 3:
        raise ValueError("%s must be a (codes, norms, flags) triple" % name)
    codes, norms = _gpu(t[0], name + " codes", torch.int8), _gpu(t[1], name + " norms", torch.int64)
    flags = None if (flags_optional and t[2] is None) else _gpu(t[2], name + " flags", torch.int32)
    if codes.dim() != 2 or codes.shape[0] < 1 or codes.shape[1] < 64 or codes.shape[1] % 64:
        raise ValueError("%s codes must be int8 [n, row_bytes] with row_bytes a multiple of 64, got %s" % (name, tuple(codes.shape)))
    n = codes.shape[0]
    if tuple(norms.shape) != (n,) or (flags is not None and tuple(flags.shape) != (n,)):
        raise ValueError("%s norms and flags must be [%d]" % (name, n))
    return codes, norms, flags


def nearest(q, r, k=3, skip=None):
    """q, r: (codes, norms, flags) triples as encode_images returns them (r's flags may be None: none flagged), rows of equal length.
    Returns (d2 int64 [Q, k], index int32 [Q, k]) on the device: per query the k references with the smallest (d2, index), -1 / -1
    in empty slots and in every slot of a flagged query.  skip: int32 [Q] on the device, the one reference index query i must not
    return (-1: none) - "nearest OTHER image" when q is part of r.  Nothing is read on the host."""
    from ._lib import check, lib
    L = lib()
    qc, qn, qf = _triple(q, "q")
    rc, rn, rf = _triple(r, "r", flags_optional=True)
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("k must be 1 .. %d, got %d" % (K_MAX, k))
    if qc.shape[1] != rc.shape[1] or qc.device != rc.device:
        raise ValueError("q and r must have rows of equal length on one device, got %s and %s" % (tuple(qc.shape), tuple(rc.shape)))
    Q, N = int(qc.shape[0]), int(rc.shape[0])
    if skip is not None:
        skip = _gpu(skip, "skip", torch.int32)
        if tuple(skip.shape) != (Q,):
            raise ValueError("skip must be int32 [%d], got %s" % (Q, tuple(skip.shape)))
    d2 = torch.empty(Q, k, dtype=torch.int64, device=qc.device)
    index = torch.empty(Q, k, dtype=torch.int32, device=qc.device)
    ws = torch.empty(max(L.locate_nn_search_workspace_bytes(Q, N, k) // 8, 1), dtype=torch.int64, device=qc.device)
    check(L.locate_nn_search(_ptr(qc), _ptr(qn), _ptr(qf), Q, _ptr(rc), _ptr(rn), _ptr(rf), N, int(qc.shape[1]), _ptr(skip), k,
                             _ptr(d2), _ptr(index), _ptr(ws), _stream()), "locate_nn_search")
    return d2, index


def canonical_params(n, H, W):
    """n records (data.PARAM_DTYPE) of the canonical view of an H x W store image: the centred square of side min(H, W), no flip,
    no jitter - the record `data.draw_params` falls back to."""
    from .data import PARAM_DTYPE, PLAIN_ORDER
    side = min(int(H), int(W))
    rec = np.zeros(int(n), dtype=PARAM_DTYPE)
    rec["side"], rec["top"], rec["left"] = side, (int(H) - side) // 2, (int(W) - side) // 2
    rec["order"] = PLAIN_ORDER
    rec["brightness"] = rec["contrast"] = rec["saturation"] = 1.0
    return rec


def rms(d2, S):
    """A squared code distance as the RMS difference per element on the [-1, 1] scale; None for -1 (no neighbour)."""
    return None if d2 < 0 else float(np.sqrt(d2 / (3.0 * S * S)) / 127.5)


def summary(values):
    """{"min", "median"} of the values that are not None (both None if there are none)."""
    v = np.asarray([x for x in values if x is not None], dtype=np.float64)
    if v.size == 0:
        return {"min": None, "median": None}
    return {"min": float(v.min()), "median": float(np.median(v))}


class CanonicalViews:
    """The canonical views of a store's images at size S: the centred square of side min(H, W), no flip, no jitter, resized to S by
    `data.transform`.  State: S, the store (None until one is given) and the cached `data._Plan`."""

    def __init__(self, S, store=None):
        self.S, self.store, self._plan = int(S), store, None
        if self.S < 4 or self.S % 4 or self.S > 4096:
            raise ValueError("image size %d: the input pipeline writes 16-byte groups, S must be a multiple of 4" % self.S)

    def views(self, index):
        """fp32 [n, 3, S, S]: the canonical views of the store images `index` (a sequence of store indices)."""
        from ._lib import lib
        from .data import _Plan, transform, validate
        if self.store is None:
            raise RuntimeError("reference_from_store() first")
        store = self.store
        idx = np.asarray(index, dtype=np.int32).reshape(-1)
        if self._plan is None:
            self._plan = _Plan(store.H, store.W, self.S, min(store.H, store.W), store.device)
        out = torch.empty(idx.size, 3, self.S, self.S, dtype=torch.float32, device=store.device)
        for a in range(0, idx.size, BANK_CHUNK):
            part = idx[a:a + BANK_CHUNK]
            n = int(part.size)
            params = canonical_params(n, store.H, store.W)
            validate(part, params, store.N, store.H, store.W, self._plan.side_lo, self._plan.side_hi)
            idx_dev = torch.from_numpy(np.ascontiguousarray(part)).to(store.device)
            params_dev = torch.from_numpy(params.view(np.uint8).copy()).to(store.device)
            ws = torch.empty(max(lib().locate_input_workspace_bytes(n, store.H, store.W), 16), dtype=torch.uint8, device=store.device)
            transform(store, idx_dev, params_dev, n, n, self._plan, self.S, out[a:a + n], None, ws)
        return out

    def encode(self, index):
        """The (codes, norms, flags) triple of those views, `BANK_CHUNK` views at a time: never more than that many are held in fp32."""
        if self.store is None:
            raise RuntimeError("reference_from_store() first")
        idx = np.asarray(index, dtype=np.int32).reshape(-1)
        dev = self.store.device
        codes = torch.empty(idx.size, row_bytes(self.S), dtype=torch.int8, device=dev)
        norms = torch.empty(idx.size, dtype=torch.int64, device=dev)
        flags = torch.empty(idx.size, dtype=torch.int32, device=dev)
        for a in range(0, idx.size, BANK_CHUNK):
            b = a + BANK_CHUNK
            _encode_into(self.views(idx[a:b]), codes[a:b], norms[a:b], flags[a:b])
        return codes, norms, flags


def _sample_args(S, k, images, chunk):
    """The checks `NearestNeighbours`, `ManifoldMetrics` and `BinnedModes` share, in their order; returns the `CanonicalViews`."""
    if not 1 <= k <= K_MAX:
        raise ValueError("k must be 1 .. %d, got %d" % (K_MAX, k))
    views = CanonicalViews(S)
    if images < 1 or chunk < 1:
        raise ValueError("images and chunk must be >= 1")
    return views


class NearestNeighbours(FixedLatents):
    """Nearest training images of `images` generated samples of size S, k (1 .. 8) per sample.

    The bank is `reference_from_store(store)`: every store image's canonical view - the centred square of side min(H, W), no flip,
    no jitter, resized to S by `data.transform` - encoded; it then holds Pillow's bytes minus 128.  N row_bytes(S) bytes of device
    memory.  Two baselines are computed with it, once, from `images` distinct bank indices drawn from a CPU generator seeded
    `seed + 5` (`baseline_index`): `real_to_real`, each drawn image's nearest OTHER bank row, and `real_among_themselves`, the nearest
    other WITHIN the drawn set - the yardstick for the generated set's own diversity at the same set size.

    Reading a record: `generated_to_real.median` far below `real_to_real.median` means memorisation;
    `generated_to_generated.median` far below `real_among_themselves.median` means collapse.

    `chunk` latents go through the generator per forward in evaluate(): InPlaceNorm takes its statistics over the batch it sees,
    so compare values only between runs with the same chunk.  The fixed latents [images, g_in] are drawn on the device on first
    use from a generator seeded `seed + 6`.  Construction needs no GPU.  Under data parallelism only rank 0 should evaluate."""

    latent_seed = 6

    def __init__(self, S, k=3, images=64, seed=999, chunk=64, device="cuda"):
        self.S, self.k, self.images, self.seed, self.chunk = int(S), int(k), int(images), int(seed), int(chunk)
        self._canonical = _sample_args(self.S, self.k, self.images, self.chunk)
        FixedLatents.__init__(self, device)
        self.row_bytes = row_bytes(self.S)
        self.bank = None
        self.baseline_index = None
        self.real_to_real = None
        self.real_among_themselves = None

    # ---- the bank -------------------------------------------------------------------------------------------------------------
    @property
    def store(self):
        return self._canonical.store

    @property
    def has_reference(self):
        return self.bank is not None

    def _need_reference(self):
        if self.bank is None:
            raise RuntimeError("reference_from_store() first")

    def canonical_views(self, index):
        """fp32 [n, 3, S, S]: the canonical views of the store images `index` (a sequence of store indices)."""
        return self._canonical.views(index)

    def reference_from_store(self, store, limit=None):
        """The bank: the canonical view of the first `limit` store images (default: all), encoded `BANK_CHUNK` images at a time; then
        the two baselines (one small device-to-host copy)."""
        self._need_gpu()
        N = len(store) if limit is None else min(int(limit), len(store))
        if N < 1:
            raise ValueError("an empty bank")
        self._canonical = CanonicalViews(self.S, store)
        dev = store.device
        self.bank = codes, norms, flags = self._canonical.encode(range(N))
        m = min(self.images, N)
        drawn = torch.randperm(N, generator=torch.Generator().manual_seed(self.seed + 5))[:m].to(torch.int32)
        self.baseline_index = drawn.tolist()
        at = drawn.to(dev)
        pick = at.long()
        subset = (codes[pick].contiguous(), norms[pick].contiguous(), flags[pick].contiguous())
        to_bank, _ = nearest(subset, self.bank, k=1, skip=at)
        among, _ = nearest(subset, subset, k=1, skip=torch.arange(m, dtype=torch.int32, device=dev))
        host = torch.cat([to_bank, among], dim=1).cpu().tolist()
        self.real_to_real = summary([rms(row[0], self.S) for row in host])
        self.real_among_themselves = summary([rms(row[1], self.S) for row in host])
        return self

    # ---- searching ------------------------------------------------------------------------------------------------------------
    def search(self, images):
        """images: any fp32 [Q, 3, S, S] device batch.  The record documented on evaluate(); ONE device-to-host copy."""
        self._need_reference()
        if torch.is_tensor(images) and images.is_cuda and (images.dim() != 4 or tuple(images.shape[1:]) != (3, self.S, self.S)):
            raise ValueError("images must be [Q, 3, %d, %d], got %s" % (self.S, self.S, tuple(images.shape)))
        q = encode_images(images)
        Q, k = int(q[0].shape[0]), self.k
        d2, index = nearest(q, self.bank, k=k)
        own, _ = nearest(q, q, k=1, skip=torch.arange(Q, dtype=torch.int32, device=q[0].device))
        host = torch.cat([d2, index.to(torch.int64), own, q[2].to(torch.int64).reshape(Q, 1)], dim=1).cpu().tolist()          # the one host copy
        value = {"images": Q, "k": k,
                 "index": [row[k:2 * k] for row in host],
                 "d2": [row[:k] for row in host]}
        value["rms"] = [rms(row[0], self.S) for row in host]
        value["generated_to_real"] = summary(value["rms"])
        value["generated_to_generated"] = summary([rms(row[2 * k], self.S) for row in host])
        value["real_to_real"] = dict(self.real_to_real)
        value["real_among_themselves"] = dict(self.real_among_themselves)
        value["nonfinite"] = sum(1 for row in host if row[2 * k + 1] != 0)
        return value

    def generate(self, gen, latents=None):
        """fp32 [Q, 3, S, S]: the generator's images of `latents` (default: the fixed ones) - eval mode, no_grad, `chunk` latents per
        forward.  Every spectral-norm u / v is snapshotted before and copied back in place after, and the training mode restored: no
        side effect on the training, eager or replayed.  Call it between two iterations, never inside one."""
        return self._generate(gen, latents)

    def evaluate(self, gen, latents=None):
        """search() of generate(gen, latents).  Returns
          "images", "k"; "index" [Q][k] and "d2" [Q][k]: each sample's k nearest bank rows and their squared code distances (-1
          where there is none: a flagged sample, fewer than k rows); "rms" [Q]: the nearest one's distance as sqrt(d2 / (3 S^2)) /
          127.5 - RMS per element on the [-1, 1] scale - or None; {"min", "median"} of it as "generated_to_real", of each sample's
          nearest OTHER sample as "generated_to_generated", and the bank's two baselines "real_to_real" and "real_among_themselves";
          "nonfinite": the number of samples that hold a NaN or an Inf."""
        self._need_reference()
        return self.search(self.generate(gen, latents))

    def save_picture(self, path, gen, latents=None):
        """A PNG of Q rows [sample | the canonical views of its k nearest training images] (a missing neighbour is black)."""
        from .monitor import image_grid, write_png
        self._need_reference()
        images = self.generate(gen, latents)
        Q, k = int(images.shape[0]), self.k
        _, index = nearest(encode_images(images), self.bank, k=k)
        index = index.cpu().reshape(-1)
        found = index >= 0
        near = torch.full((Q * k, 3, self.S, self.S), -1.0, dtype=torch.float32, device=images.device)
        if bool(found.any()):
            near[found.to(images.device)] = self.canonical_views(index[found].numpy())
        tiles = torch.cat([images.reshape(Q, 1, 3, self.S, self.S), near.reshape(Q, k, 3, self.S, self.S)], dim=1)
        rgba = image_grid(tiles.reshape(Q * (k + 1), 3, self.S, self.S), nrow=k + 1, value_range=(-1, 1))
        return write_png(path, rgba.cpu())
