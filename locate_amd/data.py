"""Device-side input pipeline: the reference's two ImageFolder transform chains (libs/utils.py:88-113) on the GPU.

The reference decodes and transforms every image on the CPU, twice per step (a plain batch and an augmented one for the
penalty).  Here the deterministic part - decode + Resize(2 S) - is done once, offline (`prepare_folder`), the result lives in
device memory as uint8 [N, H, W, 3] (`DeviceImageStore`), and each step's random part - flip, colour jitter, square crop, resize
to S, ToTensor, Normalize - is one call into csrc/input.hip per batch pair (`InputPipeline.next_batch`), in Pillow's arithmetic
bit for bit (tests/test_input_golden.py, tests/test_gpu_input.py).

Importing this module loads neither the HIP library nor Pillow."""
import ctypes
import math
import os

import numpy as np
import torch

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
PLAIN_ORDER = 0x3333                  # four no-ops: the chain without jitter
PRECISION_BITS = 22                   # Pillow's fixed point for 8-bit channels

# one record per output sample: the layout of csrc/input.hip's InputParam (locate_input_param_record_bytes() = 32)
PARAM_DTYPE = np.dtype([("flip", "<i4"), ("order", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                        ("top", "<i4"), ("left", "<i4"), ("side", "<i4")])
assert PARAM_DTYPE.itemsize == 32

_IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def pack_order(ops):
    """Up to four op codes (0 brightness, 1 contrast, 2 saturation, 3 hue = nothing) as the record's `order` word."""
    ops = list(ops) + [HUE] * (4 - len(ops))
    return sum((int(op) & 15) << (4 * k) for k, op in enumerate(ops[:4]))


def min_crop_side(H, W, min_crop_part=0.75):
    return int(round(math.sqrt(H * W * min_crop_part)))


def draw_params(generator, n, H, W, S, augment, jitter=0.2, min_crop_part=0.75):
    """n parameter records (numpy, PARAM_DTYPE) for images of H x W, on the host.

    The aim is the DISTRIBUTION of the reference's transforms - RandomResizedCrop(S, (min_crop_part, 1), (1, 1)).get_params,
    ColorJitter(jitter, jitter, jitter).get_params, RandomHorizontalFlip(0.5) - not torchvision's random stream: a seed here
    does not reproduce the crops a torchvision run would draw from the same seed.

    Crop: up to 10 tries of side = int(round(sqrt(H W U(min_crop_part, 1)))), the first with side <= min(H, W) is taken with
    top = randint(0, H - side), left = randint(0, W - side) (inclusive); if none fits, the centred square of side min(H, W).
    Jitter (augment only): a random permutation of the four ops (hue is a no-op, as in the reference) and a factor from
    U(1 - jitter, 1 + jitter) for each of brightness, contrast, saturation.  Flip (augment only): p = 0.5.

    Draw order from `generator` (a CPU torch.Generator), all float64 `torch.rand`: [n, 10] crop areas; [n, 2] crop positions
    (top, left); then, with augment, [n] flips, [n, 4] permutation keys (the order is their argsort), [n, 3] factors.
    S does not enter the draws (the crop is a share of the source area); it is part of the signature because the records are
    only meaningful for one output size."""
    if n < 0 or H < 1 or W < 1 or S < 1:
        raise ValueError("draw_params: bad sizes")
    rec = np.zeros(n, dtype=PARAM_DTYPE)
    rand = lambda *shape: torch.rand(*shape, generator=generator, dtype=torch.float64).numpy()      # noqa: E731
    area = rand(n, 10) * (1.0 - min_crop_part) + min_crop_part
    pos = rand(n, 2)
    sides = np.rint(np.sqrt(H * W * area)).astype(np.int64)
    fits = sides <= min(H, W)
    first = np.argmax(fits, axis=1)
    ok = fits.any(axis=1)
    side = np.where(ok, sides[np.arange(n), first], min(H, W))
    top = np.minimum((pos[:, 0] * (H - side + 1)).astype(np.int64), H - side)
    left = np.minimum((pos[:, 1] * (W - side + 1)).astype(np.int64), W - side)
    rec["side"] = side
    rec["top"] = np.where(ok, top, (H - side) // 2)
    rec["left"] = np.where(ok, left, (W - side) // 2)
    rec["order"] = PLAIN_ORDER
    rec["brightness"] = rec["contrast"] = rec["saturation"] = 1.0
    if augment:
        rec["flip"] = rand(n) < 0.5
        perm = np.argsort(rand(n, 4), axis=1)
        rec["order"] = sum(perm[:, k].astype(np.int32) << (4 * k) for k in range(4))
        f = rand(n, 3) * (2.0 * jitter) + (1.0 - jitter)
        rec["brightness"], rec["contrast"], rec["saturation"] = f[:, 0], f[:, 1], f[:, 2]
    return rec


def resize_table(side_lo, side_hi, S):
    """Pillow's BILINEAR (antialiased triangle filter) taps for every crop side in [side_lo, side_hi] -> S, computed in double
    on the host: int32 [sides][S][2 + ktaps] = {first tap, tap count, floor(0.5 + w 2^22)...}, and ktaps."""
    rows = []
    for side in range(side_lo, side_hi + 1):
        scale = side / S
        fs = max(scale, 1.0)
        per = []
        for i in range(S):
            c = (i + 0.5) * scale
            x0 = max(int(c - fs + 0.5), 0)
            x1 = min(int(c + fs + 0.5), side)
            w = np.maximum(0.0, 1.0 - np.abs((np.arange(x0, x1, dtype=np.float64) - c + 0.5) / fs))
            w = w / w.sum()
            per.append((x0, np.floor(0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)))
        rows.append(per)
    ktaps = max(len(k) for per in rows for _, k in per)
    table = np.zeros((len(rows), S, 2 + ktaps), dtype=np.int32)
    for a, per in enumerate(rows):
        for i, (x0, k) in enumerate(per):
            table[a, i, 0], table[a, i, 1] = x0, len(k)
            table[a, i, 2:2 + len(k)] = k
    return table, ktaps


def output_lut():
    """The 256 values of ToTensor + Normalize(0.5, 0.5): u8 / 255 in fp32 (correctly rounded), then (x - 0.5) / 0.5 in fp32."""
    x = torch.arange(256, dtype=torch.float32) / 255.0
    return (x - 0.5) / 0.5


def validate(idx, params, N, H, W, side_lo, side_hi):
    """What the kernel cannot check for the caller: indices inside the store, crops inside the image."""
    idx = np.asarray(idx)
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        raise ValueError("image index outside the store of %d images" % N)
    if len(params) != idx.size:
        raise ValueError("%d parameter records for %d indices" % (len(params), idx.size))
    side, top, left = params["side"], params["top"], params["left"]
    if params.size and (side.min() < side_lo or side.max() > side_hi or top.min() < 0 or left.min() < 0
                        or (top + side).max() > H or (left + side).max() > W):
        raise ValueError("crop outside the %d x %d image or side outside [%d, %d]" % (H, W, side_lo, side_hi))


def prepare_folder(src_dir, out_npy, image_size):
    """The reference's offline part: every image under src_dir (sorted walk, as ImageFolder lists them), decoded to RGB and
    resized like torchvision's Resize(2 * image_size) - smaller edge to 2 S, longer edge int(2 S long / short), BILINEAR -
    into one uint8 [N, H, W, 3] .npy file.  All images must come out at one size.  Returns the shape."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("prepare_folder decodes images with Pillow, which is not installed; "
                           "nothing else in locate_amd needs it (a prepared .npy file can be made elsewhere)") from e
    paths = []
    for dirpath, dirnames, files in os.walk(src_dir):
        dirnames.sort()
        paths += [os.path.join(dirpath, f) for f in sorted(files) if f.lower().endswith(_IMAGE_SUFFIXES)]
    if not paths:
        raise ValueError("no images under %s" % src_dir)
    target = 2 * int(image_size)
    out = None
    for i, path in enumerate(paths):
        with Image.open(path) as im:
            im = im.convert("RGB")
            w, h = im.size
            size = (target, int(target * h / w)) if w <= h else (int(target * w / h), target)
            arr = np.asarray(im.resize(size, Image.BILINEAR))
        if out is None:
            out = np.lib.format.open_memmap(out_npy, mode="w+", dtype=np.uint8, shape=(len(paths),) + arr.shape)
        if arr.shape != out.shape[1:]:
            raise ValueError("%s resizes to %s, the images before it to %s: the store holds one size" % (path, arr.shape, out.shape[1:]))
        out[i] = arr
    out.flush()
    return out.shape


class DeviceImageStore:
    """uint8 [N, H, W, 3] resident on the device, from a numpy array or a .npy file (memory-mapped, uploaded in chunks)."""

    def __init__(self, array_or_path, device="cuda", chunk_bytes=256 << 20):
        src = np.load(array_or_path, mmap_mode="r") if isinstance(array_or_path, (str, os.PathLike)) else np.asarray(array_or_path)
        if src.dtype != np.uint8 or src.ndim != 4 or src.shape[3] != 3 or src.shape[0] < 1:
            raise ValueError("an image store is uint8 [N, H, W, 3], got %s %s" % (src.dtype, src.shape))
        self.N, self.H, self.W = (int(d) for d in src.shape[:3])
        if torch.device(device).type != "cuda":
            raise TypeError("DeviceImageStore lives in GPU memory; there is no CPU path")
        self.data = torch.empty(src.shape, dtype=torch.uint8, device=device)
        self.device = self.data.device
        per = max(1, chunk_bytes // (self.H * self.W * 3))
        for a in range(0, self.N, per):
            self.data[a:a + per].copy_(torch.from_numpy(np.array(src[a:a + per])))

    def __len__(self):
        return self.N


class _Plan:
    """Device-side constants of one (store geometry, S): tap table, output values."""

    def __init__(self, H, W, S, side_lo, device):
        self.side_lo, self.side_hi = int(side_lo), min(H, W)
        table, self.ktaps = resize_table(self.side_lo, self.side_hi, S)
        self.coef = torch.from_numpy(table).to(device)
        self.lut = output_lut().to(device)


def transform(store, idx_dev, params_dev, n, n_first, plan, S, out_first, out_rest, workspace):
    """The C-ABI call (csrc/input.hip) on the current stream.  idx_dev / params_dev are device buffers the caller has validated."""
    from ._lib import check, lib
    L = lib()
    need = L.locate_input_workspace_bytes(n, store.H, store.W)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError("workspace of %d bytes, %d needed" % (workspace.numel() * workspace.element_size(), need))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    check(L.locate_input_transform(ptr(store.data), store.N, store.H, store.W, ptr(idx_dev), ptr(params_dev), n, n_first,
                                   ptr(plan.coef), plan.side_lo, plan.side_hi, plan.ktaps, ptr(plan.lut), S, ptr(out_first),
                                   ptr(out_rest), ptr(workspace), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "locate_input_transform")


class InputPipeline:
    """Batches for `TrainStep` / `TrainLoop` / `GraphedTrainStep` from a `DeviceImageStore`: `next_batch()` returns
    (real, aug), fp32 [batch, 3, S, S] each, like one step of the reference's two DataLoader(shuffle=True, drop_last=True)
    over its plain and its augmented ImageFolder - two independent shuffles without replacement, the tail of an epoch dropped.

    Per batch pair: the host draws the 2 x batch records (`draw_params`), writes them with the image indices into a pinned
    buffer, one asynchronous copy takes them to the device and one library call transforms both batches, all on the current
    stream.  The host never waits for the GPU unless it runs more than `SLOTS` batches ahead of it.  Call it from one stream at
    a time: consecutive batches share the workspace and a ring of `SLOTS` record buffers, ordered by that stream.

    `overfit=True` keeps returning the first pair (OVERFIT in the reference's main.py:122-136).
    Data-parallel ranks pass different seeds and shuffle on their own."""
    SLOTS = 4

    def __init__(self, store, S, batch, seed, overfit=False, jitter=0.2, min_crop_part=0.75):
        if batch < 1 or batch > len(store):
            raise ValueError("batch of %d from a store of %d images" % (batch, len(store)))
        if S < 4 or S % 4:
            raise ValueError("image size %d: the kernel writes 16-byte groups, S must be a multiple of 4" % S)
        self.store, self.S, self.batch, self.overfit = store, int(S), int(batch), bool(overfit)
        self.jitter, self.min_crop_part = jitter, min_crop_part
        self.side_lo = min(min_crop_side(store.H, store.W, min_crop_part), store.H, store.W)
        self.batches_per_epoch = len(store) // self.batch
        self._shuffle_gen = torch.Generator().manual_seed(int(seed))
        self._param_gen = torch.Generator().manual_seed(int(seed) + 0x5EED)
        self.epoch, self.pos = 0, 0
        self._start_epoch()
        self._first = None
        self._dev = None

    # ---- host bookkeeping (no GPU needed) ----
    def _start_epoch(self):
        self._epoch_state = self._shuffle_gen.get_state()
        n = len(self.store)
        self._perm_real = torch.randperm(n, generator=self._shuffle_gen).numpy()
        self._perm_aug = torch.randperm(n, generator=self._shuffle_gen).numpy()

    def _draw(self):
        """Indices [2 batch] (plain first) and records [2 batch] of the next batch pair; advances the position."""
        if self.pos >= self.batches_per_epoch:
            self.epoch, self.pos = self.epoch + 1, 0
            self._start_epoch()
        a, b = self.pos * self.batch, (self.pos + 1) * self.batch
        self.pos += 1
        idx = np.concatenate([self._perm_real[a:b], self._perm_aug[a:b]]).astype(np.int32)
        H, W = self.store.H, self.store.W
        params = np.concatenate([draw_params(self._param_gen, self.batch, H, W, self.S, False, self.jitter, self.min_crop_part),
                                 draw_params(self._param_gen, self.batch, H, W, self.S, True, self.jitter, self.min_crop_part)])
        return idx, params

    def state_dict(self):
        return {"epoch": self.epoch, "pos": self.pos, "epoch_shuffle_state": self._epoch_state.clone(),
                "param_state": self._param_gen.get_state()}

    def load_state_dict(self, state):
        self.epoch, self.pos = int(state["epoch"]), int(state["pos"])
        self._shuffle_gen.set_state(state["epoch_shuffle_state"])
        self._start_epoch()                                   # the interrupted epoch's two permutations again
        self._param_gen.set_state(state["param_state"])

    # ---- device side ----
    def _ensure_device(self):
        if self._dev is None:
            from ._lib import lib
            dev, n = self.store.device, 2 * self.batch
            assert lib().locate_input_param_record_bytes() == PARAM_DTYPE.itemsize
            self._idx_bytes = (4 * n + 31) & ~31
            nbytes = self._idx_bytes + n * PARAM_DTYPE.itemsize
            self._dev = {
                "plan": _Plan(self.store.H, self.store.W, self.S, self.side_lo, dev),
                "pinned": [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.SLOTS)],
                "events": [None] * self.SLOTS,
                "device": [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(self.SLOTS)],
                "workspace": torch.empty(max(lib().locate_input_workspace_bytes(n, self.store.H, self.store.W), 16),
                                         dtype=torch.uint8, device=dev),
                "slot": 0,
            }
        return self._dev

    def _run(self, idx, params, out_real, out_aug):
        """Uploads one batch pair's indices and records (one pinned copy) and launches the transform on the current stream."""
        d = self._ensure_device()
        validate(idx, params, self.store.N, self.store.H, self.store.W, d["plan"].side_lo, d["plan"].side_hi)
        n, slot = 2 * self.batch, d["slot"]
        d["slot"] = (slot + 1) % self.SLOTS
        if d["events"][slot] is not None:
            d["events"][slot].synchronize()                   # only when the host is SLOTS batches ahead of the device
        host = d["pinned"][slot].numpy()
        host[:4 * n] = idx.astype("<i4").view(np.uint8)
        host[self._idx_bytes:] = params.view(np.uint8)
        dev_buf = d["device"][slot]
        dev_buf.copy_(d["pinned"][slot], non_blocking=True)
        d["events"][slot] = torch.cuda.Event()
        d["events"][slot].record()
        transform(self.store, dev_buf[:4 * n], dev_buf[self._idx_bytes:], n, self.batch, d["plan"], self.S, out_real, out_aug,
                  d["workspace"])

    def _check_out(self, t, name):
        shape = (self.batch, 3, self.S, self.S)
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=self.store.device)
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.store.device:
            raise ValueError("%s must be a contiguous fp32 %s tensor on %s" % (name, shape, self.store.device))
        return t

    def next_batch(self, out_real=None, out_aug=None):
        """(real, aug) of the next step; written into out_real / out_aug when given (e.g. a GraphedTrainStep's static inputs)."""
        out_real, out_aug = self._check_out(out_real, "out_real"), self._check_out(out_aug, "out_aug")
        if self.overfit and self._first is not None:
            for dst, src in zip((out_real, out_aug), self._first):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
            return out_real, out_aug
        idx, params = self._draw()
        self._run(idx, params, out_real, out_aug)
        if self.overfit:
            self._first = (out_real.clone(), out_aug.clone())
        return out_real, out_aug
