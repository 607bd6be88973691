"""Watching a run: the reference's only check on its training (main.py:55,174-234) - a picture of the generator's output for a
fixed latent batch, written as a PNG every `image_intervall` iterations and at the end of every pass, and the two loss curves.

The reference renders on the host: `gen(fnoise).detach().cpu()`, torchvision's `make_grid(padding=8, normalize=True)`, matplotlib's
`imsave`.  Here the picture is composed on the device (csrc/grid.hip through the C ABI: the same fp32 grid and the same RGBA
bytes, tests/test_grid_golden.py and tests/test_gpu_monitor.py), and the PNG container is written with `zlib` and `struct` only -
neither torchvision, matplotlib nor Pillow is needed where the training runs.

Importing this module does not load the HIP library."""
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import torch

from .sampling import _spectral_state

def grid_geometry(n, S, nrow=8, padding=2):
    """(xmaps, ymaps, GH, GW) of the picture of n images of S x S."""
    xmaps = min(int(nrow), int(n))
    ymaps = -(-int(n) // xmaps)
    return xmaps, ymaps, (S + padding) * ymaps + padding, (S + padding) * xmaps + padding


def image_grid(x, nrow=8, padding=2, value_range=None, pad_value=0.0, out=None, as_float=False):
    """torchvision's `make_grid(x, nrow, padding, normalize=True, value_range=..., pad_value=...)` on the device, on the current
    stream, with no host synchronisation.  x: fp32 [n, 3, S, S] on the GPU.  Returns uint8 [GH, GW, 4] - RGBA with alpha 255, the
    bytes matplotlib's `imsave` makes of that grid, `(grid * 255).astype(uint8)` - or, with `as_float`, the fp32 [3, GH, GW] grid
    itself.  `out`: a contiguous device tensor of that shape and dtype to write into.

    Without `value_range` the range is (x.min(), x.max()) over the WHOLE batch (`scale_each` is not offered), found by a reduction
    launch in front of the composing one.  With `value_range=(lo, hi)` the values are clamped into it and the divisor is
    max(hi - lo, 1e-5) taken from the two Python floats, as torchvision does.  `pad_value` is not normalised and should lie in
    [0, 1].  A batch that holds a non-finite value gives unspecified bytes.

    n == 1 goes through the same formula and keeps its border.  torchvision (from memory: it cannot be checked where this was
    written, and the reference never renders a single image) returns the bare image for a batch of one.

    CPU tensors are rejected with TypeError: there is no CPU path."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise TypeError("image_grid computes on the GPU only; got %s" % (x.device if torch.is_tensor(x) else type(x).__name__))
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[0] < 1:
        raise ValueError("image_grid takes fp32 [n, 3, S, S], got %s %s" % (x.dtype, tuple(x.shape)))
    if int(nrow) < 1 or int(padding) < 0:
        raise ValueError("image_grid: nrow >= 1 and padding >= 0")
    from ._lib import check, lib
    L = lib()
    x = x.detach().contiguous()
    n, S = int(x.shape[0]), int(x.shape[2])
    _, _, GH, GW = grid_geometry(n, S, nrow, padding)
    shape, dtype = ((3, GH, GW), torch.float32) if as_float else ((GH, GW, 4), torch.uint8)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous %s %s tensor on %s" % (dtype, shape, x.device))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    if value_range is None:
        rng = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = torch.empty(max(L.locate_image_range_workspace_bytes(), 16), dtype=torch.uint8, device=x.device)
        check(L.locate_image_range(ptr(x), x.numel(), ptr(rng), ptr(ws), stream), "locate_image_range")
        divisor = 0.0
    else:
        lo, hi = float(value_range[0]), float(value_range[1])
        if not hi > lo:
            raise ValueError("value_range must be (lo, hi) with lo < hi")
        rng = torch.tensor([lo, hi], dtype=torch.float32).to(x.device)
        divisor = float(np.float32(max(hi - lo, 1e-5)))
    check(L.locate_image_grid(ptr(x), n, S, int(nrow), int(padding), float(pad_value), ptr(rng), divisor,
                              ptr(out) if as_float else None, None if as_float else ptr(out), stream), "locate_image_grid")
    return out


# ---- PNG container (8-bit RGBA, non-interlaced, filter type 0 on every row) ----
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, rgba, level=1):
    """uint8 [H, W, 4] (numpy array or CPU tensor) as an 8-bit RGBA PNG, with zlib and struct only.  Written to path + ".tmp" and
    renamed, so a reader never sees half a file.  `level`: zlib's; 1 by default - the picture of 64 images of 256 x 256 is 18 MB
    of pixels, and the encoder runs on the host beside the training loop (profiles/notes_monitor.md)."""
    if torch.is_tensor(rgba):
        if rgba.is_cuda:
            raise TypeError("write_png takes host memory: copy the picture first (Sampler.save does, through a pinned buffer)")
        rgba = rgba.numpy()
    rgba = np.ascontiguousarray(rgba)
    if rgba.dtype != np.uint8 or rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.shape[0] < 1 or rgba.shape[1] < 1:
        raise ValueError("write_png takes uint8 [H, W, 4], got %s %s" % (rgba.dtype, rgba.shape))
    H, W = rgba.shape[:2]
    rows = np.zeros((H, 1 + 4 * W), dtype=np.uint8)          # one filter byte (0: none) in front of every row
    rows[:, 1:] = rgba.reshape(H, 4 * W)
    data = (_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))
    tmp = str(path) + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, str(path))
    return str(path)


def read_png(path):
    """The inverse of write_png for files of its kind: uint8 [H, W, 4].  Anything else - another colour type or bit depth,
    interlacing, a row filter other than 0 - raises ValueError."""
    with open(str(path), "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_MAGIC:
        raise ValueError("%s is not a PNG file" % path)
    at, header, idat = 8, None, []
    while at + 12 <= len(raw):
        (size,), tag = struct.unpack(">I", raw[at:at + 4]), raw[at + 4:at + 8]
        body = raw[at + 8:at + 8 + size]
        (crc,) = struct.unpack(">I", raw[at + 8 + size:at + 12 + size])
        if len(body) != size or crc != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError("%s: damaged %r chunk" % (path, tag))
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        at += 12 + size
    if header is None or header[2:] != (8, 6, 0, 0, 0):
        raise ValueError("%s: only 8-bit RGBA, non-interlaced files are read here" % path)
    W, H = header[:2]
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if rows.size != H * (1 + 4 * W):
        raise ValueError("%s: %d bytes of pixel data for %d x %d" % (path, rows.size, W, H))
    rows = rows.reshape(H, 1 + 4 * W)
    if rows[:, 0].any():
        raise ValueError("%s uses row filters; only filter type 0 is read here" % path)
    return rows[:, 1:].reshape(H, W, 4).copy()


class Sampler:
    """The reference's sample picture (main.py:55,194-225): a FIXED latent batch through the generator in eval mode, tiled with
    padding 8 and normalised over the whole batch.

    fixed_noise: [images, gen.g_in] on the generator's device; by default `torch.randn(images, gen.g_in)` drawn there (main.py:55),
    from a generator of its own seeded with `seed` when one is given, else from the device's global one.

    sample() is ONE forward of all the latents - never chunks: InPlaceNorm takes its mean and deviation over the whole batch, so
    chunks would change the picture.  It may be called between any two training iterations, eager or replayed
    (`GraphedTrainStep.replay`), on the stream the training runs on; not inside an iteration.

    advance_spectral_norm=True is the reference: every forward of the generator runs a power iteration, so a sampling pass moves
    the generator's u and v and with them the training trajectory.  False snapshots every u and v of the generator before the pass
    and copies them back in place after it: monitoring is then free of side effects - weights, u / v and optimizer states of a
    run that samples equal those of a run that does not, bit for bit (tests/test_gpu_monitor.py).  Under data parallelism only
    rank 0 should sample, with False - the ranks' u and v would drift apart otherwise."""

    def __init__(self, gen, fixed_noise=None, images=64, seed=None, nrow=8, padding=8, advance_spectral_norm=True):
        self.gen = gen
        dev = next(gen.parameters()).device
        if dev.type != "cuda":
            raise TypeError("Sampler renders on the GPU; the generator is on %s" % dev)
        if fixed_noise is None:
            rng = None
            if seed is not None:
                rng = torch.Generator(device=dev)
                rng.manual_seed(int(seed))
            fixed_noise = torch.randn(int(images), gen.g_in, device=dev, generator=rng)
        elif fixed_noise.dim() != 2 or fixed_noise.shape[1] != gen.g_in:
            raise ValueError("fixed_noise must be [images, %d]" % gen.g_in)
        self.fixed_noise = fixed_noise.detach().to(dev, torch.float32).contiguous()
        self.nrow, self.padding = int(nrow), int(padding)
        self.advance_spectral_norm = bool(advance_spectral_norm)
        self._uv = _spectral_state(gen)
        self._saved = None
        self._picture = None
        self._pinned = None

    @property
    def images(self):
        return self.fixed_noise.shape[0]

    def sample(self):
        """gen.eval(), one forward of the fixed latents under no_grad, the previous mode restored: fp32 [images, 3, S, S]."""
        gen = self.gen
        was_training = gen.training
        keep = not self.advance_spectral_norm
        with torch.no_grad():
            if keep:
                if self._saved is None:
                    self._saved = [torch.empty_like(p) for p in self._uv]
                torch._foreach_copy_(self._saved, [p.data for p in self._uv])
            gen.eval()
            try:
                fake = gen(self.fixed_noise)
            finally:
                gen.train(was_training)
                if keep:
                    torch._foreach_copy_([p.data for p in self._uv], self._saved)          # in place: same addresses
        return fake.detach()

    def render(self):
        """The picture of sample() as device RGBA bytes [GH, GW, 4] (a buffer of this sampler, overwritten by the next call)."""
        self._picture = image_grid(self.sample(), nrow=self.nrow, padding=self.padding, out=self._picture)
        return self._picture

    def _to_host(self, rgba):
        if self._pinned is None or self._pinned.shape != rgba.shape:
            self._pinned = torch.empty(rgba.shape, dtype=torch.uint8).pin_memory()
        self._pinned.copy_(rgba, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self._pinned.numpy()

    def save(self, path):
        """render(), one copy through a pinned buffer, write_png.  Waits for the device: the only host synchronisation here."""
        return write_png(path, self._to_host(self.render()))

    def preview(self, batch, path):
        """The reference's plot_images (libs/utils.py:73-78, main.py:45-48) for a real or augmented batch: padding 2."""
        return write_png(path, self._to_host(image_grid(batch, nrow=8, padding=2)))


class LossHistory:
    """The reference's two loss curves (main.py:182-193, 226-234) without a host read per record: record() copies
    `d_error / 2` and `g_error` into a preallocated device buffer, flush() reads everything recorded since the last flush back
    in one copy.  Under hipGraph replay the two tensors have fixed addresses, so record() is two small launches.

    moving_average() is main.py:226-232 AS CODED: weights j = 1 .. W on W consecutive values, divided by (W^2 - W) / 2 - which
    is not the sum of the weights ((W^2 + W) / 2), so the curve sits (W + 1) / (W - 1) too high; the quirk is kept.  A series
    of `len` values gives `len - W` averages (none for len <= W)."""

    def __init__(self, mean_window=16, capacity=4096):
        if int(mean_window) < 2:
            raise ValueError("mean_window must be >= 2 (the reference's divisor (W^2 - W) / 2 is 0 for W = 1)")
        self.mean_window = int(mean_window)
        self.capacity = int(capacity)
        self.d, self.g = [], []
        self._buf = None
        self._count = 0
        self._last_g = None

    def record(self, out):
        """out: what an iteration returned.  An iteration without a G-step (diters > 1) repeats the last g_error, as the
        reference's loop variable does; before the first G-step nothing is recorded (main.py:184-185).  Returns whether a
        record was taken."""
        d = out["d_error"]
        g = out.get("g_error", self._last_g)
        if g is None:
            return False
        self._last_g = g
        if not d.is_cuda:
            raise TypeError("LossHistory records device tensors; there is no CPU path")
        if self._buf is None or self._buf.device != d.device:
            self._buf = torch.empty(self.capacity, 2, dtype=torch.float32, device=d.device)
        if self._count == self.capacity:
            self.flush()
        row = self._buf[self._count]
        with torch.no_grad():
            torch.mul(d.detach().reshape(()), 0.5, out=row[0])          # d_error / 2: halving is exact
            row[1].copy_(g.detach().reshape(()))
        self._count += 1
        return True

    def flush(self):
        """One device-to-host copy of the records since the last flush; returns them as a list of (d, g) pairs."""
        if self._count == 0:
            return []
        host = self._buf[:self._count].cpu().tolist()
        self._count = 0
        self.d += [r[0] for r in host]
        self.g += [r[1] for r in host]
        return [(r[0], r[1]) for r in host]

    @staticmethod
    def _moving_average(series, window):
        div = (window ** 2 - window) / 2
        return [sum(series[i + j - 1] * j for j in range(1, window + 1)) / div for i in range(len(series) - window)]

    def moving_average(self):
        self.flush()
        return self._moving_average(self.d, self.mean_window), self._moving_average(self.g, self.mean_window)

    def state_dict(self):
        self.flush()
        return {"d": list(self.d), "g": list(self.g), "mean_window": self.mean_window}

    def load_state_dict(self, state):
        self.d, self.g = [float(v) for v in state["d"]], [float(v) for v in state["g"]]
        self.mean_window = int(state["mean_window"])
        self._count = 0

    def save(self, folder, epoch):
        """`folder/{epoch}.json` with the raw and the averaged series; `{epoch}-d.svg` / `{epoch}-g.svg` (the reference's
        plot_hist of the averaged series) only where matplotlib imports.  Returns the files written."""
        os.makedirs(folder, exist_ok=True)
        ma_d, ma_g = self.moving_average()
        path = os.path.join(folder, "%d.json" % epoch)
        with open(path + ".tmp", "w") as f:
            json.dump({"mean_window": self.mean_window, "d": self.d, "g": self.g, "d_moving_average": ma_d,
                       "g_moving_average": ma_g}, f)
        os.replace(path + ".tmp", path)
        written = [path]
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except Exception:          # not installed (or unusable) on the training machine: the JSON holds everything
            return written
        for tag, series in (("d", ma_d), ("g", ma_g)):
            svg = os.path.join(folder, "%d-%s.svg" % (epoch, tag))
            plt.clf()
            plt.plot(series)
            plt.savefig(svg)
            written.append(svg)
        return written
