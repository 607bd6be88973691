"""An averaged generator: the exponential moving average (EMA) of the generator's weights that GAN practice samples and measures
instead of the live network - the live generator's pictures jump from iteration to iteration, and Karras et al. ("Progressive
Growing of GANs", the paper `locate_amd.metric` follows) report their sliced Wasserstein distances on the average.  The reference
has no such average; like the monitor and the metric this is an addition BESIDE the training step: a separate object with a kernel
of its own (csrc/average.hip through the C ABI, include/locate_hip.h) that is launched between two iterations, where
`LossHistory.record` is.  Nothing the training step runs is involved, so the trajectory of a run that averages is that of a run that
does not, bit for bit (tests/test_gpu_average.py).

    avg = AveragedGenerator(gen, half_life_images=10000, batch=64)          # or beta=0.999
    avg.update()                                                            # after every iteration: one launch, no host read
    Sampler(avg.generator, ...).save(path);  swd.evaluate(avg.generator)

Per averaged element, three fp32 operations, each rounded once and never contracted:  avg = avg + (1 - beta) * (live - avg).

Importing this module does not load the HIP library.  A generator on the CPU raises TypeError: there is no CPU path."""
import ctypes
import struct

import numpy as np
import torch

from ._tables import chunk_pairs, remember, stage


def average_weight(beta=None, half_life_images=None, batch=None):
    """(beta, one_minus_beta) as Python floats.  Exactly one of `beta` (in [0, 1)) or the pair (`half_life_images` > 0, `batch` > 0)
    is given; the pair means beta = 0.5 ** (batch / half_life_images), computed in float64: after half_life_images images the
    weight of an old value has halved, whatever the batch size.  `one_minus_beta` is 1 - beta rounded ONCE to fp32 - the number the
    kernel multiplies by.  Anything else raises ValueError."""
    pair = half_life_images is not None or batch is not None
    if (beta is None) == (not pair) or (pair and (half_life_images is None or batch is None)):
        raise ValueError("give either beta or both half_life_images and batch")
    if beta is None:
        half_life_images, batch = float(half_life_images), float(batch)
        if not (0.0 < half_life_images < float("inf") and 0.0 < batch < float("inf")):
            raise ValueError("half_life_images and batch must be positive and finite, got %r and %r" % (half_life_images, batch))
        beta = 0.5 ** (batch / half_life_images)
    beta = float(beta)
    if not 0.0 <= beta < 1.0:
        raise ValueError("beta must lie in [0, 1), got %r" % beta)
    one_minus_beta = float(np.float32(1.0 - beta))
    if one_minus_beta == 0.0:
        raise ValueError("1 - beta rounds to 0 in fp32: the average would never move")
    return beta, one_minus_beta


class AveragedGenerator:
    """The EMA of `gen`'s weights, as a `Generator` of its own.

    `generator` is `Generator(gen.cfg)` on gen's device, loaded from `gen.state_dict()` with `noise` copied (the noise map is
    constant during training: it is copied at construction, by reset() and by load_state_dict(), not by update()), the same
    `runtime.precision`, `batched_spectral_norm` and training mode as gen, `requires_grad_(False)`.  It owns its `ops.Runtime`, its
    spectral-norm ring and its weight panels: nothing mutable is shared with gen, and a forward of it - `Sampler`,
    `SlicedWasserstein.evaluate`, anything that takes a generator - leaves gen untouched.  Constructing it leaves torch's global
    random generators where they were.

    Which tensors update() moves:
      * every parameter is averaged with beta;
      * except each `SpectralNorm` layer's `weight_u` / `weight_v`, which are COPIED from the live network on every update (bit for
        bit).  The average's weights trail the live ones closely, so the live u / v are a near-converged start for the one power
        iteration the average's own forward runs; u / v that only moved when the average happened to be sampled would normalise
        its weights by a stale sigma;
      * any other `state_dict` entry (a buffer) is copied too.

    update() is ONE launch for the whole network on `torch.cuda.current_stream()`, with no allocation and no host read.  It bumps
    the version counters of the tensors it wrote, so the weight panels of `generator` are re-packed lazily by its next forward - the
    average is forwarded once per few hundred updates, so the re-pack pays for its own largest-magnitude pass then, instead of the
    update publishing those words every time (no `_locate_wmax` stamp is ever put on an averaged parameter).

    `updates` counts the calls.  state_dict() is the averaged generator's `state_dict()` (CPU copies) plus "noise", "updates" and
    "one_minus_beta" - tensors and numbers only, loadable with `weights_only=True`.

    Memory: one more copy of the generator's parameters, plus its weight panels and activation workspaces once it has been forwarded.

    Under data parallelism the weights are equal on every rank: only rank 0 needs an average, as with `Sampler`."""

    def __init__(self, gen, beta=None, half_life_images=None, batch=None):
        from .models import Generator
        from .sampling import _spectral_state
        self.beta, self.one_minus_beta = average_weight(beta, half_life_images, batch)
        dev = next(gen.parameters()).device
        if dev.type != "cuda":
            raise TypeError("AveragedGenerator computes on the GPU only; the generator is on %s" % dev)
        self.source = gen
        with torch.random.fork_rng(devices=[]):          # the constructor's draws are overwritten below: leave no trace of them
            own = Generator(gen.cfg)
        own = own.to(dev)
        own.runtime.precision = gen.runtime.precision
        own.batched_spectral_norm = gen.batched_spectral_norm
        own.requires_grad_(False)
        own.train(gen.training)
        self.generator = own
        self.updates = 0
        live, mine = gen.state_dict(keep_vars=True), own.state_dict(keep_vars=True)
        if list(live) != list(mine) or any(live[k].shape != mine[k].shape for k in live):
            raise ValueError("the generator's state_dict does not have the layout Generator(gen.cfg) has")
        copied = {id(p) for p in _spectral_state(own)}
        averaged = {id(p) for p in own.parameters()} - copied
        # (averaged tensor, live tensor, weight) per state_dict entry
        self._pairs = [(mine[k], live[k], self.one_minus_beta if id(mine[k]) in averaged else 1.0) for k in mine]
        for a, s, _ in self._pairs:
            if not (a.dtype == s.dtype == torch.float32 and a.is_contiguous() and s.is_contiguous() and s.device == dev):
                raise TypeError("AveragedGenerator: every state_dict entry must be a contiguous float32 tensor on %s" % dev)
        self._written = [a for a, _, _ in self._pairs]
        self._tables = {}
        self.reset()

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self):
        """The average becomes the live generator as it is now (weights, u / v, buffers, noise), in place; `updates` = 0."""
        torch._foreach_copy_([a for a, _, _ in self._pairs], [s.detach() for _, s, _ in self._pairs])
        self._copy_noise(self.source.noise)
        self.updates = 0
        return self

    def _copy_noise(self, noise):
        own = self.generator
        if tuple(noise.shape) != tuple(own.noise.shape):
            raise ValueError("noise map %s does not fit the generator's %s" % (tuple(noise.shape), tuple(own.noise.shape)))
        with torch.no_grad():
            own.noise.copy_(noise)          # in place: bumps its version, the forward's expanded copies follow

    def state_dict(self):
        state = {k: v.detach().to("cpu").clone() for k, v in self.generator.state_dict().items()}
        state["noise"] = self.generator.noise.detach().to("cpu").clone()
        state["updates"] = int(self.updates)
        state["one_minus_beta"] = float(self.one_minus_beta)
        return state

    def generator_state_dict(self):
        """The averaged weights alone, in the reference's `state_dict()` layout (CPU copies): what loads into a `Generator`."""
        return {k: v.detach().to("cpu").clone() for k, v in self.generator.state_dict().items()}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Copies IN PLACE (the addresses, and with them the device table, stay).  ValueError on another beta, on missing or
        unknown entries and on other shapes - checked before anything is written."""
        if float(state["one_minus_beta"]) != self.one_minus_beta:
            raise ValueError("the saved average has 1 - beta = %r, this one %r" % (float(state["one_minus_beta"]), self.one_minus_beta))
        mine = self.generator.state_dict(keep_vars=True)
        if sorted(mine) != sorted(k for k in state if k not in ("noise", "updates", "one_minus_beta")):
            raise ValueError("the saved average does not have this generator's state_dict entries")
        for k, t in mine.items():
            if tuple(state[k].shape) != tuple(t.shape):
                raise ValueError("%s: saved shape %s, this generator's %s" % (k, tuple(state[k].shape), tuple(t.shape)))
        if tuple(state["noise"].shape) != tuple(self.generator.noise.shape):
            raise ValueError("saved noise map %s, this generator's %s" % (tuple(state["noise"].shape), tuple(self.generator.noise.shape)))
        for k, t in mine.items():
            t.copy_(state[k])
        self._copy_noise(state["noise"])
        self.updates = int(state["updates"])
        return self

    # ---- the update ---------------------------------------------------------------------------------------------------------------
    def _table(self):
        """Device tables of locate_average_update, cached on ALL the addresses they hold (rebuilt when one changes)."""
        key = tuple((a.data_ptr(), s.data_ptr()) for a, s, _ in self._pairs)
        tab = self._tables.get(key)
        if tab is not None:
            return tab
        from ._lib import lib
        L = lib()
        assert L.locate_average_record_bytes() == 32
        live = [(a, s, w) for a, s, w in self._pairs if a.numel() > 0]
        rec = b"".join(struct.pack("<QQqf4x", a.data_ptr(), s.data_ptr(), a.numel(), w) for a, s, w in live)
        pairs, _ = chunk_pairs([a.numel() for a, _, _ in live], L.locate_average_chunk_elems())
        return remember(self._tables, key, stage(rec, pairs, len(live), self._pairs[0][0].device), 0)          # one table at a time

    def update(self):
        """One step of the average towards the live weights; u / v and buffers copied.  One launch on
        `torch.cuda.current_stream()`: call it on the stream the iteration - or the replay - was issued on, so that it is ordered
        behind the last write of the live weights (and in front of the next iteration's first).  No host read."""
        from ._lib import check, lib
        t_dev, c_dev, n_t, n_c = self._table()[:4]
        check(lib().locate_average_update(ctypes.c_void_p(t_dev.data_ptr()), ctypes.c_void_p(c_dev.data_ptr()), n_t, n_c,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_average_update")
        # the kernel writes through raw pointers: tell the packed-panel cache that the weights changed.  A `_locate_wmax` stamp
        # names the version its words were computed for, so none can claim the new one.
        torch._C._increment_version(self._written)
        self.updates += 1
        return self
