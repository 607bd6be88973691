"""What the sample metrics share on the Python side: sampling a generator without side effects, the fixed latents, the real images
of a plain pipeline of the metric's own, and the three ctypes helpers.

The one guarantee every metric advertises - weights, u / v and optimizer states of a run that measures equal those of a run that
does not, bit for bit - is `sampling`, and nothing else.

Importing this module does not load the HIP library.  CPU tensors raise TypeError: there is no CPU path."""
import contextlib
import ctypes

import torch


def _gpu(t, name, dtype=torch.float32):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise TypeError("%s must be a GPU tensor (there is no CPU path); got %s" % (name, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t.detach().contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _spectral_state(net):
    """every spectral-norm u and v of the network"""
    from .nn import SpectralNorm
    return [p for m in net.modules() if isinstance(m, SpectralNorm) for p in (m.module.weight_u, m.module.weight_v)]


@contextlib.contextmanager
def sampling(owner, *gens, device_type="cuda"):
    """Forwards of `gens` inside the body leave no trace on the training, eager or replayed.  On entry: a generator that is not on
    the GPU is refused (TypeError naming `owner`, the metric's class), no_grad is entered, every spectral-norm u / v of all the
    generators is cloned and all of them are put in eval mode.  On exit, whether the body returned or raised: each generator's own
    previous mode is restored and the u / v are copied back in place.  Use it between two iterations, never inside one."""
    for gen in gens:
        dev = next(gen.parameters()).device
        if dev.type != device_type:
            raise TypeError("%s computes on the GPU only; the generator is on %s" % (owner, dev))
    uv = [p for gen in gens for p in _spectral_state(gen)]
    was_training = [gen.training for gen in gens]
    with torch.no_grad():
        saved = [p.detach().clone() for p in uv]
        for gen in gens:
            gen.eval()
        try:
            yield
        finally:
            for gen, mode in zip(gens, was_training):
                gen.train(mode)
            if uv:
                torch._foreach_copy_([p.data for p in uv], saved)          # in place: same addresses


def batches(gens, latents, chunk):
    """gens(latents[at:at + chunk]) for every chunk, the last one short; for a list of generators the list of their outputs for the
    same slice.  For use inside `sampling`: this iterator restores nothing."""
    for at in range(0, latents.shape[0], chunk):
        part = latents[at:at + chunk]
        yield [gen(part) for gen in gens] if isinstance(gens, (list, tuple)) else gens(part)


def plain_batches(pipeline, S, batch, seed, total):
    """The first `total` images of the plain chain - the first output of `InputPipeline.next_batch()`, the last batch trimmed -
    from a pipeline of the metric's own over the same store, min(pipeline.batch, batch) images a batch, seeded seed + 2: the training
    pipeline's shuffle is not advanced."""
    from .data import InputPipeline
    own = InputPipeline(pipeline.store, S, min(pipeline.batch, batch), seed=seed + 2)
    left = total
    while left > 0:
        real, _ = own.next_batch()
        yield real[:left]
        left -= real.shape[0]


class FixedLatents:
    """Mixed into a metric: `device`, `_need_gpu()`, `_sampling(*gens)` and `latents(g_in)`.  The two class-level facts are
    `latent_seed`, the offset added to the metric's `seed`, and `_latent_count()`, the number of latents (`images` unless overridden)."""
    latent_seed = None

    def __init__(self, device):
        self.device = torch.device(device)
        self._latents = None

    def _latent_count(self):
        return self.images

    def _need_gpu(self):
        if self.device.type != "cuda":
            raise TypeError("%s computes on the GPU only; its device is %s" % (type(self).__name__, self.device))

    def _sampling(self, *gens):
        return sampling(type(self).__name__, *gens)

    def latents(self, g_in):
        """The fixed latents [count, g_in], drawn on the device on first use from a generator seeded seed + latent_seed; drawn again
        when g_in changes."""
        if self._latents is None or self._latents.shape[1] != int(g_in):
            self._need_gpu()
            rng = torch.Generator(device=self.device)
            rng.manual_seed(self.seed + self.latent_seed)
            self._latents = torch.randn(self._latent_count(), int(g_in), device=self.device, generator=rng)
        return self._latents

    def _generate(self, gen, latents=None):
        """fp32 [Q, 3, S, S]: the generator's images of `latents` (default: the fixed ones), `chunk` latents per forward, in `sampling`"""
        with self._sampling(gen):
            if latents is None:
                latents = self.latents(gen.g_in)
            elif not torch.is_tensor(latents) or latents.dim() != 2 or latents.shape[1] != gen.g_in or latents.shape[0] < 1:
                raise ValueError("latents must be [Q, %d]" % gen.g_in)
            return torch.cat([x.detach() for x in batches(gen, latents, self.chunk)])
