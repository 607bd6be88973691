"""Differentiable augmentation (Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN Training"): every image the
discriminator sees, real or generated, passes through one random transform T - colour, translation, cutout - and in the G-step the
gradient flows back through T into the generator.  The remedy for a run on a small image store that memorises (README, "Training
on few images").  The reference has only the consistency penalty between D(real) and D(aug), which never shows D an augmented fake.

T is affine per image and has no parameters of its own.  Its random numbers are drawn on the HOST, as the input pipeline's are
(data.py): a CPU `torch.Generator`, float64 `torch.rand`, one [rows, 7] draw whatever the policy - the stream does not depend on the
policy - turned into rows of 12 fp32 words (csrc/diffaug.hip; the definition in float64 numpy: tests/helpers/diffaug_model.py).

    y = diff_augment(x, params, policy="color,translation,cutout")     # autograd Function over locate_diffaug_fwd / _bwd
    params = draw_parameters(rows, S, generator, policy)                # float32 [rows, 12] on the host
    aug = DiffAugment(S=64, batch=64, policy="color,translation,cutout", seed=999, device="cuda:0")
    step = TrainStep(..., augment=aug);  aug.draw() before every iteration (TrainLoop.iteration and Trainer do)

The policy is static: it selects kernel variants.  An op that is off executes none of its arithmetic; its words of the row hold the
identity (0, 1, 1; zero shift; empty rectangle), but nothing relies on that."""
import numpy as np
import torch

from ._lib import check, lib

PARAM_FLOATS = 12
OPS = ("color", "translation", "cutout")          # bit 0, 1, 2 of the kernels' policy word
SIZES = (32, 64, 128, 256)


def parse_policy(policy):
    """"color,translation,cutout" (any subset, any order; or an int 0 .. 7, or an iterable of names) -> the policy bits."""
    if isinstance(policy, (int, np.integer)) and not isinstance(policy, bool):
        if not 0 <= int(policy) < 8:
            raise ValueError("policy bits %r are not in 0 .. 7" % (policy,))
        return int(policy)
    names = [n.strip() for n in policy.split(",")] if isinstance(policy, str) else list(policy)
    bits = 0
    for name in names:
        if name == "":
            continue
        if name not in OPS:
            raise ValueError("unknown augmentation %r: a policy is a subset of %s" % (name, ", ".join(OPS)))
        bits |= 1 << OPS.index(name)
    return bits


def policy_name(bits):
    return ",".join(n for k, n in enumerate(OPS) if bits >> k & 1)


def _check_size(S):
    if int(S) not in SIZES:
        raise ValueError("image size %r is not one of %s" % (S, SIZES))
    return int(S)


def draw_parameters(rows, S, generator, policy):
    """`rows` parameter rows (numpy float32 [rows, 12]) for images of S x S from ONE float64 rand(rows, 7) of `generator` (a CPU
    torch.Generator) - the paper's distributions:
      b = r0 - 0.5, s = 2 r1, c = r2 + 0.5;
      D = floor(S / 8 + 0.5): ty = floor(r3 (2 D + 1)) - D, tx likewise from r4;
      cut = floor(S / 2 + 0.5), oy = floor(r5 (S + 1 - cut % 2)): y0 = clamp(oy - cut // 2, 0, S), y1 = clamp(oy - cut // 2 + cut, 0, S),
      the columns likewise from r6.
    The words of an op that is not in the policy hold its identity."""
    S, bits = _check_size(S), parse_policy(policy)
    r = torch.rand(int(rows), 7, generator=generator, dtype=torch.float64).numpy()
    out = np.zeros((int(rows), PARAM_FLOATS), np.float64)
    out[:, 1] = out[:, 2] = 1.0
    if bits & 1:
        out[:, 0] = r[:, 0] - 0.5
        out[:, 1] = 2.0 * r[:, 1]
        out[:, 2] = r[:, 2] + 0.5
    if bits & 2:
        D = int(np.floor(S / 8 + 0.5))
        out[:, 3] = np.floor(r[:, 3] * (2 * D + 1)) - D
        out[:, 4] = np.floor(r[:, 4] * (2 * D + 1)) - D
    if bits & 4:
        cut = int(np.floor(S / 2 + 0.5))
        for col, k in ((5, 5), (7, 6)):
            o = np.floor(r[:, k] * (S + 1 - cut % 2))
            out[:, col] = np.clip(o - cut // 2, 0, S)
            out[:, col + 1] = np.clip(o - cut // 2 + cut, 0, S)
    return out.astype(np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(entry, name, src, params, S, bits):
    n = src.shape[0]
    dst = torch.empty_like(src)
    nbytes = int(lib().locate_diffaug_workspace_bytes(n, S))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=src.device) if nbytes and bits & 1 else None
    check(entry(src.data_ptr(), params.data_ptr(), dst.data_ptr(), n, S, bits, ws.data_ptr() if ws is not None else None, _stream()),
          name)
    return dst


class _DiffAugmentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, S, bits):
        ctx.save_for_backward(params)
        ctx.S, ctx.bits = S, bits
        return _run(lib().locate_diffaug_fwd, "locate_diffaug_fwd", x, params, S, bits)

    @staticmethod
    def backward(ctx, gy):
        params, = ctx.saved_tensors
        gx = _run(lib().locate_diffaug_bwd, "locate_diffaug_bwd", gy.contiguous(), params, ctx.S, ctx.bits)
        return gx, None, None, None


def _check_pair(x, params):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
            and x.shape[2] == x.shape[3] and x.is_contiguous()):
        raise TypeError("diff_augment takes a contiguous fp32 [n, 3, S, S] tensor on the GPU (there is no CPU path)")
    S, n = _check_size(x.shape[2]), x.shape[0]
    if not (torch.is_tensor(params) and params.device == x.device and params.dtype == torch.float32 and params.is_contiguous()
            and tuple(params.shape) == (n, PARAM_FLOATS)):
        raise TypeError("params must be a contiguous fp32 [%d, %d] tensor on %s" % (n, PARAM_FLOATS, x.device))
    if params.requires_grad:
        raise ValueError("the parameter rows are data, not weights: they take no gradient")
    if not 1 <= n <= 65535:
        raise ValueError("diff_augment takes 1 .. 65535 images a call, got %d" % n)
    return S


def diff_augment(x, params, policy="color,translation,cutout"):
    """T(x) for x fp32 [n, 3, S, S] and params fp32 [n, 12], both on the device; differentiable in x.  No host read, no
    synchronisation: legal under stream capture.  The backward kernel runs only when x needs a gradient."""
    S = _check_pair(x, params)
    assert lib().locate_diffaug_param_floats() == PARAM_FLOATS
    return _DiffAugmentFn.apply(x, params, S, parse_policy(policy))


def diff_augment_backward(gy, params, policy="color,translation,cutout"):
    """T's adjoint applied to gy (what diff_augment's autograd node runs), for callers that hold the gradient themselves."""
    S = _check_pair(gy, params)
    return _run(lib().locate_diffaug_bwd, "locate_diffaug_bwd", gy, params, S, parse_policy(policy))


class DiffAugment:
    """The training step's augmentation: the parameter rows of one iteration at a FIXED device address.

    `params` is one fp32 [4 * batch, 12] tensor: rows 0 .. 3B serve the D-step's real / generated / augmented thirds, each image
    with its own draw, rows 3B .. 4B the G-step (all of its passes: with minibatches > 1 they use the same rows, as they use the
    same noise).  draw() draws the iteration's 4B rows on the host and uploads them through one of two pinned staging buffers, each
    guarded by an event, so the host never rewrites a buffer whose copy is still queued.  Because the address is fixed a replayed
    hipGraph reads whatever draw() uploaded last.  Construction needs no GPU.

    Under data parallelism T has no parameters and nothing is exchanged; give each rank `seed + rank`.  state_dict() carries the
    generator's state, so a resumed run continues the uninterrupted parameter stream; a rollback (snapshot.py) does not rewind
    it, like the input pipeline's."""
    SLOTS = 2

    def __init__(self, S, batch, policy="color,translation,cutout", seed=999, device="cuda:0"):
        self.S, self.batch = _check_size(S), int(batch)
        if self.batch < 1 or 3 * self.batch > 65535:
            raise ValueError("batch must be in 1 .. 21845, got %r" % (batch,))
        self.bits = parse_policy(policy)
        if self.bits == 0:
            raise ValueError("an empty policy augments nothing: pass augment=None to the step instead")
        self.policy = policy_name(self.bits)
        self.device = torch.device(device)
        self.generator = torch.Generator().manual_seed(int(seed) + 0xD1FF)
        self._params = None
        self._pinned = self._events = None
        self._slot = 0
        self.draws = 0
        self.last_rows = None          # the host copy of the last draw (numpy float32 [4B, 12])

    @property
    def params(self):
        if self._params is None:
            self._params = torch.zeros(4 * self.batch, PARAM_FLOATS, dtype=torch.float32, device=self.device)
            self._pinned = [torch.empty(4 * self.batch, PARAM_FLOATS, dtype=torch.float32).pin_memory() for _ in range(self.SLOTS)]
            self._events = [None] * self.SLOTS
        return self._params

    def draw(self):
        """The next iteration's 4B rows: drawn on the host, uploaded on the current stream (behind everything that still reads the
        previous rows).  Returns the host rows."""
        rows = draw_parameters(4 * self.batch, self.S, self.generator, self.bits)
        return self.upload(rows)

    def upload(self, rows):
        """Hand-made rows (numpy float32 [4B, 12]) in place of a draw."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.shape != (4 * self.batch, PARAM_FLOATS):
            raise ValueError("rows must be [%d, %d], got %s" % (4 * self.batch, PARAM_FLOATS, rows.shape))
        dev = self.params
        slot = self._slot
        self._slot = (slot + 1) % self.SLOTS
        if self._events[slot] is not None:
            self._events[slot].synchronize()          # only when the host is SLOTS draws ahead of the device
        self._pinned[slot].numpy()[...] = rows
        dev.copy_(self._pinned[slot], non_blocking=True)
        self._events[slot] = torch.cuda.Event()
        self._events[slot].record()
        self.draws += 1
        self.last_rows = rows
        return rows

    def _rows(self, first, n):
        if self.draws == 0:
            raise RuntimeError("DiffAugment.draw() has not been called: the step would read rows that were never drawn")
        return self.params[first:first + n]

    def _apply(self, x, first):
        if tuple(x.shape[1:]) != (3, self.S, self.S):
            raise ValueError("this DiffAugment was made for [n, 3, %d, %d] images, got %s" % (self.S, self.S, tuple(x.shape)))
        return diff_augment(x.contiguous(), self._rows(first, x.shape[0]), self.bits)

    def d_batch(self, x):
        """T of the D-step's stacked [3B] batch (real | generated | augmented), one launch"""
        if x.shape[0] != 3 * self.batch:
            raise ValueError("the stacked D-step batch has %d images, expected %d" % (x.shape[0], 3 * self.batch))
        return self._apply(x, 0)

    def d_third(self, x, k):
        """T of third k (0 real, 1 generated, 2 augmented) of the D-step with its slice of the rows"""
        if x.shape[0] != self.batch or k not in (0, 1, 2):
            raise ValueError("third %r of the D-step has %d images, expected %d" % (k, x.shape[0], self.batch))
        return self._apply(x, k * self.batch)

    def g_batch(self, x):
        """T of the G-step's generated batch; the gradient flows back through it"""
        if x.shape[0] != self.batch:
            raise ValueError("the G-step batch has %d images, expected %d" % (x.shape[0], self.batch))
        return self._apply(x, 3 * self.batch)

    def state_dict(self):
        return {"generator_state": self.generator.get_state(), "policy": self.policy, "S": self.S, "batch": self.batch,
                "draws": int(self.draws)}

    def load_state_dict(self, state):
        if (state["policy"], int(state["S"]), int(state["batch"])) != (self.policy, self.S, self.batch):
            raise ValueError("the saved augmentation is %r at S = %d, batch %d; this run's is %r at S = %d, batch %d"
                             % (state["policy"], int(state["S"]), int(state["batch"]), self.policy, self.S, self.batch))
        self.generator.set_state(state["generator_state"])
