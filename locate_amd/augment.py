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
        self._stage(rows, self.params)
        self.draws += 1
        self.last_rows = rows
        return rows

    def _stage(self, rows, dev):
        """rows -> the device tensor `dev` through the next pinned slot, on the current stream"""
        slot = self._slot
        self._slot = (slot + 1) % self.SLOTS
        if self._events[slot] is not None:
            self._events[slot].synchronize()          # only when the host is SLOTS draws ahead of the device
        self._pinned[slot].numpy()[...] = rows
        dev.copy_(self._pinned[slot], non_blocking=True)
        self._events[slot] = torch.cuda.Event()
        self._events[slot].record()

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
        if state.get("adaptive"):
            raise ValueError("the saved augmentation is an AdaptiveDiffAugment's (it carries p and the gate's stream); this run's is a "
                             "plain DiffAugment: resume with the same --ada-target settings")
        self._load_stream(state)

    def _load_stream(self, state):
        if (state["policy"], int(state["S"]), int(state["batch"])) != (self.policy, self.S, self.batch):
            raise ValueError("the saved augmentation is %r at S = %d, batch %d; this run's is %r at S = %d, batch %d"
                             % (state["policy"], int(state["S"]), int(state["batch"]), self.policy, self.S, self.batch))
        self.generator.set_state(state["generator_state"])


# ---- adaptive augmentation ----------------------------------------------------------------------------------------------------------
ADA_STATE_WORDS = 16
ADA_RING_WORDS = 4          # {iteration, r, p, logits counted in the closed window}
# words 0 .. 9 of the device record (csrc/ada.hip; the layout is defined in tests/helpers/ada_model.py, FIELDS)
ADA_FIELDS = ("p", "r", "sum", "counted", "seen", "closed", "ups", "downs", "nan", "rows")
GATE_WORD = 9
_GATE_CAP = np.nextafter(np.float32(1.0), np.float32(0.0))          # the largest fp32 below 1


def ada_step(batch, interval, kimg):
    """What p moves by per closed window, batch * interval / (kimg * 1000): float64, rounded once to fp32 (kimg = inf: 0)."""
    return np.float32(float(batch) * float(interval) / (float(kimg) * 1000.0))


class AdaptiveDiffAugment(DiffAugment):
    """DiffAugment whose strength steers itself (adaptive discriminator augmentation; Karras et al. 2020, "Training Generative
    Adversarial Networks with Limited Data"): every op of the policy is applied to every image independently with probability p, and
    p follows the overfitting indicator

        r_t = E[sign(D(real))]          over the last `interval` batches: near 0 for a healthy discriminator, near 1 for one that
                                        has learned the training set by heart;
        p  <-  min(max(p +- step, 0), p_max)   for r_t > / < target,    step = batch * interval / (kimg * 1000)

    (p would take kimg thousand images to go from 0 to 1).  All of it runs on the device BESIDE the step, with no host read:
    observe(d_true) is one single-block launch that adds the signs of the B logits to a window kept in a 64-byte device record and,
    every interval-th call, closes the window, moves p and appends {iteration, r_t, p} to a device ring; draw() uploads the raw rows
    - the DiffAugment rows of the same seed, words 0 .. 8 unchanged, plus three uniforms per row from a SECOND generator - to a
    staging tensor and launches a gate kernel that writes `params`: op k of an image is applied iff its uniform is < p (strictly),
    and is otherwise switched off in the row's mask word, which the diffaug kernels honour bit for bit.  So a new p takes effect at
    the next draw(), never inside an iteration, and a replayed hipGraph, which reads `params` at its fixed address, needs no change.
    TrainLoop.iteration and Trainer call draw() and observe() themselves.  Construction needs no GPU.

    Two corners:  kimg=float("inf"), initial_p=1.0 is fixed-strength DiffAugment with the r_t curve recorded - any augmented run
    gets the indicator;  initial_p=0.0 with r_t below target stays at p = 0, where T is a copy and the run equals the run without
    an augment, bit for bit.

    status() is one 64-byte copy; flush() one copy of the ring rows since the last flush; curve() the flushed rows.  state_dict()
    carries both generators, the device record (one small host read), the flushed curve and the settings: a resumed run continues
    p, the open window and both streams.  A rollback (snapshot.py) rewinds none of them, like the input pipeline's.  Under data
    parallelism each rank would steer its own p from its own shard: out of scope, and refused by TrainLoop and Trainer."""

    def __init__(self, S, batch, policy="color,translation,cutout", seed=999, device="cuda:0", target=0.6, interval=4, kimg=500.0,
                 initial_p=0.0, p_max=1.0, capacity=4096):
        super().__init__(S, batch, policy=policy, seed=seed, device=device)
        self.target, self.interval, self.kimg = float(target), int(interval), float(kimg)
        self.p_max, self.initial_p, self.capacity = float(p_max), float(initial_p) + 0.0, int(capacity)
        if not np.isfinite(self.target):
            raise ValueError("target must be a finite number, got %r" % (target,))
        if self.interval < 1 or self.batch * self.interval >= 1 << 31:
            raise ValueError("interval must be >= 1 with batch * interval < 2^31, got %r" % (interval,))
        if not self.kimg > 0:
            raise ValueError("kimg must be > 0 (float('inf'): p never moves), got %r" % (kimg,))
        if not 0.0 < self.p_max <= 1.0:
            raise ValueError("p_max must be in (0, 1], got %r" % (p_max,))
        if not 0.0 <= self.initial_p <= self.p_max:
            raise ValueError("initial_p must be in [0, p_max], got %r" % (initial_p,))
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        self.step = ada_step(self.batch, self.interval, self.kimg)
        self.gate_generator = torch.Generator().manual_seed(int(seed) + 0xADA)
        self.observations = 0          # observe() calls in all, across resumes: the default iteration label
        self._record = np.zeros(ADA_STATE_WORDS, np.uint32)          # what the device record starts from, until it exists
        self._record[0] = np.array([self.initial_p], np.float32).view(np.uint32)[0]
        self._state = self._ring = self._raw = None
        self._window_seen, self._ring_rows, self._flushed = 0, 0, 0          # the host's mirror of words 4 and 9, and the rows already flushed
        self._curve = np.zeros((0, ADA_RING_WORDS), np.uint32)

    # ---- device tensors, made on first use -----------------------------------------------------------------------------------------
    @property
    def state(self):
        """the 64-byte device record (int32 [16])"""
        if self._state is None:
            self._state = torch.from_numpy(self._record.view(np.int32).copy()).to(self.device)
            self._ring = torch.zeros(self.capacity, ADA_RING_WORDS, dtype=torch.int32, device=self.device)
            self._raw = torch.zeros(4 * self.batch, PARAM_FLOATS, dtype=torch.float32, device=self.device)
        return self._state

    def draw(self):
        """The next iteration's 4B rows: DiffAugment's draw of the same seed, and in words 9 .. 11 three gate uniforms per row from
        the second generator (one float64 rand(rows, 3), rounded to fp32 and capped at the largest fp32 below 1); gated on the
        device with the p of this moment.  Returns the raw host rows."""
        rows = draw_parameters(4 * self.batch, self.S, self.generator, self.bits)
        g = torch.rand(4 * self.batch, 3, generator=self.gate_generator, dtype=torch.float64).numpy()
        rows[:, GATE_WORD:GATE_WORD + 3] = np.minimum(g.astype(np.float32), _GATE_CAP)
        return self.upload(rows)

    def upload(self, rows):
        """Hand-made RAW rows (numpy float32 [4B, 12], uniforms in words 9 .. 11) in place of a draw."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.shape != (4 * self.batch, PARAM_FLOATS):
            raise ValueError("rows must be [%d, %d], got %s" % (4 * self.batch, PARAM_FLOATS, rows.shape))
        out, state = self.params, self.state
        self._stage(rows, self._raw)
        check(lib().locate_ada_gate(self._raw.data_ptr(), state.data_ptr(), out.data_ptr(), 4 * self.batch, self.bits, _stream()),
              "locate_ada_gate")
        self.draws += 1
        self.last_rows = rows
        return rows

    def observe(self, d_true, iteration=None):
        """One launch on the current stream: D's logits on this iteration's real batch (the step's out["d_true"]) into the window.
        `iteration` labels the ring row if this observation closes a window (default: the count of observations so far)."""
        if not (torch.is_tensor(d_true) and d_true.is_cuda and d_true.dtype == torch.float32 and d_true.is_contiguous() and d_true.numel() > 0):
            raise TypeError("observe takes a contiguous, non-empty fp32 tensor of logits on the GPU")
        state = self.state
        self.observations += 1
        label = self.observations if iteration is None else int(iteration)
        check(lib().locate_ada_observe(d_true.data_ptr(), d_true.numel(), label, state.data_ptr(), self._ring.data_ptr(), self.capacity,
                                       self.interval, self.target, float(self.step), self.p_max, _stream()), "locate_ada_observe")
        self._window_seen += 1
        if self._window_seen >= self.interval:          # what the kernel does to words 4 and 9
            self._window_seen = 0
            self._ring_rows += 1

    # ---- reading ---------------------------------------------------------------------------------------------------------------------
    def _read_record(self):
        if self._state is None:
            return self._record.copy()
        return self._state.cpu().numpy().view(np.uint32).copy()

    def status(self):
        """{"p", "r_t", "updates", "ups", "downs", "nonfinite"}: one 64-byte copy from the device"""
        w = self._read_record()
        return {"p": float(w[0:1].view(np.float32)[0]), "r_t": float(w[1:2].view(np.float32)[0]), "updates": int(w[5]), "ups": int(w[6]),
                "downs": int(w[7]), "nonfinite": int(w[8])}

    def flush(self):
        """The ring rows appended since the last flush (one copy from the device) join curve(); returns them as curve() would.  Rows
        that the ring has overwritten since - more than `capacity` windows between two flushes - are lost."""
        first, last = max(self._flushed, self._ring_rows - self.capacity), self._ring_rows
        self._flushed = last
        if last == first:
            return []
        a, b = first % self.capacity, (last - 1) % self.capacity + 1
        if a < b:
            rows = self._ring[a:b].cpu().numpy()
        else:          # the span wraps: the whole ring in one copy
            ring = self._ring.cpu().numpy()
            rows = np.concatenate([ring[a:], ring[:b]])
        rows = rows.view(np.uint32)
        self._curve = np.concatenate([self._curve, rows])
        return _curve_records(rows)

    def curve(self):
        """every flushed row: [{"iteration", "r_t", "p"}]"""
        return _curve_records(self._curve)

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def _settings(self):
        return {"target": self.target, "interval": self.interval, "kimg": self.kimg, "p_max": self.p_max, "capacity": self.capacity}

    def state_dict(self):
        self.flush()
        state = super().state_dict()
        state.update({"adaptive": True, "gate_generator_state": self.gate_generator.get_state(),
                      "record": torch.from_numpy(self._read_record().view(np.int32).copy()), "observations": int(self.observations),
                      "curve": torch.from_numpy(self._curve.view(np.int32).copy()), "settings": self._settings()})
        return state

    def load_state_dict(self, state):
        if not state.get("adaptive"):
            raise ValueError("the saved augmentation is a plain DiffAugment's (no p, no gate stream); this run's is an "
                             "AdaptiveDiffAugment: resume without --ada-target")
        saved = {k: state["settings"][k] for k in ("target", "interval", "kimg", "p_max")}
        mine = {k: v for k, v in self._settings().items() if k in saved}
        if saved != mine:
            raise ValueError("the saved adaptive augmentation ran with %r, this run's has %r" % (saved, mine))
        self._load_stream(state)
        self.gate_generator.set_state(state["gate_generator_state"])
        self._record = state["record"].numpy().view(np.uint32).copy()
        self.observations = int(state["observations"])
        self._curve = state["curve"].numpy().view(np.uint32).reshape(-1, ADA_RING_WORDS).copy()
        self._window_seen, self._ring_rows = int(self._record[4]), int(self._record[9])
        self._flushed = self._ring_rows          # the ring itself is not carried: its flushed rows are in the curve
        if self._state is not None:
            self._state.copy_(torch.from_numpy(self._record.view(np.int32).copy()))


def _curve_records(rows):
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, ADA_RING_WORDS)
    it, r, p = rows[:, 0].copy().view(np.int32), rows[:, 1].copy().view(np.float32), rows[:, 2].copy().view(np.float32)
    return [{"iteration": int(it[k]), "r_t": float(r[k]), "p": float(p[k])} for k in range(len(rows))]
