"""LeCam regularisation of the discriminator (Tseng et al. 2021, "Regularizing Generative Adversarial Networks under Limited Data"):
the remedy for a discriminator that, on a small image store, pushes D(real) and D(G(z)) ever further apart (README, "Training on
few images").  DiffAugment and its adaptive controller act on what D sees; this acts on what D says.

    alpha_R, alpha_F     the anchors: exponential moving averages of the batch means of t = D(real) and f = D(G(z))
    R = mean (t - alpha_F)^2 + mean (alpha_R - f)^2          one_sided (the default): both differences through clamp(min=0) first
    total = (d_error + penalty) + weight * R

An iteration's loss uses the anchors as the EARLIER iterations left them.  All of it runs on the device with no host read:
d_loss() is the D-step's one loss launch (csrc/lecam.hip, locate_d_loss_lecam) - values and gradients with respect to D's outputs,
no second backward pass, no extra D forward; observe() is one single-block launch BESIDE the step that moves the anchors kept in a
64-byte device record and appends {iteration, alpha_R, alpha_F, mean t, mean f, accepted} to a device ring: the per-iteration curve
of E[D(real)] and E[D(G(z))].  The definition in numpy, which both kernels equal with ==: tests/helpers/lecam_model.py.

    lecam = LeCam(batch=64, weight=0.3, decay=0.99, warmup=1000)
    step = TrainStep(..., lecam=lecam);  TrainLoop.iteration and Trainer call observe() after every iteration

The regulariser is ACTIVE iff weight != 0 and at least max(warmup, 1) observations were accepted - decided on the device from the
record, so a replayed hipGraph, which reads the record at its fixed address, switches it on by itself.  While it is inactive the loss
launch computes locate_d_loss's arithmetic and nothing else: weight=0, or a warmup beyond the run, is the run without a LeCam, bit
for bit, with the anchors' curve recorded."""
import numpy as np
import torch

from ._lib import check, lib

STATE_WORDS = 16
RING_WORDS = 8          # {iteration, alpha_R, alpha_F, m_R, m_F, accepted (1 / 0), 0, 0}
# words 0 .. 7 of the device record (csrc/lecam.hip; the layout is defined in tests/helpers/lecam_model.py, FIELDS)
FIELDS = ("alpha_r", "alpha_f", "accepted", "observations", "nonfinite", "rows", "mean_r", "mean_f")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def lecam_rate(decay):
    """What an anchor moves by towards a batch mean, 1 - decay: float64, rounded once to fp32."""
    return np.float32(1.0 - float(decay))


def _logits(x, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0):
        raise TypeError("%s must be a non-empty fp32 tensor of logits on the GPU (there is no CPU path)" % what)
    return x.detach().contiguous()


class LeCam:
    """The LeCam regulariser of one training step: settings, the anchors' device record and the ring of the anchors' curve.

    weight: the regulariser's factor in the D loss; 0 records the anchors and adds nothing.  decay: the anchors' moving-average
    decay.  warmup: accepted observations before the regulariser switches on (at least one: an anchor has to exist).  one_sided:
    True clamps both differences at 0 before squaring, the form of the authors' released code; False is the paper's equation.  The
    defaults are the paper's hinge-loss settings as far as they could be established without the paper at hand: settings, nothing
    here rests on them.  capacity: rows of the device ring; flush() at least every `capacity` observations keeps every row.

    Construction needs no GPU.  The record and the ring are allocated once, at the first use - in a capture's eager warm-up at the
    latest, so their addresses are fixed before any capture.

    status() is one 64-byte copy; flush() one copy of the ring rows since the last flush; curve() the flushed rows.  state_dict()
    carries the settings, the record, the flushed curve and the unflushed ring rows.  A rollback (snapshot.py) does not rewind
    the anchors.  Under data parallelism each rank would keep anchors of its own shard: out of scope, refused by TrainLoop and
    Trainer."""

    def __init__(self, batch, weight=0.3, decay=0.99, warmup=1000, one_sided=True, capacity=4096, device="cuda:0"):
        self.batch, self.weight, self.decay = int(batch), float(weight), float(decay)
        self.warmup, self.one_sided, self.capacity = int(warmup), bool(one_sided), int(capacity)
        if self.batch < 1:
            raise ValueError("batch must be >= 1, got %r" % (batch,))
        if not abs(self.weight) <= float(np.finfo(np.float32).max):
            raise ValueError("weight must be a finite fp32 number, got %r" % (weight,))
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError("decay must be in [0, 1], got %r" % (decay,))
        if not 0 <= self.warmup < 1 << 31:
            raise ValueError("warmup must be in 0 .. 2^31 - 1, got %r" % (warmup,))
        if not 1 <= self.capacity < 1 << 24:
            raise ValueError("capacity must be in 1 .. 2^24 - 1, got %r" % (capacity,))
        self.rate = lecam_rate(self.decay)
        self.device = torch.device(device)
        self.observations = 0          # observe() calls in all, across resumes: the default iteration label and the ring rows written
        self._record = np.zeros(STATE_WORDS, np.uint32)          # what the device record starts from, until it exists
        self._pending = np.zeros((0, RING_WORDS), np.uint32)          # loaded ring rows that were never flushed
        self._state = self._ring = None
        self._flushed = 0
        self._curve = np.zeros((0, RING_WORDS), np.uint32)

    # ---- device tensors, made on first use -----------------------------------------------------------------------------------------
    @property
    def state(self):
        """the 64-byte device record (int32 [16])"""
        if self._state is None:
            self._state = torch.from_numpy(self._record.view(np.int32).copy()).to(self.device)
            self._ring = torch.zeros(self.capacity, RING_WORDS, dtype=torch.int32, device=self.device)
            if len(self._pending):          # the rows a saved state had not flushed go back where they were
                at = (np.arange(self._flushed, self._flushed + len(self._pending)) % self.capacity).astype(np.int64)
                self._ring[torch.from_numpy(at).to(self.device)] = torch.from_numpy(self._pending.view(np.int32).copy()).to(self.device)
                self._pending = self._pending[:0]
        return self._state

    @property
    def ring(self):
        self.state
        return self._ring

    def d_loss(self, d_true, d_fake, d_aug, gamma):
        """train.d_loss with the regulariser: (losses[4] = {d_error, penalty, total, R}, g_true, g_fake, g_aug), the three gradients
        the rows of one [3, B] tensor (g_true._base).  One launch, no host read: legal under stream capture once the record exists."""
        t, f, a = _logits(d_true, "d_true"), _logits(d_fake, "d_fake"), _logits(d_aug, "d_aug")
        B = t.numel()
        if B != self.batch or f.numel() != B or a.numel() != B:
            raise ValueError("this LeCam was made for batches of %d logits, got %d, %d and %d" % (self.batch, B, f.numel(), a.numel()))
        state = self.state
        losses = torch.empty(4, dtype=torch.float32, device=t.device)
        g = torch.empty(3, B, dtype=torch.float32, device=t.device)
        check(lib().locate_d_loss_lecam(t.data_ptr(), f.data_ptr(), a.data_ptr(), B, float(gamma), state.data_ptr(), self.weight,
                                        int(self.one_sided), self.warmup, losses.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                                        g[2].data_ptr(), _stream()), "locate_d_loss_lecam")
        return losses, g[0], g[1], g[2]

    def observe(self, d_true, d_gen, iteration=None):
        """One launch on the current stream: this iteration's logits - the step's out["d_true"] = D(real) and out["d_gen"] =
        -D(G(z)) - into the anchors and the ring.  `iteration` labels the ring row (default: the count of observations so far)."""
        t, g = _logits(d_true, "d_true"), _logits(d_gen, "d_gen")
        if t.numel() != self.batch or g.numel() != self.batch:
            raise ValueError("this LeCam was made for batches of %d logits, got %d and %d" % (self.batch, t.numel(), g.numel()))
        state = self.state
        label = self.observations + 1 if iteration is None else int(iteration)
        check(lib().locate_lecam_observe(t.data_ptr(), g.data_ptr(), self.batch, label, state.data_ptr(), self._ring.data_ptr(),
                                         self.capacity, float(self.rate), _stream()), "locate_lecam_observe")
        self.observations += 1          # what the kernel does to words 3 and 5

    # ---- reading ---------------------------------------------------------------------------------------------------------------------
    def _read_record(self):
        if self._state is None:
            return self._record.copy()
        return self._state.cpu().numpy().view(np.uint32).copy()

    def status(self):
        """{"anchor_real", "anchor_fake", "observations", "accepted", "nonfinite", "active"}: one 64-byte copy from the device"""
        w = self._read_record()
        return {"anchor_real": float(w[0:1].view(np.float32)[0]), "anchor_fake": float(w[1:2].view(np.float32)[0]),
                "observations": int(w[3]), "accepted": int(w[2]), "nonfinite": int(w[4]),
                "active": bool(np.float32(self.weight) != 0 and int(w[2]) >= max(self.warmup, 1))}

    def _unflushed(self):
        """the ring rows written since the last flush that the ring still holds (uint32 [n, 8]) and the count of rows written"""
        last = self.observations
        first = max(self._flushed, last - self.capacity)
        if last == first:
            return np.zeros((0, RING_WORDS), np.uint32), last
        if self._state is None:          # loaded and never used: the rows are still on the host
            return self._pending[len(self._pending) - (last - first):].copy(), last
        a, b = first % self.capacity, (last - 1) % self.capacity + 1
        if a < b:
            rows = self._ring[a:b].cpu().numpy()
        else:          # the span wraps: the whole ring in one copy
            ring = self._ring.cpu().numpy()
            rows = np.concatenate([ring[a:], ring[:b]])
        return rows.view(np.uint32), last

    def flush(self):
        """The ring rows appended since the last flush (one copy from the device) join curve(); returns them as curve() would.  Rows
        that the ring has overwritten since - more than `capacity` observations between two flushes - are lost."""
        rows, last = self._unflushed()
        self._flushed = last
        self._pending = self._pending[:0]
        if not len(rows):
            return []
        self._curve = np.concatenate([self._curve, rows])
        return _curve_records(rows)

    def curve(self):
        """every flushed row: [{"iteration", "anchor_real", "anchor_fake", "mean_real", "mean_fake", "accepted"}]"""
        return _curve_records(self._curve)

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def _settings(self):
        return {"weight": self.weight, "decay": self.decay, "warmup": self.warmup, "one_sided": self.one_sided}

    def state_dict(self):
        """Tensors and plain Python types only.  Does not flush: the unflushed ring rows travel as they are."""
        rows, last = self._unflushed()
        return {"settings": dict(self._settings(), batch=self.batch, capacity=self.capacity),
                "record": torch.from_numpy(self._read_record().view(np.int32).copy()), "observations": int(last),
                "curve": torch.from_numpy(self._curve.view(np.int32).copy()), "ring_rows": torch.from_numpy(rows.view(np.int32).copy())}

    def load_state_dict(self, state):
        saved = {k: state["settings"][k] for k in ("weight", "decay", "warmup", "one_sided")}
        if saved != self._settings():
            raise ValueError("the saved LeCam regulariser ran with %r, this run's has %r" % (saved, self._settings()))
        record = state["record"].numpy().view(np.uint32).copy()
        rows = state["ring_rows"].numpy().view(np.uint32).reshape(-1, RING_WORDS).copy()
        if record.shape != (STATE_WORDS,) or len(rows) > int(state["observations"]):
            raise ValueError("the saved LeCam state is damaged: a record of %s words, %d ring rows for %d observations"
                             % (record.shape, len(rows), int(state["observations"])))
        rows = rows[max(len(rows) - self.capacity, 0):]          # a smaller ring than the saved one keeps the newest rows
        self._record = record
        self.observations = int(state["observations"])
        self._curve = state["curve"].numpy().view(np.uint32).reshape(-1, RING_WORDS).copy()
        self._flushed = self.observations - len(rows)
        self._pending = rows
        if self._state is not None:
            state_t, self._state = self._state, None
            ring_t = self._ring
            self.state                                          # builds fresh tensors from the record and the pending rows ...
            state_t.copy_(self._state)                          # ... whose values go to the addresses a captured graph reads
            ring_t.copy_(self._ring)
            self._state, self._ring = state_t, ring_t


def _curve_records(rows):
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, RING_WORDS)
    it = rows[:, 0].copy().view(np.int32)
    ar, af, mr, mf = (rows[:, k].copy().view(np.float32) for k in (1, 2, 3, 4))
    return [{"iteration": int(it[k]), "anchor_real": float(ar[k]), "anchor_fake": float(af[k]), "mean_real": float(mr[k]),
             "mean_fake": float(mf[k]), "accepted": int(rows[k, 5])} for k in range(len(rows))]
