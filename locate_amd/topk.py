"""Top-k training of the generator (Sinha, Zhao, Goyal, Raffel, Odena 2020, "Top-k Training of GANs: Improving GAN Performance by
Throwing Away Bad Samples"): in the G-step only the k fakes with the highest D(G(z)) contribute to the loss and its gradient; k starts
at the batch size and is annealed down to a floor.  DiffAugment acts on what D sees, LeCam on what D says; this acts on what the
GENERATOR learns from: the fakes D rejects most firmly, whose gradient points away from the data, are thrown away.

    k        = max(k_min, min(B, int(floor(B * gamma ** periods + 0.5)))),  k_min = max(1, ceil(floor * B)),  periods = iterations // every
    kept     = the k logits that stand first: higher first, a NaN before everything, equal logits (-0 == +0) by lower index
    g_error  = sum_kept relu(1 - f_i) / k;   d g_error / d f_i = -(1 / k) where i is kept and (1 - f_i) >= 0, else +0

All of it runs in the G-step's one loss launch (csrc/topk.hip, locate_g_loss_topk) with no host read, no extra pass and no second
backward; k is read from word 0 of a 64-byte device record at a fixed address, so a replayed hipGraph follows the schedule: set_k() /
advance() are one 4-byte copy between two iterations, and only when k changes.  The same launch writes the plain loss over the whole
batch, the record's statistics and one row {launch, k, active, threshold, mean_all, mean_kept, nonfinite} of a device ring.  The
definition in numpy, which the kernel equals with ==: tests/helpers/topk_model.py.

    topk = TopK(batch=64, gamma=0.99, floor=0.5, every=batches_per_epoch)
    step = TrainStep(..., topk=topk);  TrainLoop.iteration and Trainer call advance() before every iteration

A NaN logit is always selected, so the loss is a NaN: nothing is laundered.  With k = B - gamma = 1, or a record never set - loss and
gradient are locate_g_loss's bits.  It keeps no statistics of the logits, so it is legal beside a data-parallel reducer: each rank
selects within its shard, and k is the same function of the iteration on every rank (not run at more than one rank)."""
import math

import numpy as np
import torch

from ._lib import check, lib

STATE_WORDS = 16
RING_WORDS = 8          # {launch ordinal, k_used, active, threshold, mean_all, mean_kept, nonfinite (1 / 0), 0}
MAX_BATCH = 4096
# words 0 .. 7 of the device record (csrc/topk.hip; the layout is defined in tests/helpers/topk_model.py, FIELDS)
FIELDS = ("k", "launches", "nonfinite", "k_used", "active", "threshold", "mean_all", "mean_kept")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def topk_k(batch, gamma, floor, periods):
    """k after `periods` annealing periods, a pure function in float64: B * gamma ** periods rounded half up, at most B and at least
    k_min = max(1, ceil(floor * B))."""
    B = int(batch)
    k_min = max(1, int(math.ceil(float(floor) * B)))
    return max(k_min, min(B, int(math.floor(B * float(gamma) ** int(periods) + 0.5))))


class TopK:
    """Top-k selection in the G-step of one training step: the schedule's settings, the device record k is read from and the ring of
    the per-launch statistics.

    gamma: k's decay per period of `every` iterations (the paper anneals once an epoch: `every` = the iterations of one pass over the
    images).  floor: the fraction of the batch k stops at.  gamma = 0.99 and floor = 0.5 are the paper's settings as far as they could
    be recalled without the paper at hand: settings, nothing here rests on them.  capacity: rows of the device ring; flush() at least
    every `capacity` launches keeps every row.

    Construction needs no GPU.  The record and the ring are allocated once, at the first use - in a capture's eager warm-up at the
    latest, so their addresses are fixed before any capture.

    status() is one 64-byte copy; flush() that and one copy of the ring rows since the last flush; curve() the flushed rows, one per
    LAUNCH of the loss (a capture's warm-up iterations and every pass of a G-step with minibatches > 1 included).  state_dict()
    carries the settings, the record, the flushed curve and the unflushed ring rows.  A rollback (snapshot.py) does not rewind it."""

    def __init__(self, batch, gamma=0.99, floor=0.5, every=1000, capacity=4096, device="cuda:0"):
        self.batch, self.gamma, self.floor = int(batch), float(gamma), float(floor)
        self.every, self.capacity = int(every), int(capacity)
        if not 1 <= self.batch <= MAX_BATCH:
            raise ValueError("batch must be in 1 .. %d, got %r" % (MAX_BATCH, batch))
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError("gamma must be in (0, 1], got %r" % (gamma,))
        if not 0.0 <= self.floor <= 1.0:
            raise ValueError("floor must be in [0, 1], got %r" % (floor,))
        if not 1 <= self.every < 1 << 31:
            raise ValueError("every must be in 1 .. 2^31 - 1, got %r" % (every,))
        if not 1 <= self.capacity < 1 << 24:
            raise ValueError("capacity must be in 1 .. 2^24 - 1, got %r" % (capacity,))
        self.device = torch.device(device)
        self._record = np.zeros(STATE_WORDS, np.uint32)          # what the device record starts from, until it exists
        self._record[0] = self.batch
        self._pending = np.zeros((0, RING_WORDS), np.uint32)          # loaded ring rows that were never flushed
        self._state = self._ring = None
        self._flushed = 0
        self._curve = np.zeros((0, RING_WORDS), np.uint32)

    @property
    def k(self):
        """what word 0 of the record holds (the host's copy: only the host writes it)"""
        return int(self._record[0:1].view(np.int32)[0])

    def scheduled_k(self, iterations_done):
        return topk_k(self.batch, self.gamma, self.floor, int(iterations_done) // self.every)

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

    def g_loss(self, d_fake, form=0):
        """train.g_loss over the k logits that stand first: (losses[2] = {loss_topk, loss_all}, g).  One launch, no host read: legal
        under stream capture once the record exists.  form: 0 lets the library choose the selection by B, 1 counts ranks, 2 sorts."""
        if not (torch.is_tensor(d_fake) and d_fake.is_cuda and d_fake.dtype == torch.float32 and d_fake.numel() > 0):
            raise TypeError("d_fake must be a non-empty fp32 tensor of logits on the GPU (there is no CPU path)")
        f = d_fake.detach().contiguous()
        B = f.numel()
        if B != self.batch:
            raise ValueError("this TopK was made for batches of %d logits, got %d" % (self.batch, B))
        state = self.state
        losses = torch.empty(2, dtype=torch.float32, device=f.device)
        g = torch.empty(B, dtype=torch.float32, device=f.device)
        check(lib().locate_g_loss_topk(f.data_ptr(), B, state.data_ptr(), self._ring.data_ptr(), self.capacity, int(form), losses.data_ptr(),
                                       g.data_ptr(), _stream()), "locate_g_loss_topk")
        return losses, g

    def set_k(self, k):
        """k of the launches from here on, on the current stream: one 4-byte copy into word 0, and none when k is what it was.  A k
        outside 1 .. batch selects everything.  Call it between two iterations: a replayed graph reads whatever was written last."""
        k = int(k)
        if not -(1 << 31) <= k < 1 << 31:
            raise ValueError("k must be an int32, got %r" % (k,))
        if k == self.k:
            return False
        self._record[0:1].view(np.int32)[0] = k
        if self._state is not None:
            self._state[:1].copy_(torch.tensor([k], dtype=torch.int32))
        return True

    def advance(self, iterations_done):
        """set_k(the schedule's k after `iterations_done` iterations); before every iteration, where DiffAugment.draw() is"""
        return self.set_k(self.scheduled_k(iterations_done))

    # ---- reading ---------------------------------------------------------------------------------------------------------------------
    def _read_record(self):
        if self._state is None:
            return self._record.copy()
        return self._state.cpu().numpy().view(np.uint32).copy()

    def status(self):
        """{"k", "k_used", "launches", "nonfinite", "active", "threshold", "mean_all", "mean_kept"}: one 64-byte copy from the device.
        mean_kept - mean_all is how far the kept fakes' mean logit lies above the batch's."""
        return _status(self._read_record())

    def _unflushed(self):
        """the record, the ring rows written since the last flush that the ring still holds (uint32 [n, 8]) and the count of rows
        written: the launches run inside replayed graphs, so only the device knows their number"""
        record = self._read_record()
        last = int(record[1])
        first = max(self._flushed, last - self.capacity)
        if last <= first:
            return record, np.zeros((0, RING_WORDS), np.uint32), max(last, self._flushed)
        if self._state is None:          # loaded and never used: the rows are still on the host
            return record, self._pending[len(self._pending) - (last - first):].copy(), last
        a, b = first % self.capacity, (last - 1) % self.capacity + 1
        if a < b:
            rows = self._ring[a:b].cpu().numpy()
        else:          # the span wraps: the whole ring in one copy
            ring = self._ring.cpu().numpy()
            rows = np.concatenate([ring[a:], ring[:b]])
        return record, rows.view(np.uint32), last

    def flush(self):
        """The ring rows appended since the last flush (one copy of the record, one of the rows) join curve(); returns them as curve()
        would.  Rows that the ring has overwritten since - more than `capacity` launches between two flushes - are lost."""
        _, rows, last = self._unflushed()
        self._flushed = last
        self._pending = self._pending[:0]
        if not len(rows):
            return []
        self._curve = np.concatenate([self._curve, rows])
        return _curve_records(rows)

    def curve(self):
        """every flushed row: [{"launch", "k", "active", "threshold", "mean_all", "mean_kept", "nonfinite"}]"""
        return _curve_records(self._curve)

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def _settings(self):
        return {"batch": self.batch, "gamma": self.gamma, "floor": self.floor, "every": self.every}

    def state_dict(self):
        """Tensors and plain Python types only.  Does not flush: the unflushed ring rows travel as they are."""
        record, rows, _ = self._unflushed()
        return {"settings": dict(self._settings(), capacity=self.capacity), "record": torch.from_numpy(record.view(np.int32).copy()),
                "curve": torch.from_numpy(self._curve.view(np.int32).copy()), "ring_rows": torch.from_numpy(rows.view(np.int32).copy())}

    def load_state_dict(self, state):
        saved = {k: state["settings"][k] for k in ("batch", "gamma", "floor", "every")}
        if saved != self._settings():
            raise ValueError("the saved top-k selection ran with %r, this run's has %r" % (saved, self._settings()))
        record = state["record"].numpy().view(np.uint32).copy()
        rows = state["ring_rows"].numpy().view(np.uint32).reshape(-1, RING_WORDS).copy()
        if record.shape != (STATE_WORDS,) or len(rows) > int(record[1]):
            raise ValueError("the saved top-k state is damaged: a record of %s words, %d ring rows for %d launches"
                             % (record.shape, len(rows), int(record[1]) if record.shape == (STATE_WORDS,) else -1))
        rows = rows[max(len(rows) - self.capacity, 0):]          # a smaller ring than the saved one keeps the newest rows
        self._record = record
        self._curve = state["curve"].numpy().view(np.uint32).reshape(-1, RING_WORDS).copy()
        self._flushed = int(record[1]) - len(rows)
        self._pending = rows
        if self._state is not None:
            state_t, self._state = self._state, None
            ring_t = self._ring
            self.state                                          # builds fresh tensors from the record and the pending rows ...
            state_t.copy_(self._state)                          # ... whose values go to the addresses a captured graph reads
            ring_t.copy_(self._ring)
            self._state, self._ring = state_t, ring_t


def _word_float(word):
    return float(np.array([word], np.uint32).view(np.float32)[0])


def _status(w):
    return {"k": int(w[0:1].view(np.int32)[0]), "k_used": int(w[3]), "launches": int(w[1]), "nonfinite": int(w[2]), "active": int(w[4]),
            "threshold": _word_float(w[5]), "mean_all": _word_float(w[6]), "mean_kept": _word_float(w[7])}


def _curve_records(rows):
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, RING_WORDS)
    th, ma, mk = (rows[:, k].copy().view(np.float32) for k in (3, 4, 5))
    return [{"launch": int(rows[n, 0]), "k": int(rows[n, 1]), "active": int(rows[n, 2]), "threshold": float(th[n]), "mean_all": float(ma[n]),
             "mean_kept": float(mk[n]), "nonfinite": int(rows[n, 6])} for n in range(len(rows))]
