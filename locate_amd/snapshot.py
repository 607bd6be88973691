"""A last-good copy of the training state in device memory, and the way back to it.  The run statistics notice a non-finite value,
the guarded optimizer makes a bad GRADIENT cost one step - but once a WEIGHT is NaN or Inf every further gradient is, and all a run
could do was stop and lose everything since the last save (once per epoch; an epoch is (e + 1)^2 passes over the data).  Long runs
keep a copy of the state a few hundred iterations old in device memory, return to it and carry on with the next batches, with no
file I/O and no restart.  The reference has nothing of the kind; like the average, the statistics and the guard this is opt-in, a
separate object with kernels of its own (csrc/snapshot.hip through the C ABI, include/locate_hip.h) launched BETWEEN two iterations:
the trajectory of a run that takes snapshots and never restores one is that of a run without them, bit for bit
(tests/test_gpu_snapshot.py).

    snap = TrainingSnapshot(step, average=avg)          # two slots of device memory, allocated once
    snap.take(iteration)                                # two launches, no host read: copy + classify, then commit if all was finite
    snap.restore()                                      # -> the iteration of the state the run now holds; NoSnapshot if there is none

take() copies every tensor into the slot that is NOT the last good one and counts, in the same pass, the words that are NaN or Inf.
A one-block launch behind it makes that slot the good one only when the count is zero - so the good slot never holds a non-finite
value, and a rejected take costs nothing but its bandwidth.  The decision is taken on the device: take() can sit inside a captured
hipGraph and decides anew at every replay.

Limits:
  * the commit test is "every copied word is finite".  A state that is finite but already diverging can be committed; the run then
    fails again after the rollback, and the trainer stops, as it always did, once `max_rollbacks` is used up;
  * data parallelism is out of scope - every rank would have to take the same decision: `TrainingSnapshot` over a step with a
    gradient reducer raises ValueError;
  * a slot lives in device memory only; `locate_amd.spill.SnapshotSpill` writes a committed slot to disk in the background, and
    the checkpoint files persist the state at the end of an epoch.

Importing this module does not load the HIP library.  A tensor on the CPU raises TypeError: there is no CPU path."""
import ctypes
import struct

import torch

from ._tables import arena_layout, chunk_pairs, remember, stage  # noqa: F401  (arena_layout is part of this module's interface)

RECORD_BYTES = 48
COMMIT_BYTES = 64
_COMMIT = "<iiQqqqqqii"          # csrc/snapshot.hip, SnapshotCommit
_NO_TENSOR = 0x7fffffff
KINDS = {torch.int32: 0, torch.float32: 1, torch.float64: 2}          # how a tensor's 4-byte words are judged, by default
ZERO_FILL = (0, 0, 0, 0)
SCHED_FILL = struct.unpack("<4I", struct.pack("<2d", 0.0, 1.0))          # Nadam's fresh (step, m_schedule) pair


class NoSnapshot(RuntimeError):
    """restore() without a committed slot: no take has passed its check yet (or the run was just resumed)."""


def _fill_words(fill):
    """a fill pattern of 1, 2 or 4 uint32 words -> the four words a 16-byte store holds"""
    words = [int(w) for w in fill]
    if len(words) not in (1, 2, 4) or any(not 0 <= w <= 0xffffffff for w in words):
        raise ValueError("a fill pattern is 1, 2 or 4 words of 32 bits, got %r" % (fill,))
    return tuple(words * (4 // len(words)))


def _decode_commit(raw, names):
    good, _, _, iteration, taken, rejected, r_iteration, r_count, r_tensor, _ = struct.unpack(_COMMIT, raw)
    return {"good": good, "iteration": iteration, "taken": taken, "rejected": rejected, "last_rejected_iteration": r_iteration,
            "last_rejected_count": r_count, "last_rejected_tensor": names[r_tensor] if 0 <= r_tensor < len(names) else None}


class StateSnapshot:
    """Two slots over any list of device tensors.

    named: [(name, getter, n_words, kind, fill)].  `getter()` returns the live tensor - contiguous, on `device`, float32, float64 or
    int32, of n_words 4-byte words - or None while it does not exist yet; its address may change between takes.  kind: 0 the words
    are never judged, 1 they are fp32, 2 they are the halves of fp64 values (n_words even).  fill: 1, 2 or 4 words of 32 bits that
    take() writes, repeating, in place of a tensor that does not exist - so a slot always holds a complete image, and restoring
    it gives a tensor that appeared since the take the value of fresh state.

    The two slots are one allocation each, made here and never moved; bytes between two tensors are zero and never written.  The
    64-byte commit record is a device tensor.  The device table is cached on ALL the live addresses and rebuilt when one changes or
    appears (one table at a time: a captured take names its table's arrays, so capture only once every tensor exists).

    take(iteration): the two launches on `torch.cuda.current_stream()`; no host read.
    status(): one 64-byte device-to-host copy -> {"good": -1 | 0 | 1, "iteration": of the good slot, "taken", "rejected",
      "last_rejected_iteration", "last_rejected_count": words that were NaN or Inf (an fp64 counts once),
      "last_rejected_tensor": the first such entry's name, or None}.
    restore(): reads the status; raises NoSnapshot if no slot is committed; otherwise copies the good slot back into the live
      tensors, bumps their version counters and returns the snapshot's iteration.
    slot(i): slot i as a uint8 tensor."""

    def __init__(self, named, device):
        self.device = torch.device(device)
        self._named = []
        for name, getter, n_words, kind, fill in named:
            n_words, kind = int(n_words), int(kind)
            if n_words < 0 or kind not in (0, 1, 2) or (kind == 2 and n_words % 2):
                raise ValueError("%s: %d words of kind %d" % (name, n_words, kind))
            self._named.append((str(name), getter, n_words, kind, _fill_words(fill)))
        if not any(n for _, _, n, _, _ in self._named):
            raise ValueError("StateSnapshot: nothing to copy")
        self.names = [name for name, _, _, _, _ in self._named]
        self._live()          # a tensor that cannot be copied is refused before any memory is taken
        if self.device.type != "cuda":
            raise TypeError("StateSnapshot keeps its slots on the GPU only; the device is %s" % self.device)
        self.offsets, self.slot_bytes = arena_layout([n for _, _, n, _, _ in self._named])
        self._slots = [torch.zeros(self.slot_bytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
        first = struct.pack(_COMMIT, -1, _NO_TENSOR, 0, 0, 0, 0, 0, 0, -1, 0)
        self._commit = torch.frombuffer(bytearray(first), dtype=torch.int64).to(self.device)
        self._tables = {}

    def _live(self):
        """the live tensors (None: does not exist yet), checked"""
        out = []
        for name, getter, n_words, _, _ in self._named:
            t = getter()
            if t is not None:
                if not torch.is_tensor(t) or t.device.type != "cuda":
                    raise TypeError("%s: a snapshot copies GPU tensors only; got %s" % (name, t.device if torch.is_tensor(t) else type(t).__name__))
                if t.device != self.device and (t.device.index is not None and self.device.index is not None):
                    raise TypeError("%s is on %s, the snapshot on %s" % (name, t.device, self.device))
                if t.dtype not in KINDS or not t.is_contiguous():
                    raise TypeError("%s: a snapshot copies contiguous float32, float64 or int32 tensors, got %s%s"
                                    % (name, t.dtype, "" if t.is_contiguous() else " (strided)"))
                if t.numel() * t.element_size() != 4 * n_words:
                    raise ValueError("%s holds %d bytes, its entry says %d words" % (name, t.numel() * t.element_size(), n_words))
            out.append(t)
        return out

    def slot(self, i):
        return self._slots[i]

    def _table(self, live):
        key = tuple(0 if t is None else t.data_ptr() for t in live)
        tab = self._tables.get(key)
        if tab is not None:
            return tab
        from ._lib import lib
        L = lib()
        assert L.locate_snapshot_record_bytes() == RECORD_BYTES and L.locate_snapshot_commit_bytes() == COMMIT_BYTES
        rec = b"".join(struct.pack("<Qqqi4I4x", ptr, off, n, kind, *fill)
                       for ptr, off, (_, _, n, kind, fill) in zip(key, self.offsets, self._named))
        pairs, _ = chunk_pairs([n for _, _, n, _, _ in self._named], L.locate_snapshot_chunk_elems())
        return remember(self._tables, key, stage(rec, pairs, len(self._named), self.device), 0)          # one table at a time

    def take(self, iteration):
        from ._lib import check, lib
        tab = self._table(self._live())
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
        check(lib().locate_snapshot_take(ptr(tab.records), ptr(tab.chunks), tab.n_tensors, tab.n_chunks, ptr(self._slots[0]),
                                         ptr(self._slots[1]), ptr(self._commit), int(iteration),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_snapshot_take")
        return self

    def status(self):
        return _decode_commit(self._commit.cpu().numpy().tobytes(), self.names)          # the one device-to-host copy

    def restore(self):
        from ._lib import check, lib
        state = self.status()
        if state["good"] < 0:
            raise NoSnapshot("no snapshot has been committed: %d taken, %d rejected" % (state["taken"], state["rejected"]))
        live = self._live()
        tab = self._table(live)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
        check(lib().locate_snapshot_restore(ptr(tab.records), ptr(tab.chunks), tab.n_tensors, tab.n_chunks, ptr(self._slots[state["good"]]),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_snapshot_restore")
        # the kernel wrote through raw pointers: tell autograd and the packed-panel cache that the tensors changed
        written = [t for t, (_, _, n, _, _) in zip(live, self._named) if t is not None and n]
        torch._C._increment_version(written)
        return state["iteration"]


def _optimizer_state(opt, p, key):
    st = opt.state.get(p)          # .get: looking must not create the entry
    return st.get(key) if st else None


class TrainingSnapshot(StateSnapshot):
    """The whole training state of a `TrainStep` (and of an `AveragedGenerator` beside it) as a `StateSnapshot`.

    For G, then D, in `state_dict()` order: every `state_dict` entry (the spectral-norm u / v are among them), "G/NAME"; for every
    parameter of the network's optimizer its moments, "G/opt/NAME/exp_avg" and ".../exp_avg_sq" (zero where Nadam has not created
    them yet: D's u / v gain state at the second D-step, G's unused `i_norm.weight`s never do); then every parameter's float64
    (step, m_schedule) pair, ".../sched" (judged as fp64; (0.0, 1.0) where it does not exist).  With `average`: every `state_dict`
    entry of `average.generator`, "A/NAME", and `average.updates`, which is kept on the host beside each take.  `G.noise` is
    constant during training and left out.

    take(iteration): ValueError for iteration < 1 - before the first G-step D's u / v are not trainable yet (the reference's
    main.py:172), and that flag is host state a restore would not return.

    restore(), beyond the copy and the version bumps:
      * optimizer state that did not exist at the take needs nothing special: the slot holds its fill, the in-place copy makes it
        equal to fresh state, and addresses - with them device tables and captured graphs - stay valid;
      * `average.updates` becomes what it was at the take;
      * `ops.refresh_panels` re-packs both networks' weight panels on the same stream: a hipGraph replay reads the panels packed
        behind the PREVIOUS step and would otherwise contract with the discarded weights.  The version bump has un-stamped every
        `_locate_wmax`, so the re-pack takes its own maximum pass; no stamp is put back;
      * a `GuardedNadam`'s `consecutive_skips` restarts at 0; its other counters keep counting.
    What is NOT rewound: the input pipeline, the latent stream, iteration counters, loss history and statistics records - the run
    goes on with the NEXT batches.

    Memory: two slots of (weights + two moments) of both networks plus the average - about 365 MB each at 64 x 64, full width."""

    def __init__(self, step, average=None):
        if getattr(step, "reducer_g", None) is not None or getattr(step, "reducer_d", None) is not None:
            raise ValueError("TrainingSnapshot: data parallelism is out of scope - every rank would have to take the same decision")
        self.step, self.average = step, average
        named = []
        for tag, net, opt in (("G", step.gen, step.gen_opt), ("D", step.dis, step.dis_opt)):
            named += self._network(tag, net)
            names = {id(p): n for n, p in net.named_parameters()}
            params = [p for group in opt.param_groups for p in group["params"]]
            for key in ("exp_avg", "exp_avg_sq"):
                named += [("%s/opt/%s/%s" % (tag, names.get(id(p), i), key), lambda opt=opt, p=p, key=key: _optimizer_state(opt, p, key),
                           p.numel(), 1, ZERO_FILL) for i, p in enumerate(params)]
            named += [("%s/opt/%s/sched" % (tag, names.get(id(p), i)), lambda opt=opt, p=p: _optimizer_state(opt, p, "sched"), 4, 2, SCHED_FILL)
                      for i, p in enumerate(params)]
        if average is not None:
            named += self._network("A", average.generator)
        self._updates = {}          # iteration of a take -> average.updates then
        super().__init__(named, next(step.gen.parameters()).device)

    @staticmethod
    def _network(tag, net):
        entries = []
        for k, t in net.state_dict(keep_vars=True).items():
            if t.dtype not in KINDS:
                raise TypeError("%s/%s: a snapshot copies float32, float64 or int32 tensors, got %s" % (tag, k, t.dtype))
            entries.append(("%s/%s" % (tag, k), lambda t=t: t.detach(), t.numel() * t.element_size() // 4, KINDS[t.dtype], ZERO_FILL))
        return entries

    def take(self, iteration):
        if int(iteration) < 1:
            raise ValueError("TrainingSnapshot.take: iteration %r - the first snapshot follows the first whole iteration" % (iteration,))
        super().take(iteration)
        if self.average is not None:
            self._updates[int(iteration)] = int(self.average.updates)
        return self

    def status(self):
        state = super().status()
        for it in [it for it in self._updates if it < state["iteration"]]:          # no take that old can be the good one any more
            del self._updates[it]
        return state

    def restore(self):
        from . import ops
        iteration = super().restore()
        if self.average is not None:
            self.average.updates = self._updates[iteration]
        for net in (self.step.gen, self.step.dis):
            ops.refresh_panels([p for p in net.parameters() if "_locate_panels" in p.__dict__])
        for opt in (self.step.gen_opt, self.step.dis_opt):
            if hasattr(opt, "load_counters_state"):
                opt.load_counters_state({**opt.counters(), "consecutive_skips": 0})
        return iteration
