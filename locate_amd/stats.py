"""Checking a run's health: per-tensor statistics of every weight and every gradient of both networks - the sum of squares, the
largest magnitude, the number of non-finite elements - and a guard that stops a run whose numbers have stopped being numbers
before its last good state is overwritten.  The reference has nothing of the kind; like the monitor, the metric and the averaged
generator this is an addition BESIDE the training step: a separate object with a kernel of its own (csrc/stats.hip through the C
ABI, include/locate_hip.h) that is launched between two iterations, where `LossHistory.record` and `AveragedGenerator.update` are.
It only READS what the step left in device memory - the post-step weights, and in every parameter's `.grad` the gradient its
optimizer step consumed - so the trajectory of a run that records is that of a run that does not, bit for bit
(tests/test_gpu_stats.py).

    sumsq, absmax, nonfinite = tensor_statistics([t0, t1, ...])        # ad hoc: three device tensors
    stats = RunStatistics(gen, dis, capacity=256)
    stats.record(iteration)                                             # between two iterations: no host read
    rows = stats.flush()                                                # one device-to-host copy of everything since the last flush
    stats.check()                                                       # flush, then NonFiniteError if a new record has a non-finite
    stats.global_norms();  stats.save(folder, epoch)

Per tensor (csrc/stats.hip): `sumsq` is the float64 sum of the exact squares of the FINITE elements (within n * 2^-52 relative of
the exact sum, the same bits from call to call and wherever the tensor sits in the table), `absmax` the largest finite magnitude
(exact, denormals included, 0 if there is none), `nonfinite` the count of NaN and +-Inf elements.

Importing this module does not load the HIP library.  A tensor on the CPU raises TypeError: there is no CPU path."""
import ctypes
import os
import struct

import numpy as np
import torch

from ._tables import chunk_pairs, require_device_tensors, stage


class NonFiniteError(RuntimeError):
    """A record holds NaN or Inf.  `iteration`: that of the first such record; `tensors`: [(name, count), ...] of that record,
    in entry order."""

    def __init__(self, iteration, tensors):
        self.iteration = int(iteration)
        self.tensors = [(str(name), int(count)) for name, count in tensors]
        shown = ", ".join("%s (%d)" % t for t in self.tensors[:4])
        if len(self.tensors) > 4:
            shown += ", ... %d more" % (len(self.tensors) - 4)
        super().__init__("non-finite values at iteration %d in %d tensor%s: %s"
                         % (self.iteration, len(self.tensors), "" if len(self.tensors) == 1 else "s", shown))


def _device_table(tensors):
    """The table (_tables.Table, the workspace as its `scratch`) of locate_stats_reduce for non-empty device tensors."""
    from ._lib import lib
    L = lib()
    assert L.locate_stats_tensor_record_bytes() == 24 and L.locate_stats_record_bytes() == 16
    pairs, first = chunk_pairs([t.numel() for t in tensors], L.locate_stats_chunk_elems())
    rec = b"".join(struct.pack("<Qqi4x", t.data_ptr(), t.numel(), at) for t, at in zip(tensors, first))
    dev = tensors[0].device
    ws = torch.empty(max(L.locate_stats_workspace_bytes(len(pairs)) // 8, 2), dtype=torch.int64, device=dev)
    return stage(rec, pairs, len(tensors), dev, scratch=ws)


def _launch(table, row):
    """row: int64 [1 + n_tensors, 2] device memory - the summary's 8 bytes (and 8 unused), then the 16-byte records"""
    from ._lib import check, lib
    t_dev, c_dev, n_t, n_c, ws = table[:5]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    check(lib().locate_stats_reduce(ptr(t_dev), ptr(c_dev), n_t, n_c, ptr(row[1]), ptr(row[0]), ptr(ws),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_stats_reduce")


def tensor_statistics(tensors):
    """(sumsq float64 [k], absmax float32 [k], nonfinite int64 [k]) of k contiguous float32 device tensors, as device tensors:
    one pass over their memory (a launch that reduces every 4096-element chunk, and a small one that combines the chunks of each
    tensor) on `torch.cuda.current_stream()`, no host read.  A zero-element tensor gives (0, 0, 0)."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("tensor_statistics needs at least one tensor")
    require_device_tensors(tensors, "tensor_statistics")
    dev = tensors[0].device
    live = [i for i, t in enumerate(tensors) if t.numel() > 0]
    k = len(tensors)
    if not live:
        return (torch.zeros(k, dtype=torch.float64, device=dev), torch.zeros(k, dtype=torch.float32, device=dev),
                torch.zeros(k, dtype=torch.int64, device=dev))
    row = torch.zeros(1 + len(live), 2, dtype=torch.int64, device=dev)
    _launch(_device_table([tensors[i].detach() for i in live]), row)
    sumsq = row[1:, 0].contiguous().view(torch.float64)
    absmax = (row[1:, 1] & 0xFFFFFFFF).to(torch.int32).view(torch.float32)
    nonfinite = (row[1:, 1] >> 32) & 0xFFFFFFFF
    if len(live) == k:
        return sumsq, absmax, nonfinite
    at = torch.tensor(live, dtype=torch.int64).to(dev)
    return (torch.zeros(k, dtype=torch.float64, device=dev).index_copy_(0, at, sumsq),
            torch.zeros(k, dtype=torch.float32, device=dev).index_copy_(0, at, absmax),
            torch.zeros(k, dtype=torch.int64, device=dev).index_copy_(0, at, nonfinite))


def _decode(words):
    """int64 [n, 2] host records -> (sumsq float64 [n], absmax float32 [n], nonfinite uint32 [n])"""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, 2)
    second = np.ascontiguousarray(words[:, 1]).view(np.uint64)
    return (np.ascontiguousarray(words[:, 0]).view(np.float64).copy(),
            (second & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32),
            (second >> np.uint64(32)).astype(np.uint32))


class RunStatistics:
    """Statistics of every parameter of `gen` and `dis` (spectral-norm u / v included) and of every gradient, one record per call
    of record().

    Entries, in this order: for the generator ("G") and then the discriminator ("D"), every `named_parameters()` entry as
    "G/<name>", directly followed by "G/<name>.grad" where the parameter's `.grad` is not None at that record.  Before the first
    backward no gradient entry exists; a parameter that never receives a gradient (the generator's unused `i_norm.weight`s) never
    has one.  Zero-element tensors are skipped.  `entry_names()` lists the entries a record taken now would have.

    record(iteration) writes one row of a preallocated device ring [capacity, 1 + 2 * parameters] of 16-byte words - the launch's
    8-byte summary, then one {sumsq, absmax, nonfinite} per entry - with no allocation and no host read, on
    `torch.cuda.current_stream()`: call it on the stream the iteration (or the replay) was issued on.  The iteration number stays
    on the host.  A full ring flushes first, as `LossHistory` does.  The device table is cached on ALL the addresses it holds and
    rebuilt when one changes (eagerly `zero_grad()` drops the gradients and the next backward allocates new ones; under hipGraph
    replay and under data parallelism the gradients sit in fixed buffers).

    flush() reads the rows recorded since the last flush back in ONE device-to-host copy and returns them; every row is a dict
    {"iteration", "names" (tuple), "sumsq" float64 [n], "absmax" float32 [n], "nonfinite" uint32 [n], "total", "first"} - the last
    two are the launch's summary: the number of non-finite elements in all, and the index of the first entry that has one or -1.
    All rows since construction (or clear()) stay in `rows`.

    check() flushes and raises NonFiniteError for the first row not checked before that holds a non-finite value; it decides from
    the row's summary.  The rows - the bad one and those before it - stay in `rows`.

    global_norms(): per row {"iteration", "G/weight", "G/grad", "D/weight", "D/grad"}: sqrt of the summed `sumsq` of a network's
    parameter entries and of its gradient entries, in float64 on the host (0.0 where there is none).  A number for a curve.

    save(folder, epoch) writes `folder/{epoch}-stats.npz` (to a .tmp, then renamed): `names` [entries] - the union over the rows,
    in entry order - `iterations` [records], `sumsq` [records, entries] float64, `absmax` float32 and `nonfinite` uint32; an entry
    that did not exist at a record is held as NaN / 0 / 0.

    Under data parallelism the weights are equal on every rank and the gradients are after the exchange: only rank 0 needs one,
    as with `Sampler`."""

    def __init__(self, gen, dis, capacity=256):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        self.nets = (("G", gen), ("D", dis))
        self.capacity = int(capacity)
        self.rows = []
        self._checked = 0
        self._ring = None
        self._pending = []          # (iteration, names) of the rows the ring holds
        self._key = None
        self._tab = None
        self._names = ()
        self._order = None
        self._params = None
        self.last_iteration = None          # that of the latest record, read or not

    # ---- entries ------------------------------------------------------------------------------------------------------------------
    def _parameters(self):
        """[(entry name, parameter)] of both networks, listed once: the set of parameters does not change during a run"""
        if self._params is None:
            self._params = [("%s/%s" % (tag, name), p) for tag, net in self.nets for name, p in net.named_parameters() if p.numel() > 0]
        return self._params

    def _entries(self):
        out = []
        for name, p in self._parameters():
            out.append((name, p))
            if p.grad is not None:
                out.append((name + ".grad", p.grad))
        return out

    def entry_names(self):
        return [name for name, _ in self._entries()]

    def _position(self, name):
        """place of an entry among all the entries there can be"""
        if self._order is None:
            self._order = {}
            for tag, net in self.nets:
                for pname, _ in net.named_parameters():
                    for full in ("%s/%s" % (tag, pname), "%s/%s.grad" % (tag, pname)):
                        self._order[full] = len(self._order)
        return self._order.get(name, len(self._order))

    @property
    def names(self):
        """the union of the rows' entries, in entry order"""
        seen = set()
        for row in self.rows:
            seen.update(row["names"])
        return sorted(seen, key=self._position)

    # ---- recording ------------------------------------------------------------------------------------------------------------------
    def record(self, iteration):
        params = self._parameters()
        if not params:
            raise ValueError("RunStatistics: the networks have no parameters")
        key = []          # ALL the addresses the table holds, a missing gradient as 0
        for _, p in params:
            g = p.grad
            key.append(p.data_ptr())
            key.append(0 if g is None else g.data_ptr())
        if key != self._key:
            entries = self._entries()
            tensors = [t.detach() for _, t in entries]
            require_device_tensors(tensors, "RunStatistics")
            self._tab = _device_table(tensors)
            self._key = key
            self._names = tuple(name for name, _ in entries)
        if self._ring is None:
            self._ring = torch.zeros(self.capacity, 1 + 2 * len(params), 2, dtype=torch.int64, device=params[0][1].device)
        if len(self._pending) == self.capacity:
            self.flush()
        _launch(self._tab, self._ring[len(self._pending)])
        self._pending.append((int(iteration), self._names))
        self.last_iteration = int(iteration)
        return self

    def flush(self):
        if not self._pending:
            return []
        host = self._ring[:len(self._pending)].cpu().numpy()          # the one device-to-host copy
        rows = []
        for r, (iteration, names) in enumerate(self._pending):
            sumsq, absmax, nonfinite = _decode(host[r, 1:1 + len(names)])
            summary = np.ascontiguousarray(host[r, 0, :1]).view(np.uint32)
            rows.append({"iteration": iteration, "names": names, "sumsq": sumsq, "absmax": absmax, "nonfinite": nonfinite,
                         "total": int(summary[0]), "first": int(summary[1:2].view(np.int32)[0])})
        self._pending = []
        self.rows += rows
        return rows

    def check(self):
        self.flush()
        fresh, self._checked = self.rows[self._checked:], len(self.rows)
        for row in fresh:
            if row["total"] or row["first"] >= 0:
                raise NonFiniteError(row["iteration"], [(n, int(c)) for n, c in zip(row["names"], row["nonfinite"]) if c])
        return self

    def clear(self):
        """forget the rows read so far (the ring's unread rows stay)"""
        self.rows, self._checked = [], 0
        return self

    # ---- reading ------------------------------------------------------------------------------------------------------------------
    def global_norms(self):
        self.flush()
        out = []
        for row in self.rows:
            sums = {"G/weight": 0.0, "G/grad": 0.0, "D/weight": 0.0, "D/grad": 0.0}
            for name, s in zip(row["names"], row["sumsq"]):
                sums[name[:2] + ("grad" if name.endswith(".grad") else "weight")] += float(s)
            rec = {k: float(np.sqrt(np.float64(v))) for k, v in sums.items()}
            rec["iteration"] = row["iteration"]
            out.append(rec)
        return out

    def save(self, folder, epoch):
        self.flush()
        names = self.names
        at = {name: j for j, name in enumerate(names)}
        shape = (len(self.rows), len(names))
        sumsq = np.full(shape, np.nan, dtype=np.float64)
        absmax = np.zeros(shape, dtype=np.float32)
        nonfinite = np.zeros(shape, dtype=np.uint32)
        for r, row in enumerate(self.rows):
            cols = [at[name] for name in row["names"]]
            sumsq[r, cols], absmax[r, cols], nonfinite[r, cols] = row["sumsq"], row["absmax"], row["nonfinite"]
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "%d-stats.npz" % epoch)
        with open(path + ".tmp", "wb") as f:
            np.savez(f, names=np.array(names, dtype=np.str_), iterations=np.array([row["iteration"] for row in self.rows], dtype=np.int64),
                     sumsq=sumsq, absmax=absmax, nonfinite=nonfinite)
        os.replace(path + ".tmp", path)
        return [path]
