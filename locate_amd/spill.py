"""The last-good snapshot on disk, written in the background.  The statistics, the guard and the rollback protect a run against
its own arithmetic; nothing protected it against a machine reset, a pre-emption or a killed job: `Trainer.save_state()` runs once per
epoch (an epoch is (e + 1)^2 passes over the data), synchronises the device, clones every tensor to the host one at a time and
pickles the lot, so it cannot run every few hundred iterations.  `TrainingSnapshot` (snapshot.py) already keeps a checked, finite,
contiguous image of the whole training state in device memory.  Here a committed slot goes to a file on the run's disk, and the
training stream never waits for it:

    spill = SnapshotSpill(snapshot, folder)             # one pinned host buffer of a slot's size, a side stream, a writer thread
    spill.take(iteration, host_state)                   # snapshot.take behind a wait for the copy in flight, if any
    spill.begin()                                       # digests + device-to-host copy on the side stream; a thread writes the file
    found = SnapshotSpill.latest(folder)                # the valid file with the highest iteration, or None
    restore_training_state(found, step, average)        # into fresh objects, through the ordinary loading paths

Every entry of a slot carries a 128-bit digest over its 4-byte words, modulo 2^64:  A = sum w_i,  B = sum ((i + 1) mod 2^32) w_i
(csrc/digest.hip through the C ABI, include/locate_hip.h; `digest_model` is the same sums in numpy).  The device computes them over
the slot in device memory, the writer thread recomputes them from the bytes that arrived in the pinned buffer - a difference means
the copy raced a take or the memory is bad, and no file is written - and the loader recomputes them from the file.

Ordering.  The file holds the slot committed at an EARLIER take: it was finite then, and the run has passed its checks again
since.  begin() makes the side stream wait for an event on the current stream (the take that filled the slot lies in front of it)
and records an event behind the copy; take() makes the current stream wait for that event before the next take's first store, so
a take never overwrites a slot that is still being read.  Nothing else is issued on the training stream.

The file:  the 8-byte magic;  the JSON header's length as a little-endian uint64;  the header;  zero bytes up to a multiple of
4096;  the arena - a slot byte for byte in `arena_layout`'s order (snapshot.py);  the host blob (`torch.save` bytes, loaded with
`weights_only=True`).  The header holds the format version, `iteration`, `slot_bytes`, per entry `name`, `offset`, `n_words`, `kind`,
`dtype`, `shape`, `existed` and `digest` [A, B], and the blob's length and `zlib.crc32`.  A file is written to `path + ".tmp"`,
flushed, fsynced and renamed over `path`: a reader never sees half a file, and `read_spill` refuses anything else that is wrong.

Memory: one pinned host buffer of `snapshot.slot_bytes` (about 366 MB at 64 x 64, full width, with an average).  Cost, measured
there (profiles/notes_spill.md): begin() takes 0.5 ms of the caller's time; the stream does not wait for the copy, but the
iterations that run beside it share the device with it and were 2.6 ms slower each, about 5 ms per spill.

Out of scope: data parallelism (`TrainingSnapshot` already refuses a reducer); compression; making the epoch-end `save_state()`
asynchronous; bit-exact graphed resumes (a graphed run's two warm-up iterations per resume advance the state, as today).

Importing this module does not load the HIP library; the file format and `digest_model` need neither it nor a GPU."""
import ctypes
import glob
import io
import json
import os
import struct
import threading
import time
import zlib
from collections import namedtuple

import numpy as np
import torch

from ._tables import chunk_pairs, stage

MAGIC = b"LOCSPILL"
FORMAT_VERSION = 1
ALIGN = 4096
RECORD_BYTES = 16
_DTYPES = {"float32": np.float32, "float64": np.float64, "int32": np.int32}
_KIND_DTYPE = {0: "int32", 1: "float32", 2: "float64"}
_MODEL_BLOCK = 1 << 20          # words per step of digest_model: bounds its temporaries at a few MB


class SpillCorrupt(RuntimeError):
    """A spill file that cannot be trusted: .path, .what"""

    def __init__(self, path, what):
        super().__init__("%s: %s" % (path, what))
        self.path, self.what = path, what


class SpillMismatch(RuntimeError):
    """The bytes that arrived on the host do not have the digests the device computed: no file was written."""


class Spill(namedtuple("Spill", "header arrays host_state")):
    """What read_spill returns: (header, {name: np.ndarray}, host_state), plus .path and .skipped (`SnapshotSpill.latest`)"""
    path = None
    skipped = ()


# ---- the digest -----------------------------------------------------------------------------------------------------------------------
def digest_model(words, start=0):
    """(A, B) as Python ints for a 1-d array of 4-byte words (any 4-byte dtype is read as uint32): the sums csrc/digest.hip takes,
    modulo 2^64.  numpy's uint64 arithmetic wraps exactly like the kernel's.  start: the index of words[0] in its tensor - the
    digests of the pieces of a tensor add up to the tensor's."""
    w = np.ascontiguousarray(words).reshape(-1)
    if w.dtype.itemsize != 4:
        raise TypeError("digest_model reads 4-byte words, got %s" % w.dtype)
    w = w.view(np.uint32)
    a = b = np.uint64(0)
    with np.errstate(over="ignore"):
        for at in range(0, w.size, _MODEL_BLOCK):
            w64 = w[at:at + _MODEL_BLOCK].astype(np.uint64)
            index = np.arange(int(start) + at + 1, int(start) + at + 1 + w64.size, dtype=np.uint64) & np.uint64(0xffffffff)
            a = a + w64.sum(dtype=np.uint64)
            b = b + (index * w64).sum(dtype=np.uint64)
    return int(a), int(b)


def _digest_table(pointers, word_counts, device):
    """device table of locate_digest over tensors at `pointers` of `word_counts` words -> (Table, first, partials, out)"""
    from ._lib import lib
    L = lib()
    assert L.locate_digest_record_bytes() == RECORD_BYTES
    rec = b"".join(struct.pack("<Qq", p, n) for p, n in zip(pointers, word_counts))
    pairs, first = chunk_pairs(word_counts, L.locate_digest_chunk_elems())
    tab = stage(rec, pairs, len(word_counts), device) if pairs else None
    first_host = torch.tensor(first + [len(pairs)], dtype=torch.int32).pin_memory()
    first_dev = first_host.to(device, non_blocking=True)
    partials = torch.empty(max(len(pairs), 1), 2, dtype=torch.int64, device=device)
    out = torch.zeros(len(word_counts), 2, dtype=torch.int64, device=device)
    return tab, (first_dev, first_host), partials, out


def _launch_digest(table, stream):
    from ._lib import check, lib
    tab, (first, _), partials, out = table
    if tab is None:          # nothing but empty tensors: their digests are the zeros `out` was made with
        return out
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    check(lib().locate_digest(ptr(tab.records), ptr(tab.chunks), ptr(first), tab.n_tensors, tab.n_chunks, ptr(partials), ptr(out),
                              ctypes.c_void_p(stream.cuda_stream)), "locate_digest")
    return out


def tensor_digests(tensors):
    """uint64 [n, 2] on the device: {A, B} of every tensor's 4-byte words, for ad hoc use.  Contiguous float32, float64 or int32
    GPU tensors; TypeError for a CPU or strided one.  Two launches on the current stream, no host read."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("tensor_digests: no tensors")
    for i, t in enumerate(tensors):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise TypeError("tensor %d: digests are taken of GPU tensors only" % i)
        if t.dtype not in (torch.float32, torch.float64, torch.int32) or not t.is_contiguous():
            raise TypeError("tensor %d: digests are taken of contiguous float32, float64 or int32 tensors, got %s%s"
                            % (i, t.dtype, "" if t.is_contiguous() else " (strided)"))
    counts = [t.numel() * t.element_size() // 4 for t in tensors]
    table = _digest_table([t.data_ptr() if n else 0 for t, n in zip(tensors, counts)], counts, tensors[0].device)
    out = _launch_digest(table, torch.cuda.current_stream())
    result = out.view(torch.uint64)
    result._locate_digest_table = table          # the launches (a captured graph's too) read the table: it lives as long as the result
    return result


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
def _serialise(host_state):
    buf = io.BytesIO()
    torch.save(host_state, buf)
    return buf.getvalue()


def write_spill(path, header, arena_bytes, host_blob):
    """header: {"iteration", "slot_bytes", "entries": [{name, offset, n_words, kind, dtype, shape, existed, digest}]}; the format
    version and the blob's length and CRC are added here.  Atomic: written beside `path`, fsynced, renamed."""
    arena = memoryview(arena_bytes).cast("B")
    if arena.nbytes != int(header["slot_bytes"]):
        raise ValueError("the arena holds %d bytes, the header says %d" % (arena.nbytes, int(header["slot_bytes"])))
    host_blob = bytes(host_blob)
    head = dict(header, version=FORMAT_VERSION, blob_bytes=len(host_blob), blob_crc32=zlib.crc32(host_blob) & 0xffffffff)
    text = json.dumps(head).encode("utf-8")
    front = MAGIC + struct.pack("<Q", len(text)) + text
    front += b"\0" * (-len(front) % ALIGN)
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(front)
        f.write(arena)
        f.write(host_blob)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)
    return path


def _read_header(path, data):
    if len(data) < len(MAGIC) + 8 or data[:len(MAGIC)] != MAGIC:
        raise SpillCorrupt(path, "bad magic")
    (n,) = struct.unpack_from("<Q", data, len(MAGIC))
    start = len(MAGIC) + 8
    if n > len(data) - start:
        raise SpillCorrupt(path, "truncated inside the header")
    try:
        header = json.loads(bytes(data[start:start + n]).decode("utf-8"))
        iteration, slot_bytes, blob_bytes = int(header["iteration"]), int(header["slot_bytes"]), int(header["blob_bytes"])
        int(header["blob_crc32"])
        entries = header["entries"]
        if header["version"] != FORMAT_VERSION or min(iteration, slot_bytes, blob_bytes) < 0 or not isinstance(entries, list):
            raise ValueError("version %r" % (header["version"],))
    except (ValueError, KeyError, TypeError, UnicodeDecodeError) as err:
        raise SpillCorrupt(path, "bad header: %s" % err) from None
    return header, (start + n + ALIGN - 1) // ALIGN * ALIGN


def read_spill(path):
    """-> Spill(header, {name: np.ndarray of the entry's dtype and shape}, host_state).  Every entry's digest and the blob's CRC
    are recomputed: SpillCorrupt on any mismatch, truncation, bad magic, bad JSON, an offset past the arena or trailing garbage."""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError as err:
        raise SpillCorrupt(path, "unreadable: %s" % err) from None
    header, at = _read_header(path, data)
    slot_bytes, blob_bytes = int(header["slot_bytes"]), int(header["blob_bytes"])
    if len(data) < at + slot_bytes + blob_bytes:
        raise SpillCorrupt(path, "truncated: %d bytes, the header describes %d" % (len(data), at + slot_bytes + blob_bytes))
    if len(data) > at + slot_bytes + blob_bytes:
        raise SpillCorrupt(path, "%d bytes behind the host blob" % (len(data) - at - slot_bytes - blob_bytes))
    arena = np.frombuffer(data, dtype=np.uint8, count=slot_bytes, offset=at)
    arrays = {}
    for e in header["entries"]:
        try:
            name, off, n, dtype, shape = str(e["name"]), int(e["offset"]), int(e["n_words"]), _DTYPES[e["dtype"]], [int(s) for s in e["shape"]]
            want = (int(e["digest"][0]), int(e["digest"][1]))
            bool(e["existed"]), int(e["kind"])
        except (KeyError, ValueError, TypeError, IndexError) as err:
            raise SpillCorrupt(path, "bad entry: %r" % (err,)) from None
        if off < 0 or n < 0 or off % 4 or off + 4 * n > slot_bytes:
            raise SpillCorrupt(path, "%s: bytes [%d, %d) of an arena of %d" % (name, off, off + 4 * n, slot_bytes))
        words = arena[off:off + 4 * n].view(np.uint32)
        if digest_model(words) != want:
            raise SpillCorrupt(path, "%s: the digest does not match" % name)
        if int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize != 4 * n or name in arrays:
            raise SpillCorrupt(path, "%s: shape %s of %s does not hold %d words" % (name, shape, e["dtype"], n))
        arrays[name] = words.view(dtype).reshape(shape)
    blob = data[at + slot_bytes:]
    if zlib.crc32(blob) & 0xffffffff != int(header["blob_crc32"]):
        raise SpillCorrupt(path, "the host blob's CRC does not match")
    try:
        host_state = torch.load(io.BytesIO(blob), map_location="cpu", weights_only=True)
    except Exception as err:          # noqa: BLE001 - whatever the unpickler makes of damaged bytes
        raise SpillCorrupt(path, "the host blob does not load: %s" % err) from None
    found = Spill(header, arrays, host_state)
    found.path = path
    return found


def _peek_iteration(path):
    """the iteration a file's header names, unchecked; -1 where there is none"""
    try:
        with open(path, "rb") as f:
            front = f.read(len(MAGIC) + 8)
            (n,) = struct.unpack_from("<Q", front, len(MAGIC)) if len(front) == len(MAGIC) + 8 else (0,)
            front += f.read(min(n, 1 << 26))
        return int(_read_header(path, front)[0]["iteration"])
    except (OSError, SpillCorrupt, struct.error):
        return -1


# ---- the spill ------------------------------------------------------------------------------------------------------------------------
class SnapshotSpill:
    """A `StateSnapshot` / `TrainingSnapshot`'s committed slot to `folder/spill-<n % keep>.bin`, n counting the spills begun.

    Owns one pinned host buffer of `snapshot.slot_bytes`, a small pinned digest buffer, one side stream, one writer thread (a
    daemon, started with the first job) and the device digest table over each of the two slots - built here once: the slots never
    move.

    take(iteration, host_state=None): the current stream waits for the copy in flight, if any; then `snapshot.take(iteration)`.
      `host_state`, a tree of tensors and plain values, is serialised here, on the caller's thread, and kept by iteration with the
      record of which entries existed (a getter that returns None: lazily created Nadam state, whose fill the slot then holds).
    begin(): reads `snapshot.status()` (the one 64-byte device-to-host copy).  False - nothing is issued - if no slot is committed,
      if the good slot's iteration is not newer than the last spill begun, or if the writer is still busy (`skipped_busy` counts).
      Otherwise the side stream waits for an event recorded on the current stream, runs the two digest launches over the good
      slot and copies slot and digests into the pinned buffers; an event is recorded behind them, the job goes to the writer, True.
    The writer: `event.synchronize()` - the only GPU call it ever makes -, `digest_model` over every entry of the pinned bytes
      against the device's digests (`SpillMismatch`, no file, on a difference), then `write_spill`.  An exception in the writer is
      kept and raised from the next begin() / wait() / close().
    wait(): until the writer is idle.  status(): {"begun", "written", "skipped_busy", "last_iteration", "last_path", "last_seconds"}
      (`last_seconds`: begin() to the rename; `timing`: the last spill's {"event", "digest", "write"} shares).  close(): ends the writer.
    latest(folder) (static): `read_spill` of the valid `spill-*.bin` with the highest iteration, its `.skipped` naming the corrupt
      files passed over; None if no file is valid."""

    def __init__(self, snapshot, folder, keep=2):
        if int(keep) < 1:
            raise ValueError("keep must be >= 1, got %r" % (keep,))
        self.snapshot, self.folder, self.keep = snapshot, str(folder), int(keep)
        dev = snapshot.device
        self._counts = [n for _, _, n, _, _ in snapshot._named]
        self._pinned = torch.empty(snapshot.slot_bytes, dtype=torch.uint8).pin_memory()
        self._pinned_digests = torch.empty(len(self._counts), 2, dtype=torch.int64).pin_memory()
        self._stream = torch.cuda.Stream(device=dev)
        self._tables = [_digest_table([snapshot.slot(i).data_ptr() + off for off in snapshot.offsets], self._counts, dev) for i in (0, 1)]
        self._copy_event = None
        self._host = {}          # iteration of a take -> (host blob, [(existed, dtype, shape)])
        self._last_begun = 0
        self._cond = threading.Condition()
        self._job, self._busy, self._error, self._thread, self._closed = None, False, None, None, False
        self._hold = None          # a test hook: an Event the writer waits for before it touches a job
        self.begun = self.written = self.skipped_busy = 0
        self.last_iteration, self.last_path, self.last_seconds, self.timing = None, None, None, {}
        os.makedirs(self.folder, exist_ok=True)
        # go on behind the newest file a previous run left, so that it is the last to be replaced
        seen = [_peek_iteration(self._path(k)) for k in range(self.keep)]
        self._next = (max(range(self.keep), key=lambda k: seen[k]) + 1) % self.keep if max(seen) >= 0 else 0

    def _path(self, k):
        return os.path.join(self.folder, "spill-%d.bin" % k)

    # ---- the caller's thread --------------------------------------------------------------------------------------------------------
    def take(self, iteration, host_state=None):
        if self._copy_event is not None:
            torch.cuda.current_stream().wait_event(self._copy_event)          # the slot this take writes may still be read
        shapes = []
        for t, (_, _, n, kind, _) in zip(self.snapshot._live(), self.snapshot._named):
            if t is None:
                shapes.append((False, _KIND_DTYPE[kind], [n // 2 if kind == 2 else n]))
            else:
                shapes.append((True, str(t.dtype).replace("torch.", ""), list(t.shape)))
        blob = _serialise(host_state)
        self.snapshot.take(iteration)
        self._host[int(iteration)] = (blob, shapes)
        return self

    def _raise_kept(self):
        with self._cond:
            err, self._error = self._error, None
        if err is not None:
            raise err

    def begin(self):
        self._raise_kept()
        if self._closed:
            raise RuntimeError("SnapshotSpill.begin after close()")
        state = self.snapshot.status()
        iteration = int(state["iteration"])
        if state["good"] < 0 or iteration <= self._last_begun:
            return False
        for it in [it for it in self._host if it < iteration]:          # no take that old can be the good one any more
            del self._host[it]
        with self._cond:
            if self._busy:
                self.skipped_busy += 1
                return False
        if iteration not in self._host:
            raise RuntimeError("the good slot holds iteration %d, which was not taken through SnapshotSpill.take" % iteration)
        blob, shapes = self._host[iteration]
        good = state["good"]
        started = time.perf_counter()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())          # the only thing issued on the current stream
        self._stream.wait_event(ready)
        with torch.cuda.stream(self._stream):
            digests = _launch_digest(self._tables[good], self._stream)
            self._pinned.copy_(self.snapshot.slot(good), non_blocking=True)
            self._pinned_digests.copy_(digests, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._stream)
        self._copy_event = done
        path = self._path(self._next)
        self._next = (self._next + 1) % self.keep
        self._last_begun = iteration
        self.begun += 1
        with self._cond:
            self._job, self._busy = (done, iteration, blob, shapes, path, started), True
            if self._thread is None:
                self._thread = threading.Thread(target=self._writer, name="locate-spill-writer", daemon=True)
                self._thread.start()
            self._cond.notify_all()
        return True

    def wait(self):
        with self._cond:
            while self._busy:
                self._cond.wait()
        self._raise_kept()
        return self

    def status(self):
        with self._cond:
            return {"begun": self.begun, "written": self.written, "skipped_busy": self.skipped_busy, "last_iteration": self.last_iteration,
                    "last_path": self.last_path, "last_seconds": self.last_seconds}

    def close(self):
        with self._cond:
            while self._busy:
                self._cond.wait()
            self._closed = True
            self._cond.notify_all()
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        self._raise_kept()

    # ---- the writer thread ----------------------------------------------------------------------------------------------------------
    def _writer(self):
        while True:
            with self._cond:
                while self._job is None and not self._closed:
                    self._cond.wait()
                if self._job is None:
                    return
                job, self._job = self._job, None
            try:
                if self._hold is not None:
                    self._hold.wait()
                result = self._write(*job)
                with self._cond:
                    self.written += 1
                    self.last_iteration, self.last_path, self.last_seconds, self.timing = result
            except BaseException as err:          # noqa: BLE001 - kept for the caller's thread
                with self._cond:
                    self._error = err
            finally:
                with self._cond:
                    self._busy = False
                    self._cond.notify_all()

    def _write(self, done, iteration, blob, shapes, path, started):
        t0 = time.perf_counter()
        done.synchronize()          # the only GPU call of this thread
        t1 = time.perf_counter()
        arena = self._pinned.numpy()
        device = self._pinned_digests.numpy().view(np.uint64)
        entries = []
        for i, ((name, _, n, kind, _), off, (existed, dtype, shape)) in enumerate(zip(self.snapshot._named, self.snapshot.offsets, shapes)):
            got = digest_model(arena[off:off + 4 * n].view(np.uint32))
            want = (int(device[i, 0]), int(device[i, 1]))
            if got != want:
                raise SpillMismatch("iteration %d, %s: the device's digest of the slot is %016x %016x, the copy on the host has "
                                    "%016x %016x - the copy raced a take or the memory is bad; no file was written"
                                    % (iteration, name, want[0], want[1], got[0], got[1]))
            entries.append({"name": name, "offset": off, "n_words": n, "kind": kind, "dtype": dtype, "shape": shape, "existed": existed,
                            "digest": [got[0], got[1]]})
        t2 = time.perf_counter()
        write_spill(path, {"iteration": iteration, "slot_bytes": self.snapshot.slot_bytes, "entries": entries}, arena, blob)
        t3 = time.perf_counter()
        return iteration, path, t3 - started, {"event": t1 - t0, "digest": t2 - t1, "write": t3 - t2}

    # ---- reading ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def latest(folder):
        best, skipped = None, []
        for path in sorted(glob.glob(os.path.join(str(folder), "spill-*.bin"))):
            try:
                found = read_spill(path)
            except SpillCorrupt:
                skipped.append(path)
                continue
            if best is None or int(found.header["iteration"]) > int(best.header["iteration"]):
                best = found
        if best is not None:
            best.skipped = tuple(skipped)
        return best


# ---- back into a run ------------------------------------------------------------------------------------------------------------------
def _optimizer_names(tag, net, opt):
    """[(parameter index in state_dict()'s numbering, "TAG/opt/NAME")], as TrainingSnapshot names them"""
    names = {id(p): n for n, p in net.named_parameters()}
    params = [p for group in opt.param_groups for p in group["params"]]
    return [(i, p, "%s/opt/%s" % (tag, names.get(id(p), i))) for i, p in enumerate(params)]


def restore_training_state(found, step, average=None):
    """What a spill file holds into FRESH objects, through the ordinary loading paths - so what follows a normal resume (version
    bumps, the lazy panel re-pack, dropped Nadam tables) follows here too.  "G/..." and "D/..." go to `load_state_dict`;
    `gen.noise` and the `dis_uv_trainable` flag come from the host state ("noise", "dis_uv_trainable"), as `load_checkpoint`
    handles them; the optimizers' `exp_avg`, `exp_avg_sq` and float64 `sched` entries that `existed` are assembled in torch.optim's
    layout with `param_groups` taken from `opt.state_dict()` and go to `opt.load_state_dict` - an entry with `existed` False creates
    no state: a resumed optimizer must not gain state the uninterrupted run did not have; "A/...", the noise and the host state's
    "average" {"updates", "one_minus_beta"} go to `average.load_state_dict`.  ValueError on a name, shape or dtype that does not
    fit, before anything is written.  Returns the spill's iteration."""
    header, arrays, host = found[0], found[1], found[2]
    host = host if isinstance(host, dict) else {}
    existed = {e["name"]: bool(e["existed"]) for e in header["entries"]}
    want = {}          # name -> (shape, numpy dtype)
    for tag, net in (("G", step.gen), ("D", step.dis)) + ((("A", average.generator),) if average is not None else ()):
        for k, t in net.state_dict().items():
            want["%s/%s" % (tag, k)] = (tuple(t.shape), str(t.dtype).replace("torch.", ""))
    opts = []
    for tag, net, opt in (("G", step.gen, step.gen_opt), ("D", step.dis, step.dis_opt)):
        named = _optimizer_names(tag, net, opt)
        opts.append((opt, named))
        for _, p, name in named:
            want[name + "/exp_avg"] = want[name + "/exp_avg_sq"] = (tuple(p.shape), "float32")
            want[name + "/sched"] = ((2,), "float64")
    missing, unknown = sorted(set(want) - set(arrays)), sorted(k for k in set(arrays) - set(want) if average is not None or not k.startswith("A/"))
    if missing or unknown:
        raise ValueError("the spill does not fit this run: missing %s, unknown %s" % (missing[:4], unknown[:4]))
    for name, (shape, dtype) in want.items():
        a = arrays[name]
        if existed[name] and (tuple(a.shape) != shape or a.dtype.name != dtype):
            raise ValueError("%s: the spill holds %s %s, this run's is %s %s" % (name, a.dtype.name, tuple(a.shape), dtype, shape))
        if not existed[name] and a.size * a.dtype.itemsize != int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize:
            raise ValueError("%s: the spill holds %d bytes, this run's has %s %s" % (name, a.size * a.dtype.itemsize, dtype, shape))
    for _, named in opts:
        for _, _, name in named:
            if len({existed[name + k] for k in ("/exp_avg", "/exp_avg_sq", "/sched")}) != 1:
                raise ValueError("%s: Nadam creates its three state entries together, the spill holds some of them" % name)
    noise = host.get("noise")
    if noise is None or tuple(noise.shape) != tuple(step.gen.noise.shape):
        raise ValueError("the spill's host state holds no noise map of shape %s" % (tuple(step.gen.noise.shape),))
    if average is not None:
        if not isinstance(host.get("average"), dict) or float(host["average"]["one_minus_beta"]) != average.one_minus_beta:
            raise ValueError("the spill's host state does not hold this average's updates and 1 - beta = %r" % average.one_minus_beta)

    tensor = lambda name: torch.from_numpy(arrays[name].copy())          # noqa: E731
    for tag, net in (("G", step.gen), ("D", step.dis)):
        net.load_state_dict({k: tensor("%s/%s" % (tag, k)) for k in net.state_dict()})
    if host.get("dis_uv_trainable", False):
        step.dis.requires_grad_(True)          # main.py:172 has already run in the spilled state
    with torch.no_grad():
        step.gen.noise.copy_(noise)
    for opt, named in opts:
        state = {i: {k: tensor("%s/%s" % (name, k)) for k in ("exp_avg", "exp_avg_sq", "sched")} for i, _, name in named if existed[name + "/sched"]}
        opt.load_state_dict({"state": state, "param_groups": opt.state_dict()["param_groups"]})
    if average is not None:
        sd = {k: tensor("A/" + k) for k in average.generator.state_dict()}
        sd.update(noise=noise, updates=int(host["average"]["updates"]), one_minus_beta=float(host["average"]["one_minus_beta"]))
        average.load_state_dict(sd)
    return int(header["iteration"])
