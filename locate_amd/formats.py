"""Asking whether a number format would hold: for the tensors the matrix cores actually consume - the gathered activations, the
output gradients and the weights of every dense contraction of a real iteration - how much of each a candidate format flushes to
zero, pushes into its subnormals or clamps, and what signal-to-quantisation-noise ratio is left.  The reference has nothing of the
kind; like the run statistics and dynamics this is an addition BESIDE the training step: a separate object with kernels of its own
(csrc/formats.hip through the C ABI, include/locate_hip.h) that only READ the step's tensors, so the trajectory of a run that audits
is that of a run that does not, bit for bit (tests/test_gpu_formats.py).

    recs = format_errors([x, w], axis=2)                 # ad hoc: decoded records of two device tensors
    audit = FormatAudit(gen, dis, capacity=64)
    with audit.iteration(i):                             # the tap is installed: every dense contraction's operands are audited
        ...one EAGER iteration...
    rows = audit.flush()                                 # one device-to-host copy of everything since the last flush
    audit.report();  audit.save(folder, epoch);  audit.clear()

The five formats (csrc/formats.hip; `format_names()`), every one rounded to nearest even onto its grid, subnormals included:
`e4m3_tensor` - what `--dtype fp8` does today: e4m3 behind one power-of-two scale per tensor - `e5m2_tensor`, the block-scaled
`mxfp8_e4m3` and `mxfp4_e2m1` of OCP MX v1.0 (one power of two per 32 elements) and `bf16`.  The e4m3 / e5m2 grids go through the
conversion instructions the fp8 contractions use.  Per tensor view the kernels count exactly and add exactly known terms in a fixed
order: the same bits from call to call.

A tensor is audited as a VIEW [B, C, P] (element (b, c, p) at b * batch_stride + c * P + p) with its 32-element scale blocks
along c (`axis` 1) or along p (`axis` 2); only the two MX formats depend on the axis.

Importing this module does not load the HIP library.  A tensor on the CPU raises TypeError: there is no CPU path."""
import contextlib
import ctypes
import os
import struct

import numpy as np
import torch

ROLES = ("fwd.x", "fwd.w", "dgrad.gy", "dgrad.w", "wgrad.x", "wgrad.gy")
FORMATS = 5
HIST = 32
BASE_WORDS = 6 + HIST          # int64 words: n, zeros, nonfinite, calls, sumsq, {absmax, pad}, hist[32]
SLOT_WORDS = BASE_WORDS + 4 * FORMATS          # ... then {err_sumsq, flushed, subnormal, clamped} per format: 464 bytes
MAX_VIEWS = 8


def format_names():
    """the formats' names in record order, from the library"""
    from ._lib import lib
    L = lib()
    return tuple(L.locate_formats_name(i).decode() for i in range(L.locate_formats_count()))


def _layout_check(L):
    assert L.locate_formats_count() == FORMATS and L.locate_formats_max_views() == MAX_VIEWS and L.locate_formats_view_record_bytes() == 40
    assert L.locate_formats_base_record_bytes() == 8 * BASE_WORDS and L.locate_formats_format_record_bytes() == 32


def _view(t, axis):
    """(tensor that owns the memory, B, C, P, batch_stride) of a float32 device tensor of 1 to 4 dimensions:
        [n]          -> [1, 1, n]
        [R, K]       -> [1, R, K]           (a weight as a matrix: rows are c, columns p)
        [B, C, P]    -> itself
        [B, C, H, W] -> [B, C, H * W]
    A 3- or 4-dimensional tensor is read in place where its [C, P] planes are dense (a channel slice of a wider tensor: the batch
    stride is free); anything else is copied with .contiguous() first - on the audit's side, the caller's tensor is never written."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise TypeError("the format audit computes on the GPU only; got %s" % (t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.float32:
        raise TypeError("the format audit takes float32 tensors, got %s" % t.dtype)
    if axis not in (1, 2):
        raise ValueError("axis must be 1 (blocks along c) or 2 (blocks along p), got %r" % (axis,))
    if not 1 <= t.dim() <= 4 or t.numel() == 0:
        raise ValueError("the format audit takes non-empty tensors of 1 to 4 dimensions, got shape %s" % (tuple(t.shape),))
    t = t.detach()
    if t.dim() <= 2:
        t = t if t.is_contiguous() else t.contiguous()
        rows = t.shape[0] if t.dim() == 2 else 1
        return t, 1, rows, t.numel() // rows, t.numel()
    B, C = t.shape[0], t.shape[1]
    P = t.numel() // (B * C)
    dense, expect = True, 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != expect:
            dense = False
        expect *= size
    if not dense or (B > 1 and t.stride(0) < C * P):
        t = t.contiguous()
    return t, B, C, P, (t.stride(0) if B > 1 else C * P)


def _pack(views):
    """[(tensor, B, C, P, batch_stride, axis)] -> the host records of locate_formats_audit"""
    return b"".join(struct.pack("<Qiii4xqi4x", t.data_ptr(), B, C, P, bs, axis) for t, B, C, P, bs, axis in views)


class _Workspaces:
    """one growing device workspace per stream: calls on one stream are ordered, calls on two (the weight-gradient side stream)
    must not share"""

    def __init__(self):
        self.by_stream = {}

    def get(self, L, rec, n):
        need = L.locate_formats_workspace_bytes(rec, n)
        if need == 0:
            from ._lib import check
            check(1, "locate_formats_workspace_bytes")
        stream = torch.cuda.current_stream()
        ws = self.by_stream.get(stream.cuda_stream)
        if ws is None or ws.numel() * 8 < need:
            # allocated with this stream current: the allocator hands the old block out again only behind this stream's work
            ws = torch.empty((max(need, 1 << 16) * 3 // 2 + 7) // 8, dtype=torch.int64, device=torch.cuda.current_device())
            self.by_stream[stream.cuda_stream] = ws
        return ws, stream.cuda_stream


def _audit(views, slots, rows, workspaces):
    """one call of locate_formats_audit: views [(tensor, B, C, P, batch_stride, axis)] (at most 8) add into `slots` of `rows`
    (int64 [..., SLOT_WORDS] device memory) on the current stream"""
    from ._lib import check, lib
    L = lib()
    rec = _pack(views)
    ws, stream = workspaces.get(L, rec, len(views))
    check(L.locate_formats_audit(rec, len(views), (ctypes.c_int * len(slots))(*slots), ctypes.c_void_p(rows.data_ptr()),
                                 ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(stream)), "locate_formats_audit")


def decode(words):
    """int64 [k, SLOT_WORDS] host slots -> {"n", "zeros", "nonfinite", "calls" uint64 [k]; "sumsq" float64 [k]; "absmax" float32 [k];
    "hist" uint64 [k, 32]; "err_sumsq" float64 [k, 5]; "flushed", "subnormal", "clamped" uint64 [k, 5]}"""
    w = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, SLOT_WORDS)
    u = w.view(np.uint64)
    f = w.view(np.float64)
    per_format = u[:, BASE_WORDS:].reshape(-1, FORMATS, 4)
    return {"n": u[:, 0].copy(), "zeros": u[:, 1].copy(), "nonfinite": u[:, 2].copy(), "calls": u[:, 3].copy(), "sumsq": f[:, 4].copy(),
            "absmax": (u[:, 5] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32), "hist": u[:, 6:BASE_WORDS].copy(),
            "err_sumsq": f[:, BASE_WORDS:].reshape(-1, FORMATS, 4)[:, :, 0].copy(), "flushed": per_format[:, :, 1].copy(),
            "subnormal": per_format[:, :, 2].copy(), "clamped": per_format[:, :, 3].copy()}


def snr_db(sumsq, err_sumsq):
    """10 log10(sumsq / err_sumsq) per format: inf where the error is 0, NaN where there is no signal either"""
    s = np.asarray(sumsq, np.float64)[..., None]
    e = np.asarray(err_sumsq, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(s / e)
    out = np.where(e == 0, np.inf, out)
    return np.where((e == 0) & (s == 0), np.nan, out)


def format_errors(views, axis=2):
    """The records of k float32 device tensors of 1 to 4 dimensions (`_view` documents the mapping to [B, C, P] and when a tensor
    is copied first), the scale blocks along `axis` (one value, or one per tensor): a list of k dicts {"n", "zeros", "nonfinite",
    "sumsq", "absmax", "hist" [32], and per format name {"err_sumsq", "snr_db", "flushed", "subnormal", "clamped"}}.  Launches on
    `torch.cuda.current_stream()`, eight tensors per call, then ONE device-to-host copy."""
    views = list(views)
    if not views:
        raise ValueError("format_errors needs at least one tensor")
    axes = [axis] * len(views) if isinstance(axis, int) else list(axis)
    if len(axes) != len(views):
        raise ValueError("format_errors: %d axes for %d tensors" % (len(axes), len(views)))
    packed = [_view(t, a) + (a,) for t, a in zip(views, axes)]
    from ._lib import lib
    _layout_check(lib())
    rows = torch.zeros(len(packed), SLOT_WORDS, dtype=torch.int64, device=packed[0][0].device)
    workspaces = _Workspaces()
    for at in range(0, len(packed), MAX_VIEWS):
        part = packed[at:at + MAX_VIEWS]
        _audit(part, list(range(at, at + len(part))), rows, workspaces)
    d = decode(rows.cpu().numpy())          # the one device-to-host copy
    snr = snr_db(d["sumsq"], d["err_sumsq"])
    names = format_names()
    out = []
    for i in range(len(packed)):
        rec = {"n": int(d["n"][i]), "zeros": int(d["zeros"][i]), "nonfinite": int(d["nonfinite"][i]), "sumsq": float(d["sumsq"][i]),
               "absmax": d["absmax"][i], "hist": d["hist"][i].copy()}
        for f, name in enumerate(names):
            rec[name] = {"err_sumsq": float(d["err_sumsq"][i, f]), "snr_db": float(snr[i, f]), "flushed": int(d["flushed"][i, f]),
                         "subnormal": int(d["subnormal"][i, f]), "clamped": int(d["clamped"][i, f])}
        out.append(rec)
    return out


def dense_layers(net):
    """[(name of the weight_bar parameter, weight_bar)] of every SpectralNorm layer of `net` whose contraction is a dense one
    (Linear, Conv1d, Conv2d / ConvTranspose2d with groups == 1), in `modules()` order: the depthwise and grouped full-size layers
    have kernels of their own and are not audited."""
    from .nn import SpectralNorm
    name_of = {id(p): name for name, p in net.named_parameters()}
    out = []
    for sn in net.modules():
        if isinstance(sn, SpectralNorm) and getattr(sn.module, "groups", 1) == 1:
            bar = getattr(sn.module, sn.name + "_bar")
            if bar.numel() > 0:
                out.append((name_of[id(bar)], bar))
    return out


class FormatAudit:
    """The contraction operands of whole iterations, one record per audited iteration.

    Entries are known at construction (which needs no GPU): every weight that can reach a dense contraction (`dense_layers`: of
    the generator as "G/<name>", then of the discriminator as "D/<name>", named after the `weight_bar` parameter as in
    `RunDynamics`), times the six roles `fwd.x`, `fwd.w`, `dgrad.gy`, `dgrad.w`, `wgrad.x`, `wgrad.gy` - the layer's input and weight
    where its forward consumes them, its output gradient and weight in the input-gradient contraction, its input and output
    gradient in the weight-gradient contraction.  `entries()` lists (name, role) in slot order.

    Block axes (they matter to the two MX formats only) follow the reduction:
      fwd.x, dgrad.gy    an activation [B, C, H, W] as [B, C, H * W], blocks along the channels (axis 1);
      wgrad.x, wgrad.gy  blocks along the pixels (axis 2): that reduction runs over batch and pixels;
      fwd.w              the weight as a matrix [shape[0], rest]: blocks along the flattened Cin * kh * kw of one output channel
                         (axis 2);
      dgrad.w            the same matrix, blocks along the output channels (axis 1).
    For a ConvTranspose2d, whose forward is the adjoint contraction, the two weight axes swap with the reductions.  This
    APPROXIMATES the K order of the packed panels, which interleaves the taps with the channels: a real MX panel's 32-blocks would
    mix kernel taps where these take consecutive channels (or consecutive Cin * kh * kw).  The per-tensor formats and bf16 do not
    depend on it.

    `with audit.iteration(i):` installs `ops.CONTRACTION_TAP`, zeroes the next row of a device ring [capacity, entries, 464
    bytes] and removes the tap on exit, also when the body raises.  Inside, every dense contraction's operands are audited by
    one call (two views) on the stream the contraction is issued on - the weight-gradient side stream included, each stream with
    a workspace of its own - keyed by the ADDRESS of the weight; a call whose weight is unknown is skipped and counted in
    `unmatched`.  Several calls of one key in an iteration - the discriminator's four forwards - add up (`calls` counts them;
    `absmax` is their maximum, `hist` is relative to each call's own absmax).  Only eager iterations can be audited: a replayed
    hipGraph runs no Python, so no tap.

    flush() reads the rows recorded since the last flush in ONE device-to-host copy and returns them: dicts {"iteration"} +
    `decode`'s arrays over the entries.  All rows since construction (or clear()) stay in `rows`.
    report(): per row {"iteration", "entries", "formats", "snr_db" [entries, 5] (10 log10(sumsq / err_sumsq), inf where the error
    is 0, NaN for an entry without calls), "flushed", "subnormal", "clamped" [entries, 5]: fractions of the entry's finite
    elements, "hist" [entries, 32]}.
    save(folder, epoch) writes `folder/{epoch}-formats.npz` (to a .tmp, then renamed): `names`, `roles` [entries], `formats` [5],
    `iterations` [records], and [records, entries, ...] `n`, `zeros`, `nonfinite`, `calls`, `sumsq`, `absmax`, `hist`, `err_sumsq`,
    `flushed`, `subnormal`, `clamped`, `snr_db`.

    Under data parallelism the operands differ per rank only by their share of the batch: only rank 0 needs one."""

    FORMAT_NAMES = ("e4m3_tensor", "e5m2_tensor", "mxfp8_e4m3", "mxfp4_e2m1", "bf16")

    def __init__(self, gen, dis, capacity=64):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        self.nets = (("G", gen), ("D", dis))
        self.capacity = int(capacity)
        self.layers = [("%s/%s" % (tag, name), w) for tag, net in self.nets for name, w in dense_layers(net)]
        if not self.layers:
            raise ValueError("FormatAudit: the networks have no dense contraction")
        self.rows = []
        self.unmatched = 0
        self.last_iteration = None
        self._ring = None
        self._pending = []
        self._keys = {}
        self._row = None
        self._workspaces = _Workspaces()

    # ---- entries ------------------------------------------------------------------------------------------------------------------
    def entries(self):
        return [(name, role) for name, _ in self.layers for role in ROLES]

    def slot(self, name, role):
        """place of an entry in a row"""
        return [n for n, _ in self.layers].index(name) * len(ROLES) + ROLES.index(role)

    def key_map(self):
        """{address of a weight: its layer's index}, as the addresses are now"""
        return {w.data_ptr(): i for i, (_, w) in enumerate(self.layers)}

    # ---- recording ------------------------------------------------------------------------------------------------------------------
    def _tap(self, role, w, a, b, forward_of_r):
        layer = self._keys.get(w.data_ptr()) if w is not None else None
        if layer is None:
            self.unmatched += 1
            return
        base = layer * len(ROLES)
        if role == "wgrad":
            views = [_view(a, 2) + (2,), _view(b, 2) + (2,)]
            slots = [base + 4, base + 5]
        else:
            wm = w.detach()
            wm = wm if wm.is_contiguous() else wm.contiguous()
            rest = wm.numel() // wm.shape[0]
            views = [_view(a, 1) + (1,), (wm, 1, wm.shape[0], rest, wm.numel(), 2 if forward_of_r else 1)]
            slots = [base, base + 1] if role == "fwd" else [base + 2, base + 3]
        _audit(views, slots, self._row, self._workspaces)

    @contextlib.contextmanager
    def iteration(self, iteration):
        from . import ops
        from ._lib import lib
        _layout_check(lib())
        self._keys = self.key_map()
        dev = self.layers[0][1].device
        if dev.type != "cuda":
            raise TypeError("FormatAudit computes on the GPU only; the networks are on %s" % dev)
        if self._ring is None:
            self._ring = torch.zeros(self.capacity, len(self.layers) * len(ROLES), SLOT_WORDS, dtype=torch.int64, device=dev)
        if len(self._pending) == self.capacity:
            self.flush()
        self._row = self._ring[len(self._pending)]
        self._row.zero_()
        before = ops.CONTRACTION_TAP
        ops.CONTRACTION_TAP = self._tap
        try:
            yield self
        finally:
            ops.CONTRACTION_TAP = before
            self._row = None
        self._pending.append(int(iteration))
        self.last_iteration = int(iteration)

    def flush(self):
        if not self._pending:
            return []
        torch.cuda.synchronize(self._ring.device)          # the side stream's calls too
        host = self._ring[:len(self._pending)].cpu().numpy()          # the one device-to-host copy
        rows = []
        for r, iteration in enumerate(self._pending):
            row = decode(host[r])
            row["iteration"] = iteration
            rows.append(row)
        self._pending = []
        self.rows += rows
        return rows

    def clear(self):
        """forget the rows read so far (the ring's unread rows stay)"""
        self.rows = []
        return self

    # ---- reading ------------------------------------------------------------------------------------------------------------------
    def report(self):
        self.flush()
        out = []
        entries = self.entries()
        for row in self.rows:
            finite = (row["n"] - row["nonfinite"]).astype(np.float64)[:, None]
            snr = np.where((row["calls"] == 0)[:, None], np.nan, snr_db(row["sumsq"], row["err_sumsq"]))
            rec = {"iteration": row["iteration"], "entries": entries, "formats": self.FORMAT_NAMES, "snr_db": snr, "hist": row["hist"]}
            with np.errstate(divide="ignore", invalid="ignore"):
                for key in ("flushed", "subnormal", "clamped"):
                    rec[key] = np.where(finite > 0, row[key].astype(np.float64) / finite, np.nan)
            out.append(rec)
        return out

    def save(self, folder, epoch):
        self.flush()
        entries = self.entries()
        e = len(entries)

        def stack(key, dtype, *tail):
            return np.array([row[key] for row in self.rows], dtype=dtype).reshape((len(self.rows), e) + tail)
        sumsq, err = stack("sumsq", np.float64), stack("err_sumsq", np.float64, FORMATS)
        calls = stack("calls", np.uint64)
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "%d-formats.npz" % epoch)
        with open(path + ".tmp", "wb") as f:
            np.savez(f, names=np.array([n for n, _ in entries], dtype=np.str_), roles=np.array([r for _, r in entries], dtype=np.str_),
                     formats=np.array(self.FORMAT_NAMES, dtype=np.str_), iterations=np.array([row["iteration"] for row in self.rows], dtype=np.int64),
                     n=stack("n", np.uint64), zeros=stack("zeros", np.uint64), nonfinite=stack("nonfinite", np.uint64), calls=calls,
                     sumsq=sumsq, absmax=stack("absmax", np.float32), hist=stack("hist", np.uint64, HIST), err_sumsq=err,
                     flushed=stack("flushed", np.uint64, FORMATS), subnormal=stack("subnormal", np.uint64, FORMATS),
                     clamped=stack("clamped", np.uint64, FORMATS),
                     snr_db=np.where((calls == 0)[..., None], np.nan, snr_db(sumsq, err)))
        os.replace(path + ".tmp", path)
        return [path]
