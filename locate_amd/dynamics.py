"""Telling a healthy run from a stalled one: per optimizer step the update-to-weight ratio |dw| / |w| of every tensor of both
networks, and per spectrally normalised layer the sigma its forward divides by next to the layer's true top singular value.  The
reference has nothing of the kind; like the run statistics this is an addition BESIDE the training step: a separate object with a
kernel of its own (csrc/dynamics.hip through the C ABI, include/locate_hip.h) that is launched between two iterations.  It only
READS what the step left in device memory and writes buffers of its own, so the trajectory of a run that records is that of a
run that does not, bit for bit (tests/test_gpu_dynamics.py).

    recs = tensor_deltas([w0, w1], [b0, b1])           # ad hoc: five device tensors
    dyn = RunDynamics(gen, dis, capacity=256, sigma_rounds=4)
    dyn.mark()                                         # before an iteration: base <- weights, one pass, no host read
    ...one iteration...
    dyn.record(iteration)                              # after it: delta records + sigmas into a device ring row, no host read
    rows = dyn.flush()                                 # one device-to-host copy of everything since the last flush
    dyn.ratios();  dyn.save(folder, epoch);  dyn.clear()

The update is not the gradient - Nadam's warm-up schedule, its second moment and a clipping guard sit between the two - so it is
measured, not reconstructed: a copy of the weights taken before the iteration (`mark`) and ONE pass afterwards that subtracts
(`record`).  That is optimizer-agnostic and sees a guard's clip or skip as what it did to the weights.

Per entry (csrc/dynamics.hip), with d = w - base in fp32: `delta_sumsq` and `base_sumsq` are float64 sums of exact squares over the
finite d resp. the finite base elements (within n * 2^-52 relative of the exact sums, the same bits from call to call),
`delta_absmax` the largest finite |d|, `unchanged` the number of elements with w == base, `nonfinite` that of NaN / Inf deltas.

Importing this module does not load the HIP library.  A tensor on the CPU raises TypeError: there is no CPU path."""
import ctypes
import os
import struct

import numpy as np
import torch

from ._tables import arena_layout, chunk_pairs, require_device_tensors, stage

RECORD, REBASE = 1, 2          # the modes of locate_dyn_pass; 3 is both in one pass
WORDS = 4          # int64 words of a 32-byte record


def _device_table(live, bases):
    """The table (_tables.Table, the workspace as its `scratch`) of locate_dyn_pass for non-empty device tensors and their slots."""
    from ._lib import lib
    L = lib()
    assert L.locate_dyn_tensor_record_bytes() == 32 and L.locate_dyn_record_bytes() == 8 * WORDS
    pairs, first = chunk_pairs([t.numel() for t in live], L.locate_dyn_chunk_elems())
    rec = b"".join(struct.pack("<QQqi4x", t.data_ptr(), b.data_ptr(), t.numel(), at) for t, b, at in zip(live, bases, first))
    dev = live[0].device
    ws = torch.empty(max(L.locate_dyn_workspace_bytes(len(pairs)) // 8, WORDS), dtype=torch.int64, device=dev)
    return stage(rec, pairs, len(live), dev, scratch=ws)


def _launch(table, mode, records=None):
    """records: int64 [n_tensors, 4] device memory (a recording mode), or None (REBASE alone)"""
    from ._lib import check, lib
    t_dev, c_dev, n_t, n_c, ws = table[:5]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    recording = bool(mode & RECORD)
    check(lib().locate_dyn_pass(ptr(t_dev), ptr(c_dev), n_t, n_c, int(mode), ptr(records) if recording else None,
                                ptr(ws) if recording else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_dyn_pass")


def _decode(words):
    """int64 [n, 4] host records -> (delta_sumsq float64, base_sumsq float64, delta_absmax float32, unchanged uint32, nonfinite uint32)"""
    words = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, WORDS)
    third = np.ascontiguousarray(words[:, 2]).view(np.uint64)
    fourth = np.ascontiguousarray(words[:, 3]).view(np.uint64)
    low = np.uint64(0xFFFFFFFF)
    return (np.ascontiguousarray(words[:, 0]).view(np.float64).copy(), np.ascontiguousarray(words[:, 1]).view(np.float64).copy(),
            (third & low).astype(np.uint32).view(np.float32), (third >> np.uint64(32)).astype(np.uint32), (fourth & low).astype(np.uint32))


def tensor_deltas(tensors, bases):
    """(delta_sumsq float64 [k], base_sumsq float64 [k], delta_absmax float32 [k], unchanged int64 [k], nonfinite int64 [k]) of k
    contiguous float32 device tensors against k bases of the same sizes, as device tensors: one pass over their memory on
    `torch.cuda.current_stream()`, no host read; neither list is written.  A zero-element pair gives zeros."""
    tensors, bases = list(tensors), list(bases)
    if not tensors or len(tensors) != len(bases):
        raise ValueError("tensor_deltas needs as many bases as tensors, and at least one: got %d and %d" % (len(tensors), len(bases)))
    require_device_tensors(tensors + bases, "tensor_deltas")
    for t, b in zip(tensors, bases):
        if t.numel() != b.numel():
            raise ValueError("tensor_deltas: a tensor of %d elements against a base of %d" % (t.numel(), b.numel()))
    dev, k = tensors[0].device, len(tensors)
    live = [i for i, t in enumerate(tensors) if t.numel() > 0]
    row = torch.zeros(max(len(live), 1), WORDS, dtype=torch.int64, device=dev)
    if live:
        _launch(_device_table([tensors[i].detach() for i in live], [bases[i].detach() for i in live]), RECORD, row)
    row = row[:len(live)]
    out = (row[:, 0].contiguous().view(torch.float64), row[:, 1].contiguous().view(torch.float64),
           (row[:, 2] & 0xFFFFFFFF).to(torch.int32).view(torch.float32), (row[:, 2] >> 32) & 0xFFFFFFFF, row[:, 3] & 0xFFFFFFFF)
    if len(live) == k:
        return out
    at = torch.tensor(live, dtype=torch.int64).to(dev)
    return tuple(torch.zeros(k, dtype=o.dtype, device=dev).index_copy_(0, at, o) for o in out)


def _is_uv(name):
    return name.endswith(("weight_u", "weight_v"))


class RunDynamics:
    """What one iteration did to every parameter of `gen` and `dis`, and how tight every spectral normalisation is.

    Delta entries: every `named_parameters()` entry of the generator, then of the discriminator, as "G/<name>" and "D/<name>" -
    exactly `RunStatistics`' weight entries, so the two files join by name.  The spectral norm's u / v are included: their delta
    shows how far the power iteration's vectors turn per iteration.  Zero-element parameters are skipped.  `entry_names()`.

    mark() copies every entry into its slot of the base arena - one fp32 buffer allocated once, every slot on a 16-byte boundary -
    by one launch on `torch.cuda.current_stream()`.  record(iteration) writes, by one pass over weights and arena, one 32-byte
    record per entry into a row of a preallocated int64 device ring; record(iteration, rebase=True) also starts the next window in
    the same pass (the records describe the displacement since the last base).  record() before any mark() raises ValueError.
    Neither allocates nor reads on the host; the iteration number stays on the host.  A full ring flushes first.  The device
    tables are cached on ALL the addresses they hold and rebuilt when one changes; the arena keeps its contents.

    Sigma entries (`sigma_rounds` > 0; 0 turns the part off): every `SpectralNorm` module of the generator, then of the
    discriminator, in `modules()` order, named after its `weight_bar` parameter.  `layer_names()`.  ONE `SnLayer` table over both
    networks points at the live `weight_bar`s; u, v, sigma and all scratch are buffers of this object, advanced by
    `locate_sn_power_iter_batched` - the live u / v / sigma are never written.  Two sets of shadow vectors:
      train  at every record u / v are copied from the live ones (a REBASE pass of the delta kernel over the u / v tensors), then
             the layers' `power_iterations` rounds run: `sigma_train` is what a forward entered now would divide by;
      top    persistent: initialised from the live u / v at the first record (and after reset_sigma()), `sigma_rounds` rounds per
             record.  The weights move little between two records, so it follows the top singular pair and converges ACROSS
             records: `sigma_top` approaches the layer's largest singular value.
    One power iteration's sigma is a lower bound of the top singular value, so the normalised layer's Lipschitz constant is
    sigma_1 / sigma_train >= 1; `ratios()` reports sigma_top / sigma_train as "lipschitz".  Until the top set has converged -
    the first records of a run - sigma_top is itself a lower bound and can sit below a sigma_train whose live vectors have had
    more rounds.

    A ring row holds the delta records followed by [layers, 2] float32 (sigma_train, sigma_top): flush() reads the rows recorded
    since the last flush back in ONE device-to-host copy and returns them; every row is a dict {"iteration", "names" (tuple),
    "delta_sumsq" float64 [n], "base_sumsq" float64 [n], "delta_absmax" float32 [n], "unchanged" uint32 [n], "nonfinite" uint32 [n],
    "layers" (tuple), "sigma_train" float32 [l], "sigma_top" float32 [l]}.  All rows since construction (or clear()) stay in `rows`.

    ratios(): per row {"iteration", "update": sqrt(delta_sumsq / base_sumsq) per entry (NaN where the base is 0), "lipschitz":
    sigma_top / sigma_train per layer, "G/update", "D/update": the same update ratio per network over its entries other than
    u / v}, float64 on the host.

    save(folder, epoch) writes `folder/{epoch}-dynamics.npz` (to a .tmp, then renamed): `names` [entries], `layers` [layers],
    `iterations` [records], the five record fields [records, entries], `sigma_train` and `sigma_top` [records, layers], and of
    ratios() `update` [records, entries], `lipschitz` [records, layers], `G_update` and `D_update` [records].

    An iteration that does not step a network's optimizer (miniter > 1) shows `unchanged == n` for its weights.  Under data
    parallelism the weights are equal on every rank: only rank 0 needs one."""

    def __init__(self, gen, dis, capacity=256, sigma_rounds=4):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %r" % (capacity,))
        if int(sigma_rounds) < 0:
            raise ValueError("sigma_rounds must be >= 0, got %r" % (sigma_rounds,))
        self.nets = (("G", gen), ("D", dis))
        self.capacity, self.sigma_rounds = int(capacity), int(sigma_rounds)
        self.rows = []
        self.last_iteration = None          # that of the latest record, read or not
        self._params = None
        self._layers = None
        self._names, self._layer_names = (), ()
        self._key = None
        self._marked = False
        self._top_live = False          # the top set holds vectors of its own
        self._ring = None
        self._pending = []          # iterations of the rows the ring holds
        self._arena = self._slots = None
        self._tab = None
        self._sn = None

    # ---- entries ------------------------------------------------------------------------------------------------------------------
    def _parameters(self):
        """[(entry name, parameter)] of both networks, listed once: the set of parameters does not change during a run"""
        if self._params is None:
            self._params = [("%s/%s" % (tag, name), p) for tag, net in self.nets for name, p in net.named_parameters() if p.numel() > 0]
        return self._params

    def _sn_layers(self):
        """[(layer name, wrapped module)] of every SpectralNorm of both networks; nothing when sigma_rounds is 0"""
        if self._layers is None:
            from .nn import SpectralNorm
            self._layers = []
            for tag, net in self.nets if self.sigma_rounds else ():
                name_of = {id(p): name for name, p in net.named_parameters()}
                for sn in net.modules():
                    if isinstance(sn, SpectralNorm):
                        bar = getattr(sn.module, sn.name + "_bar")
                        self._layers.append(("%s/%s" % (tag, name_of[id(bar)]), sn))
        return self._layers

    def entry_names(self):
        return [name for name, _ in self._parameters()]

    def layer_names(self):
        return [name for name, _ in self._sn_layers()]

    # ---- device side ----------------------------------------------------------------------------------------------------------------
    def _prepare(self):
        params = self._parameters()
        if not params:
            raise ValueError("RunDynamics: the networks have no parameters")
        key = [p.data_ptr() for _, p in params]
        if key == self._key:
            return
        tensors = [p.detach() for _, p in params]
        require_device_tensors(tensors, "RunDynamics")
        dev = tensors[0].device
        layers = self._sn_layers()
        if self._arena is None:
            offsets, nbytes = arena_layout([t.numel() for t in tensors])          # every slot starts on a 16-byte boundary
            self._arena = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
            assert self._arena.data_ptr() % 16 == 0
            self._slots = [self._arena[o // 4:o // 4 + t.numel()] for o, t in zip(offsets, tensors)]
            self._ring = torch.zeros(self.capacity, WORDS * len(tensors) + len(layers), dtype=torch.int64, device=dev)
            self._names, self._layer_names = tuple(n for n, _ in params), tuple(n for n, _ in layers)
        self._tab = _device_table(tensors, self._slots)
        if layers:
            self._build_sigma(layers, dev)
        self._key = key

    def _build_sigma(self, layers, dev):
        """The shadow buffers (once) and, for the addresses as they are now, the u / v copy tables and the SnLayer table: records
        [0, n) are the train set, [n, 2n) the top set; both read the live weight_bar and share the scratch (they run in turn)."""
        from ._lib import lib
        rounds = {int(sn.power_iterations) for _, sn in layers}
        if len(rounds) > 1:
            raise NotImplementedError("RunDynamics advances all layers together: one power_iterations value for both networks")
        n = len(layers)
        geometry = []
        for _, sn in layers:
            w = getattr(sn.module, sn.name + "_bar")
            h = w.shape[0]
            geometry.append((h, w.numel() // h, (h + 63) // 64))
        if self._sn is None or "shadow" not in self._sn:
            sizes = {}
            for s in range(2):          # train, top
                for i, (h, wd, nch) in enumerate(geometry):
                    sizes.update({(s, i, "u"): h, (s, i, "v"): wd, (s, i, "wv"): h})
            for i, (h, wd, nch) in enumerate(geometry):
                sizes.update({(i, "t"): wd, (i, "s"): h, (i, "tpart"): nch * wd})
            offsets, nbytes = arena_layout(sizes.values())
            at = {key: o // 4 for key, o in zip(sizes, offsets)}
            self._sn = {"shadow": torch.zeros(nbytes // 4, dtype=torch.float32, device=dev), "at": at,
                        "sigma": torch.zeros(2, n, 2, dtype=torch.float32, device=dev)}          # [set, layer, {sigma, 1 / sigma}]
        sn_state = self._sn
        shadow, at, sigma = sn_state["shadow"], sn_state["at"], sn_state["sigma"]
        assert lib().locate_sn_table_record_bytes() == 80
        base = shadow.data_ptr()
        buf = bytearray()
        copies = ([], []), ([], [])          # per set: (live u / v tensors, their shadow slots)
        for s in range(2):
            for i, ((_, sn), (h, wd, nch)) in enumerate(zip(layers, geometry)):
                m = sn.module
                w, u, v = (getattr(m, sn.name + suffix).detach() for suffix in ("_bar", "_u", "_v"))
                if u.numel() != h or v.numel() != wd:
                    raise ValueError("RunDynamics: u / v of %s do not fit its weight" % self._layer_names[i])
                buf += struct.pack("<8Q4i", w.data_ptr(), base + 4 * at[s, i, "u"], base + 4 * at[s, i, "v"], sigma[s, i].data_ptr(),
                                   base + 4 * at[s, i, "wv"], base + 4 * at[i, "t"], base + 4 * at[i, "s"], base + 4 * at[i, "tpart"], h, wd, nch, 0)
                copies[s][0].extend((u, v))
                copies[s][1].extend((shadow[at[s, i, "u"]:at[s, i, "u"] + h], shadow[at[s, i, "v"]:at[s, i, "v"] + wd]))
        host = torch.frombuffer(buf, dtype=torch.uint8).clone().pin_memory()
        sn_state.update(table=host.to(dev, non_blocking=True), host=host, n=n, rounds=rounds.pop(),
                        max_h=max(h for h, _, _ in geometry), max_wd=max(wd for _, wd, _ in geometry),
                        copy_train=_device_table(*copies[0]), copy_top=_device_table(*copies[1]))

    def _power_iterations(self, which, rounds):
        from ._lib import check, lib
        s = self._sn
        for _ in range(rounds):
            check(lib().locate_sn_power_iter_batched(ctypes.c_void_p(s["table"].data_ptr() + 80 * s["n"] * which), s["n"], s["max_h"], s["max_wd"],
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_sn_power_iter_batched")

    def _sigmas(self, row):
        """both sets' power iterations on the weights as they are now; (sigma_train, sigma_top) per layer into the row's tail"""
        s = self._sn
        _launch(s["copy_train"], REBASE)          # train u / v <- live u / v
        if not self._top_live:
            _launch(s["copy_top"], REBASE)
            self._top_live = True
        self._power_iterations(0, s["rounds"])
        self._power_iterations(1, self.sigma_rounds)
        row[WORDS * len(self._names):].view(torch.float32).view(s["n"], 2).copy_(s["sigma"][:, :, 0].t())          # [layers, 2] float32

    def mark(self):
        """base <- weights: the window that the next record() closes starts here"""
        self._prepare()
        _launch(self._tab, REBASE)
        self._marked = True
        return self

    def reset_sigma(self):
        """the next record starts the top set again from the live u / v"""
        self._top_live = False
        return self

    def record(self, iteration, rebase=False):
        if not self._marked:
            raise ValueError("RunDynamics.record() before any mark(): there is no base to measure from")
        self._prepare()
        if len(self._pending) == self.capacity:
            self.flush()
        row = self._ring[len(self._pending)]
        _launch(self._tab, RECORD | REBASE if rebase else RECORD, row)
        if self._layer_names:
            self._sigmas(row)
        self._pending.append(int(iteration))
        self.last_iteration = int(iteration)
        return self

    def flush(self):
        if not self._pending:
            return []
        host = self._ring[:len(self._pending)].cpu().numpy()          # the one device-to-host copy
        e, n = len(self._names), len(self._layer_names)
        rows = []
        for r, iteration in enumerate(self._pending):
            delta_sumsq, base_sumsq, delta_absmax, unchanged, nonfinite = _decode(host[r, :WORDS * e])
            sigma = np.ascontiguousarray(host[r, WORDS * e:]).view(np.float32).reshape(n, 2)
            rows.append({"iteration": iteration, "names": self._names, "delta_sumsq": delta_sumsq, "base_sumsq": base_sumsq,
                         "delta_absmax": delta_absmax, "unchanged": unchanged, "nonfinite": nonfinite, "layers": self._layer_names,
                         "sigma_train": sigma[:, 0].copy(), "sigma_top": sigma[:, 1].copy()})
        self._pending = []
        self.rows += rows
        return rows

    def clear(self):
        """forget the rows read so far (the ring's unread rows stay)"""
        self.rows = []
        return self

    # ---- reading ------------------------------------------------------------------------------------------------------------------
    def ratios(self):
        self.flush()
        out = []
        for row in self.rows:
            d, b = np.asarray(row["delta_sumsq"], np.float64), np.asarray(row["base_sumsq"], np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rec = {"iteration": row["iteration"], "update": np.where(b > 0, np.sqrt(d / b), np.nan),
                       "lipschitz": np.asarray(row["sigma_top"], np.float64) / np.asarray(row["sigma_train"], np.float64)}
            for tag in ("G", "D"):
                own = np.array([name.startswith(tag + "/") and not _is_uv(name) for name in row["names"]], dtype=bool)
                total = float(b[own].sum())
                rec[tag + "/update"] = float(np.sqrt(d[own].sum() / total)) if total > 0 else float("nan")
            out.append(rec)
        return out

    def save(self, folder, epoch):
        ratios = self.ratios()          # flushes
        names = list(self.rows[0]["names"]) if self.rows else list(self._names or self.entry_names())
        layers = list(self.rows[0]["layers"]) if self.rows else list(self._layer_names or self.layer_names())
        for row in self.rows:
            if list(row["names"]) != names or list(row["layers"]) != layers:
                raise ValueError("RunDynamics.save: the rows do not describe the same entries")

        def stack(rows, key, dtype, width):
            return np.array([r[key] for r in rows], dtype=dtype).reshape(len(rows), width)
        e, n = len(names), len(layers)
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, "%d-dynamics.npz" % epoch)
        with open(path + ".tmp", "wb") as f:
            np.savez(f, names=np.array(names, dtype=np.str_), layers=np.array(layers, dtype=np.str_),
                     iterations=np.array([row["iteration"] for row in self.rows], dtype=np.int64),
                     delta_sumsq=stack(self.rows, "delta_sumsq", np.float64, e), base_sumsq=stack(self.rows, "base_sumsq", np.float64, e),
                     delta_absmax=stack(self.rows, "delta_absmax", np.float32, e), unchanged=stack(self.rows, "unchanged", np.uint32, e),
                     nonfinite=stack(self.rows, "nonfinite", np.uint32, e), sigma_train=stack(self.rows, "sigma_train", np.float32, n),
                     sigma_top=stack(self.rows, "sigma_top", np.float32, n), update=stack(ratios, "update", np.float64, e),
                     lipschitz=stack(ratios, "lipschitz", np.float64, n),
                     G_update=np.array([r["G/update"] for r in ratios], dtype=np.float64),
                     D_update=np.array([r["D/update"] for r in ratios], dtype=np.float64))
        os.replace(path + ".tmp", path)
        return [path]
