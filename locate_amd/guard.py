"""Guarding the optimizer step: `GuardedNadam` is `Nadam` behind a verdict that is taken on the device, at every step, from the
gradients the step is about to consume (csrc/guard.hip through the C ABI, include/locate_hip.h):

  * skip: with `skip_nonfinite` (the default) a step whose gradients hold a NaN or an Inf anywhere - in any parameter group - is
    not taken: every weight, moment and schedule state keeps its bits, and one bad batch costs one optimizer step;
  * clip: with `max_norm > 0` the gradients are scaled by `max_norm / norm` when their global L2 norm (over every gradient of the
    optimizer, accumulated in float64 from exact squares) exceeds `max_norm`.  The scale is computed in double and rounded once to
    fp32; every gradient element is multiplied by it in one fp32 multiplication of its own inside the update kernel, `.grad` itself
    is never written, and weight decay is added after the scaling.  torch.nn.utils.clip_grad_norm_ divides by `norm + 1e-6`
    instead and clamps the result to 1: THIS DIFFERS - here a clipped gradient has the norm `max_norm` up to rounding, and a norm
    at or below `max_norm` gives a scale of exactly 1.

The reference has nothing of the kind.  Like the averaged generator and the run statistics this is opt-in and a separate object
with kernels of its own: `Nadam` (optim.py, csrc/nadam.hip) stays the default.  Both steps instantiate one spelled-out update
(csrc/nadam_step.h), so a guard that has nothing to do (finite gradients, no limit or a norm below it) is `Nadam` bit for bit
(tests/test_gpu_guard.py).

The verdict needs no host read, so the step can be captured in a hipGraph together with the backward pass (`GraphedTrainStep`);
the decision is taken anew at every replay.  What the guard did is kept in running counters on the device: `counters()` reads
them in one small device-to-host copy.  The run statistics (stats.py) read `.grad`, so their records show the UNCLIPPED gradient.
Under data parallelism the gradients are equal on every rank after the exchange, so every rank reaches the same verdict without
communication.

Importing this module does not load the HIP library."""
import ctypes
import math
import struct

import torch

from ._tables import chunk_pairs, remember, stage
from .optim import Nadam

COUNTER_KEYS = ("steps", "skipped", "clipped", "consecutive_skips", "last_norm", "last_scale", "last_nonfinite")


class GuardExhausted(RuntimeError):
    """`GuardedNadam` has skipped `consecutive_skips` steps in a row: the gradients are non-finite whatever the batch - usually
    because a weight is - and every further step would be skipped too.  `iteration`: the trainer's iteration count when it was
    noticed; `network`: "G" or "D"."""

    def __init__(self, iteration, network, consecutive_skips=0):
        self.iteration, self.network, self.consecutive_skips = int(iteration), str(network), int(consecutive_skips)
        super().__init__("the guarded optimizer of %s has skipped %d steps in a row at iteration %d: its gradients are non-finite "
                         "whatever the batch" % (self.network, self.consecutive_skips, self.iteration))


def _decode_verdict(raw):
    """the 64-byte device record (csrc/guard.hip, GuardVerdict) -> the counters() dictionary"""
    norm, nonfinite, scale, _skip, steps, skipped, clipped, consecutive, _sumsq = struct.unpack("<dQfi4qd", raw)
    return {"steps": steps, "skipped": skipped, "clipped": clipped, "consecutive_skips": consecutive, "last_norm": norm,
            "last_scale": scale, "last_nonfinite": nonfinite}


def _encode_verdict(c):
    norm = float(c.get("last_norm", 0.0))
    return struct.pack("<dQfi4qd", norm, int(c.get("last_nonfinite", 0)), float(c.get("last_scale", 0.0)), 0, int(c["steps"]),
                       int(c["skipped"]), int(c["clipped"]), int(c["consecutive_skips"]), norm * norm)


class GuardedNadam(Nadam):
    """Nadam(params, lr, betas, eps, weight_decay, schedule_decay) plus `max_norm` (0: no clipping) and `skip_nonfinite`.  Both are
    attributes of the optimizer, not of a parameter group: the norm and the verdict are those of ALL gradients of the optimizer.
    They are not part of `state_dict()`, whose layout is `Nadam`'s: either class loads the other's.

    step(): one pass over every gradient and a one-block launch take the verdict, then the guarded schedule / update pair runs per
    parameter group; version counters and largest-magnitude words are stamped as after `Nadam.step()`, skipped or not.

    counters(): {"steps": verdicts taken, "skipped", "clipped", "consecutive_skips": skipped steps since the last one taken,
    "last_norm": the unclipped global gradient norm of the latest step (finite elements only), "last_scale", "last_nonfinite"}.
    counters_state() / load_counters_state() carry them through a checkpoint."""

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, schedule_decay=4e-3, max_norm=0.0,
                 skip_nonfinite=True):
        max_norm = float(max_norm)
        if not (math.isfinite(max_norm) and max_norm >= 0.0):
            raise ValueError("max_norm must be finite and >= 0 (0: no clipping), got %r" % (max_norm,))
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, schedule_decay=schedule_decay)
        self.max_norm, self.skip_nonfinite = max_norm, bool(skip_nonfinite)
        self._guard_tables = {}
        self._verdict = None          # int64 [8] on the device: the 64-byte record, zero until the first step
        self._pending_counters = None

    def _restore_invariants(self):
        super()._restore_invariants()
        self._guard_tables = {}

    # ---- the device record ------------------------------------------------------------------------------------------------------
    def _record(self, device):
        fresh = self._verdict is None or self._verdict.device != device
        if (fresh or self._pending_counters is not None) and device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # a captured zero fill would reset the counters at every replay, and the copy of restored counters comes from
            # pageable memory: both belong in front of the capture
            raise RuntimeError("GuardedNadam: the counter record must exist before a stream capture - take one step eagerly (or call "
                               "_table()) first, as GraphedTrainStep's warm-up does")
        if fresh:
            from ._lib import lib
            assert lib().locate_guard_verdict_bytes() == 64
            self._verdict = torch.zeros(8, dtype=torch.int64, device=device)
        if self._pending_counters is not None:          # written in place: a captured graph holds the record's address
            self._verdict.copy_(torch.frombuffer(bytearray(_encode_verdict(self._pending_counters)), dtype=torch.int64))
            self._pending_counters = None
        return self._verdict

    def counters(self):
        if self._verdict is None:
            c = dict(self._pending_counters or {})
            return {k: c.get(k, 0.0 if k in ("last_norm", "last_scale") else 0) for k in COUNTER_KEYS}
        return _decode_verdict(self._verdict.cpu().numpy().tobytes())          # the one device-to-host copy

    def counters_state(self):
        return self.counters()

    def load_counters_state(self, state):
        missing = [k for k in COUNTER_KEYS[:4] if k not in state]
        if missing:
            raise KeyError("guard counters without %s" % ", ".join(missing))
        self._pending_counters = {k: state[k] for k in COUNTER_KEYS if k in state}
        if self._verdict is not None:
            self._record(self._verdict.device)
        return self

    # ---- tables -----------------------------------------------------------------------------------------------------------------
    def _with_gradients(self):
        return [p for group in self.param_groups for p in group["params"] if p.grad is not None]

    def _guard_table(self, plist):
        """Device table over the gradients of ALL parameter groups, cached on the addresses it holds."""
        key = tuple((p.grad.data_ptr(), p.numel()) for p in plist)
        tab = self._guard_tables.get(key)
        if tab is not None:
            return tab
        from ._lib import lib
        L = lib()
        assert L.locate_guard_tensor_record_bytes() == 16
        rec = b"".join(struct.pack("<Qq", p.grad.data_ptr(), p.numel()) for p in plist)
        pairs, _ = chunk_pairs([p.numel() for p in plist], L.locate_guard_chunk_elems())
        dev = plist[0].device
        ws = torch.empty(max(L.locate_guard_workspace_bytes(len(pairs)) // 8, 2), dtype=torch.int64, device=dev)
        # bounded like Nadam._tables: eagerly every backward may bring new gradient addresses
        return remember(self._guard_tables, key, stage(rec, pairs, len(plist), dev, scratch=ws), 8)

    def _table(self, plist):
        """Nadam's tables for one parameter group - and the guard's, over every gradient the optimizer has now
        (`GraphedTrainStep._prime` calls this for the gradient buffers the captured backward allocated)."""
        tab = super()._table(plist)
        every = self._with_gradients()
        if every:
            self._guard_table(every)
            self._record(every[0].device)
        return tab

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        groups = self._groups_with_gradients()
        if not groups:
            return loss
        from ._lib import check, lib
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
        g = self._guard_table([p for _, plist in groups for p in plist])
        verdict = self._record(groups[0][1][0].device)
        reduce_args = (ptr(g.records), ptr(g.chunks), g.n_tensors, g.n_chunks, ptr(g.scratch))
        for group, plist in groups:
            tab = Nadam._table(self, plist)
            b1, b2 = group["betas"]
            check(lib().locate_guarded_nadam_step(*reduce_args, ptr(verdict), self.max_norm, int(self.skip_nonfinite), ptr(tab.records),
                                                  ptr(tab.scratch), ptr(tab.chunks), tab.n_tensors, tab.n_chunks, float(group["lr"]),
                                                  float(b1), float(b2), float(group["eps"]), float(group["schedule_decay"]),
                                                  float(group["weight_decay"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "locate_guarded_nadam_step")
            reduce_args = (None, None, 0, 0, None)          # the later groups of this step apply the same verdict
            self._stamp(plist)
        return loss
