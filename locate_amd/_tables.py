"""Host side of the kernels driven by a device chunk table (csrc/multitensor.h): the Nadam step, the guard, the averaged
generator, the run statistics and dynamics, the snapshot, the digest and the gradient bucket copies.  Each packs its own records;
the (tensor, chunk) list, the staging, the bounded cache, the check of the arguments and the layout of an arena are here.
Importing this module does not load the HIP library."""
from collections import namedtuple

import torch

# records / chunks: device tensors; scratch: the device buffer that goes with the table (coefficients, a workspace) or None;
# host: the pinned buffers the copies came from
Table = namedtuple("Table", "records chunks n_tensors n_chunks scratch host")


def chunk_pairs(sizes, chunk):
    """([(tensor, chunk), ...] covering tensors of `sizes` elements in `chunk`-element pieces, a tensor's pieces consecutive and in
    order; [position of each tensor's first pair])"""
    pairs, first = [], []
    for i, n in enumerate(sizes):
        first.append(len(pairs))
        pairs.extend((i, c) for c in range((n + chunk - 1) // chunk))
    return pairs, first


def stage(records, pairs, n_tensors, device, scratch=None):
    """Packed records (bytes) and the pair list -> Table on `device`.  Pinned staging + async copies: legal inside a hipGraph
    capture (the memcpy nodes re-read the host buffers on every replay, so they are kept alive with the table)."""
    t_host = torch.frombuffer(bytearray(records), dtype=torch.uint8).clone().pin_memory()
    c_host = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).pin_memory()
    return Table(t_host.to(device, non_blocking=True), c_host.to(device, non_blocking=True), n_tensors, len(pairs), scratch,
                 (t_host, c_host))


def remember(cache, key, table, bound):
    """cache[key] = table, after emptying a cache (a plain dict) that holds more than `bound` tables.  Dropping a table frees its
    device arrays, which a graph that captured a launch with it still names: a captured launch's tensors must keep their addresses
    (one key, never evicted by itself)."""
    if len(cache) > bound:
        cache.clear()
    cache[key] = table
    return table


def require_device_tensors(tensors, what):
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise TypeError("%s computes on the GPU only; got %s" % (what, t.device if torch.is_tensor(t) else type(t).__name__))
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("%s takes contiguous float32 tensors, got %s%s" % (what, t.dtype, "" if t.is_contiguous() else " (strided)"))


def arena_layout(word_counts):
    """(byte offset of every tensor in a slot, slot_bytes) for tensors of `word_counts` 4-byte words: in order, every offset a
    multiple of 16, a zero-length tensor takes no space."""
    offsets, at = [], 0
    for n in word_counts:
        n = int(n)
        if n < 0:
            raise ValueError("a tensor of %d words" % n)
        offsets.append(at)
        at += (4 * n + 15) // 16 * 16
    return offsets, at

