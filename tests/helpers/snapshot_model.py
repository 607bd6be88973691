"""A numpy model of the snapshot kernels (locate_amd/csrc/snapshot.hip) over uint32 views: the arena, the classification of a word,
take with its commit decision, and restore.  Written from include/locate_hip.h, not from the kernel: the tests hold both the
kernel and locate_amd.snapshot to it."""
import numpy as np

NO_TENSOR = 0x7fffffff


def words(array):
    """any float32 / float64 / int32 / uint32 array -> its 4-byte words"""
    return np.ascontiguousarray(array).reshape(-1).view(np.uint32)


def layout(word_counts):
    """(byte offsets, slot bytes): in order, every tensor padded to 16 bytes"""
    offsets, at = [], 0
    for n in word_counts:
        offsets.append(at)
        at += -(-4 * int(n) // 16) * 16
    return offsets, at


def nonfinite(w, kind):
    """how many of the uint32 words `w` are non-finite for their kind: 0 never; 1 an fp32 whose exponent field is all ones; 2 the
    HIGH word (odd index, little endian) of an fp64 whose exponent field is all ones"""
    w = np.asarray(w, dtype=np.uint32)
    if kind == 0:
        return 0
    if kind == 1:
        return int(np.count_nonzero((w & np.uint32(0x7f800000)) == np.uint32(0x7f800000)))
    assert kind == 2 and w.size % 2 == 0
    high = w[1::2]
    return int(np.count_nonzero((high & np.uint32(0x7ff00000)) == np.uint32(0x7ff00000)))


def fill_words(fill):
    fill = [int(x) for x in fill]
    return np.array(fill * (4 // len(fill)), dtype=np.uint32)


class Model:
    """entries: [(n_words, kind, fill)].  `live` everywhere: a list of uint32 arrays, None for a tensor that does not exist."""

    def __init__(self, entries):
        self.entries = [(int(n), int(kind), fill_words(fill)) for n, kind, fill in entries]
        self.offsets, self.slot_bytes = layout([n for n, _, _ in self.entries])
        self.slots = [np.zeros(self.slot_bytes // 4, dtype=np.uint32) for _ in range(2)]
        self.record = {"good": -1, "iteration": 0, "taken": 0, "rejected": 0, "last_rejected_iteration": 0, "last_rejected_count": 0,
                       "last_rejected_tensor": -1}

    def destination(self):
        return 1 if self.record["good"] == 0 else 0

    def take(self, live, iteration):
        dest = self.slots[self.destination()]
        count, first = 0, NO_TENSOR
        for i, ((n, kind, fill), off, t) in enumerate(zip(self.entries, self.offsets, live)):
            if n == 0:
                continue
            if t is None:
                dest[off // 4:off // 4 + n] = np.resize(fill, n)          # the fill is written, never judged
                continue
            t = words(t)
            assert t.size == n
            dest[off // 4:off // 4 + n] = t
            bad = nonfinite(t, kind)
            if bad:
                count, first = count + bad, min(first, i)
        r = self.record
        if count == 0:
            r["good"], r["iteration"], r["taken"] = self.destination(), int(iteration), r["taken"] + 1
        else:
            r["rejected"] += 1
            r["last_rejected_iteration"], r["last_rejected_count"], r["last_rejected_tensor"] = int(iteration), count, first
        return count == 0

    def restore(self, live):
        """-> (the good slot's iteration, what the live tensors hold afterwards); None when nothing is committed"""
        if self.record["good"] < 0:
            return None
        src = self.slots[self.record["good"]]
        out = []
        for (n, _, _), off, t in zip(self.entries, self.offsets, live):
            out.append(None if t is None else src[off // 4:off // 4 + n].copy())
        return self.record["iteration"], out

    def status(self, names):
        r = dict(self.record)
        r["last_rejected_tensor"] = names[r["last_rejected_tensor"]] if r["last_rejected_tensor"] >= 0 else None
        return r


# bit patterns every test covers: (fp32 word, finite?)
SPECIAL_F32 = [(0x7f800000, False), (0xff800000, False),          # +-Inf
               (0x7fc00000, False), (0xffc00001, False), (0x7fc12345, False),          # quiet NaNs, payloads
               (0x7f800001, False), (0xffa00000, False), (0x7fbfffff, False),          # signalling NaNs
               (0x7f7fffff, True), (0xff7fffff, True),          # the largest finite values
               (0x00000001, True), (0x807fffff, True),          # denormals
               (0x80000000, True), (0x00000000, True)]          # -0.0, +0.0
# (fp64 as (low word, high word), finite?)
SPECIAL_F64 = [((0x00000000, 0x7ff00000), False), ((0x00000000, 0xfff00000), False),          # +-Inf
               ((0x00000001, 0x7ff80000), False), ((0xdeadbeef, 0xfff7ffff), False),          # quiet, signalling NaN
               ((0xffffffff, 0x7fefffff), True),          # the largest finite value
               ((0x00000001, 0x00000000), True), ((0xffffffff, 0x800fffff), True),          # denormals
               ((0x00000000, 0x80000000), True),          # -0.0
               ((0x7fc00000, 0x3ff00000), True), ((0x7f800000, 0x40000000), True)]          # the LOW word alone looks like an fp32 NaN / Inf
