"""What the spill tests hold the product to (locate_amd/spill.py, csrc/digest.hip) and that is not the code under test: the
per-tensor digest in numpy and in Python integers, and a reader of the spill file format written from its description alone -
plain struct and json, nothing imported from the package."""
import json
import struct
import zlib

import numpy as np

MAGIC = b"LOCSPILL"
MASK64 = (1 << 64) - 1


def words(array):
    """any float32 / float64 / int32 / uint32 array -> its 4-byte words"""
    return np.ascontiguousarray(array).reshape(-1).view(np.uint32)


def digest(w, start=0):
    """(A, B) of uint32 words: A = sum w_i, B = sum ((i + 1) mod 2^32) w_i, modulo 2^64; `start`: the index of w[0] in its tensor"""
    w64 = words(w).astype(np.uint64)
    n = w64.size
    with np.errstate(over="ignore"):
        a = w64.sum(dtype=np.uint64)
        b = ((np.arange(start + 1, start + n + 1, dtype=np.uint64) & np.uint64(0xffffffff)) * w64).sum(dtype=np.uint64)
    return int(a), int(b)


def digest_python(w, start=0):
    """the same sums in Python's unbounded integers, reduced once at the end"""
    values = [int(v) for v in words(w)]
    a = sum(values)
    b = sum(((start + i + 1) % (1 << 32)) * v for i, v in enumerate(values))
    return a & MASK64, b & MASK64


def read_file(path):
    """(header, arena bytes, blob bytes) of a spill file, checked for its framing only: magic, header length, padding to 4096,
    slot_bytes of arena, blob_bytes of blob, nothing behind them"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == MAGIC
    (n,) = struct.unpack("<Q", data[8:16])
    header = json.loads(data[16:16 + n].decode("utf-8"))
    at = -(-(16 + n) // 4096) * 4096
    assert not any(data[16 + n:at])
    arena = data[at:at + header["slot_bytes"]]
    blob = data[at + header["slot_bytes"]:]
    assert len(arena) == header["slot_bytes"] and len(blob) == header["blob_bytes"]
    assert zlib.crc32(blob) & 0xffffffff == header["blob_crc32"]
    return header, arena, blob


def entry_words(header, arena, name):
    e = next(e for e in header["entries"] if e["name"] == name)
    return np.frombuffer(arena, dtype=np.uint32, count=e["n_words"], offset=e["offset"])
