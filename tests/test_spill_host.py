"""The spill's host side (locate_amd/spill.py, the hooks in locate_amd/run.py) without a GPU and without the HIP library: the
digest's numpy model against Python's integers, the file format against a reader written from its description alone
(tests/helpers/spill_model.py), everything `read_spill` has to refuse, `SnapshotSpill.latest`, and what the constructors and the
command line refuse."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spill_model as PM  # noqa: E402


def test_importing_the_module_loads_no_library():
    code = ("import locate_amd.spill, locate_amd._lib as L\n"
            "from locate_amd import SnapshotSpill, SpillCorrupt, digest_model, read_spill, write_spill, restore_training_state, tensor_digests\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "assert 'liblocate_hip' not in open('/proc/self/maps').read(), 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


# ---- the digest ---------------------------------------------------------------------------------------------------------------------
def test_digest_model_against_python_integers():
    from locate_amd import digest_model
    rng = np.random.default_rng(41)
    w = rng.integers(0, 1 << 32, size=5000, dtype=np.uint64).astype(np.uint32)
    w[:4] = 0xffffffff          # the largest words first: the sums pass 2^64 only with the index factor, the model must still wrap
    want = PM.digest_python(w)
    assert digest_model(w) == want == PM.digest(w)
    assert want[0] == sum(int(v) for v in w) and want[1] < 1 << 64
    assert digest_model(w.view(np.float32)) == want and digest_model(w.view(np.int32)) == want          # any 4-byte dtype, by its bits
    assert digest_model(np.zeros(0, np.uint32)) == (0, 0) == PM.digest_python(np.zeros(0, np.uint32))
    # (i + 1) passes 2^32 inside the array: the factor wraps to 0, 1, ... - in the mask, not in the 64-bit sum
    start = (1 << 32) - 100
    w = rng.integers(0, 1 << 32, size=200, dtype=np.uint64).astype(np.uint32)
    want = PM.digest_python(w, start)
    assert digest_model(w, start=start) == want == PM.digest(w, start)
    unmasked = sum((start + i + 1) * int(v) for i, v in enumerate(w)) & PM.MASK64
    assert want[1] != unmasked
    # the digests of a tensor's pieces add up to the tensor's
    a0, b0 = digest_model(w[:77])
    a1, b1 = digest_model(w[77:], start=77)
    assert ((a0 + a1) & PM.MASK64, (b0 + b1) & PM.MASK64) == digest_model(w)
    # and B wraps past 2^64 exactly like Python's integers reduced at the end: 2^12 words of 2^32 - 1 with factors near 2^31
    big = np.full(1 << 12, 0xffffffff, np.uint32)
    assert digest_model(big, start=1 << 31) == PM.digest_python(big, 1 << 31)
    assert sum(((1 << 31) + i + 1) * 0xffffffff for i in range(big.size)) >= 1 << 64
    with pytest.raises(TypeError):
        digest_model(np.zeros(4, np.float64))


# ---- the file -----------------------------------------------------------------------------------------------------------------------
ENTRIES = [("w", 5, 1, "float32", [5]), ("empty", 0, 1, "float32", [0]), ("sched", 4, 2, "float64", [2]), ("later", 7, 1, "float32", [7]),
           ("raw", 3, 0, "int32", [3])]
HOST = {"iterations": 12, "names": ["a", "b"], "t": torch.arange(6, dtype=torch.float64).reshape(2, 3), "flag": True, "x": 0.25}


def small_spill(path, iteration=12, seed=0):
    """a small arena with a zero-length entry, an fp64 pair and an entry that did not exist (the arena holds its fill)"""
    from locate_amd import arena_layout, digest_model, write_spill
    from locate_amd.spill import _serialise
    rng = np.random.default_rng(seed)
    offsets, slot_bytes = arena_layout([n for _, n, _, _, _ in ENTRIES])
    arena = np.zeros(slot_bytes // 4, np.uint32)
    contents = {"w": PM.words(rng.standard_normal(5).astype(np.float32)), "empty": np.zeros(0, np.uint32),
                "sched": PM.words(np.array([float(iteration), 0.996 ** iteration])), "later": np.array([0x3fc00000, 0xbf800000] * 4, np.uint32)[:7],
                "raw": np.array([0x7fc00000, 0xff800000, 0x80000000], np.uint32)}
    entries = []
    for (name, n, kind, dtype, shape), off in zip(ENTRIES, offsets):
        arena[off // 4:off // 4 + n] = contents[name]
        a, b = digest_model(contents[name])
        entries.append({"name": name, "offset": off, "n_words": n, "kind": kind, "dtype": dtype, "shape": shape, "existed": name != "later",
                        "digest": [a, b]})
    blob = _serialise(dict(HOST, iterations=iteration))
    write_spill(str(path), {"iteration": iteration, "slot_bytes": slot_bytes, "entries": entries}, arena.view(np.uint8), blob)
    return contents, arena, blob, offsets


def test_round_trip_and_the_independent_reader(tmp_path):
    from locate_amd import read_spill
    path = tmp_path / "spill-0.bin"
    contents, arena, blob, offsets = small_spill(path)
    assert not os.path.exists(str(path) + ".tmp")
    header, arrays, host = found = read_spill(str(path))
    assert found.path == str(path) and found.skipped == ()
    assert header["iteration"] == 12 and header["slot_bytes"] == arena.nbytes and header["version"] == 1
    assert [e["name"] for e in header["entries"]] == [e[0] for e in ENTRIES] and [e["offset"] for e in header["entries"]] == offsets
    assert [e["existed"] for e in header["entries"]] == [True, True, True, False, True]
    for name, n, kind, dtype, shape in ENTRIES:
        assert arrays[name].dtype == np.dtype(dtype) and list(arrays[name].shape) == shape
        assert np.array_equal(PM.words(arrays[name]), contents[name]), name
    assert arrays["sched"].tolist() == [12.0, 0.996 ** 12] and arrays["later"].tolist() == [1.5, -1.0] * 3 + [1.5]
    assert host["iterations"] == 12 and host["names"] == ["a", "b"] and host["flag"] is True and host["x"] == 0.25
    assert torch.equal(host["t"], HOST["t"])
    # the reader that shares no code with the product agrees byte for byte
    h2, arena2, blob2 = PM.read_file(str(path))
    assert h2 == header and arena2 == arena.tobytes() and blob2 == blob
    for e in h2["entries"]:
        assert list(PM.digest(PM.entry_words(h2, arena2, e["name"]))) == e["digest"], e["name"]
    assert os.path.getsize(str(path)) == 4096 + arena.nbytes + len(blob)
    from locate_amd import write_spill
    with pytest.raises(ValueError):
        write_spill(str(tmp_path / "x.bin"), {"iteration": 1, "slot_bytes": 64, "entries": []}, b"\0" * 48, b"")


def damaged(path, change):
    with open(str(path), "rb") as f:
        data = bytearray(f.read())
    data = change(data)
    with open(str(path), "wb") as f:
        f.write(bytes(data))


def flip(at):
    def change(data):
        data[at] ^= 0x10
        return data
    return change


def swap_words(a, b):
    def change(data):
        assert data[a:a + 4] != data[b:b + 4]
        data[a:a + 4], data[b:b + 4] = data[b:b + 4], data[a:a + 4]
        return data
    return change


def header_offset_past_the_arena(data):
    import json
    import struct
    (n,) = struct.unpack("<Q", data[8:16])
    header = json.loads(bytes(data[16:16 + n]).decode())
    header["entries"][0]["offset"] = header["slot_bytes"] - 8          # 5 words from there end 12 bytes past the arena
    text = json.dumps(header).encode()
    front = bytes(data[:8]) + struct.pack("<Q", len(text)) + text
    assert len(front) <= 4096
    return bytearray(front + b"\0" * (4096 - len(front))) + data[4096:]


DAMAGE = {"a flipped arena byte": flip(4096 + 2), "a flipped byte of the fill": flip(4096 + 48 + 5),
          "two swapped unequal arena words": swap_words(4096, 4096 + 8),
          "a flipped blob byte": flip(-40), "truncated in the header": lambda d: d[:12], "truncated in the arena": lambda d: d[:4096 + 20],
          "truncated in the blob": lambda d: d[:-1], "a bad magic": flip(3), "a header offset past the arena": header_offset_past_the_arena,
          "an appended byte": lambda d: d + b"\0", "bad JSON": flip(16), "an empty file": lambda d: d[:0]}


@pytest.mark.parametrize("what", list(DAMAGE))
def test_a_damaged_file_is_refused(tmp_path, what):
    from locate_amd import SpillCorrupt, read_spill
    path = tmp_path / "spill-0.bin"
    small_spill(path)
    read_spill(str(path))
    damaged(path, DAMAGE[what])
    with pytest.raises(SpillCorrupt) as info:
        read_spill(str(path))
    assert info.value.path == str(path) and info.value.what


def test_latest(tmp_path):
    from locate_amd import SnapshotSpill
    assert SnapshotSpill.latest(str(tmp_path)) is None          # an empty folder
    assert SnapshotSpill.latest(str(tmp_path / "nowhere")) is None
    small_spill(tmp_path / "spill-0.bin", iteration=40, seed=1)
    small_spill(tmp_path / "spill-1.bin", iteration=24, seed=2)
    shutil.copy(str(tmp_path / "spill-0.bin"), str(tmp_path / "spill-0.bin.tmp"))          # a leftover of a writer that died
    damaged(tmp_path / "spill-0.bin.tmp", lambda d: d[:5000])
    found = SnapshotSpill.latest(str(tmp_path))
    assert found.header["iteration"] == 40 and found.host_state["iterations"] == 40 and found.skipped == ()
    assert found.path == str(tmp_path / "spill-0.bin")
    damaged(tmp_path / "spill-0.bin", flip(4096 + 1))          # the newer one corrupt: the older one, and the skipped file named
    found = SnapshotSpill.latest(str(tmp_path))
    assert found.header["iteration"] == 24 and found.skipped == (str(tmp_path / "spill-0.bin"),)
    damaged(tmp_path / "spill-1.bin", lambda d: d[:-3])
    assert SnapshotSpill.latest(str(tmp_path)) is None


# ---- what the trainer and the command line refuse ---------------------------------------------------------------------------------------
def test_trainer_needs_a_snapshot_to_spill(tmp_path):
    from locate_amd import Trainer
    net = torch.nn.Linear(2, 2)
    step = types.SimpleNamespace(gen=net, dis=net, gen_opt=object(), dis_opt=object(), minibatches=1)
    pipeline = types.SimpleNamespace(batch=16, batches_per_epoch=100)
    with pytest.raises(ValueError, match="snapshot"):
        Trainer(step, pipeline, str(tmp_path / "out"), spill_every=4)
    with pytest.raises(ValueError, match="spill_every"):
        Trainer(step, pipeline, str(tmp_path / "out"), spill_every=-1)
    t = Trainer(step, pipeline, str(tmp_path / "out"))          # the default: no spill, no folder
    assert t.spill is None and t.spill_every == 0 and not os.path.exists(str(tmp_path / "out"))


def test_command_line(monkeypatch, capsys):
    from locate_amd import _lib, run

    class Reached(Exception):
        pass

    def no_gpu():
        raise Reached()
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = ["--store", "S.npy", "--image-size", "32", "--batch", "8", "--out", "OUT"]
    for extra in ([], ["--spill-every", "0"], ["--spill-every", "256", "--rollback-every", "64", "--stats-every", "16"]):
        with pytest.raises(Reached):          # parsed; the next thing main() does is to ask for the GPU
            run.main(base + extra)
    for extra in (["--spill-every", "4"], ["--spill-every", "4", "--stats-every", "1"], ["--spill-every", "-1", "--rollback-every", "2", "--stats-every", "1"],
                  ["--spill-every"]):
        with pytest.raises(SystemExit) as info:
            run.main(base + extra)
        assert info.value.code != 0
    assert "--rollback-every" in capsys.readouterr().err
    done = subprocess.run([sys.executable, "-m", "locate_amd.run"] + base + ["--spill-every", "4"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode != 0 and "--spill-every needs --rollback-every" in done.stderr
    with pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--spill-every N" in capsys.readouterr().out
