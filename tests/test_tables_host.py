"""The host side of the chunk tables (locate_amd/_tables.py) without a GPU: the (tensor, chunk) list, the bounded cache, and an
import that loads no library."""
import subprocess
import sys

from conftest import ROOT


def test_pairs_and_first_positions():
    from locate_amd._tables import chunk_pairs
    pairs, first = chunk_pairs([1, 4096, 4097, 3], 4096)
    assert pairs == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)]          # 1 + 1 + 2 + 1
    assert first == [0, 1, 2, 4]
    assert chunk_pairs([], 4096) == ([], [])
    assert chunk_pairs([0, 5], 4) == ([(1, 0), (1, 1)], [0, 0])          # an empty tensor has no pair


def test_importing_the_module_loads_no_library():
    code = ("import sys, locate_amd._tables, locate_amd._lib as L\n"
            "assert L._lib is None, 'the HIP library was loaded'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'liblocate_hip' not in maps, 'the HIP library is mapped'\n"
            "print('clean')\n")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]


def test_the_cache_clears_at_its_bound():
    from locate_amd._tables import remember
    cache = {}
    for k in range(9):
        assert remember(cache, k, "table %d" % k, 8) == "table %d" % k
    assert sorted(cache) == list(range(9))          # 9 entries: "more than 8" is not reached before the tenth
    remember(cache, 9, "table 9", 8)
    assert cache == {9: "table 9"} and type(cache) is dict
    remember(cache, 10, "table 10", 0)          # bound 0: one table at a time
    assert cache == {10: "table 10"}
