"""The order of every addition in the multi-tensor reductions, held to recorded bits: the raw record words of the statistics, of
the dynamics in modes 1 and 3 and of a guarded step's verdict on the case of tests/helpers/reduction_bits.py against
tests/golden/p02_reduction_bits.npz - this project's own output, recorded by tools/record_reduction_bits.py before the chunk
readers and the block total moved into csrc/multitensor.h (profiles/notes_multitensor.md names the commit)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import reduction_bits as RB  # noqa: E402

pytestmark = pytest.mark.gpu


def test_reductions_keep_their_recorded_bits():
    """Every entry of the fixture, word for word: float64 sums, maxima, counts, the verdict's norm and scale.  Equality of bits."""
    z = load_golden("p02_reduction_bits")
    got = RB.run(torch.device("cuda:0"))
    torch.cuda.empty_cache()
    compared = set()
    for key in z.files:
        want, have = z[key], got[key]
        assert want.dtype == np.int64 and have.dtype == np.int64 and want.shape == have.shape, (key, want.shape, have.shape)
        differ = np.flatnonzero(want.reshape(-1) != have.reshape(-1))
        assert differ.size == 0, "%s: %d of %d words differ, the first at %d: recorded %016x, now %016x" % (
            key, differ.size, want.size, differ[0], int(want.reshape(-1)[differ[0]]) & (2 ** 64 - 1),
            int(have.reshape(-1)[differ[0]]) & (2 ** 64 - 1))
        compared.add(key)
    assert compared == set(z.files) == set(RB.KEYS), (sorted(compared), sorted(z.files))
