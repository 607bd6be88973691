"""Records tests/golden/p02_reduction_bits.npz: the raw record words of the statistics, of the dynamics in modes 1 and 3 and of one
guarded step's verdict on the case of tests/helpers/reduction_bits.py.  Run it on the commit whose order of additions is to be
pinned (profiles/notes_multitensor.md names the one the committed file is from).
Usage (GPU box): python tools/record_reduction_bits.py [--out tests/golden/p02_reduction_bits.npz]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import reduction_bits as RB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "p02_reduction_bits.npz"))
    args = ap.parse_args()
    from locate_amd._lib import require_gpu
    require_gpu()
    got = RB.run(torch.device("cuda:0"))
    again = RB.run(torch.device("cuda:0"))
    assert all(np.array_equal(got[key], again[key]) for key in got), "two runs of the same case differ"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **got)
    print("wrote %s: %d entries, %d bytes" % (args.out, len(got), os.path.getsize(args.out)))
    for key in RB.KEYS:
        print(key, got[key].shape, " ".join("%016x" % (int(v) & 0xFFFFFFFFFFFFFFFF) for v in got[key].reshape(-1)[:8]))


if __name__ == "__main__":
    main()
