"""Records tests/golden/p01_nadam_bits.npz: the bits of three `Nadam` steps on the case of tests/helpers/nadam_bits.py, per weight
decay: every tensor of the last step in full, a SHA-256 per tensor of the steps before it, and the untouched words around them.
Run it on the commit whose arithmetic is to be pinned (profiles/notes_multitensor.md names the one the committed file is from).
Usage (GPU box): python tools/record_nadam_bits.py [--out tests/golden/p01_nadam_bits.npz]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nadam_bits as NB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "p01_nadam_bits.npz"))
    args = ap.parse_args()
    from locate_amd._lib import require_gpu
    require_gpu()
    rec = {}
    for k, wd in enumerate(NB.WEIGHT_DECAYS):
        got = NB.run(wd, torch.device("cuda:0"))
        again = NB.run(wd, torch.device("cuda:0"))
        assert all(NB.sha(got[key]) == NB.sha(again[key]) for key in got), "two runs of the same steps differ"
        for key, a in got.items():
            if key.startswith("step") and not key.startswith("step%d/" % NB.STEPS):
                rec["wd%d/%s/sha256" % (k, key)] = np.array(NB.sha(a))
            else:
                rec["wd%d/%s" % (k, key)] = a
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **rec)
    print("wrote %s: %d entries, %d bytes" % (args.out, len(rec), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
