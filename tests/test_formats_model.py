"""The numpy model of the format audit (tests/helpers/formats_model.py) against independent references: its quantiser against
torch's CPU casts (round to nearest even, checked here on planted ties of both parities) and against a brute-force search of the
e2m1 grid; and the fixture family the GPU test runs on, which has to exercise every counter of every format."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import formats_model as M  # noqa: E402

GRIDS = {name: (mbits, emin, top) for name, mbits, emin, top, _ in M.FORMATS}


def log_uniform_with_ties(mbits, emin, top):
    """200 000 float32 values: log-uniform magnitudes from well below the grid's smallest subnormal to above its maximum, mixed
    signs, +-0, and exact ties of both parities in the normals and the subnormals"""
    rng = np.random.default_rng(5)
    lo, hi = emin - mbits - 4, np.log2(top) + 1
    x = (rng.choice([-1.0, 1.0], size=200000) * 2.0 ** rng.uniform(max(lo, -148), min(hi, 127.9), size=200000)).astype(np.float32)
    ties = []
    for e in range(emin, min(emin + 12, int(np.log2(top)))):          # normals: (m + 0.5) steps, m even and odd
        step = 2.0 ** (e - mbits)
        ties += [(2 ** mbits + m + 0.5) * step for m in range(2 ** mbits)]
    sub = 2.0 ** (emin - mbits)
    if sub * 0.5 >= 2.0 ** -149:
        ties += [(m + 0.5) * sub for m in range(2 ** mbits)]          # subnormals, and the tie between 0 and the smallest
    ties = np.array(ties + [-t for t in ties] + [0.0, -0.0], dtype=np.float32)
    assert np.array_equal(ties.astype(np.float64)[:len(ties) // 2 - 1], np.array(ties[:len(ties) // 2 - 1], dtype=np.float64))
    x[:ties.size] = ties
    x[-2:] = np.finfo(np.float32).max, -np.finfo(np.float32).max          # past every grid's maximum, bf16's included
    return x


@pytest.mark.parametrize("name, dtype", [("e4m3_tensor", "float8_e4m3fn"), ("e5m2_tensor", "float8_e5m2"), ("bf16", "bfloat16")])
def test_quantiser_agrees_with_torch_casts(name, dtype):
    if not hasattr(torch, dtype):
        pytest.skip("this torch has no %s" % dtype)
    mbits, emin, top = GRIDS[name]
    x = log_uniform_with_ties(mbits, emin, top)
    q, clamped = M.quantise(x.astype(np.float64), mbits, emin, top)
    want = torch.from_numpy(x).to(getattr(torch, dtype)).to(torch.float32).numpy().astype(np.float64)
    keep = ~clamped
    assert keep.sum() > 150000 and clamped.any()
    assert np.array_equal(q[keep], want[keep])
    assert np.array_equal(np.signbit(q[keep]), np.signbit(want[keep]))
    assert (np.abs(q[clamped]) == top).all() and (np.abs(x[clamped].astype(np.float64)) > top).all()
    # the planted ties went to the even neighbour: torch's casts are round-to-nearest-even, and so is the model
    step = 2.0 ** (emin - mbits)
    tie = np.array([(2 ** mbits + 0.5) * step, (2 ** mbits + 1.5) * step])
    got, _ = M.quantise(tie, mbits, emin, top)
    assert np.array_equal(got, np.array([2 ** mbits * step, (2 ** mbits + 2) * step]))


def test_e2m1_against_brute_force():
    grid = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0])          # 8: where a value past 6 would round to, were it there
    even = np.array([True, False, True, False, True, False, True, False, True])          # parity of the mantissa
    rng = np.random.default_rng(6)
    a = np.concatenate([2.0 ** rng.uniform(-6, 3.2, size=20000), (grid[:-1] + grid[1:]) / 2, grid, [0.0, 6.9, 7.0, 7.1, 0.25, 0.24999]])
    mbits, emin, top = GRIDS["mxfp4_e2m1"]
    q, clamped = M.quantise(np.concatenate([a, -a]), mbits, emin, top)
    for i, v in enumerate(a):
        d = np.abs(grid - v)
        near = np.flatnonzero(d == d.min())
        pick = near[0] if near.size == 1 else [j for j in near if even[j]][0]
        want, over = (6.0, True) if grid[pick] > 6.0 else (grid[pick], False)
        assert (q[i], clamped[i]) == (want, over), (v, q[i], clamped[i])
        assert (q[a.size + i], clamped[a.size + i]) == (-want, over) and np.signbit(q[a.size + i])


def test_scale_rules():
    bits = lambda v: int(np.array([v], dtype=np.float32).view(np.uint32)[0])          # noqa: E731
    assert M.tensor_scale_exp(7, bits(448.0)) == -1 and M.tensor_scale_exp(7, bits(1.0)) == 7 and M.tensor_scale_exp(14, bits(1.0)) == 14
    assert M.tensor_scale_exp(7, 0) == 0 and M.tensor_scale_exp(7, bits(2.0 ** -140)) == 0 and M.tensor_scale_exp(7, 0x7F800000) == 0
    assert M.tensor_scale_exp(7, bits(2.0 ** -125)) == 126 and M.tensor_scale_exp(7, bits(M.FLT_MAX_NEAR)) == -120
    x = np.array([bits(1.0), bits(448.0), 0, bits(2.0 ** -140), bits(M.FLT_MAX_NEAR)], dtype=np.uint32)
    assert M.block_scale_exp(x, 8).tolist() == [-8, 0, -127, -127, 119] and M.block_scale_exp(x, 2).tolist() == [-2, 6, -127, -127, 125]


def test_fixture_family_exercises_every_counter():
    """what keeps the GPU test from being vacuous: over the family every counter of every format is non-zero somewhere - except
    `clamped` of the two per-tensor formats, which their scale rule makes impossible"""
    seen = {(f, key): 0 for f in range(len(M.FORMATS)) for key in ("flushed", "subnormal", "clamped")}
    base = {"zeros": 0, "nonfinite": 0, "last_bin": 0}
    for what, x in M.fixtures():
        for axis in (1, 2):
            rec = M.audit(x, axis)
            assert rec["n"] == x.size and sum(rec["hist"]) == rec["n"] - rec["zeros"] - rec["nonfinite"]
            base["zeros"] += rec["zeros"]
            base["nonfinite"] += rec["nonfinite"]
            base["last_bin"] += rec["hist"][-1]
            for f, fr in enumerate(rec["formats"]):
                for key in ("flushed", "subnormal", "clamped"):
                    seen[f, key] += fr[key]
                if "max" in what and x.size > 1 and f < 2:
                    assert fr["subnormal"] == 0, "beside FLT_MAX the per-tensor formats flush everything else"
    assert all(base.values()), base
    for (f, key), count in seen.items():
        if f < 2 and key == "clamped":
            assert count == 0, (M.NAMES[f], key)
        else:
            assert count > 0, (M.NAMES[f], key)


def test_block_axis_and_partial_blocks():
    """a [1, 33, 2] tensor by hand: along c there are two blocks per line, the second holding ONE element, which is then its own
    largest magnitude and survives mxfp4; along p every block has two members"""
    x = np.full((1, 33, 2), 2.0 ** -10, dtype=np.float32)
    x[0, 0, :] = 1.0
    a1, a2 = M.audit(x, 1), M.audit(x, 2)
    assert a1["formats"][3]["flushed"] == 2 * 31 and a2["formats"][3]["flushed"] == 0
    assert a1["absmax"] == a2["absmax"] == 0x3F800000 and a1["hist"][10] == a2["hist"][10] == 64
    assert a1["sumsq"] == a2["sumsq"] == 2.0 + 64 * 2.0 ** -20
