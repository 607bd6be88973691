"""The input pipeline's arithmetic on the CPU: the numpy integer model (tests/helpers/input_model.py) against what Pillow itself
computed (tests/golden/g22_input_pipeline.npz, written by tools/gen_input_golden.py), and the product's host-side tables against
the same model.  Equality, not a tolerance: the device kernels are then held to the same bytes (tests/test_gpu_input.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import input_model as M  # noqa: E402


def fixture_records(z):
    """(set name, record number, source image, S, flip, order, factors, top, left, side, Pillow's output)"""
    for name in ("large", "small"):
        src = z["src_" + name]
        for i in range(len(z["rec_%s_source" % name])):
            top, left, side = (int(v) for v in z["rec_%s_crop" % name][i])
            yield (name, i, src[z["rec_%s_source" % name][i]], int(z["rec_%s_size" % name][i]), int(z["rec_%s_flip" % name][i]),
                   [int(o) for o in z["rec_%s_order" % name][i]], z["rec_%s_factors" % name][i], top, left, side, z["out_" + name][i])


def test_fixture_covers_what_it_should():
    z = load_golden("g22_input_pipeline")
    recs = list(fixture_records(z))
    assert len(recs) >= 24 and str(z["pillow_version"])
    assert z["src_large"].shape[1:] == (157, 128, 3) and z["src_small"].shape[1:] == (78, 64, 3)
    assert {r[5].index(M.CONTRAST) for r in recs if M.CONTRAST in r[5]} == {0, 1, 2, 3}
    assert {r[4] for r in recs} == {0, 1}
    large = [r for r in recs if r[0] == "large"]
    assert {128, 64} <= {r[9] for r in large} and any(64 < r[9] < 128 for r in large)
    assert any(r[7] == 0 and r[8] == 0 for r in large) and any(r[7] + r[9] == 157 and r[8] + r[9] == 128 for r in large)
    assert any(all(o == M.HUE for o in r[5]) for r in recs)
    f = np.concatenate([r[6] for r in recs])
    assert f.min() == 0.8 and f.max() == 1.2


def test_integer_model_reproduces_pillow():
    z = load_golden("g22_input_pipeline")
    for name, i, src, S, flip, order, factors, top, left, side, want in fixture_records(z):
        got = M.transform_u8(src, S, flip, order, factors, top, left, side)
        assert got.shape == want.shape and np.array_equal(got, want), (name, i, int((got != want).sum()))


def test_pillow_regenerates_the_fixture():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_input_golden
    z = load_golden("g22_input_pipeline")
    out = gen_input_golden.generate()
    for k in out:
        if k != "pillow_version":
            assert np.array_equal(out[k], z[k]), k


def test_product_tables_match_the_model():
    from locate_amd import data
    for side_lo, side_hi, S in ((32, 64, 32), (123, 128, 64), (64, 64, 64), (250, 256, 128)):
        table, ktaps = data.resize_table(side_lo, side_hi, S)
        assert table.shape == (side_hi - side_lo + 1, S, 2 + ktaps) and table.dtype == np.int32
        for a, side in enumerate(range(side_lo, side_hi + 1)):
            for i, (x0, k) in enumerate(M.resize_coeffs(side, S)):
                assert table[a, i, 0] == x0 and table[a, i, 1] == len(k)
                assert np.array_equal(table[a, i, 2:2 + len(k)], k) and not table[a, i, 2 + len(k):].any()
    lut = data.output_lut()
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    assert torch.equal(lut, torch.from_numpy(M.to_float(u8))[0, 0])
    assert data.pack_order([1, 0, 2, 3]) == 0x3201 and data.pack_order([]) == data.PLAIN_ORDER


def test_data_module_is_lazy():
    """importing locate_amd.data loads neither the HIP library nor Pillow (checked in a fresh interpreter)"""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import locate_amd.data, locate_amd._lib as L; "
            "assert L._lib is None; assert 'PIL' not in sys.modules; print('lazy')" % ROOT)
    assert "lazy" in subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
