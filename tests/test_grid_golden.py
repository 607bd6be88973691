"""The sample grid's arithmetic on the CPU: the numpy model (tests/helpers/grid_model.py) against what the reference's chain
itself produced - make_grid's steps in torch CPU ops and the bytes of matplotlib's imsave (tests/golden/g23_sample_grid.npz,
written by tools/gen_grid_golden.py).  Equality, not a tolerance: the device kernel is held to the same values
(tests/test_gpu_monitor.py)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_model as M  # noqa: E402

NAMES = ["tanh13", "randn16", "tiny5", "const4", "nrow5", "range6"]


def case(z, name):
    nrow, padding = (int(v) for v in z["args_" + name])
    vr = tuple(float(v) for v in z["range_" + name]) or None
    return z["x_" + name], nrow, padding, vr


def test_fixture_covers_what_it_should():
    z = load_golden("g23_sample_grid")
    assert list(z["names"]) == NAMES and str(z["matplotlib_version"])
    x, nrow, padding, vr = case(z, "tanh13")
    assert x.shape == (13, 3, 32, 32) and padding == 8 and 13 % min(nrow, 13)           # ragged last row
    assert z["rgba_tanh13"].shape == (2 * 40 + 8, 8 * 40 + 8, 4)
    assert case(z, "randn16")[2] == 2 and z["x_randn16"].shape == (16, 3, 32, 32)
    assert 0 < np.abs(z["x_tiny5"]).max() < 1e-6
    assert z["x_const4"].min() == z["x_const4"].max() and not z["rgba_const4"][:, :, :3].any()
    assert case(z, "nrow5")[1] == 5
    x, _, _, vr = case(z, "range6")
    assert vr == (-1.0, 1.0) and x.min() < -1 and x.max() > 1
    for name in NAMES:
        assert (z["rgba_" + name][:, :, 3] == 255).all(), name


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_recorded_chain(name):
    z = load_golden("g23_sample_grid")
    x, nrow, padding, vr = case(z, name)
    grid, rgba = M.model(x, nrow, padding, vr)
    _, _, GH, GW = M.geometry(x.shape[0], x.shape[2], nrow, padding)
    assert rgba.shape == (GH, GW, 4) and grid.shape == (3, GH, GW)
    assert np.array_equal(rgba, z["rgba_" + name])
    if "grid_" + name in z.files:
        assert np.array_equal(grid, z["grid_" + name])
    assert 0.0 <= grid.min() and grid.max() <= 1.0
