"""The host side of the differentiable augmentation (locate_amd/augment.py) without a GPU: the draws' ranges and distributions'
end points, their reproducibility from a seed and through state_dict(), the policy parser, and the command line's flag."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import diffaug_model as M  # noqa: E402

from locate_amd import DiffAugment, draw_parameters  # noqa: E402
from locate_amd.augment import PARAM_FLOATS, parse_policy, policy_name  # noqa: E402

FULL = "color,translation,cutout"


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("S", [32, 64, 128, 256])
def test_draw_ranges_over_ten_thousand_rows(S):
    rows = draw_parameters(10000, S, gen(1), FULL)
    assert rows.shape == (10000, PARAM_FLOATS) and rows.dtype == np.float32
    b, s, c, ty, tx, y0, y1, x0, x1 = rows[:, :9].T
    assert (rows[:, 9:] == 0).all()
    assert (b >= -0.5).all() and (b <= 0.5).all() and (s >= 0).all() and (s <= 2).all() and (c >= 0.5).all() and (c <= 1.5).all()
    assert b.min() < -0.49 and b.max() > 0.49 and s.min() < 0.01 and s.max() > 1.99 and c.min() < 0.51 and c.max() > 1.49
    D, cut = M.shift_bound(S), M.cut_size(S)
    assert (D, cut) == (S // 8, S // 2)
    for t in (ty, tx):
        assert (t == np.rint(t)).all() and set(np.unique(t)) == set(range(-D, D + 1))          # every shift, both ends included
    for lo, hi in ((y0, y1), (x0, x1)):
        assert (lo == np.rint(lo)).all() and (hi == np.rint(hi)).all()
        assert (lo >= 0).all() and (hi <= S).all() and (lo <= hi).all() and (hi - lo <= cut).all()
        assert (hi - lo).min() == cut - cut // 2 and (hi - lo).max() == cut          # clipped at a corner, whole in the middle
        assert lo.min() == 0 and hi.max() == S
    # the same numbers as the float64 definition makes of the same uniform draw
    r = torch.rand(10000, 7, generator=gen(1), dtype=torch.float64).numpy()
    assert np.array_equal(rows, M.rows_from_uniform(r, S))


def test_the_random_stream_does_not_depend_on_the_policy():
    full = draw_parameters(64, 64, gen(2), FULL)
    ident = M.identity_row()
    for policy, cols in (("color", [0, 1, 2]), ("translation", [3, 4]), ("cutout", [5, 6, 7, 8]), ("cutout,color", [0, 1, 2, 5, 6, 7, 8])):
        g = gen(2)
        rows = draw_parameters(64, 64, g, policy)
        other = [k for k in range(PARAM_FLOATS) if k not in cols]
        assert np.array_equal(rows[:, cols], full[:, cols])
        assert (rows[:, other] == ident[other]).all()          # an op that is off holds its identity
        g_full = gen(2)
        draw_parameters(64, 64, g_full, FULL)
        assert torch.equal(g.get_state(), g_full.get_state())


def test_policy_parsing():
    assert parse_policy(FULL) == 7 and parse_policy("cutout, color") == 5 and parse_policy("") == 0 and parse_policy(6) == 6
    assert parse_policy(["translation"]) == 2
    assert policy_name(5) == "color,cutout" and policy_name(0) == ""
    for bad in ("colour", "color,flip", "color;cutout", 8, -1):
        with pytest.raises(ValueError):
            parse_policy(bad)
    with pytest.raises(ValueError):
        DiffAugment(S=64, batch=8, policy="")
    with pytest.raises(ValueError):
        DiffAugment(S=48, batch=8)
    with pytest.raises(ValueError):
        draw_parameters(4, 64, gen(0), "color,rotate")


def test_draws_reproduce_from_a_seed_and_state_dict_round_trips():
    a = DiffAugment(S=64, batch=4, policy=FULL, seed=5, device="cuda:0")          # construction touches no device
    b = DiffAugment(S=64, batch=4, policy=FULL, seed=5, device="cuda:0")
    c = DiffAugment(S=64, batch=4, policy=FULL, seed=6, device="cuda:0")
    draw = lambda aug: draw_parameters(16, 64, aug.generator, aug.bits)          # noqa: E731  (what draw() uploads)
    first = draw(a)
    assert np.array_equal(first, draw(b)) and not np.array_equal(first, draw(c))
    assert not np.array_equal(first, draw(a))          # the stream moves on
    state = a.state_dict()
    assert state["policy"] == FULL and state["S"] == 64 and state["batch"] == 4
    want = [draw(a) for _ in range(3)]
    fresh = DiffAugment(S=64, batch=4, policy=FULL, seed=77, device="cuda:0")
    fresh.load_state_dict(state)
    assert all(np.array_equal(w, draw(fresh)) for w in want)
    # through torch.save with weights_only, as trainer.torch and the spill's host blob carry it
    import io
    buf = io.BytesIO()
    torch.save({"augment": state}, buf)
    buf.seek(0)
    again = DiffAugment(S=64, batch=4, policy=FULL, seed=78, device="cuda:0")
    again.load_state_dict(torch.load(buf, map_location="cpu", weights_only=True)["augment"])
    assert np.array_equal(want[0], draw(again))
    for other in (DiffAugment(S=32, batch=4, policy=FULL), DiffAugment(S=64, batch=8, policy=FULL), DiffAugment(S=64, batch=4, policy="color")):
        with pytest.raises(ValueError):
            other.load_state_dict(state)


def test_no_cpu_path():
    from locate_amd import diff_augment
    with pytest.raises(TypeError):
        diff_augment(torch.zeros(2, 3, 32, 32), torch.zeros(2, 12))
    aug = DiffAugment(S=32, batch=2, policy=FULL)
    with pytest.raises(ValueError):
        aug.d_batch(torch.zeros(5, 3, 32, 32))
    with pytest.raises(RuntimeError):
        aug._rows(0, 2)          # nothing drawn yet


def test_command_line_flag_is_parsed_and_off_by_default():
    from locate_amd.run import parser
    base = ["--store", "s.npy", "--image-size", "64", "--batch", "8", "--out", "o"]
    assert parser().parse_args(base).diffaugment == ""
    assert parser().parse_args(base + ["--diffaugment", "color,cutout"]).diffaugment == "color,cutout"


def test_step_and_loop_take_an_augment_and_default_to_none():
    import inspect
    from locate_amd import TrainStep
    assert inspect.signature(TrainStep.__init__).parameters["augment"].default is None
