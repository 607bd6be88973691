"""The float64 definition of the differentiable augmentation (tests/helpers/diffaug_model.py) checked against itself: the closed
colour form against the paper's three steps, the backward formula against torch autograd of the same definition, the adjoint
identity, the extreme rows, the static policy, and the derived error bounds against an fp32 emulation of the kernels' sequence."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import diffaug_model as M  # noqa: E402

SIZES = [32, 64]


def images(seed, n, S):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3, S, S))


def drawn_rows(seed, n, S, policy=M.FULL):
    return M.rows_from_uniform(np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 7)), S, policy)


def extreme_rows(S):
    """cut at each corner, shifts of +-D on both axes, an empty rectangle, s = 0 (grey), c = 0.5"""
    D, cut = M.shift_bound(S), M.cut_size(S)
    return np.stack([
        M.make_row(b=0.25, s=0.0, c=0.5, ty=D, tx=D, y0=0, y1=cut // 2, x0=0, x1=cut // 2),
        M.make_row(b=-0.5, s=2.0, c=1.5, ty=-D, tx=-D, y0=S - cut // 2, y1=S, x0=S - cut // 2, x1=S),
        M.make_row(b=0.1, s=0.7, c=0.5, ty=D, tx=-D, y0=0, y1=cut // 2, x0=S - cut // 2, x1=S),
        M.make_row(b=0.0, s=1.3, c=0.9, ty=-D, tx=D, y0=S - cut // 2, y1=S, x0=0, x1=cut // 2),
        M.make_row(b=0.3, s=0.4, c=1.2, ty=0, tx=0, y0=5, y1=5, x0=0, x1=0),
    ])


@pytest.mark.parametrize("S", SIZES)
def test_closed_colour_form_equals_the_papers_sequence(S):
    x = images(1, 6, S)
    rows = drawn_rows(2, 6, S)
    for xi, r in zip(x, rows):
        assert np.abs(M.colour(xi, r) - M.colour_sequential(xi, r)).max() <= 1e-12
    for r in extreme_rows(S):
        assert np.abs(M.colour(x[0], r) - M.colour_sequential(x[0], r)).max() <= 1e-12


def torch_forward(x, row):
    """the definition once more, in differentiable float64 torch ops"""
    b, s, c = (float(v) for v in row[:3])
    ty, tx, y0, y1, x0, x1 = (int(v) for v in row[3:9])
    S = x.shape[-1]
    mu = x.mean(dim=0, keepdim=True)
    z = c * (s * (x - mu) + mu - x.mean()) + x.mean() + b
    D = M.shift_bound(S)
    padded = torch.nn.functional.pad(z, (D, D, D, D))
    w = padded[:, D - ty:D - ty + S, D - tx:D - tx + S]
    keep = torch.ones(S, S, dtype=torch.float64)
    keep[y0:y1, x0:x1] = 0.0
    return keep[None] * w


@pytest.mark.parametrize("S", SIZES)
def test_backward_formula_equals_autograd_of_the_definition(S):
    rows = np.concatenate([drawn_rows(3, 4, S), extreme_rows(S)])
    x = images(4, len(rows), S)
    g = images(5, len(rows), S)
    for xi, gi, r in zip(x, g, rows):
        xt = torch.tensor(xi, requires_grad=True)
        y = torch_forward(xt, r)
        assert np.abs(y.detach().numpy() - M.forward_image(xi, r)).max() <= 1e-12
        y.backward(torch.tensor(gi))
        assert np.abs(xt.grad.numpy() - M.backward_image(gi, r)).max() <= 1e-12


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("policy", range(8))
def test_adjoint_identity(S, policy):
    """T is affine: <T(x) - T(0), g> == <x, T^T g>"""
    rows = np.concatenate([drawn_rows(6, 3, S, policy), extreme_rows(S)])
    x = images(7, len(rows), S)
    g = images(8, len(rows), S)
    lhs = ((M.forward(x, rows, policy).astype(np.float64) - M.forward(np.zeros_like(x), rows, policy)) * g).sum(axis=(1, 2, 3))
    rhs = (x * M.backward(g, rows, policy)).sum(axis=(1, 2, 3))
    scale = np.abs(x).sum(axis=(1, 2, 3))
    assert (np.abs(lhs - rhs) <= 1e-12 * scale).all(), np.abs(lhs - rhs).max()


def test_extreme_rows_are_handled():
    S = 32
    D, cut = M.shift_bound(S), M.cut_size(S)
    assert (D, cut) == (4, 16) and (M.shift_bound(64), M.cut_size(64)) == (8, 32)
    x = images(9, 1, S)[0]
    r = extreme_rows(S)[0]                                   # +D, +D; cut at the top-left corner
    y = M.forward_image(x, r)
    assert (y[:, :D, :] == 0).all() and (y[:, :, :D] == 0).all()          # the border
    assert (y[:, :cut // 2, :cut // 2] == 0).all()                        # the cut
    z = M.colour(x, r)
    assert np.array_equal(y[:, cut // 2:, cut // 2:], z[:, cut // 2 - D:S - D, cut // 2 - D:S - D])
    r = extreme_rows(S)[1]                                   # -D, -D; cut at the bottom-right corner
    y = M.forward_image(x, r)
    assert (y[:, S - D:, :] == 0).all() and (y[:, :, S - D:] == 0).all() and (y[:, S - cut // 2:, S - cut // 2:] == 0).all()
    assert np.array_equal(y[:, :S - cut // 2, :S - cut // 2], M.colour(x, r)[:, D:S - cut // 2 + D, D:S - cut // 2 + D])
    # an empty rectangle cuts nothing
    r = extreme_rows(S)[4]
    assert np.array_equal(M.forward_image(x, r), M.colour(x, r))


def test_without_colour_the_values_are_moved_not_computed():
    S = 32
    x = images(10, 2, S).astype(np.float32)
    x[0, 1, 3, 4] = np.float32(1e-40)                        # a subnormal and a negative zero travel as they are
    x[0, 2, 5, 6] = np.float32(-0.0)
    rows = extreme_rows(S)[:2]                               # their colour words are far from the identity
    for policy in (0, M.TRANSLATION, M.CUTOUT, M.TRANSLATION | M.CUTOUT):
        y = M.forward(x, rows, policy)
        assert y.dtype == np.float32
        g = M.backward(x, rows, policy)
        assert g.dtype == np.float32
        if policy == 0:
            assert np.array_equal(y.view(np.int32), x.view(np.int32)) and np.array_equal(g.view(np.int32), x.view(np.int32))
    D = M.shift_bound(S)
    y = M.forward(x, rows, M.TRANSLATION)
    assert np.array_equal(y[0, :, D:, D:].view(np.int32), x[0, :, :S - D, :S - D].view(np.int32))


def test_non_finite_values_survive_the_cut_and_stay_out_of_the_border():
    S = 32
    x = images(11, 1, S)[0].astype(np.float32)
    r = M.make_row(ty=4, tx=0, y0=8, y1=16, x0=8, x1=16)
    x[1, 6, 10] = np.nan                                     # lands at (10, 10): under the cut
    y = M.forward_image(x, r, M.TRANSLATION | M.CUTOUT)
    assert np.isnan(y[1, 10, 10]) and np.isnan(y).sum() == 1 and (y[:, :4, :] == 0).all()
    y = M.forward_image(x, r, M.FULL)
    assert np.isnan(y[:, 4:, :]).all() and (y[:, :4, :] == 0).all()


# ---- the bounds: an fp32 emulation of the kernels' sequence stays inside them, and they are tight enough to mean something ----------
def f32(v):
    return np.asarray(v, np.float32)


def emulate_forward(x, row):
    x = f32(x)
    b, s, c = (np.float32(v) for v in row[:3])
    M_ = np.float32(x.astype(np.float64).sum() / x.size)
    mu = f32(f32(f32(x[0] + x[1]) + x[2]) / np.float32(3))
    d = f32(x - mu[None])
    t = f32(s.astype(np.float64) * d.astype(np.float64) + mu[None].astype(np.float64))                    # fma: one rounding
    t2 = f32(t - M_)
    Mb = np.float32(M_ + b)
    z = f32(c.astype(np.float64) * t2.astype(np.float64) + np.float64(Mb))
    ty, tx, y0, y1, x0, x1 = (int(v) for v in row[3:9])
    return M.keep_mask(x.shape[-1], y0, y1, x0, x1, np.float32)[None] * M.translate(z, ty, tx)


def emulate_backward(gy, row):
    b, s, c = (np.float32(v) for v in row[:3])
    gz = M.gz_image(f32(gy), row)
    G = np.float32(gz.astype(np.float64).sum() / gz.size)
    cs, c1s, k = np.float32(c * s), np.float32(c * np.float32(np.float32(1) - s)), np.float32(np.float32(np.float32(1) - c) * G)
    m = f32(f32(f32(gz[0] + gz[1]) + gz[2]) / np.float32(3))
    r = f32(np.float64(c1s) * m.astype(np.float64) + np.float64(k))
    return f32(np.float64(cs) * gz.astype(np.float64) + r[None].astype(np.float64))


@pytest.mark.parametrize("S", SIZES)
def test_bounds_hold_for_an_fp32_emulation_and_are_of_the_size_of_a_few_roundings(S):
    rows = np.concatenate([drawn_rows(12, 4, S), extreme_rows(S)])
    x = images(13, len(rows), S).astype(np.float32)
    g = images(14, len(rows), S).astype(np.float32)
    for name, emulate, model, bound in (("forward", emulate_forward, M.forward, M.forward_bound),
                                        ("backward", emulate_backward, M.backward, M.backward_bound)):
        src = x if name == "forward" else g
        got = np.stack([emulate(v, r) for v, r in zip(src, rows)]).astype(np.float64)
        want, lim = model(src, rows), bound(src, rows)
        assert (np.abs(got - want) <= lim).all(), (name, float((np.abs(got - want) / np.maximum(lim, 1e-300)).max()))
        # the double-rounded fma of the emulation costs at most 2^-53 relative on top; the bound is a handful of fp32 roundings
        assert lim.max() < 64 * M.U32 * max(1.0, float(np.abs(want).max()))
    assert (M.forward_bound(x, rows, M.TRANSLATION | M.CUTOUT) == 0).all() and (M.backward_bound(g, rows, M.CUTOUT) == 0).all()
