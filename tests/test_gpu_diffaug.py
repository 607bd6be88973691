"""The differentiable augmentation's two kernels on the MI355X (csrc/diffaug.hip) against the float64 definition
(tests/helpers/diffaug_model.py), at the smallest shapes that reach every path:

    S = 32, n = 5 (an odd n) | S = 64, n = 3 (the largest one-launch size) | S = 128, n = 2 | S = 256, n = 2 (two launches)

Inputs are uniform in [-1, 1]; the rows are hand-made (zero shift; +D and -D on both axes; the rectangle at each corner; an empty
rectangle; s = 0; c = 0.5; an odd shift with an odd rectangle) plus three drawn ones, fed to the kernels n at a time.
Worst observed shares of the derived bounds: profiles/notes_diffaug.md."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import diffaug_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(32, 5), (64, 3), (128, 2), (256, 2)]
NO_COLOUR = [0, M.TRANSLATION, M.CUTOUT, M.TRANSLATION | M.CUTOUT]
WITH_COLOUR = [M.COLOR, M.COLOR | M.TRANSLATION, M.COLOR | M.CUTOUT, M.FULL]
SENTINEL = 0x7FC0DEAD


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def hand_rows(S):
    D, cut = M.shift_bound(S), M.cut_size(S)
    h = cut // 2
    rows = [
        M.make_row(b=0.25, s=0.0, c=0.5, ty=0, tx=0, y0=0, y1=0, x0=0, x1=0),                       # zero shift, empty rectangle, grey
        M.make_row(b=-0.5, s=2.0, c=1.5, ty=D, tx=D, y0=0, y1=h, x0=0, x1=h),                       # +D, +D; top-left corner
        M.make_row(b=0.1, s=0.7, c=0.5, ty=-D, tx=-D, y0=S - h, y1=S, x0=S - h, x1=S),              # -D, -D; bottom-right corner
        M.make_row(b=0.0, s=1.3, c=0.9, ty=D, tx=-D, y0=0, y1=h, x0=S - h, x1=S),                   # top-right
        M.make_row(b=0.3, s=0.4, c=1.2, ty=-D, tx=D, y0=S - h, y1=S, x0=0, x1=h),                   # bottom-left
        M.make_row(b=-0.2, s=1.9, c=0.6, ty=1, tx=-3, y0=5, y1=5 + cut, x0=3, x1=3 + cut),          # odd shift, odd whole rectangle
        M.make_row(b=0.45, s=0.05, c=1.45, ty=-2, tx=1, y0=7, y1=7, x0=2, x1=9),                    # empty in y only
    ]
    drawn = M.rows_from_uniform(np.random.default_rng(100 + S).uniform(0.0, 1.0, size=(3, 7)), S)
    return np.concatenate([np.stack(rows), drawn])


_CASES = {}


def cases(S, n):
    """(x, g, rows) for every row, image k being image k % n of the n distinct ones; made once per size"""
    if S not in _CASES:
        rows = hand_rows(S)
        rng = np.random.default_rng(S)
        x = rng.uniform(-1.0, 1.0, size=(n, 3, S, S)).astype(np.float32)
        g = rng.uniform(-1.0, 1.0, size=(n, 3, S, S)).astype(np.float32)
        idx = np.arange(len(rows)) % n
        _CASES[S] = (x[idx], g[idx], rows)
    return _CASES[S]


_WANT = {}


def want(S, n, policy):
    """the float64 definition's (y, gx, forward bound, backward bound), computed once per (size, policy) and not changed afterwards"""
    if (S, policy) not in _WANT:
        x, g, rows = cases(S, n)
        out = (M.forward(x, rows, policy), M.backward(g, rows, policy), M.forward_bound(x, rows, policy), M.backward_bound(g, rows, policy))
        for a in out:
            a.setflags(write=False)
        _WANT[(S, policy)] = out
    return _WANT[(S, policy)]


def run(src, rows, policy, backward=False, n=None):
    """the kernel over src [K, 3, S, S], n images a call"""
    from locate_amd import diff_augment, diff_augment_backward
    fn = diff_augment_backward if backward else diff_augment
    n = n or len(src)
    out = []
    for k in range(0, len(src), n):
        xs = torch.from_numpy(np.ascontiguousarray(src[k:k + n])).to(DEV)
        ps = torch.from_numpy(np.ascontiguousarray(rows[k:k + n])).to(DEV)
        out.append(fn(xs, ps, policy).cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("S,n", SHAPES)
def test_policy_without_color_moves_and_masks_bit_for_bit(S, n):
    x, g, rows = cases(S, n)
    D, h = M.shift_bound(S), M.cut_size(S) // 2
    for policy in NO_COLOUR:
        wy, wg, by, bg = want(S, n, policy)
        assert wy.dtype == np.float32 and not by.any() and not bg.any()
        y, gx = run(x, rows, policy, n=n), run(g, rows, policy, backward=True, n=n)
        assert (y == wy).all(), "policy %d: %d elements of y differ" % (policy, int((y != wy).sum()))
        assert (gx == wg).all(), "policy %d: %d elements of gx differ" % (policy, int((gx != wg).sum()))
    # row 1 (+D, +D, top-left cut) under translation + cutout: the border and the cut are exactly 0.0, the rest is the source's bits
    y = run(x[1:2], rows[1:2], M.TRANSLATION | M.CUTOUT)[0]
    assert (bits(y[:, :D, :]) == 0).all() and (bits(y[:, :, :D]) == 0).all() and (y[:, :h, :h] == 0).all()          # the cut: 0.0f * x
    assert np.array_equal(bits(y[:, h:, h:]), bits(x[1][:, h - D:S - D, h - D:S - D]))
    y = run(x[1:2], rows[1:2], 0)[0]          # the empty policy: a copy, whatever the row says
    assert np.array_equal(bits(y), bits(x[1]))


def share(got, wanted, bound):
    err = np.abs(got.astype(np.float64) - wanted)
    assert (bound > 0).all()
    return err, float((err / bound).max())


@pytest.mark.parametrize("S,n", SHAPES)
def test_policy_with_color_forward_within_the_derived_bound(S, n):
    x, _, rows = cases(S, n)
    for policy in WITH_COLOUR:
        wy, _, by, _ = want(S, n, policy)
        y = run(x, rows, policy, n=n)
        zero = by == 0                                          # the border and the cut: exactly 0.0 there
        assert (y[zero] == 0).all() and (wy[zero] == 0).all()
        err, worst = share(y[~zero], wy[~zero], by[~zero])
        print("forward S = %d policy %d: worst share of FORWARD_BOUND %.3f, largest error %.3e" % (S, policy, worst, err.max()))
        assert (err <= by[~zero]).all(), "policy %d: %d elements outside the bound, worst share %.3f" % (policy, int((err > by[~zero]).sum()), worst)


@pytest.mark.parametrize("S,n", SHAPES)
def test_policy_with_color_backward_within_the_derived_bound(S, n):
    _, g, rows = cases(S, n)
    for policy in WITH_COLOUR:
        _, wg, _, bg = want(S, n, policy)
        gx = run(g, rows, policy, backward=True, n=n)
        err, worst = share(gx, wg, bg)
        print("backward S = %d policy %d: worst share of BACKWARD_BOUND %.3f, largest error %.3e" % (S, policy, worst, err.max()))
        assert (err <= bg).all(), "policy %d: %d elements outside the bound, worst share %.3f" % (policy, int((err > bg).sum()), worst)


def offset_views(values, words):
    """`values` inside a larger allocation, `words` fp32 words past a 16-byte boundary, between sentinel guards"""
    flat = torch.full((values.size + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[32 + words:32 + words + values.size].view(torch.float32).view(values.shape)
    view.copy_(torch.from_numpy(values).to(DEV))
    return flat, view


@pytest.mark.parametrize("S,n", SHAPES)
def test_independence_and_determinism(S, n):
    from locate_amd._lib import check, lib
    x, g, rows = cases(S, n)
    x, g, rows = x[:n], g[:n], rows[1:n + 1]
    perm = np.roll(np.arange(n), 1)
    for policy in (M.FULL, M.TRANSLATION | M.CUTOUT):
        for backward, src in ((False, x), (True, g)):
            first = run(src, rows, policy, backward)
            assert np.array_equal(bits(first), bits(run(src, rows, policy, backward))), "two calls differ"
            moved = run(src[perm], rows[perm], policy, backward)
            assert np.array_equal(bits(moved), bits(first[perm])), "the batch order shows"
            alone = run(src[n - 1:], rows[n - 1:], policy, backward)
            assert np.array_equal(bits(alone[0]), bits(first[n - 1])), "an image alone differs from itself in a batch"
            # input and output one word past a 16-byte boundary, through the raw ABI; nothing outside the output is written
            _, src_view = offset_views(src, 1)
            out_flat, out_view = offset_views(np.zeros_like(src), 1)
            assert src_view.data_ptr() % 16 == 4 and out_view.data_ptr() % 16 == 4
            p = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
            nbytes = lib().locate_diffaug_workspace_bytes(n, S)
            assert (nbytes == 0) == (S <= 64)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
            entry = lib().locate_diffaug_bwd if backward else lib().locate_diffaug_fwd
            check(entry(src_view.data_ptr(), p.data_ptr(), out_view.data_ptr(), n, S, policy, ws.data_ptr(),
                        torch.cuda.current_stream().cuda_stream), "locate_diffaug")
            torch.cuda.synchronize()
            assert np.array_equal(bits(out_view.cpu().numpy()), bits(first)), "the buffer's alignment shows"
            guard = out_flat.cpu().numpy()
            assert (guard[:33] == SENTINEL).all() and (guard[33 + src.size:] == SENTINEL).all(), "a word outside the output was written"


@pytest.mark.parametrize("S,n", SHAPES)
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_non_finite_values_are_kept(S, n, poison):
    x, g, rows = cases(S, n)
    x, rows = x[:n].copy(), rows[:n].copy()
    D, cut = M.shift_bound(S), M.cut_size(S)
    rows[1] = M.make_row(b=0.1, s=0.8, c=1.1, ty=D, tx=0, y0=8, y1=8 + cut, x0=8, x1=8 + cut)
    x[1, 1, 12, 12] = poison                                  # lands at (D + 12, 12): under the cut
    others = [k for k in range(n) if k != 1]
    clean = run(np.where(np.isfinite(x), x, 0).astype(np.float32), rows, M.FULL)
    # without colour: the one element stays what it was multiplied into - NaN for both (0 * Inf) - and nothing else changes
    y = run(x, rows, M.TRANSLATION | M.CUTOUT)
    assert np.isnan(y[1, 1, D + 12, 12]) and int((~np.isfinite(y)).sum()) == 1
    # with colour: the whole image inside the frame is non-finite, the translation border stays 0, the other images are untouched
    y = run(x, rows, M.FULL)
    assert not np.isfinite(y[1][:, D:, :]).any() and (bits(y[1][:, :D, :]) == 0).all()
    if np.isnan(poison):
        assert np.isnan(y[1][:, D:, :]).all()
    assert np.array_equal(bits(y[others]), bits(clean[others]))
    # backward: a non-finite gradient under the cut
    g = g[:n].copy()
    g[1, 2, D + 12, 12] = poison                              # read by (12, 12), masked where it is read
    gx = run(g, rows, M.TRANSLATION | M.CUTOUT, backward=True)
    assert np.isnan(gx[1, 2, 12, 12]) and int((~np.isfinite(gx)).sum()) == 1
    gx = run(g, rows, M.FULL, backward=True)
    assert np.isnan(gx[1]).all() and np.isfinite(gx[others]).all()


def test_autograd_runs_the_backward_kernel_and_only_when_asked():
    from locate_amd import diff_augment, diff_augment_backward
    S, n = 64, 3
    x, g, rows = cases(S, n)
    xs, gs, ps = (torch.from_numpy(np.ascontiguousarray(a[:n])).to(DEV) for a in (x, g, rows))
    for policy in ("color,translation,cutout", "translation"):
        leaf = xs.clone().requires_grad_()
        y = diff_augment(leaf, ps, policy)
        assert y.requires_grad and torch.equal(y.detach(), diff_augment(xs, ps, policy))
        y.backward(gs)
        assert torch.equal(leaf.grad, diff_augment_backward(gs, ps, policy))
        plain = diff_augment(xs, ps, policy)
        assert not plain.requires_grad and plain.grad_fn is None          # no node: no backward is ever launched
    with pytest.raises(ValueError):
        diff_augment(xs, ps, "color,flip")
    with pytest.raises(TypeError):
        diff_augment(xs, ps[:2])
    with pytest.raises(TypeError):
        diff_augment(xs[:, :, :, :60], ps)


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    assert L.locate_diffaug_param_floats() == 12
    assert L.locate_diffaug_workspace_bytes(2, 64) == 0 and L.locate_diffaug_workspace_bytes(2, 128) == 2 * 12 * 8
    assert L.locate_diffaug_workspace_bytes(3, 256) == 3 * 48 * 8
    buf = torch.zeros(2 * 3 * 128 * 128 + 64, dtype=torch.float32, device=DEV)
    x, y, p = buf.data_ptr(), buf.data_ptr() + 4 * 3 * 128 * 128, buf.data_ptr()
    for args in ((None, p, y, 1, 32, 7, None), (x, None, y, 1, 32, 7, None), (x, p, x, 1, 32, 7, None), (x, p, y, 0, 32, 7, None),
                 (x, p, y, 1, 48, 7, None), (x, p, y, 1, 32, 8, None), (x, p, y, 1, 128, 7, None), (x + 2, p, y, 1, 32, 7, None)):
        for entry, name in ((L.locate_diffaug_fwd, b"locate_diffaug_fwd"), (L.locate_diffaug_bwd, b"locate_diffaug_bwd")):
            assert entry(*args, None) == 1
            assert name in L.locate_last_error()
    assert L.locate_diffaug_fwd(x, p, y, 1, 128, 6, None, None) == 0          # without colour S = 128 needs no workspace
    torch.cuda.synchronize()
