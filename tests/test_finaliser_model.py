"""The float64 models of the deferred end-of-pass gradient kernels (tests/helpers/finaliser_model.py) against float64 autograd, on
the CPU: the models are what tests/test_gpu_finalisers.py and tests/test_gpu_deferred_layers.py hold the kernels to, so they are
held to something themselves - the oracle's InPlaceNorm / RootTanh applied slice by slice, autograd of W / sigma(W), a direct
restatement of the power iteration."""
import os
import sys

import pytest
import torch

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import finaliser_model as M  # noqa: E402

TOL = 1e-12


def _close(got, want, what):
    e = rel_err(got, want)
    assert e <= TOL, "%s: normalised max error %.3e" % (what, e)


NORM_ROWS = [((6, 34, 1, 1), False, 3), ((12, 20, 2, 2), True, 3), ((8, 17, 4, 4), False, 4), ((3, 5, 5, 7), False, 1),
             ((9, 40, 6, 6), True, 3), ((6, 18, 12, 12), False, 3), ((34, 10, 2, 2), False, 2)]


@pytest.mark.parametrize("with_act", [False, True])
@pytest.mark.parametrize("shape,per_sample,groups", NORM_ROWS)
def test_norm_model_vs_oracle_autograd(shape, per_sample, groups, with_act):
    from oracle import locate_oracle as O
    torch.manual_seed(shape[0] * 100 + shape[1])
    B, C = shape[:2]
    x = (torch.randn(shape) * 1.7 + 0.4).double()
    scale = torch.randn(B if per_sample else 1, C, 1, 1).double()
    bias = torch.randn(1, C, 1, 1).double()
    g = torch.randn(shape).double()
    xr, sr, br = (t.clone().requires_grad_(True) for t in (x, scale, bias))
    Bg = B // groups
    outs, stats = [], []
    for k in range(groups):
        sl = slice(k * Bg, (k + 1) * Bg)
        o = O.inplace_norm(xr[sl], sr[sl] if per_sample else sr, br)
        outs.append(O.root_tanh(o) if with_act else o)
        stats.append([float(x[sl].mean()), float(x[sl].std())])
    ref = torch.cat(outs)
    ref.backward(g)
    out, st = M.norm_fwd(x, scale, bias, per_sample, groups, with_act)
    dx, dscale, dbias, st2 = M.norm_bwd(x, g, scale, bias, per_sample, groups, with_act)
    _close(out, ref.detach(), "out")
    _close(st, torch.tensor(stats, dtype=torch.float64), "stats")
    assert torch.equal(st, st2)
    _close(dx, xr.grad, "dx")
    _close(dscale, sr.grad, "dscale")
    _close(dbias, br.grad, "dbias")
    assert dscale.shape == scale.shape and dbias.shape == bias.shape


@pytest.mark.parametrize("h,wd", [(1, 1), (3, 4), (7, 75), (33, 100)])
def test_rank1_model_one_call_vs_autograd(h, wd):
    """groups = 0: loss = <G, W / sigma(W)> with sigma = u . W v; the record's partials sum to <G, W> of the unscaled gradient."""
    torch.manual_seed(h * 7 + wd)
    W = torch.randn(h, wd, dtype=torch.float64, requires_grad=True)
    u = torch.randn(h, dtype=torch.float64, requires_grad=True)
    v = torch.randn(wd, dtype=torch.float64)
    G = torch.randn(h, wd, dtype=torch.float64)
    sigma = u.dot(W.mv(v))
    (G * (W / sigma)).sum().backward()
    sg = sigma.detach()
    inner = (G * W.detach()).reshape(-1)
    partial = torch.stack([inner[i::5].sum() for i in range(5)])          # any split of <G, W> into partial sums
    gw, du, total = M.sn_rank1(G / sg, partial, u.detach(), v, torch.stack([sg, 1 / sg]), W.detach().mv(v), 0)
    _close(gw, W.grad, "gw")
    _close(du, u.grad, "du")
    _close(total, -(G * W.detach()).sum() / sg ** 2, "dsigma")


@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_rank1_model_stacked_calls_vs_autograd(groups):
    """groups >= 1: every call has its own sigma_k = u_k . W v_k and W v_k, the backward sees the LATEST u, v (the reference writes
    them through .data, oracle.SigmaFn); the record's partials of call k sum to <G_k, W> / sigma_k = <gy_k, y_k - bias>."""
    from oracle import locate_oracle as O
    torch.manual_seed(groups)
    h, wd = 6, 10
    W = torch.randn(h, wd, dtype=torch.float64, requires_grad=True)
    u = torch.randn(h, dtype=torch.float64, requires_grad=True)
    v = torch.randn(wd, dtype=torch.float64, requires_grad=True)
    Gs = torch.randn(groups, h, wd, dtype=torch.float64)
    loss, sig, wvs = 0, [], []
    for k in range(groups):
        u.data.copy_(torch.randn(h))
        v.data.copy_(torch.randn(wd))
        s = O.SigmaFn.apply(W, u, v)
        sig.append(s.detach())
        wvs.append(W.detach().mv(v.detach()))
        loss = loss + (Gs[k] * (W / s)).sum()
    loss.backward()
    sig = torch.stack(sig)
    gw_in = sum(Gs[k] / sig[k] for k in range(groups))
    partial = torch.stack([torch.stack([((Gs[k] * W.detach()) / sig[k]).reshape(-1)[i::3].sum() for i in range(3)]) for k in range(groups)])
    tab = torch.stack([sig, 1 / sig, torch.zeros_like(sig)], 1)          # a table with a stride of its own
    gw, du, total = M.sn_rank1(gw_in, partial, u.detach(), v.detach(), tab, torch.stack(wvs), groups)
    _close(gw, W.grad, "gw")
    _close(du, u.grad, "du")
    _close(M.dv(W.detach(), u.detach(), torch.cat([total.reshape(1), torch.zeros(3, dtype=torch.float64)])), v.grad, "dv")


def test_dots_and_channel_sums_models():
    torch.manual_seed(2)
    gy, y, bias = torch.randn(6, 5, 3, 4).double(), torch.randn(6, 5, 3, 4).double(), torch.randn(5).double()
    for b in (None, bias):
        dots, mags = M.sn_dots(gy, y, b, 3)
        for k in range(3):
            yy = y[2 * k:2 * k + 2] - (0 if b is None else b.view(1, 5, 1, 1))
            _close(dots[k], (gy[2 * k:2 * k + 2] * yy).sum(), "dot %d" % k)
            _close(mags[k], (gy[2 * k:2 * k + 2] * yy).abs().sum(), "magnitudes %d" % k)
    sums, mags = M.channel_sums(gy)
    _close(sums, torch.stack([gy[:, c].sum() for c in range(5)]), "channel sums")
    _close(mags, gy.abs().sum((0, 2, 3)), "channel magnitudes")


@pytest.mark.parametrize("h,wd", [(1, 5), (8, 1), (65, 300)])
def test_power_iteration_model_vs_restatement(h, wd):
    from oracle import locate_oracle as O
    torch.manual_seed(h + wd)
    W = torch.randn(h, wd, dtype=torch.float64)
    u = O._l2n(torch.randn(h, dtype=torch.float64))
    u2, v2, sigma, wv = M.power_iteration(W, u)
    v_ref = O._l2n(W.t().mv(u))              # libs/spectral_norm.py:26-29 as the oracle states it
    u_ref = O._l2n(W.mv(v_ref))
    _close(v2, v_ref, "v")
    _close(u2, u_ref, "u")
    _close(wv, W.mv(v_ref), "wv")
    _close(sigma, u_ref.dot(W.mv(v_ref)), "sigma")
    _close(M.dv(W, u, torch.tensor([0.5, -2.0, 0.25, 3.0])), 1.75 * W.t().mv(u), "dv")
