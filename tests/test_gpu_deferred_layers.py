"""The deferred end-of-pass path through the autograd layer: single layers on an ops.Runtime() of their own - deferral on, as in
Generator, Discriminator, TrainStep and bench.py - with leaf parameters, out.backward(g) and the gradients read from .grad after
the pass, against the float64 models of tests/helpers/finaliser_model.py and float64 autograd.  (tests/test_gpu_ops.py drives
the same layers through ops.DEFAULT_RUNTIME, which finishes every gradient inside its own backward node.)

Every test counts the calls of the runtime's queues and asserts the expected one was taken: a silent fall-back to the immediate
path fails.  Needs an MI355X: run with -m gpu.

Tolerances (conftest's normalised max error): what the immediate path is held to on the same kind of input - norm dx / dscale /
dbias 5e-5, norm out 1e-5 (test_inplace_norm_fused_activation_and_big); gate dgamma 2e-5, da 2e-5, out / dx 1e-6
(test_residual_gate_large_vs_oracle); conv gw and dx 3e-5, du / dv 5e-4 (dsigma out of a real weight gradient:
test_spectral_norm_layers_golden).  Statistics hand-off: mean and std within 1e-6 of std - the partials are fp64, only the
final fp32 rounding may show, 1e-6 is eight ulps.  Bias gradients of the convs: 2e-6 of sum |gy| (under 32 additions of relative
rounding 2^-24 each, see tests/test_gpu_finalisers.py)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import finaliser_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

QUEUES = ("queue_norm_channels", "queue_sum", "queue_sn_rank1", "queue_sn_dots", "queue_channel_sum")


def dev():
    return torch.device("cuda:0")


def counted_runtime():
    """A runtime as the networks make it (deferral on, precision 0) whose queues count their calls (and keep their arguments)."""
    from locate_amd import ops
    rt = ops.Runtime()
    assert rt.defer_finalisers and rt.precision == 0
    rt.calls = {q: [] for q in QUEUES}
    for q in QUEUES:
        def wrap(*args, _inner=getattr(rt, q), _log=rt.calls[q]):
            _log.append(args)
            return _inner(*args)
        setattr(rt, q, wrap)
    return rt


def counts(rt):
    return {q: len(rt.calls[q]) for q in QUEUES if rt.calls[q]}


def leaf(t):
    return t.to(dev()).requires_grad_(True)


def assert_within(got, want, magnitude, tol, what):
    got, want, magnitude = (torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, want, magnitude))
    err = ((got - want).abs() / magnitude.clamp_min(1e-300)).max().reshape(1)
    one = torch.ones(1, dtype=torch.float64)
    assert_close(torch.cat([err, one]), torch.cat([0 * one, one]), tol, what)


# ------------------------------------------------------------------------------------------------ InPlaceNorm
# ((B, C, H, W), per-sample scale, groups) - what each row reaches in csrc/norm.hip:
NORM_ROWS = [((6, 34, 1, 1), False, 3),        # lane-per-plane body; last channel block of 2
             ((12, 20, 2, 2), True, 3),        # one lane per plane
             ((8, 17, 4, 4), False, 4),        # four groups
             ((3, 5, 5, 7), False, 1),         # scalar bodies, hw = 35
             ((9, 40, 6, 6), True, 3),         # 16 lanes per plane, q4 = 9
             ((6, 48, 8, 16), True, 3),        # 32 lanes per plane, hw = 128
             ((6, 18, 12, 12), False, 3),      # wave-per-plane float4 body
             ((34, 10, 2, 2), False, 2),       # more than 16 batch slots in the channel finaliser
             ((192, 768, 1, 1), True, 3),      # more than 2048 planes: the 512-block cap
             ((6, 96, 32, 32), False, 3)]      # several passes of the dx grid


def _norm_inputs(seed, shape, per_sample):
    gen = torch.Generator().manual_seed(seed)
    B, C = shape[:2]
    x = torch.randn(shape, generator=gen) * 1.7 + 0.4
    scale = torch.randn(B if per_sample else 1, C, 1, 1, generator=gen)
    bias = torch.randn(1, C, 1, 1, generator=gen)
    g = torch.randn(shape, generator=gen)
    return x, scale, bias, g


@pytest.mark.parametrize("with_act", [False, True])
@pytest.mark.parametrize("shape,per_sample,groups", NORM_ROWS)
def test_norm_under_stacked_calls(shape, per_sample, groups, with_act):
    from locate_amd import ops
    assert groups == 1 or (shape[0] // groups) * shape[1] * shape[2] * shape[3] % 4 == 0          # required of stacked calls
    x, scale, bias, g = _norm_inputs(shape[0] * 17 + shape[1] + with_act, shape, per_sample)
    rt = counted_runtime()
    xg, sg, bg = leaf(x), leaf(scale), leaf(bias)
    with rt.stacked_calls(groups):
        out = ops.inplace_norm(xg, sg, bg, with_act, runtime=rt)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    assert counts(rt) == {"queue_norm_channels": 1}
    want_out, _ = M.norm_fwd(x, scale, bias, per_sample, groups, with_act)
    dx, dscale, dbias, _ = M.norm_bwd(x, g, scale, bias, per_sample, groups, with_act)
    what = "norm %s per_sample %d groups %d act %d" % (shape, per_sample, groups, with_act)
    assert_close(out.detach().cpu(), want_out, 1e-5, what + " out")
    assert_close(xg.grad.cpu(), dx, 5e-5, what + " dx")
    assert_close(sg.grad.cpu(), dscale, 5e-5, what + " dscale")
    assert_close(bg.grad.cpu(), dbias, 5e-5, what + " dbias")


@pytest.mark.parametrize("with_act", [False, True])
def test_norm_as_second_consumer_of_a_forked_tensor(with_act):
    """Two norms on the two aliases of ops.fork: whichever backward kernel runs second adds into the first one's buffer
    (accumulate_dx = 1 of locate_norm_bwd_fused)."""
    from locate_amd import ops
    shape, groups = (9, 40, 6, 6), 3
    x, s1, b1, g1 = _norm_inputs(5, shape, True)
    _, s2, b2, g2 = _norm_inputs(6, shape, False)
    rt = counted_runtime()
    xg, p1, q1, p2, q2 = leaf(x), leaf(s1), leaf(b1), leaf(s2), leaf(b2)
    with rt.stacked_calls(groups):
        a, b = ops.fork(xg)
        o1 = ops.inplace_norm(a, p1, q1, with_act, runtime=rt)
        o2 = ops.inplace_norm(b, p2, q2, not with_act, runtime=rt)
    torch.autograd.backward([o1, o2], [g1.to(dev()), g2.to(dev())])
    torch.cuda.synchronize()
    assert counts(rt) == {"queue_norm_channels": 2}
    dx1, ds1, db1, _ = M.norm_bwd(x, g1, s1, b1, True, groups, with_act)
    dx2, ds2, db2, _ = M.norm_bwd(x, g2, s2, b2, False, groups, not with_act)
    assert_close(xg.grad.cpu(), dx1 + dx2, 5e-5, "forked dx")
    for got, want, what in ((p1, ds1, "dscale 1"), (q1, db1, "dbias 1"), (p2, ds2, "dscale 2"), (q2, db2, "dbias 2")):
        assert_close(got.grad.cpu(), want, 5e-5, "forked " + what)


def test_norm_with_a_per_sample_scale_that_is_no_leaf():
    """The style scale of a generator block: dscale comes back through autograd (to the tensor the scale was made from), dbias is
    late."""
    from locate_amd import ops
    shape, groups = (12, 20, 2, 2), 3
    x, scale, bias, g = _norm_inputs(8, shape, True)
    rt = counted_runtime()
    xg, pre, bg = leaf(x), leaf(scale), leaf(bias)
    sg = ops.tanh(pre)
    assert not sg.is_leaf
    with rt.stacked_calls(groups):
        out = ops.inplace_norm(xg, sg, bg, True, runtime=rt)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    assert counts(rt) == {"queue_norm_channels": 1}
    th = torch.tanh(scale.double())
    dx, dscale, dbias, _ = M.norm_bwd(x, g, th, bias, True, groups, True)
    assert_close(xg.grad.cpu(), dx, 5e-5, "dx")
    assert_close(pre.grad.cpu(), dscale * (1 - th * th), 5e-5, "dscale through autograd")
    assert_close(bg.grad.cpu(), dbias, 5e-5, "late dbias")


# ------------------------------------------------------------------------------------------------ residual gate
GATE_SHAPES = [(5, 7, 2, 2), (6, 33, 4, 4), (3, 64, 1, 1), (8, 48, 64, 64)]


@pytest.mark.parametrize("per_plane", [False, True])
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_gate_dgamma_is_late(shape, per_plane):
    from locate_amd import ops
    gen = torch.Generator().manual_seed(shape[1] * 2 + per_plane)
    x, g = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    a = torch.randn((shape[0], shape[1], 1, 1) if per_plane else shape, generator=gen)
    gamma = torch.tensor([[3.0]])
    rt = counted_runtime()
    xg, ag, gg = leaf(x), leaf(a), leaf(gamma)
    out = ops.residual_gate(xg, ag, gg, runtime=rt)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    assert counts(rt) == {"queue_sum": 1}
    xd, ad, gd = x.double(), a.double(), g.double()
    what = "gate %s per_plane %d" % (shape, per_plane)
    assert_close(out.detach().cpu(), (3.0 * ad + 1) * xd, 1e-6, what + " out")
    assert_close(xg.grad.cpu(), (3.0 * ad + 1) * gd, 1e-6, what + " dx")
    assert_close(ag.grad.cpu(), (3.0 * xd * gd).sum_to_size(a.shape), 2e-5, what + " da")
    assert_close(gg.grad.cpu(), (xd * xd * gd).sum().reshape(1, 1), 2e-5, what + " dgamma")          # x^2 g, as the reference codes it


# ------------------------------------------------------------------------------------------------ statistics hand-off
@pytest.mark.parametrize("per_plane", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
@pytest.mark.parametrize("C,H,W", [(24, 6, 34), (6, 5, 7)])
def test_gate_statistics_feed_the_norm(groups, C, H, W, per_plane, monkeypatch):
    """residual_gate(with_stats=True) leaves the fp64 partial sums of its output per stacked call, the norm behind it skips its
    own statistics pass.  (2 groups, 24, 6, 34): 9792 elements per call - 2.4 of the 4096 a gate block covers per visit, so the
    calls' boundaries fall inside what a flat indexing would give one block, and hw = 204 takes the 16-byte body of either
    gate form; (2 groups, 6, 5, 7): hw = 35, the scalar body of the per-plane form."""
    from locate_amd import ops
    from locate_amd._lib import lib
    shape = (2 * groups, C, H, W)
    gen = torch.Generator().manual_seed(groups * 10 + C + per_plane)
    x = torch.randn(shape, generator=gen) * (1 + torch.arange(shape[0]).view(-1, 1, 1, 1)) + 0.3          # every call its own statistics
    a = torch.randn((shape[0], C, 1, 1) if per_plane else shape, generator=gen)
    scale, bias = torch.randn(1, C, 1, 1, generator=gen), torch.randn(1, C, 1, 1, generator=gen)
    handed = []
    inner = lib().locate_norm_fwd

    def norm_fwd(*args):
        handed.append(args[12])
        return inner(*args)

    monkeypatch.setattr(lib(), "locate_norm_fwd", norm_fwd)
    rt = counted_runtime()
    xg, ag, gg, sg, bg = leaf(x), leaf(a), leaf(torch.tensor([[0.7]])), leaf(scale), leaf(bias)
    with rt.stacked_calls(groups):
        gated = ops.residual_gate(xg, ag, gg, runtime=rt, with_stats=True)
        out = ops.inplace_norm(gated, sg, bg, False, runtime=rt)
    torch.cuda.synchronize()
    assert handed and handed[0], "the norm did not take the gate's statistics partials"
    stats = out.grad_fn.saved_tensors[3].cpu().double().view(groups, 2)
    gated_host = gated.detach().cpu()
    want_out, want_stats = M.norm_fwd(gated_host, scale, bias, False, groups, False)
    what = "hand-off %s groups %d per_plane %d" % (shape, groups, per_plane)
    assert_within(stats[:, 0], want_stats[:, 0], want_stats[:, 1], 1e-6, what + " mean")
    assert_within(stats[:, 1], want_stats[:, 1], want_stats[:, 1], 1e-6, what + " std")
    assert_close(out.detach().cpu(), want_out, 1e-5, what + " out")
    assert_close(gated_host, (0.7 * a.double() + 1) * x.double(), 1e-6, what + " gate out")


# ------------------------------------------------------------------------------------------------ spectral-normalised conv
def _sn_conv_case(seed, cin, cout, k, pad, H, B, calls):
    """`calls` forward calls stacked along the batch of one sn_conv, each after a power iteration of its own; backward; float64
    autograd of the spectral-normalised layer with the reference's view of u, v (the latest state: oracle.SigmaFn).  Returns the
    runtime, the GPU gradients and the float64 ones."""
    from locate_amd import ops
    from oracle import locate_oracle as O
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=gen) * 0.3
    u0 = torch.randn(cout, generator=gen)
    v0 = torch.randn(cin * k * k, generator=gen)
    u0, v0 = u0 / u0.norm(), v0 / v0.norm()
    bias = torch.randn(cout, generator=gen)
    x = torch.randn(B, cin, H, H, generator=gen)
    spec = ops.ConvSpec("conv", k, k, 1, pad, pad)
    rt = counted_runtime()
    wg, ug, vg, bg, xg = leaf(w), leaf(u0), leaf(v0), leaf(bias), leaf(x)
    sig, wvs, us, vs = [], [], [], []
    for _ in range(calls):
        s, wv = ops.sn_power_iteration(wg, ug, vg)
        sig.append(s)
        wvs.append(wv)
        us.append(ug.detach().clone())
        vs.append(vg.detach().clone())
    sigma_wv = (torch.stack(sig), torch.stack(wvs)) if calls > 1 else (sig[0], wvs[0])
    y = ops.sn_conv(xg, wg, ug, vg, bg, spec, sigma_wv, runtime=rt)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy.to(dev()))
    torch.cuda.synchronize()
    got = {"y": y.detach(), "gw": wg.grad, "du": ug.grad, "dv": vg.grad, "dbias": bg.grad, "dx": xg.grad}
    assert all(t is not None for t in got.values()), [n for n, t in got.items() if t is None]
    # float64: the same state after every power iteration, widened
    W, ud, vd, bd, xd = (t.double().requires_grad_(True) for t in (w, u0, v0, bias, x))
    Bg = B // calls
    ys = []
    for c in range(calls):
        ud.data.copy_(us[c].cpu())
        vd.data.copy_(vs[c].cpu())
        sigma = O.SigmaFn.apply(W.reshape(cout, -1), ud, vd)
        ys.append(F.conv2d(xd[c * Bg:(c + 1) * Bg], W / sigma, bd, 1, pad))
    yd = torch.cat(ys)
    yd.backward(gy.double())
    want = {"y": yd.detach(), "gw": W.grad, "du": ud.grad, "dv": vd.grad, "dbias": bd.grad, "dx": xd.grad}
    return rt, got, want, gy


def _verify_sn_conv(got, want, gy, what):
    assert_close(got["y"].cpu(), want["y"], 2e-5, what + " y")
    assert_close(got["dx"].cpu(), want["dx"], 3e-5, what + " dx")
    assert_close(got["gw"].cpu(), want["gw"], 3e-5, what + " gw")
    assert_close(got["du"].cpu(), want["du"], 5e-4, what + " du")
    assert_close(got["dv"].cpu(), want["dv"], 5e-4, what + " dv")
    sums, mags = M.channel_sums(gy)
    assert_close(sums, want["dbias"], 1e-12, what + " (the model's channel sums are the bias gradient)")
    assert_within(got["dbias"], sums, mags, 2e-6, what + " dbias")


def test_sn_conv_one_call():
    """1x1 conv 16 -> 24 on 8x8 with bias: rank-1 record of the one-call meaning, bias gradient through the channel-sum queue."""
    rt, got, want, gy = _sn_conv_case(21, 16, 24, 1, 0, 8, 4, 1)
    assert counts(rt) == {"queue_sn_rank1": 1, "queue_channel_sum": 1}
    assert rt.calls["queue_sn_rank1"][0][2] == 0
    _verify_sn_conv(got, want, gy, "sn_conv 1x1 16->24")


def test_sn_conv_three_stacked_calls_weight_side_dots():
    """3x3 conv 12 -> 20 on 6x6, three calls: the split reduction of the weight gradient emits the per-call dots itself."""
    from locate_amd import ops
    from locate_amd._lib import lib
    geom, _ = ops.ConvSpec("conv", 3, 3, 1, 1, 1).geometry((12, 12, 6, 6), (20, 12, 3, 3))
    assert lib().locate_conv_wgrad_group_partials((ctypes.c_int * 12)(*geom), 3) > 0
    rt, got, want, gy = _sn_conv_case(22, 12, 20, 3, 1, 6, 12, 3)
    assert counts(rt) == {"queue_sn_rank1": 1, "queue_channel_sum": 1}
    assert rt.calls["queue_sn_rank1"][0][2] == 3
    _verify_sn_conv(got, want, gy, "sn_conv 3x3 12->20 x3")


def test_sn_conv_three_stacked_calls_activation_side_dots():
    """A 1x1 map: locate_conv_wgrad_group_partials is 0, the dots are taken from gy and y at the end of the pass."""
    from locate_amd import ops
    from locate_amd._lib import lib
    geom, _ = ops.ConvSpec("conv", 1, 1, 1, 0, 0).geometry((12, 16, 1, 1), (24, 16, 1, 1))
    assert lib().locate_conv_wgrad_group_partials((ctypes.c_int * 12)(*geom), 3) == 0
    rt, got, want, gy = _sn_conv_case(23, 16, 24, 1, 0, 1, 12, 3)
    assert counts(rt) == {"queue_sn_dots": 1, "queue_sn_rank1": 1, "queue_channel_sum": 1}
    assert rt.calls["queue_sn_rank1"][0][2] == 3
    _verify_sn_conv(got, want, gy, "sn_conv 1x1 map x3")
