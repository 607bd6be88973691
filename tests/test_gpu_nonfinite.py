"""No kernel launders a NaN or an Inf that the reference keeps (tests/helpers/nonfinite_model.py states the contract): a special
value put into an activation, an image, a gradient or a discriminator output must arrive wherever the reference - the oracle and
ATen on the CPU, in float32 and in float64 - has it arrive, with the reference's class; and an element the reference keeps finite
stays finite and within the tolerance the operation's own test already uses.  The guards of a training run (statistics, the guarded
optimizer step, the snapshots) all decide from the weights, gradients and losses at the end of a step: they rest on this.

Needs an MI355X: run with -m gpu.  Shapes are the smallest that reach each kernel variant; every configuration runs all its
injections and reports every offender."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import nonfinite_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def S():
    return torch.cuda.current_stream().cuda_stream


def _leaf(t):
    return t.to(dev()).requires_grad_(True)


def _cpu(d):
    return {k: v.detach().cpu() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the kernels, family by family
def gpu_act(case):
    from locate_amd import ops
    from locate_amd._lib import check, lib
    i = case.inputs
    if case.family == "roottanh_acc":          # the second consumer of a forked tensor: dx added into what the first one left
        x, g, gx = i["x"].to(dev()), i["g"].to(dev()), i["acc"].to(dev())
        check(lib().locate_roottanh_bwd(x.data_ptr(), g.data_ptr(), gx.data_ptr(), x.numel(), 1, None, S()), "locate_roottanh_bwd")
        return {"dx": gx}
    x = _leaf(i["x"])
    y = (ops.tanh if case.family == "tanh" else ops.root_tanh)(x)
    y.backward(i["g"].to(dev()))
    return {"y": y, "dx": x.grad}


def gpu_act_rows(case):
    from locate_amd import ops
    i = case.inputs
    latent, pre = _leaf(i["latent"]), _leaf(i["pre"])
    out, as_scale = ops.ActCatFn.apply(latent, pre)
    g = i["g"].to(dev())
    if case.cfg:
        torch.autograd.backward([out, as_scale], [g, i["g_add"].to(dev())])
        return {"out": out, "dlatent": latent.grad, "dpre": pre.grad}
    # no gradient through the scale: the entry point with a null g_add (autograd would hand the Function a tensor of zeros)
    from locate_amd._lib import check, lib
    rows, z = latent.shape
    w = pre.shape[1]
    gpre = torch.empty_like(pre)
    check(lib().locate_act_rows_bwd(pre.data_ptr(), g.data_ptr() + 4 * z, g.stride(0), None, gpre.data_ptr(), rows, w, S()),
          "locate_act_rows_bwd")
    return {"out": out, "dlatent": g[:, :z], "dpre": gpre}


def gpu_norm(case):
    from locate_amd import ops
    i = case.inputs
    x, s, b = _leaf(i["x"]), _leaf(i["scale"]), _leaf(i["bias"])
    out = ops.inplace_norm(x, s, b, case.cfg[1])
    out.backward(i["g"].to(dev()))
    got = {"out": out, "dx": x.grad, "dscale": s.grad, "dbias": b.grad}
    got.update(_norm_two_launch(x.detach(), s.detach(), b.detach(), i["g"].to(dev()), case.cfg[2], case.cfg[1]))
    return got


def _norm_two_launch(x, scale, bias, g, per_sample, with_act):
    """the backward a training step runs: locate_norm_bwd_fused now, the per-channel sums by locate_fin_norm_channels at the end
    of the pass (the rig of tests/test_gpu_finalisers.py's NormCase, on these operands)"""
    import test_gpu_finalisers as FIN
    from locate_amd._lib import check, lib
    Lb = lib()
    B, C = x.shape[:2]
    hw = x[0, 0].numel()
    stats = torch.empty(2, device=dev())
    out = torch.empty_like(x)
    ws = torch.empty(Lb.locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=dev())
    check(Lb.locate_norm_fwd(x.data_ptr(), scale.data_ptr(), int(per_sample), bias.data_ptr(), out.data_ptr(), int(with_act),
                             stats.data_ptr(), B, C, hw, 1, ws.data_ptr(), None, None, S()), "locate_norm_fwd")
    dx, dscale, dbias = (torch.full_like(t, float("nan")) for t in (x, scale, bias))
    ws2 = torch.empty(Lb.locate_norm_bwd_fused_workspace_bytes(B, C), dtype=torch.uint8, device=dev())
    check(Lb.locate_norm_bwd_fused(x.data_ptr(), g.data_ptr(), stats.data_ptr(), scale.data_ptr(), int(per_sample), bias.data_ptr(),
                                   int(with_act), dx.data_ptr(), dscale.data_ptr() if per_sample else None, B, C, hw, 1, ws2.data_ptr(),
                                   0, S()), "locate_norm_bwd_fused")
    s1 = ws2.data_ptr() + Lb.locate_norm_bwd_fused_plane_offset()
    FIN.run("locate_fin_norm_channels", [FIN.rec([s1, s1 + 4 * B * C, stats, None if per_sample else dscale, dbias], [], [B, C, 1])])
    return {"dx_two_launch": dx, "dscale_two_launch": dscale, "dbias_two_launch": dbias}


def gpu_gate(case):
    from locate_amd import ops
    i = case.inputs
    x, a, gamma = _leaf(i["x"]), _leaf(i["a"]), _leaf(i["gamma"])
    out = ops.residual_gate(x, a, gamma)
    out.backward(i["g"].to(dev()))
    return {"out": out, "dx": x.grad, "da": a.grad, "dgamma": gamma.grad}


def gpu_softmax(case):
    from locate_amd import ops
    x = _leaf(case.inputs["x"])
    y = ops.softmax_lastdim(x)
    y.backward(case.inputs["g"].to(dev()))
    return {"y": y, "dx": x.grad}


def gpu_stencil(case):
    from locate_amd import ops
    from locate_amd._lib import check, lib
    op, shape = case.cfg
    i = case.inputs
    B, C = shape[:2]
    if op == "add3":                            # a is a channel slice of a wider tensor, as the concatenation's gradient arrives
        wide = torch.zeros((B, C + 3) + tuple(shape[2:]), device=dev())
        a = wide[:, :C]
        a.copy_(i["a"])
        b, c = i["b"].to(dev()), i["c"].to(dev())
        out = torch.empty(shape, device=dev())
        check(lib().locate_add3(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0), out.data_ptr(), B,
                                b[0].numel(), S()), "locate_add3")
        return {"sum": out}
    if op == "fork3":                           # aliases in the order (identity, conv, norm); the sum is (norm + identity) + conv
        x = _leaf(torch.zeros(shape))
        ident, conv, norm = ops.fork3(x)
        torch.autograd.backward([norm, ident, conv], [i["a"].to(dev()), i["b"].to(dev()), i["c"].to(dev())])
        return {"sum": x.grad}
    if op == "cat":
        a, b = _leaf(i["a"]), _leaf(i["b"])
        out = ops.cat_channels(a, b)
        out.backward(i["g"].to(dev()))
        return {"out": out, "da": a.grad, "db": b.grad}
    x = _leaf(i["x"])
    y = {"upsample": ops.upsample2x, "avgpool": ops.avgpool2, "pool_upsample": lambda t: ops.pool_upsample(t, C // 2),
         "feature_pool2": lambda t: ops.feature_pool(t, C // 2), "feature_pool4": lambda t: ops.feature_pool(t, C // 4)}[op](x)
    y.backward(i["g"].to(dev()))
    return {"y": y, "dx": x.grad}


def gpu_loss(case):
    from locate_amd.train import d_loss, g_loss
    t, f, a = (case.inputs[k].to(dev()) for k in ("t", "f", "a"))
    losses, gt, gf, ga = d_loss(t, f, a)
    loss, g = g_loss(f)
    return {"d_losses": losses, "gt": gt, "gf": gf, "ga": ga, "g_loss": loss, "g_gf": g}


GPU = {"roottanh": gpu_act, "tanh": gpu_act, "roottanh_acc": gpu_act, "act_rows": gpu_act_rows, "norm": gpu_norm, "norm_scale_inf": gpu_norm,
       "gate": gpu_gate,
       "softmax": gpu_softmax, "stencil": gpu_stencil, "loss": gpu_loss}


def _report(bad, n):
    assert not bad, "%d of %d injections break the contract:\n  %s" % (len(bad), n, "\n  ".join(bad[:12]))


@pytest.mark.parametrize("family,cfg", M.stream_configs(), ids=lambda v: str(v).replace(" ", ""))
def test_stream_kernels_keep_the_reference_class(family, cfg):
    """Rules 1 and 2 with equal classes (stream kernels take no exemption) on every output and gradient, for every injection of
    the configuration: one quiet NaN, +Inf or -Inf at a named place of one operand."""
    _, cases, _, tols = M.STREAM_FAMILIES[family]
    bad, n = [], 0
    for case in cases(cfg):
        n += 1
        want32, want64 = M.both_references(family, case)
        got = _cpu(GPU[family](case))
        bad += ["%s: %s" % (case.id, line) for line in M.check_outputs(got, want32, want64, tols)]
    _report(bad, n)


# ------------------------------------------------------------------------------------------------ contractions
_REFS = {}


def _contraction_refs(case, ref):
    key = (case.id, ref.__name__)
    if key not in _REFS:
        _REFS[key] = (ref(case, torch.float32), ref(case, torch.float64))
    return _REFS[key]


def gpu_contraction(case, form):
    """through the SpectralNorm module, as tests/test_gpu_ops.py runs the contractions; f16x2: the operands carry their
    largest-magnitude words, which is what selects the fp16-piece form"""
    from locate_amd import SpectralNorm, ops
    layer, _ = M.contraction_layer(case.cfg)
    mod = SpectralNorm(layer)
    mod.load_state_dict(M.contraction_state_dict(case))
    mod = mod.to(dev())
    x, g = _leaf(case.inputs["x"]), case.inputs["g"].to(dev())
    if form == "f16x2":
        x, g = ops.tag_amax(x), ops.tag_amax(g)
    y = mod(x)
    y.backward(g)
    return {"y": y, "dx": x.grad, "dw": mod.module.weight_bar.grad, "u": mod.module.weight_u}


def gpu_contraction_fp8(case):
    """the same layer with e4m3 operands, selected as tests/test_gpu_fp8.py selects them: a runtime of precision 3"""
    from locate_amd import SpectralNorm, ops
    layer, _ = M.contraction_layer(case.cfg)
    mod = SpectralNorm(layer)
    mod.load_state_dict(M.contraction_state_dict(case))
    mod = mod.to(dev())
    mod.runtime = ops.Runtime()
    mod.runtime.precision = 3
    mod.runtime.defer_finalisers = False
    x = _leaf(case.inputs["x"])
    y = mod(x)
    y.backward(case.inputs["g"].to(dev()))
    return {"y": y, "dx": x.grad, "dw": mod.module.weight_bar.grad, "u": mod.module.weight_u}


def _escape(case):
    """rule 2's "or non-finite": only the forms that scale by a largest-magnitude word, and only under an Inf operand"""
    return M.special_of(case)[1] in (M.PINF, M.NINF)


CONTRACTION_RUNS = [(name, form) for name in M.CONTRACTIONS for form in (("bf16x3", "f16x2") if M.CONTRACTIONS[name][0] == "dense" else ("fp32",))]


@pytest.mark.parametrize("name,form", CONTRACTION_RUNS, ids=lambda v: str(v))
def test_contractions_keep_what_the_reference_keeps(name, form, monkeypatch):
    """Rules 1 and 2 on y, dx, dW_bar (and the advanced u) of one geometry per kernel family: a special in x (interior pixel, corner
    pixel), in one weight, in gy.  Non-finite where the reference is (an Inf may arrive as a NaN); the reference's finite elements
    finite and within 2e-5 / 5e-5 - under an Inf operand the fp16-piece form may make them non-finite, never finite and wrong."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0 if form == "f16x2" else 1e30)
    if M.CONTRACTIONS[name][-1]:
        monkeypatch.setattr(ops, "WIN_MODE", 2)
    ops._WIN_CACHE.clear()
    f16_before, win_before = ops.F16_CALLS["fwd"], ops.WIN_CALLS[0]
    bad, n = [], 0
    for case in M.contraction_cases(name):
        n += 1
        want32, want64 = _contraction_refs(case, M.contraction_reference)
        got = _cpu(gpu_contraction(case, form))
        lines = M.check_outputs(got, want32, want64, M.CONTRACTION_TOL, strict_class=False,
                                allow_nonfinite_for_finite=form == "f16x2" and _escape(case))
        bad += ["%s [%s]: %s" % (case.id, form, line) for line in lines]
    ops._WIN_CACHE.clear()
    if form == "f16x2":
        assert ops.F16_CALLS["fwd"] >= f16_before + n, "the fp16-piece form was not taken"
    if M.CONTRACTIONS[name][-1]:
        assert ops.WIN_CALLS[0] > win_before, "the window form was not taken"
    _report(bad, n)


@pytest.mark.parametrize("name", M.FP8_CONTRACTIONS)
def test_fp8_contractions_keep_what_the_reference_keeps(name):
    """The same for e4m3 operands, at that form's own bound (2 u = 0.125, tests/test_gpu_fp8.py; u and sigma stay fp32: 1e-5)."""
    from locate_amd import ops
    before = ops.FP8_CALLS[0]
    bad, n = [], 0
    for case in M.contraction_cases(name):
        n += 1
        want32, want64 = _contraction_refs(case, M.contraction_reference)
        got = _cpu(gpu_contraction_fp8(case))
        lines = M.check_outputs(got, want32, want64, M.FP8_TOL, strict_class=False, allow_nonfinite_for_finite=_escape(case))
        bad += ["%s [fp8]: %s" % (case.id, line) for line in lines]
    assert ops.FP8_CALLS[0] == before + 2 * n
    _report(bad, n)


# ------------------------------------------------------------------------------------------------ spectral norm and finalisers
def L():
    from locate_amd._lib import lib
    return lib()


def _sn_check(got, ref, args, relaxed=()):
    """check_contract per output; `relaxed` outputs (gw: rule 1 only asks for non-finite) need not keep the class"""
    want32, want64 = ref(*args, torch.float32), ref(*args, torch.float64)
    assert set(got) == set(want64)
    bad = []
    for k in sorted(got):
        msg = M.check_contract(got[k].detach().cpu(), want32[k], want64[k], M.SN_TOL[k], strict_class=k not in relaxed)
        if msg:
            bad.append("%s: %s" % (k, msg))
    return bad


def _sn_injections(h, wd, with_W=True):
    wp, up = M.sn_places(h, wd)
    for operand, places in ((("W", wp),) if with_W else ()) + (("u", up),):
        for pname, idx in places.items():
            for sname, val in M.SPECIALS.items():
                yield operand, idx, val, "%s[%s]=%s" % (operand, pname, sname)


@pytest.mark.parametrize("h,wd", M.SN_SIZES)
def test_power_iteration_follows_the_reference(h, wd):
    """One NaN or Inf in W or in u: sigma, 1 / sigma, u, v and W v have the reference's class element by element (rule 3)."""
    import test_gpu_finalisers as FIN
    from locate_amd._lib import check
    bad, n = [], 0
    for operand, idx, val, tag in _sn_injections(h, wd):
        n += 1
        c = FIN.SnLayerCase(90 + h, h, wd)
        if operand == "W":
            c.W[idx] = val
            c.d_W.copy_(c.W)
        else:
            c.u0[idx] = val
            c.d_u.copy_(c.u0)
        check(L().locate_sn_power_iter(c.d_W.data_ptr(), c.d_u.data_ptr(), c.d_v.data_ptr(), c.d_sigma.data_ptr(), c.d_wv.data_ptr(),
                                       c.h, c.wd, c.scratch.data_ptr(), S()), "locate_sn_power_iter")
        got = {"u": c.d_u, "v": c.d_v, "wv": c.d_wv, "sigma": c.d_sigma[:1], "inv_sigma": c.d_sigma[1:2]}
        bad += ["power iteration %dx%d %s: %s" % (h, wd, tag, line) for line in _sn_check(got, M.sn_power_reference, (c.W, c.u0))]
    _report(bad, n)


@pytest.mark.parametrize("h,wd", M.SN_SIZES)
def test_rank1_finaliser_follows_the_reference(h, wd):
    """locate_fin_sn_rank1, one call's record: a special in one inner_partial or in u.  dsigma and du keep the reference's class;
    gw is non-finite wherever the reference's is."""
    import test_gpu_finalisers as FIN
    injections = [("partial", i, v, "partial[%d]=%s" % (i, s)) for i in (0, 100, 256) for s, v in M.SPECIALS.items()]
    injections += list(_sn_injections(h, wd, with_W=False))
    bad = []
    for operand, idx, val, tag in injections:
        c = FIN.Rank1Case(7000 + h, h, wd, 0, (257, 2, 0, True, True))
        if operand == "partial":
            c.partial[0, idx] = val
            c.d_partial.copy_(c.partial)
        else:
            c.u[idx] = val
            c.d_u.copy_(c.u)
        FIN.run("locate_fin_sn_rank1", [c.record()])
        got = {"gw": c.d_gw, "du": c.d_du, "dsigma": c.d_dsig}
        args = (c.gw_in, c.partial.reshape(-1), c.u, c.v, c.tab[0, 0], c.wv[0, :h])
        bad += ["rank-1 %dx%d %s: %s" % (h, wd, tag, line) for line in _sn_check(got, M.sn_rank1_reference, args, relaxed=("gw",))]
    _report(bad, len(injections))


@pytest.mark.parametrize("h,wd", M.SN_SIZES)
def test_dv_follows_the_reference(h, wd):
    """locate_sn_dv_batched: dv = (sum of the dsigma slots) W^T u with a special in W, in u or in one slot."""
    import test_gpu_finalisers as FIN
    from locate_amd._lib import check
    injections = list(_sn_injections(h, wd)) + [("slot", 2, v, "slot[2]=%s" % s) for s, v in M.SPECIALS.items()]
    bad = []
    for operand, idx, val, tag in injections:
        c = FIN.SnLayerCase(95 + h, h, wd)
        slots = torch.tensor([0.75, -1.5, 0.375, 2.0])
        if operand == "W":
            c.W[idx] = val
            c.d_W.copy_(c.W)
        elif operand == "u":
            c.u0[idx] = val
            c.d_u.copy_(c.u0)
        else:
            slots[idx] = val
        c.d_sigma.copy_(slots)
        table, max_h, max_wd = FIN._table([c])
        check(L().locate_sn_dv_batched(table.data_ptr(), 1, max_h, max_wd, S()), "locate_sn_dv_batched")
        bad += ["dv %dx%d %s: %s" % (h, wd, tag, line) for line in _sn_check({"dv": c.d_v}, M.sn_dv_reference, (c.W, c.u0, slots))]
    _report(bad, len(injections))


@pytest.mark.parametrize("Bg,Mn,plane,groups,with_bias", [(3, 5, 7, 3, True), (4, 16, 64, 2, False), (2, 33, 1028, 1, True)])
def test_dot_finaliser_follows_the_reference(Bg, Mn, plane, groups, with_bias):
    """locate_fin_sn_dots, which leaves the inner partials of <gy, y - bias> per stacked call: a special in gy, in y or in the bias
    makes the dot of the calls the reference poisons non-finite with the reference's class, and leaves the other calls' dots alone."""
    import test_gpu_finalisers as FIN
    shape = (Bg * groups, Mn, plane)
    places = {"first": (0, 0, 0), "inner": (shape[0] // 2, Mn // 2, plane // 2 + 1), "last": (shape[0] - 1, Mn - 1, plane - 1)}
    injections = [(op, idx, val, "%s[%s]=%s" % (op, pn, sn)) for op in ("gy", "y") for pn, idx in places.items() for sn, val in M.SPECIALS.items()]
    if with_bias:
        injections += [("bias", (Mn - 1,), val, "bias[last]=%s" % sn) for sn, val in M.SPECIALS.items()]
    bad = []
    for operand, idx, val, tag in injections:
        c = FIN.DotCase(Bg * 1000 + Mn + groups, Bg, Mn, plane, groups, with_bias)
        host, device = {"gy": (c.gy, c.d_gy), "y": (c.y, c.d_y), "bias": (c.bias, c.d_bias)}[operand]
        host[idx] = val
        device[idx] = val
        FIN.run("locate_fin_sn_dots", [c.record()])

        def ref(dtype):
            y = c.y.to(dtype) - (c.bias.to(dtype).reshape(1, Mn, 1) if with_bias else 0)
            return (c.gy.to(dtype) * y).reshape(groups, -1)
        w64 = ref(torch.float64).sum(1)
        # the finaliser's own bound, 2e-5 of a call's sum of magnitudes, restated for an error normalised by the largest dot
        ok = torch.isfinite(w64)
        tol = 2e-5 * float(ref(torch.float64).abs().sum(1)[ok].max()) / float(w64[ok].abs().max()) if bool(ok.any()) else 0.0
        msg = M.check_contract(c.d_partial.cpu().sum(1), ref(torch.float32).sum(1), w64, tol)
        if msg:
            bad.append("dots %s groups %d %s: %s" % (shape, groups, tag, msg))
    _report(bad, len(injections))


def _sum_reference(t, dims):
    return lambda dtype: {"sum": t.to(dtype).sum(dims) if dims is not None else t.to(dtype).sum().reshape(1)}


@pytest.mark.parametrize("B,C,hw,view", [(3, 20, 35, False), (8, 6, 1024, True)])
def test_channel_sum_finaliser_follows_the_reference(B, C, hw, view):
    """locate_fin_channel_sums (bias gradients), unsliced and sliced: a special in g poisons exactly its channel's sum."""
    import test_gpu_finalisers as FIN
    bad, n = [], 0
    for place, idx in (("first", (0, 0, 0)), ("inner", (B // 2, C // 2, hw // 2 + 1)), ("last", (B - 1, C - 1, hw - 1))):
        for sname, val in M.SPECIALS.items():
            n += 1
            c = FIN.ChannelCase(B * 100 + C, B, C, hw, view)
            c.d_g[idx] = val
            c.g[idx] = val
            FIN.run("locate_fin_channel_sums", [c.record()])
            ref = _sum_reference(c.g, (0, 2))
            # the finaliser's own bound, 2e-6 of a channel's sum of magnitudes, restated for an error normalised by the largest sum
            w64 = ref(torch.float64)["sum"]
            ok = torch.isfinite(w64)
            tol = 2e-6 * float(c.g.double().abs().sum((0, 2))[ok].max()) / float(w64[ok].abs().max())
            msg = M.check_contract(c.out.cpu(), ref(torch.float32)["sum"], w64, tol)
            if msg:
                bad.append("channel sums %s g[%s]=%s: %s" % ((B, C, hw), place, sname, msg))
    _report(bad, n)


@pytest.mark.parametrize("per_plane", [False, True])
def test_sum_finaliser_follows_the_reference(per_plane):
    """locate_fin_sums over a gate workspace's block sums (dgamma): a special in one partial is a special in the sum."""
    import test_gpu_finalisers as FIN
    bad, n = [], 0
    for idx_name in ("first", "last"):
        for sname, val in M.SPECIALS.items():
            n += 1
            c = FIN.GateCase(33 + per_plane, (6, 33, 4, 4), per_plane)
            idx = 0 if idx_name == "first" else c.count - 1
            c.ws[idx] = val
            FIN.run("locate_fin_sums", [c.record()])
            ref = _sum_reference(c.ws[:c.count].cpu(), None)
            msg = M.check_contract(c.out.cpu(), ref(torch.float32)["sum"], ref(torch.float64)["sum"], 1e-6)
            if msg:
                bad.append("sums per_plane %d partial[%s]=%s: %s" % (per_plane, idx_name, sname, msg))
    _report(bad, n)


# ------------------------------------------------------------------------------------------------ one step of the small networks
class _GuardedOracleNadam:
    """The oracle's optimizer under the guarded step's rule: gradients with a non-finite element leave the state alone."""

    def __init__(self, inner):
        self.inner = inner

    def step(self, P, grads):
        if all(bool(torch.isfinite(g).all()) for g in grads.values()):
            self.inner.step(P, grads)


def _oracle_step_losses(z, latent, real, aug, dtype):
    from oracle import locate_oracle as O
    cfg = O.NetConfig(image_size=32, base_feature_factor=1)
    PG = O.make_params({k[len("G/sd0/"):]: z[k] for k in z.files if k.startswith("G/sd0/")}, dtype=dtype)
    PD = O.make_params({k[len("D/sd0/"):]: z[k] for k in z.files if k.startswith("D/sd0/")}, dtype=dtype)
    rec = O.train_step(PG, PD, torch.as_tensor(z["G/noise"]).to(dtype), _GuardedOracleNadam(O.Nadam(cfg.glr, (cfg.beta1, cfg.beta2))),
                       _GuardedOracleNadam(O.Nadam(cfg.dlr, (cfg.beta1, cfg.beta2))), latent.to(dtype), real.to(dtype), aug.to(dtype), cfg)
    return {k: rec[k].reshape(1) for k in ("d_error", "penalty", "g_error")}


STEP_PLACES = {"real": (1, 2, 5, 7), "latent": (2, 3)}


@pytest.mark.parametrize("special", ["nan", "+inf"])
@pytest.mark.parametrize("where", sorted(STEP_PLACES))
def test_a_special_in_a_step_input_is_seen_in_that_step(where, special):
    """32 x 32, base width 1, batch 4, batched spectral norm, guarded optimizers and the run statistics: a NaN or an Inf in one pixel
    of the real batch or in one latent element must set off a detector in that same step - the statistics' check raises, or an
    optimizer's verdict counts non-finite gradients, skips, and leaves its network's trained weights bit for bit - and the losses
    the step returns have the class of the oracle's step (its optimizers under the same skip rule) on the same inputs."""
    import test_gpu_guard as GUARD
    from conftest import load_golden
    from locate_amd import NonFiniteError, RunStatistics
    z = load_golden("g8_tiny_e2e")
    G, D, step, inputs = GUARD.build_tiny(GUARD.guarded_factory({"G": 0.0, "D": 0.0}))
    host = {k: torch.as_tensor(z["step1/" + k])[:4].clone() for k in ("latent", "real", "aug")}
    host[where][STEP_PLACES[where]] = M.SPECIALS[special]
    stats = RunStatistics(G, D, capacity=4)

    def trained(net):          # what the optimizer moves (u and v also advance with every forward's power iteration)
        return {k: p.detach().clone() for k, p in net.named_parameters() if not k.endswith(("weight_u", "weight_v"))}
    before = {"G": trained(G), "D": trained(D)}
    out = step(*(host[k].to(dev()) for k in ("latent", "real", "aug")))
    torch.cuda.synchronize()
    stats.record(1)
    raised = False
    try:
        stats.check()
    except NonFiniteError:
        raised = True
    skipped = []
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        c = opt.counters()
        if c["last_nonfinite"] > 0:
            after = trained(net)
            changed = [k for k in after if not torch.equal(after[k], before[tag][k])]
            assert c["skipped"] == 1 and not changed, "%s: non-finite gradients counted, but skipped %d and %s changed" % (tag, c["skipped"], changed[:3])
            skipped.append(tag)
    assert raised or skipped, "a %s in %s set off no detector: statistics clean, no verdict counted a non-finite gradient" % (special, where)
    got = {k: out[k].detach().cpu().reshape(1) for k in ("d_error", "penalty", "g_error")}
    want32 = _oracle_step_losses(z, host["latent"], host["real"], host["aug"], torch.float32)
    want64 = _oracle_step_losses(z, host["latent"], host["real"], host["aug"], torch.float64)
    bad = M.check_outputs(got, want32, want64, {"d_error": 1e-4, "penalty": 1e-4, "g_error": 1e-4})      # (the smoke run's bound)
    assert not bad, "%s in %s: %s" % (special, where, "; ".join(bad))


# ------------------------------------------------------------------------------------------------ the averaged generator
def _tiny_average():
    """the tiny fixture networks of tests/test_gpu_guard.py with an averaged generator over the live one"""
    import test_gpu_guard as GUARD
    from locate_amd import AveragedGenerator
    G, D, step, inputs = GUARD.build_tiny(GUARD.guarded_factory({"G": 0.0, "D": 0.0}))
    return G, D, AveragedGenerator(G, beta=0.75)


@pytest.mark.parametrize("special", ["nan", "+inf"])
def test_a_special_in_the_averaged_generators_latent_is_seen(special):
    """The third way into a step: one element of the latents the averaged generator is sampled with.  Nothing downstream of it is
    a weight or a gradient, so neither the run statistics nor an optimizer's verdict can see it; the detector that has to fire is
    the statistics kernel over the sampled batch (locate_amd.tensor_statistics, the kernel RunStatistics runs): its non-finite
    count must be positive.  And nothing is laundered on the way: the images have a non-finite value wherever the oracle's forward
    on the same weights has one (contractions on the path: an Inf may arrive as a NaN), finite ones within the step's 1e-4, and
    every weight of the averaged generator - the u / v its forward advances included - keeps the oracle's class."""
    from conftest import load_golden
    from locate_amd.stats import tensor_statistics
    from oracle import locate_oracle as O
    z = load_golden("g8_tiny_e2e")
    G, D, avg = _tiny_average()
    latent = torch.as_tensor(z["step1/latent"])[:4].clone()
    latent[STEP_PLACES["latent"]] = M.SPECIALS[special]
    with torch.no_grad():
        images = avg.generator(latent.to(dev()))
    _, _, nonfinite = tensor_statistics([images.contiguous()])
    assert int(nonfinite[0]) > 0, "a %s in the averaged generator's latent: the statistics of the sampled batch count no non-finite value" % special
    cfg = O.NetConfig(image_size=32, base_feature_factor=1)
    want, weights = {}, {}
    for dtype in (torch.float32, torch.float64):
        P = O.make_params({k[len("G/sd0/"):]: z[k] for k in z.files if k.startswith("G/sd0/")}, dtype=dtype)
        with torch.no_grad():
            want[dtype] = O.generator_forward(P, torch.as_tensor(z["G/noise"]).to(dtype), latent.to(dtype), cfg)
        weights[dtype] = {k: v.detach() for k, v in P.items()}
    msg = M.check_contract(images.cpu(), want[torch.float32], want[torch.float64], 1e-4, strict_class=False)
    assert msg is None, "sampled images: " + msg
    assert int((M.classify(want[torch.float64]) != M.FINITE).sum()) > 0
    got = {k: v.detach().cpu() for k, v in avg.generator.state_dict().items()}
    assert sorted(got) == sorted(weights[torch.float64])
    bad = []
    for k in sorted(got):
        msg = M.check_contract(got[k], weights[torch.float32][k], weights[torch.float64][k], 1e-4)
        if msg:
            bad.append("%s: %s" % (k, msg))
    assert not bad, "weights of the averaged generator after its forward: " + "; ".join(bad[:6])


@pytest.mark.parametrize("special", ["nan", "+inf", "-inf"])
def test_a_special_in_the_averaged_generators_update_is_seen(special):
    """... and one element of what update() reads, a live generator weight: the averaged element has the class of the host model
    (tests/helpers/average_model.py) in float32 and float64, every other element stays finite and within the model's bound, and
    the run statistics over the AVERAGED generator raise in that same step, naming the tensor."""
    import numpy as np
    import average_model as AM
    from locate_amd import NonFiniteError, RunStatistics
    G, D, avg = _tiny_average()
    name, live = next((n, p) for n, p in G.named_parameters() if n.endswith("weight_bar") and p.numel() > 16)
    with torch.no_grad():          # the live weights move, as after an optimizer step, and one element goes bad
        for p in G.parameters():
            p.mul_(1.25)
        live.view(-1)[11] = M.SPECIALS[special]
    before = {k: v.detach().cpu().numpy().copy() for k, v in avg.generator.state_dict().items()}
    source = {k: v.detach().cpu().numpy().copy() for k, v in G.state_dict().items()}
    avg.update()
    torch.cuda.synchronize()
    weight_of = {id(a): w for a, _, w in avg._pairs}
    bad = []
    for k, t in avg.generator.state_dict(keep_vars=True).items():
        w = weight_of[id(t)]
        want32, want64 = AM.update32(before[k], source[k], w), AM.update64(before[k].astype(np.float64), source[k], w)
        # the model's bound per unit of the largest expected magnitude (check_contract normalises by it): the operands reach 1.25 of it
        tol = AM.bound(1, w, 1.25) if w != 1.0 else 0.0
        msg = M.check_contract(t.detach().cpu(), torch.as_tensor(want32), torch.as_tensor(want64), tol)
        if msg:
            bad.append("%s: %s" % (k, msg))
    assert not bad, "; ".join(bad[:6])
    poisoned = dict(avg.generator.named_parameters())[name]
    assert int((~torch.isfinite(poisoned)).sum()) == 1
    stats = RunStatistics(avg.generator, D, capacity=2)
    stats.record(1)
    with pytest.raises(NonFiniteError) as info:
        stats.check()
    assert info.value.iteration == 1 and info.value.tensors == [("G/" + name, 1)]
