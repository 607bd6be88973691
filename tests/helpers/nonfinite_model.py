"""Host model of the non-finite contract: what a kernel may do with a NaN or an Inf that the reference keeps.

"Reference" is oracle/locate_oracle.py and ATen on the CPU, evaluated in float32 AND in float64; "class" is one of finite, NaN,
+Inf, -Inf.
  1. Nothing is laundered: where the reference's element is non-finite, ours is non-finite (stream kernels: the same class;
     contractions: any non-finite class - the bf16 split of an Inf is (Inf, NaN, NaN)).
  2. Nothing is finite and wrong: where the reference's element is finite, ours is within the operation's tolerance (error
     normalised by the largest FINITE expected magnitude) - or, only for the forms that scale by a largest-magnitude word and only
     under an Inf operand, non-finite.
The finite inputs are bounded (|x| <= 8, |g| <= 4) so that the two references agree on every element's class: the injected specials
are the only source of non-finite values and no position is ever left out of a comparison.

This file holds classify / inject / check_contract, the named places, and - shared by the CPU test of the references and the GPU
test of the kernels - the case lists of every operation with their reference in either precision."""
import math

import torch
import torch.nn.functional as F

from oracle import locate_oracle as O

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
CLASS_NAMES = ("finite", "NaN", "+Inf", "-Inf")
SPECIALS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
X_BOUND, G_BOUND = 8.0, 4.0


def classify(t):
    """int8 class code per element"""
    t = torch.as_tensor(t)
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isnan(t)] = NAN
    c[t == float("inf")] = PINF
    c[t == float("-inf")] = NINF
    return c


def inject(x, places, values):
    """A copy of x with values[k] (one value for all, if a scalar) written at places[k]: flat indices or index tuples."""
    out = x.clone()
    if not isinstance(values, (list, tuple)):
        values = [values] * len(places)
    assert len(values) == len(places)
    for p, v in zip(places, values):
        if isinstance(p, tuple):
            out[p] = v
        else:
            out.view(-1)[p] = v
    return out


def references_agree(want32, want64):
    """number of elements on whose class the float32 and the float64 reference disagree (the contract allows none)"""
    return int((classify(want32) != classify(want64)).sum())


def check_contract(got, want32, want64, tol, strict_class=True, allow_nonfinite_for_finite=False):
    """None if `got` keeps rules 1 and 2 against the two references, else a one-line description of the first offender."""
    got = torch.as_tensor(got).detach().cpu()
    want32, want64 = torch.as_tensor(want32).detach(), torch.as_tensor(want64).detach().double()
    if tuple(got.shape) != tuple(want64.shape) or tuple(want32.shape) != tuple(want64.shape):
        return "shape %s against the references' %s / %s" % (tuple(got.shape), tuple(want32.shape), tuple(want64.shape))
    cw, c32, cg = classify(want64).reshape(-1), classify(want32).reshape(-1), classify(got).reshape(-1)
    if bool((cw != c32).any()):
        i = int((cw != c32).nonzero()[0])
        raise AssertionError("the references disagree at flat index %d: float32 %s, float64 %s - the case is not admissible"
                             % (i, CLASS_NAMES[c32[i]], CLASS_NAMES[cw[i]]))
    g, w = got.double().reshape(-1), want64.reshape(-1)
    fin = cw == FINITE
    # rule 1
    bad = ~fin & ((cg != cw) if strict_class else (cg == FINITE))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        return "laundered: flat index %d is %s (%r) where the reference has %s; %d such element(s)" % (
            i, CLASS_NAMES[cg[i]], float(g[i]), CLASS_NAMES[cw[i]], int(bad.sum()))
    # rule 2
    if bool(fin.any()):
        nonfin_got = fin & (cg != FINITE)
        if not allow_nonfinite_for_finite and bool(nonfin_got.any()):
            i = int(nonfin_got.nonzero()[0])
            return "poisoned: flat index %d is %s where the reference has the finite %r; %d such element(s)" % (
                i, CLASS_NAMES[cg[i]], float(w[i]), int(nonfin_got.sum()))
        both = fin & (cg == FINITE)
        if bool(both.any()):
            scale = max(float(w[fin].abs().max()), 1e-30)
            err = torch.where(both, (g - w).abs(), torch.zeros_like(w)) / scale
            i = int(err.argmax())
            if not float(err[i]) <= tol:
                return "finite and wrong: flat index %d is %r, the reference has %r: normalised error %.3e > %.1e; %d such element(s)" % (
                    i, float(g[i]), float(w[i]), float(err[i]), tol, int((err > tol).sum()))
    return None


# ------------------------------------------------------------------------------------------------ named places
def vector_places(n):
    """flat positions of a stream of n floats processed as 16-byte vectors with a scalar tail"""
    p = {"first": 0, "last": n - 1}
    if n >= 8:
        p["body"] = 4 * (n // 8) + 1            # inside a full four-float vector, not at its edge
    if n % 4 and n > 4:
        p["tail"] = (n // 4) * 4                # the first element of the scalar tail
    return p


def plane_places(shape, b=None, c=None):
    """first and last element of the tensor and of one inner plane of an NCHW tensor (default: the last but one plane)"""
    B, C = shape[0], shape[1]
    hw = int(math.prod(shape[2:]))
    plane = (B * C - 2 if B * C > 1 else 0) if b is None else b * C + c
    p = {"first": 0, "last": B * C * hw - 1, "plane_first": plane * hw}
    if hw > 1:
        p["plane_last"] = plane * hw + hw - 1
    return p


def row_places(rows, n, row=None):
    """first / last element of one row (default: the middle one) and the element next to the lanes a row kernel pads"""
    r = rows // 2 if row is None else row
    p = {"row_first": r * n, "row_last": r * n + n - 1}
    q = ((n // 4) * 4 - 1) if n % 4 else n - 2      # last element of the last full vector / the one before the row's end
    if 0 < q < n - 1:
        p["pad_neighbour"] = r * n + q
    return p


def finite_values(shape, bound, seed):
    """uniform in [-bound, bound], float32, from a seed of its own"""
    gen = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound).float()


# ------------------------------------------------------------------------------------------------ case lists
class Case:
    """One injection: `inputs` (float32 tensors by name, the special already written), the family's configuration, an id."""
    __slots__ = ("family", "cfg", "inputs", "id")

    def __init__(self, family, cfg, inputs, id):
        self.family, self.cfg, self.inputs, self.id = family, cfg, inputs, id


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


def _single_injections(base, targets):
    """every (target tensor, named place, special) of a configuration, one at a time.  targets: {name: {place name: index}}"""
    for name, places in targets.items():
        for pname, idx in places.items():
            for sname, val in SPECIALS.items():
                inputs = dict(base)
                inputs[name] = inject(base[name], [idx], val)
                yield inputs, "%s[%s]=%s" % (name, pname, sname)


# --- RootTanh / tanh -------------------------------------------------------------------------------
ACT_SIZES = (7, 1027)            # tail only; vector body plus tail


def act_cases(kind):
    """kind: 'roottanh', 'tanh' (special in x, in g) or 'roottanh_acc' (the accumulating backward: special in the accumulator)"""
    for n in ACT_SIZES:
        base = {"x": finite_values((n,), X_BOUND, 10 + n), "g": finite_values((n,), G_BOUND, 20 + n)}
        if kind == "roottanh_acc":
            base["acc"] = finite_values((n,), G_BOUND, 30 + n)
            targets = {"acc": vector_places(n)}
        else:
            targets = {"x": vector_places(n), "g": vector_places(n)}
        for inputs, tag in _single_injections(base, targets):
            yield Case(kind, n, inputs, "%s n=%d %s" % (kind, n, tag))


def act_reference(case, dtype):
    x = _leaf(case.inputs["x"], dtype)
    y = torch.tanh(x) if case.family == "tanh" else O.root_tanh(x)
    y.backward(case.inputs["g"].to(dtype))
    dx = x.grad
    if case.family == "roottanh_acc":
        return {"dx": case.inputs["acc"].to(dtype) + dx}
    return {"y": y.detach(), "dx": dx}


ACT_TOL = {"roottanh": {"y": 2e-6, "dx": 3e-6}, "roottanh_acc": {"dx": 3e-6}, "tanh": {"y": 2e-6, "dx": 5e-6}}

ACT_ROWS = (3, 5, 7)             # rows, z, w of the style chain's concatenation


def act_rows_cases():
    rows, z, w = ACT_ROWS
    for with_add in (False, True):
        base = {"latent": finite_values((rows, z), X_BOUND, 41), "pre": finite_values((rows, w), X_BOUND, 42),
                "g": finite_values((rows, z + w), G_BOUND, 43)}
        targets = {"latent": {"first": 0, "last": rows * z - 1}, "pre": {"first": 0, "row_last": 2 * w - 1, "last": rows * w - 1},
                   "g": {"first": 0, "row_pre_first": (z + w) + z, "last": rows * (z + w) - 1}}
        if with_add:
            base["g_add"] = finite_values((rows, w, 1, 1), G_BOUND, 44)
            targets["g_add"] = {"first": 0, "last": rows * w - 1}
        for inputs, tag in _single_injections(base, targets):
            yield Case("act_rows", with_add, inputs, "act_rows g_add=%d %s" % (with_add, tag))


def act_rows_reference(case, dtype):
    latent, pre = _leaf(case.inputs["latent"], dtype), _leaf(case.inputs["pre"], dtype)
    out = torch.cat([latent, O.root_tanh(pre)], 1)
    outs, grads = [out], [case.inputs["g"].to(dtype)]
    if case.cfg:
        outs.append(pre.view(pre.shape[0], pre.shape[1], 1, 1) * 1)
        grads.append(case.inputs["g_add"].to(dtype))
    torch.autograd.backward(outs, grads)
    return {"out": out.detach(), "dlatent": latent.grad, "dpre": pre.grad}


ACT_ROWS_TOL = {"out": 2e-6, "dlatent": 1e-6, "dpre": 3e-6}

# --- in-place norm ---------------------------------------------------------------------------------
NORM_SHAPES = ((3, 5, 1, 1), (5, 7, 2, 4), (6, 33, 4, 4), (7, 13, 8, 8), (2, 9, 8, 16), (2, 3, 64, 64))


def norm_configs():
    for shape in NORM_SHAPES:
        for with_act in (False, True):
            for per_sample in (False, True):
                yield (shape, with_act, per_sample)


def norm_cases(cfg, scale_inf=False):
    """scale_inf = False: a special in x, in g, in the bias, a NaN in the scale.  scale_inf = True: the two Inf injections into the
    scale, a list of their own ("norm_scale_inf"): the reference multiplies the scale into every element BEFORE it sums a plane,
    so an infinite scale over a plane with gradients of both signs is a NaN there - what a kernel that sums the plane first and
    multiplies afterwards turns into an Inf."""
    shape, with_act, per_sample = cfg
    B, C = shape[:2]
    seed = 100 + sum(shape) + 2 * with_act + per_sample
    base = {"x": finite_values(shape, X_BOUND, seed), "scale": finite_values((B if per_sample else 1, C, 1, 1), 2.0, seed + 1),
            "bias": finite_values((1, C, 1, 1), 2.0, seed + 2), "g": finite_values(shape, G_BOUND, seed + 3)}
    pp = plane_places(shape)
    targets = {"x": {k: pp[k] for k in ("first", "plane_first") if k in pp}, "g": pp,
               "scale": {"last": base["scale"].numel() - 1}, "bias": {"first": 0}}
    for inputs, tag in _single_injections(base, targets):
        if (tag.startswith("scale[") and tag.endswith("inf")) == scale_inf:
            yield Case("norm", cfg, inputs, "norm %s act=%d per_sample=%d %s" % (shape, with_act, per_sample, tag))


def norm_reference(case, dtype):
    x, s, b = (_leaf(case.inputs[k], dtype) for k in ("x", "scale", "bias"))
    out = O.inplace_norm(x, s, b)
    if case.cfg[1]:
        out = O.root_tanh(out)
    out.backward(case.inputs["g"].to(dtype))
    # (the *_two_launch entries: the same gradients from the backward a training step runs, whose per-channel sums wait for the
    # end-of-pass finaliser)
    return {"out": out.detach(), "dx": x.grad, "dscale": s.grad, "dbias": b.grad,
            "dx_two_launch": x.grad, "dscale_two_launch": s.grad, "dbias_two_launch": b.grad}


NORM_TOL = {"out": 1e-5, "dx": 5e-5, "dscale": 5e-5, "dbias": 5e-5, "dx_two_launch": 5e-5, "dscale_two_launch": 5e-5, "dbias_two_launch": 5e-5}

# --- residual gate ---------------------------------------------------------------------------------
GATE_SHAPES = ((5, 7, 2, 2), (6, 33, 4, 4), (2, 9, 8, 16), (2, 4, 32, 32))


def gate_configs():
    for shape in GATE_SHAPES:
        for per_plane in (False, True):
            yield (shape, per_plane)


def gate_cases(cfg):
    shape, per_plane = cfg
    seed = 200 + sum(shape) + per_plane
    ashape = (shape[0], shape[1], 1, 1) if per_plane else shape
    base = {"x": finite_values(shape, X_BOUND, seed), "a": finite_values(ashape, 2.0, seed + 1), "gamma": torch.tensor([[3.0]]),
            "g": finite_values(shape, G_BOUND, seed + 2)}
    pp = plane_places(shape)
    ap = {"first": 0, "last": base["a"].numel() - 1, "inner": base["a"].numel() - 2} if per_plane else pp
    for inputs, tag in _single_injections(base, {"x": pp, "a": ap, "gamma": {"only": 0}, "g": pp}):
        yield Case("gate", cfg, inputs, "gate %s per_plane=%d %s" % (shape, per_plane, tag))


def gate_reference(case, dtype):
    x, a, gamma = (_leaf(case.inputs[k], dtype) for k in ("x", "a", "gamma"))
    out = O.residual_gate(x, a.expand_as(x), gamma)
    out.backward(case.inputs["g"].to(dtype))
    return {"out": out.detach(), "dx": x.grad, "da": a.grad, "dgamma": gamma.grad}


GATE_TOL = {"out": 1e-6, "dx": 1e-6, "da": 2e-5, "dgamma": 2e-5}

# --- softmax ---------------------------------------------------------------------------------------
SOFTMAX_ROWS = 3
SOFTMAX_SIZES = (3, 64, 192, 1000, 1028, 2500, 4094, 5000)


def softmax_cases(n):
    rows = SOFTMAX_ROWS
    base = {"x": finite_values((rows, n), X_BOUND, 300 + n), "g": finite_values((rows, n), G_BOUND, 301 + n)}
    rp = row_places(rows, n)
    for inputs, tag in _single_injections(base, {"x": rp, "g": rp}):
        yield Case("softmax", n, inputs, "softmax n=%d %s" % (n, tag))
    x = base["x"].clone()
    x[1] = float("-inf")
    yield Case("softmax", n, dict(base, x=x), "softmax n=%d row of -inf" % n)
    x = inject(base["x"], [n + 0, n + n - 1], float("inf"))
    yield Case("softmax", n, dict(base, x=x), "softmax n=%d two +inf in a row" % n)


def softmax_reference(case, dtype):
    x = _leaf(case.inputs["x"], dtype)
    y = torch.softmax(x, -1)
    y.backward(case.inputs["g"].to(dtype))
    return {"y": y.detach(), "dx": x.grad}


SOFTMAX_TOL = {"y": 2e-6, "dx": 2e-5}

# --- linear stencils -------------------------------------------------------------------------------
STENCIL_SHAPES = ((2, 3, 5, 7), (1, 2, 2, 2), (2, 3, 3, 16), (1, 1, 1, 8), (2, 4, 8, 8))
STENCIL_OPS = ("upsample", "avgpool", "pool_upsample", "feature_pool2", "feature_pool4", "cat", "add3", "fork3")


def stencil_applies(op, shape):
    B, C, H, W = shape
    if op == "avgpool":
        return H >= 2 and W >= 2
    if op in ("pool_upsample", "feature_pool2"):
        return C % 2 == 0
    if op == "feature_pool4":
        return C % 4 == 0
    return True


def stencil_configs():
    for op in STENCIL_OPS:
        for shape in STENCIL_SHAPES:
            if stencil_applies(op, shape):
                yield (op, shape)


def _stencil_forward(op, x):
    C = x.shape[1]
    if op == "upsample":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    if op == "avgpool":
        return F.avg_pool2d(x, 2, 2)
    if op == "pool_upsample":
        return F.interpolate(O.feature_pooling(x, C // 2), scale_factor=2, mode="bilinear", align_corners=False)
    if op == "feature_pool2":
        return O.feature_pooling(x, C // 2)
    if op == "feature_pool4":
        return O.feature_pooling(x, C // 4)
    raise ValueError(op)


def _with_inner_places(pp, H, W):
    """... plus an interior element and the corner's neighbours: a bilinear stencil clamped at the border gives them weight 0, and
    0 times a special is a NaN in ATen"""
    if H * W > 2:
        pp["interior"] = pp["plane_first"] + (H // 2) * W + W // 2
    if W > 1:
        pp["beside_corner"] = pp["plane_first"] + 1
    if H > 1:
        pp["below_corner"] = pp["plane_first"] + W
    return pp


def stencil_cases(cfg):
    op, shape = cfg
    B, C, H, W = shape
    seed = 400 + sum(shape) + STENCIL_OPS.index(op)
    pp = _with_inner_places(plane_places(shape), H, W)
    if op in ("add3", "fork3"):
        base = {k: finite_values(shape, G_BOUND, seed + i) for i, k in enumerate(("a", "b", "c"))}
        targets = {"a": pp, "b": {"plane_first": pp["plane_first"]}, "c": {"last": pp["last"]}}
    elif op == "cat":
        bshape = (B, C + 2, H, W)
        base = {"a": finite_values(shape, X_BOUND, seed), "b": finite_values(bshape, X_BOUND, seed + 1),
                "g": finite_values((B, 2 * C + 2, H, W), G_BOUND, seed + 2)}
        targets = {"a": pp, "b": plane_places(bshape), "g": plane_places((B, 2 * C + 2, H, W))}
    else:
        base = {"x": finite_values(shape, X_BOUND, seed)}
        gshape = tuple(_stencil_forward(op, base["x"]).shape)
        base["g"] = finite_values(gshape, G_BOUND, seed + 1)
        targets = {"x": pp, "g": _with_inner_places(plane_places(gshape), gshape[2], gshape[3])}
    for inputs, tag in _single_injections(base, targets):
        yield Case("stencil", cfg, inputs, "%s %s %s" % (op, shape, tag))


def stencil_reference(case, dtype):
    op = case.cfg[0]
    if op in ("add3", "fork3"):             # fork3's backward adds the three consumers' gradients: (norm + identity) + conv
        a, b, c = (case.inputs[k].to(dtype) for k in ("a", "b", "c"))
        return {"sum": (a + b) + c}
    if op == "cat":
        a, b = _leaf(case.inputs["a"], dtype), _leaf(case.inputs["b"], dtype)
        out = torch.cat([a, b], 1)
        out.backward(case.inputs["g"].to(dtype))
        return {"out": out.detach(), "da": a.grad, "db": b.grad}
    x = _leaf(case.inputs["x"], dtype)
    y = _stencil_forward(op, x)
    y.backward(case.inputs["g"].to(dtype))
    return {"y": y.detach(), "dx": x.grad}


STENCIL_TOL = {"y": 1e-6, "dx": 1e-6, "out": 0.0, "da": 0.0, "db": 0.0, "sum": 2e-7}

# --- loss glue -------------------------------------------------------------------------------------
LOSS_BATCHES = (8, 300)


def loss_cases(B):
    base = {"t": finite_values((B,), X_BOUND, 500 + B), "f": finite_values((B,), X_BOUND, 501 + B),
            "a": finite_values((B,), X_BOUND, 502 + B)}
    ends = {"first": 0, "last": B - 1}
    for inputs, tag in _single_injections(base, {"t": ends, "f": ends, "a": ends}):
        yield Case("loss", B, inputs, "loss B=%d %s" % (B, tag))


def loss_reference(case, dtype):
    t, f, a = (_leaf(case.inputs[k], dtype) for k in ("t", "f", "a"))
    d_err = (O.hinge(t) + O.hinge(-f)).mean()               # d_gen = -D(generated)
    pen = O.consistency_penalty(t, a)
    (d_err + pen).backward()
    f2 = _leaf(case.inputs["f"], dtype)
    g_err = O.hinge(f2).mean()
    g_err.backward()
    return {"d_losses": torch.stack([d_err, pen, d_err + pen]).detach(), "gt": t.grad, "gf": f.grad, "ga": a.grad,
            "g_loss": g_err.detach().reshape(1), "g_gf": f2.grad}


LOSS_TOL = {"d_losses": 2e-6, "gt": 1e-5, "gf": 1e-6, "ga": 1e-5, "g_loss": 2e-6, "g_gf": 1e-6}


# ------------------------------------------------------------------------------------------------ contractions
# One geometry per kernel family, taken from CONV_CASES / WINDOW_CASES / GROUPED_CASES of tests/test_gpu_ops.py:
# name: (mode, kind, cin, cout - for grouped layers the channel multiplier / group count -, k, stride, pad, B, H, W, window form)
CONTRACTIONS = {
    "gather": ("dense", "conv", 32, 32, 5, 2, 2, 3, 12, 12, False),                # regular forward, adjoint input gradient
    "gather_adjoint": ("dense", "convT", 64, 64, 4, 2, 1, 3, 2, 2, False),         # adjoint phases forward
    "window": ("dense", "conv", 64, 64, 5, 2, 2, 24, 8, 8, True),                  # WIN_MODE = 2
    "window_adjoint": ("dense", "convT", 64, 64, 4, 2, 1, 16, 4, 4, True),
    "pointwise_wgrad": ("dense", "conv", 24, 32, 1, 1, 0, 64, 6, 12, False),
    "pointwise_adjoint": ("dense", "convT", 96, 48, 1, 1, 0, 2, 8, 8, False),      # transposed 1x1: no padding anywhere
    "skinny": ("dense", "conv", 112, 48, 1, 1, 0, 64, 1, 1, False),                # 1x1 maps: skinny_rows / skinny_wgrad
    "one_pixel_wgrad": ("dense", "conv", 24, 160, 5, 2, 2, 6, 2, 2, False),
    "useful_taps": ("dense", "conv", 64, 64, 5, 2, 2, 6, 2, 2, False),             # 4 of 25 taps ever see data
    "split_k": ("dense", "conv", 260, 64, 3, 1, 1, 2, 8, 8, False),
    "dwconv": ("grouped", "conv", 20, 2, 5, 2, 2, 2, 9, 7, False),
    "dwconv_adjoint": ("grouped", "convT", 10, 1, 4, 2, 1, 1, 5, 3, False),
    "groupdot": ("grouped", "full", 6, 3, 5, 1, 0, 2, 5, 5, False),
}
CONTRACTION_TOL = {"y": 2e-5, "dx": 2e-5, "dw": 5e-5, "u": 1e-5}


def contraction_layer(name):
    """(the torch.nn layer that SpectralNorm wraps, its group count) - weights left at their seeded default initialisation"""
    mode, kind, cin, cout, k, s, p = CONTRACTIONS[name][:7]
    nn = torch.nn
    torch.manual_seed(600 + sorted(CONTRACTIONS).index(name))
    if mode == "dense":
        return (nn.Conv2d if kind == "conv" else nn.ConvTranspose2d)(cin, cout, k, stride=s, padding=p, bias=False), 1
    if kind == "conv":
        return nn.Conv2d(cin, cin * cout, k, stride=s, padding=p, bias=False, groups=cin), cin
    if kind == "convT":
        return nn.ConvTranspose2d(cin, cin * cout, k, stride=s, padding=p, bias=False, groups=cin), cin
    return nn.Conv2d(cin, cout, k, bias=False, groups=cout), cout


def _contraction_apply(name, x, w, groups):
    kind, s, p = CONTRACTIONS[name][1], CONTRACTIONS[name][5], CONTRACTIONS[name][6]
    if kind == "convT":
        return F.conv_transpose2d(x, w, None, s, p, groups=groups)
    return F.conv2d(x, w, None, s, p, groups=groups)


def _unit(n, seed):
    t = finite_values((n,), 1.0, seed).double()
    return (t / t.norm()).float()


def contraction_base(name):
    """the finite operands of a geometry: x, the incoming gradient g and the spectral-norm state (w = weight_bar, u, v)"""
    cfg = CONTRACTIONS[name]
    cin, B, H, W = cfg[2], cfg[7], cfg[8], cfg[9]
    layer, groups = contraction_layer(name)
    w = layer.weight.detach().clone()
    seed = 700 + 10 * sorted(CONTRACTIONS).index(name)
    x = finite_values((B, cin, H, W), X_BOUND, seed)
    gshape = tuple(_contraction_apply(name, x, w, groups).shape)
    return {"x": x, "g": finite_values(gshape, G_BOUND, seed + 1), "w": w, "u": _unit(w.shape[0], seed + 2),
            "v": _unit(w.numel() // w.shape[0], seed + 3)}


def _centre(shape):
    return tuple(n // 2 for n in shape)


def contraction_cases(name):
    """One special in x at an interior pixel, in x at a corner pixel (most of its taps see padding), in one weight, in g."""
    base = contraction_base(name)
    xs, gs, ws = tuple(base["x"].shape), tuple(base["g"].shape), tuple(base["w"].shape)
    targets = {"x": {"interior": _centre(xs), "corner": tuple(n - 1 for n in xs)}, "w": {"centre": _centre(ws)}, "g": {"interior": _centre(gs)}}
    if targets["x"]["interior"] == targets["x"]["corner"]:
        del targets["x"]["corner"]
    for inputs, tag in _single_injections(base, targets):
        yield Case("contraction", name, inputs, "%s %s" % (name, tag))


def contraction_state_dict(case):
    return {"module.weight_u": case.inputs["u"].clone(), "module.weight_v": case.inputs["v"].clone(),
            "module.weight_bar": case.inputs["w"].clone()}


def contraction_reference(case, dtype):
    """through the oracle's spectral norm (one power iteration, W_bar / sigma): y, dx, dW_bar and the advanced u"""
    _, groups = contraction_layer(case.cfg)
    P = O.make_params(contraction_state_dict(case), dtype=dtype)
    x = _leaf(case.inputs["x"], dtype)
    y = _contraction_apply(case.cfg, x, O.sn_weight(P, "module."), groups)
    y.backward(case.inputs["g"].to(dtype))
    return {"y": y.detach(), "dx": x.grad, "dw": P["module.weight_bar"].grad, "u": P["module.weight_u"].detach()}


FP8_CONTRACTIONS = ("gather", "pointwise_adjoint", "split_k")
FP8_TOL = {"y": 0.125, "dx": 0.125, "dw": 0.125, "u": 1e-5}          # 2 u, u = 2^-4: tests/test_gpu_fp8.py, one contraction


def special_of(case):
    """(name of the operand that holds the special, its class)"""
    for k, t in case.inputs.items():
        c = classify(t)
        if bool((c != FINITE).any()):
            return k, int(c[c != FINITE][0])
    raise ValueError("no special in " + case.id)


# ------------------------------------------------------------------------------------------------ spectral norm, finalisers
SN_SIZES = ((6, 100), (70, 1028), (5, 2048))      # narrow / wide rowdot, more than one column chunk, (un)aligned sn_row_partial
SN_TOL = {"u": 1e-5, "v": 1e-5, "wv": 1e-5, "sigma": 1e-5, "inv_sigma": 1e-5, "gw": 3e-5, "du": 1e-5, "dsigma": 1e-5, "dv": 1e-5}


def sn_power_reference(W, u, dtype, eps=1e-12):
    """one power iteration (spectral_norm.py:21-32) in `dtype`: the advanced u, v, sigma = u . W v, its inverse and W v"""
    W, u = W.to(dtype), u.to(dtype)
    t = W.t().mv(u)
    v = t / (t.norm() + eps)
    wv = W.mv(v)
    u2 = wv / (wv.norm() + eps)
    sigma = u2.dot(wv).reshape(1)
    return {"u": u2, "v": v, "wv": wv, "sigma": sigma, "inv_sigma": 1 / sigma}


def sn_rank1_reference(gw_in, partial, u, v, sigma, wv, dtype):
    """one call's rank-1 record: dsigma = -sum(partial) / sigma^2, du = dsigma wv, gw = gw_in + dsigma u v^T"""
    gw_in, partial, u, v, wv = (t.to(dtype) for t in (gw_in, partial, u, v, wv))
    sigma = torch.as_tensor(sigma).to(dtype)
    total = -partial.sum() / (sigma * sigma)
    return {"gw": gw_in + total * torch.outer(u, v), "du": total * wv, "dsigma": total.reshape(1)}


def sn_dv_reference(W, u, slots, dtype):
    """dv = (sum of the layer's dsigma slots) W^T u"""
    W, u, slots = W.to(dtype), u.to(dtype), slots.to(dtype)
    return {"dv": slots.sum() * W.t().mv(u)}


def sn_places(h, wd):
    """(row, column) places of a special in W, and the places in u: first, last, an inner one"""
    return ({"first": (0, 0), "inner": (h // 2, wd // 2 + 1), "last": (h - 1, wd - 1)}, {"first": 0, "inner": h // 2, "last": h - 1})


# ------------------------------------------------------------------------------------------------ the stream families
# family -> (configurations, cases of one configuration, reference, tolerances)
STREAM_FAMILIES = {
    "roottanh": (lambda: ["roottanh"], act_cases, act_reference, ACT_TOL["roottanh"]),
    "tanh": (lambda: ["tanh"], act_cases, act_reference, ACT_TOL["tanh"]),
    "roottanh_acc": (lambda: ["roottanh_acc"], act_cases, act_reference, ACT_TOL["roottanh_acc"]),
    "act_rows": (lambda: [None], lambda _: act_rows_cases(), act_rows_reference, ACT_ROWS_TOL),
    "norm": (lambda: list(norm_configs()), norm_cases, norm_reference, NORM_TOL),
    "norm_scale_inf": (lambda: list(norm_configs()), lambda cfg: norm_cases(cfg, True), norm_reference, NORM_TOL),
    "gate": (lambda: list(gate_configs()), gate_cases, gate_reference, GATE_TOL),
    "softmax": (lambda: list(SOFTMAX_SIZES), softmax_cases, softmax_reference, SOFTMAX_TOL),
    "stencil": (lambda: list(stencil_configs()), stencil_cases, stencil_reference, STENCIL_TOL),
    "loss": (lambda: list(LOSS_BATCHES), loss_cases, loss_reference, LOSS_TOL),
}


def stream_configs():
    """[(family, configuration)] of every stream-kernel case list"""
    return [(fam, cfg) for fam, (configs, _, _, _) in STREAM_FAMILIES.items() for cfg in configs()]


def both_references(family, case):
    """(float32 reference, float64 reference) of a case, as dicts of tensors by output name"""
    ref = STREAM_FAMILIES[family][2]
    return ref(case, torch.float32), ref(case, torch.float64)


def check_outputs(got, want32, want64, tols, strict_class=True, allow_nonfinite_for_finite=False):
    """check_contract over a dict of outputs: the list of 'name: offender' lines (empty when the contract holds)"""
    assert set(got) == set(want64) == set(want32), (sorted(got), sorted(want64))
    bad = []
    for k in sorted(want64):
        msg = check_contract(got[k], want32[k], want64[k], tols[k], strict_class, allow_nonfinite_for_finite)
        if msg:
            bad.append("%s: %s" % (k, msg))
    return bad
