"""The gate backward kernels with an incoming-gradient term (locate_gate_bwd_term) against the launches they replace.

A gate's output out = (gamma a + 1) x feeds the next gate and a norm (or the output head's RootTanh).  The folded form leaves that
consumer's element-wise backward - the norm's dx pass, the RootTanh derivative - to the gate's own backward kernel, which recomputes
`out` and forms the value with the same operations in the same order.  So every comparison here is BITWISE (int32 / int64 views:
NaN payloads count): the folded call against locate_norm_bwd_fused (or locate_roottanh_bwd) followed by locate_gate_bwd on the same
inputs, and a module's gradients with the fold on against LOCATE_GATE_FOLD=0's launches.

Needs an MI355X: run with -m gpu.  Shapes are the smallest that reach each kernel variant (planes of 1 ... 4096 elements)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def S():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(a, b, what, ctx):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "%s differs (%d of %d words) in %s" % (
        what, int((bits(a) != bits(b)).sum()), a.numel(), ctx)


def _buf(n, off, gen=None, fill=None):
    """n floats, `off` floats past a 16-byte boundary"""
    base = torch.empty(n + off, device=dev())
    t = base[off:]
    if gen is not None:
        t.copy_(torch.randn(n, generator=gen).to(dev()))
    elif fill is not None:
        t.fill_(fill)
    return t


def _p(t):
    return None if t is None else t.data_ptr()


class Seam:
    """One gate -> (norm | RootTanh) seam's operands: x, a, gamma of the producing gate, its stored output, the consumer's incoming
    gradient go and the other consumer's share."""

    def __init__(self, B, C, hw, groups=1, a_pp=0, act=0, per_sample=0, has_share=1, acc=0, off=0, seed=0):
        from locate_amd._lib import check, lib
        L = lib()
        gen = torch.Generator().manual_seed(1000 + seed)
        self.cfg = dict(B=B, C=C, hw=hw, groups=groups, a_pp=a_pp, act=act, per_sample=per_sample, has_share=has_share, acc=acc, off=off)
        self.B, self.C, self.hw, self.groups, self.a_pp, self.act = B, C, hw, groups, a_pp, act
        self.per_sample, self.has_share, self.acc, self.off = per_sample, has_share, acc, off
        planes = B * C
        n = planes * hw
        self.planes, self.n = planes, n
        self.x = _buf(n, off, gen)
        self.a = _buf(planes if a_pp else n, off, gen)
        self.gamma = _buf(1, off, gen)
        self.go = _buf(n, off, gen)
        self.share = _buf(n, off, gen)
        self.dx0 = _buf(n, off, gen)
        self.scale = _buf(planes if per_sample else C, off, gen)
        self.bias = _buf(C, off, gen)
        self.stats = _buf(2 * groups, off)
        self.out = _buf(n, off)
        self.L, self.check = L, check

    def forward(self):
        L, check = self.L, self.check
        check(L.locate_gate_fwd(_p(self.x), _p(self.a), self.a_pp, _p(self.gamma), _p(self.out), self.planes, self.hw, S()), "gate_fwd")
        ws = torch.empty(L.locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=dev())
        out, stats = self.out.clone(), self.stats.clone()          # (the forward wants 16-byte aligned tensors; the statistics are the same)
        y = torch.empty_like(out)
        check(L.locate_norm_fwd(_p(out), _p(self.scale), self.per_sample, _p(self.bias), _p(y), self.act, _p(stats), self.B,
                                self.C, self.hw, self.groups, _p(ws), None, None, S()), "norm_fwd")
        self.stats.copy_(stats)

    def _gate_outputs(self):
        L = self.L
        dx = _buf(self.n, self.off)
        dx.copy_(self.dx0)
        da = _buf(self.a.numel(), self.off, fill=float("nan"))
        wsg = torch.zeros(L.locate_gate_bwd_workspace_bytes(self.planes) // 8, dtype=torch.float64, device=dev())
        amax = torch.zeros(L.locate_absmax_words(), dtype=torch.int32, device=dev())
        return dx, da, wsg, amax

    def _norm_ws(self):
        L = self.L
        ws = torch.zeros(L.locate_norm_bwd_fused_workspace_bytes(self.B, self.C), dtype=torch.uint8, device=dev())
        dss = torch.full((self.planes,), float("nan"), device=dev()) if self.per_sample else None
        return ws, dss

    def _collect(self, dx, da, wsg, amax, ws=None, dss=None):
        L = self.L
        got = {"dx_skip": dx, "da": da, "dgamma partials": wsg[:L.locate_gate_bwd_partials(self.planes, self.hw)], "absmax words": amax}
        if ws is not None:
            o = L.locate_norm_bwd_fused_plane_offset()
            got["S1/S2"] = ws[o:o + 8 * self.planes].view(torch.float32)
            got["group partials"] = ws[:16 * 4 * L.locate_norm_bwd_fused_partials(self.B, self.C)].view(torch.float64)
        if dss is not None:
            got["dscale (per sample)"] = dss
        return got

    def pair_norm(self):
        """locate_norm_bwd_fused into the fork buffer, then locate_gate_bwd reading it"""
        L, check = self.L, self.check
        buf = _buf(self.n, self.off, fill=float("nan"))
        if self.has_share:
            buf.copy_(self.share)
        ws, dss = self._norm_ws()
        check(L.locate_norm_bwd_fused(_p(self.out), _p(self.go), _p(self.stats), _p(self.scale), self.per_sample, _p(self.bias), self.act,
                                      _p(buf), _p(dss), self.B, self.C, self.hw, self.groups, _p(ws), self.has_share, S()), "norm_bwd_fused")
        dx, da, wsg, amax = self._gate_outputs()
        check(L.locate_gate_bwd(_p(self.x), _p(self.a), self.a_pp, _p(self.gamma), _p(buf), _p(dx), _p(da), None, self.planes, self.hw,
                                _p(wsg), self.acc, _p(amax), S()), "gate_bwd")
        return self._collect(dx, da, wsg, amax, ws, dss)

    def folded_norm(self):
        from locate_amd._lib import GateTerm
        L, check = self.L, self.check
        buf = _buf(self.n, self.off, fill=float("nan"))          # without a share the buffer must not be read: NaNs would show
        if self.has_share:
            buf.copy_(self.share)
        ws, dss = self._norm_ws()
        check(L.locate_norm_bwd_planes(_p(self.out), _p(self.go), _p(self.stats), _p(self.scale), self.per_sample, _p(self.bias), self.act,
                                       _p(dss), self.B, self.C, self.hw, self.groups, _p(ws), S()), "norm_bwd_planes")
        term = GateTerm(kind=GateTerm.NORM, with_act=self.act, per_sample=self.per_sample, has_share=self.has_share, go=_p(self.go),
                        stats=_p(self.stats), scale=_p(self.scale), bias=_p(self.bias), partial=_p(ws),
                        npartial=L.locate_norm_bwd_fused_partials(self.B, self.C), B=self.B, C=self.C, groups=self.groups)
        dx, da, wsg, amax = self._gate_outputs()
        check(L.locate_gate_bwd_term(_p(self.x), _p(self.a), self.a_pp, _p(self.gamma), _p(buf), _p(dx), _p(da), None, self.planes,
                                     self.hw, _p(wsg), self.acc, _p(amax), term, S()), "gate_bwd_term")
        if self.has_share:
            same(buf, self.share, "the share (read-only)", self.cfg)
        return self._collect(dx, da, wsg, amax, ws, dss)

    def pair_roottanh(self):
        L, check = self.L, self.check
        gx = torch.full((self.n,), float("nan"), device=dev())
        out, go = self.out.clone(), self.go.clone()          # (locate_roottanh_bwd wants 16-byte aligned operands)
        check(L.locate_roottanh_bwd(_p(out), _p(go), _p(gx), self.n, 0, None, S()), "roottanh_bwd")
        g = _buf(self.n, self.off)
        g.copy_(gx)
        dx, da, wsg, amax = self._gate_outputs()
        check(L.locate_gate_bwd(_p(self.x), _p(self.a), self.a_pp, _p(self.gamma), _p(g), _p(dx), _p(da), None, self.planes, self.hw,
                                _p(wsg), self.acc, _p(amax), S()), "gate_bwd")
        return self._collect(dx, da, wsg, amax)

    def folded_roottanh(self):
        from locate_amd._lib import GateTerm
        L, check = self.L, self.check
        dx, da, wsg, amax = self._gate_outputs()
        check(L.locate_gate_bwd_term(_p(self.x), _p(self.a), self.a_pp, _p(self.gamma), _p(self.go), _p(dx), _p(da), None, self.planes,
                                     self.hw, _p(wsg), self.acc, _p(amax), GateTerm(kind=GateTerm.ROOTTANH), S()), "gate_bwd_term")
        return self._collect(dx, da, wsg, amax)


def compare(want, got, ctx):
    assert set(want) == set(got)
    for k in want:
        same(got[k], want[k], k, ctx)


HWS = [1, 4, 16, 64, 128, 100, 256, 1024, 4096]


def _abi_cases():
    """~40 combinations that take every value of every axis (not the full product): the plane size walks HWS while the flags count
    through their bit patterns (9 sizes against powers of two: every size meets every flag value) and B, C, groups rotate."""
    cases = []
    for k in range(36):
        hw = HWS[k % 9]
        B, C = (4, 8)[(k // 9 + k) % 2], (3, 5)[(k // 2) % 2]
        if hw == 1:
            B, C = ((8, 24), (4, 48))[(k // 9) % 2]          # planes a multiple of 64 (the map re-read as planes of 64), C wraps inside a wave
        cases.append(dict(B=B, C=C, hw=hw, groups=(1, 2, 4)[(k + k // 9) % 3], a_pp=k & 1, act=(k >> 1) & 1, per_sample=(k >> 2) & 1,
                          has_share=(k >> 3) & 1, acc=(k >> 4) & 1, seed=k))
    cases.append(dict(B=4, C=3, hw=1, groups=1, a_pp=1, act=1, per_sample=1, has_share=1, acc=1, seed=36))      # 1x1, planes % 64 != 0
    cases.append(dict(B=8, C=5, hw=64, groups=2, a_pp=0, act=1, per_sample=1, has_share=1, acc=1, off=1, seed=37))      # unaligned: scalar paths
    cases.append(dict(B=4, C=3, hw=1024, groups=4, a_pp=1, act=0, per_sample=0, has_share=1, acc=0, off=1, seed=38))
    cases.append(dict(B=8, C=8, hw=1, groups=2, a_pp=0, act=1, per_sample=1, has_share=1, acc=0, off=1, seed=39))       # 1x1 re-read, unaligned
    return cases


def _id(c):
    return "-".join("%s%s" % (k, v) for k, v in c.items() if k != "seed")


@pytest.mark.parametrize("cfg", _abi_cases(), ids=_id)
def test_norm_term_matches_the_two_calls(cfg):
    s = Seam(**cfg)
    s.forward()
    compare(s.pair_norm(), s.folded_norm(), cfg)


@pytest.mark.parametrize("hw", HWS)
def test_roottanh_term_matches_the_two_calls(hw):
    for k, (B, C) in enumerate(((8, 24), (4, 5)) if hw == 1 else ((4, 3), (8, 5))):
        cfg = dict(B=B, C=C, hw=hw, a_pp=k, acc=1 - k, seed=50 + k)
        s = Seam(**cfg)
        s.forward()
        compare(s.pair_roottanh(), s.folded_roottanh(), cfg)
    s = Seam(B=4, C=3, hw=hw, a_pp=1, acc=1, off=1, seed=52)
    s.forward()
    compare(s.pair_roottanh(), s.folded_roottanh(), s.cfg)


SPECIALS = {"inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}


@pytest.mark.parametrize("hw", [4, 64, 256, 1024])
@pytest.mark.parametrize("value", list(SPECIALS))
@pytest.mark.parametrize("where", ["gamma", "scale", "go", "share"])
def test_nonfinite_operands_keep_the_pair_s_bits(where, value, hw):
    """A special value in gamma, the norm's scale, its incoming gradient or the other consumer's share: the folded form's words are
    the unfolded pair's, the per-plane da under a non-finite gamma (gate_plane_da_nonfinite's walk) included.  Every combination
    runs; all offenders are reported.

    gamma = nan is the sharp case: the gate's multiplier (gamma a + 1) and the incoming gradient are then BOTH NaNs, of opposite
    sign (the norm's dx negates its mean term), and the multiplier instruction returns the first NaN operand it meets - so
    dx_skip's sign bit (0xFFC00000 against 0x7FC00000) follows the operand ORDER of one product, which the term kernels pin to
    the order of the kernels that read g (gate_mul_g_first, csrc/elementwise.hip)."""
    v = SPECIALS[value]
    bad = []
    k = 0
    for a_pp in (0, 1):
        for act in (0, 1):
            cfg = dict(B=4, C=3, hw=hw, groups=2, a_pp=a_pp, act=act, per_sample=k & 1, has_share=1, acc=(k >> 1) & 1, seed=100 + k)
            k += 1
            s = Seam(**cfg)
            t = getattr(s, where)
            if where in ("go", "share"):
                t[::max(1, t.numel() // 7)] = v          # a few elements, in several planes
                t[1] = -v
            else:
                t[0] = v
            s.forward()          # (the stored output and the statistics see a special gamma, like a training step's would)
            runs = [("norm", s.pair_norm, s.folded_norm)]
            if where in ("gamma", "go"):
                runs.append(("roottanh", s.pair_roottanh, s.folded_roottanh))
            for term, pair, folded in runs:
                want, got = pair(), folded()
                for key in want:
                    if not torch.equal(bits(want[key]), bits(got[key])):
                        bad.append("%s term, a_pp %d act %d: %s differs in %d of %d words (e.g. %#x against %#x)" % (
                            term, a_pp, act, key, int((bits(want[key]) != bits(got[key])).sum()), want[key].numel(),
                            int(bits(want[key]).flatten()[(bits(want[key]) != bits(got[key])).flatten().nonzero()[0, 0]]) & 0xFFFFFFFF,
                            int(bits(got[key]).flatten()[(bits(want[key]) != bits(got[key])).flatten().nonzero()[0, 0]]) & 0xFFFFFFFF))
    print("\n".join(bad))
    assert not bad, "%d output(s) differ from the unfolded pair:\n%s" % (len(bad), "\n".join(bad))


# ------------------------------------------------------------------------------------------------ the Python layer's hand-over
def _adopt(mod, rt):
    from locate_amd.nn import _Bound
    for m in mod.modules():
        if isinstance(m, _Bound):
            object.__setattr__(m, "runtime", rt)


def _grads(build, run, fold):
    """parameter and input gradients of one forward / backward of a freshly built (seeded) module, fold on or off"""
    from locate_amd import ops
    prev, ops.GATE_FOLD[0] = ops.GATE_FOLD[0], fold
    prev_min, ops.GATE_FOLD_ACT_MIN_NUMEL[0] = ops.GATE_FOLD_ACT_MIN_NUMEL[0], 0          # (the size gate is a speed matter: tiny maps here)
    try:
        torch.manual_seed(7)
        mod, x = build()
        rt = ops.Runtime()
        _adopt(mod, rt)
        rt.reset()
        launches = run(mod, x, rt)
        torch.cuda.synchronize()
        got = {"x": x.grad}
        got.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
        return got, launches
    finally:
        ops.GATE_FOLD[0] = prev
        ops.GATE_FOLD_ACT_MIN_NUMEL[0] = prev_min


def _count(monkeypatch_target, names):
    """counts the calls of the named C entries made through lib()"""
    counts = dict.fromkeys(names, 0)
    originals = {n: getattr(monkeypatch_target, n) for n in names}

    def wrap(n):
        def call(*a):
            counts[n] += 1
            return originals[n](*a)
        return call
    return counts, {n: wrap(n) for n in names}, originals


ENTRIES = ("locate_gate_bwd_term", "locate_norm_bwd_planes", "locate_norm_bwd_fused", "locate_roottanh_bwd")


def _run_counted(fn):
    from locate_amd._lib import lib
    L = lib()
    counts, wrapped, originals = _count(L, ENTRIES)
    for n, w in wrapped.items():
        setattr(L, n, w)
    try:
        fn()
    finally:
        for n, o in originals.items():
            setattr(L, n, o)
    return counts


def _module_case(build, stacked):
    def run(mod, x, rt):
        def go():
            with rt.stacked_calls(stacked):
                y = mod(x)
            y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(dev()))
        return _run_counted(go)
    want, base = _grads(build, run, False)
    got, folded = _grads(build, run, True)
    assert base["locate_gate_bwd_term"] == 0 and base["locate_norm_bwd_planes"] == 0
    assert set(want) == set(got)
    for k in want:
        same(got[k], want[k], k, "stacked %d" % stacked)
    return base, folded


@pytest.mark.parametrize("stacked", [1, 3])
def test_chained_seams_fold_on_equals_fold_off(stacked):
    """three chained ResModule(identity, Norm(...)) gates: two seams whose norm dx pass moves into the producing gate's kernel"""
    from locate_amd.nn import Norm, ResModule, RootTanhModule, _identity

    def build():
        mod = torch.nn.Sequential(*[ResModule(_identity, Norm(5, RootTanhModule())) for _ in range(3)]).to(dev())
        for p in mod.parameters():
            p.data.add_(0.1 * torch.randn_like(p))
        return mod, torch.randn(6, 5, 16, 16, device=dev(), requires_grad=True)
    base, folded = _module_case(build, stacked)
    assert folded["locate_gate_bwd_term"] == 2 and folded["locate_norm_bwd_planes"] == 2
    assert folded["locate_norm_bwd_fused"] == base["locate_norm_bwd_fused"] - 2


@pytest.mark.parametrize("stacked", [1, 3])
def test_attention_block_fold_on_equals_fold_off(stacked):
    from locate_amd import Block, NetConfig

    def build():
        blk = Block(8, 16, 8, 2, True, 0, cfg=NetConfig()).to(dev())
        assert blk.attention
        return blk, torch.randn(6, 16, 4, 4, device=dev(), requires_grad=True)          # -> [6, 8, 8, 8]
    base, folded = _module_case(build, stacked)
    assert folded["locate_gate_bwd_term"] == 2          # res_module_i -> res_module_f -> res_module_s: two seams
    assert folded["locate_norm_bwd_fused"] == base["locate_norm_bwd_fused"] - 2


def _seam_by_hand(norm_first, extra_consumer=False, grad_of_out=False, head=False):
    """gate -> fork -> (next gate's skip input | norm) with the forward order chosen so that autograd runs the norm's backward
    before (norm_first) or after the skip consumer's: the later node of the forward runs first."""
    from locate_amd import ops
    rt = ops.Runtime()
    rt.reset()
    gen = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev()).requires_grad_(True)      # noqa: E731
    x, a1, a2, g1, g2, sc, bi = r(4, 3, 8, 8), r(4, 3, 8, 8), r(4, 3, 8, 8), r(1, 1), r(1, 1), r(1, 3, 1, 1), r(1, 3, 1, 1)
    leaves = [x, a1, a2, g1, g2, sc, bi]
    out = ops.residual_gate(x, a1, g1, rt)
    if head:
        y = ops.root_tanh(out)
        (y * y).sum().backward()
        return [t.grad for t in (x, a1, g1)]
    skip, feed = ops.fork(out)
    if norm_first:
        nxt = ops.residual_gate(skip, a2, g2, rt)
        nrm = ops.inplace_norm(feed, sc, bi, False, rt)
    else:
        nrm = ops.inplace_norm(feed, sc, bi, False, rt)
        nxt = ops.residual_gate(skip, a2, g2, rt)
    loss = (nxt * nxt).sum() + (nrm * nrm * nrm).sum()
    if extra_consumer:
        loss = loss + (out * 2.0).sum()
    if grad_of_out:
        return torch.autograd.grad(loss, [out])
    loss.backward()
    return [t.grad for t in leaves]


@pytest.mark.parametrize("norm_first", [False, True])
def test_either_backward_order_gives_the_same_bits(norm_first):
    from locate_amd import ops

    def run(fold):
        prev, ops.GATE_FOLD[0] = ops.GATE_FOLD[0], fold
        try:
            box = []
            counts = _run_counted(lambda: box.append(_seam_by_hand(norm_first)))
            return box[0], counts
        finally:
            ops.GATE_FOLD[0] = prev
    want, base = run(False)
    got, folded = run(True)
    assert base["locate_gate_bwd_term"] == 0 and folded["locate_gate_bwd_term"] == 1 and folded["locate_norm_bwd_fused"] == 0
    for i, (w, g) in enumerate(zip(want, got)):
        same(g, w, "gradient %d" % i, "norm first" if norm_first else "skip consumer first")


def test_output_head_roottanh_folds_with_the_same_bits():
    from locate_amd import ops

    def run(fold):
        prev, ops.GATE_FOLD[0] = ops.GATE_FOLD[0], fold
        try:
            box = []
            counts = _run_counted(lambda: box.append(_seam_by_hand(False, head=True)))
            return box[0], counts
        finally:
            ops.GATE_FOLD[0] = prev
    want, base = run(False)
    got, folded = run(True)
    assert base["locate_roottanh_bwd"] == 1 and folded["locate_roottanh_bwd"] == 0 and folded["locate_gate_bwd_term"] == 1
    for i, (w, g) in enumerate(zip(want, got)):
        same(g, w, "gradient %d" % i, "head")


def test_a_third_consumer_of_the_gate_output_raises():
    """autograd then sums the handed-over buffer with the third gradient: what reaches the gate is not the record's buffer"""
    from locate_amd import ops
    assert ops.GATE_FOLD[0]
    with pytest.raises(RuntimeError, match="gate fold: the gradient that reached the gate"):
        _seam_by_hand(False, extra_consumer=True)


def test_a_record_left_over_raises():
    """a pass that ends in front of the gate (the gradient w.r.t. the gate's OUTPUT): the norm's record is never taken"""
    from locate_amd import ops
    assert ops.GATE_FOLD[0]
    with pytest.raises(RuntimeError, match="gate fold: 1 consumer"):
        _seam_by_hand(False, grad_of_out=True)
