"""The contractions (csrc/conv.hip, convwin.hip, convwgrad.hip, grouped.hip, convfp8.hip) on the operands a training step really
hands them: channel slices of wider tensors (CatChannelsFn.backward returns g[:, :ca] and g[:, ca:] as views; sn_conv(out=buf[:, c:])
writes into a slice of the concatenation buffer) and weight-gradient homes packed back to back in one flat buffer
(GradAllReducer.make_homes: after a 1-element gate gamma every later gw is only 4-byte aligned).  tests/test_gpu_ops.py hands the
same kernels fresh, dense, 16-byte aligned allocations only, so the pointer and batch-stride half of every launcher predicate is
always true there.

The contract under test (include/locate_hip.h, above locate_conv_fwd): a contraction's results depend on the elements of its own
operands only, and it writes the elements of its own outputs only, wherever those lie.

Operands live in sentinel-filled buffers (tests/helpers/placed_operands.py): a slice view's neighbouring channels, the images
between, the guard words around the parent - all the quiet NaN 0x7FC0BEEF.  A neighbour read against a zero weight gives NaN
(0 x NaN), a store outside the view changes a sentinel, an element never stored keeps the second payload 0x7FC0DEAD.  Every case
asserts, against a float64 CPU convolution of dense copies (F.conv2d / F.conv_transpose2d, torch.autograd.grad; sigma = 1,
u = v = 0, so dw is the raw gradient):
  (a) y and dx within 2e-5, dw within 5e-5 normalised max error - the bounds of test_gpu_ops.py::test_conv_igemm_vs_cpu - no NaN;
  (b) every sentinel word intact, inputs unchanged;
  (c) where the placed call and the call on dense aligned copies run the same kernel (no predicate mentions what changed):
      bit-equal results.
Each case's comment cites the launcher condition it was derived from; where the library answers a query about the route
(locate_conv_win_ok, ops.WIN_CALLS / F16_CALLS / FP8_CALLS, the workspace and partial sizes, locate_wgrad_batch_record) the test
asserts the answer.

Defects this file found (each reverted -> the named test fails):
  * groupdot_fwd_kernel took its 16-byte loads on L % 4 == 0 and x_bs % 4 == 0 alone - a 4-byte aligned x (a channel slice that
    starts on an odd element) got 16-byte loads at that address.  The pointer clause is now part of the predicate:
    test_groupdot_forward_bodies (the offset call must equal the scalar body's bits).
  * ops._raw_weight_grad forwarded a 4-byte aligned operand, or one with a batch stride that is no multiple of 4, into
    locate_conv_wgrad's narrow 1x1 route and 192-row plan, which refuse it (status 1): the operator raised.  It now asks
    locate_conv_wgrad_operand_align and copies once: test_operator_accepts_what_the_weight_gradient_routes_refuse,
    test_pointwise_stream_clauses (odd x batch stride).

Needs an MI355X: run with -m gpu."""
import ctypes
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT, assert_close

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from placed_operands import (SENTINEL, UNWRITTEN, bits, conv_ref64, dev, intact, offset_out, offset_view,  # noqa: E402
                             slice_out, slice_view, written)

pytestmark = pytest.mark.gpu

TOL_Y, TOL_DX, TOL_DW = 2e-5, 2e-5, 5e-5          # test_conv_igemm_vs_cpu's bounds for the same three quantities


def S():
    return torch.cuda.current_stream().cuda_stream


def L():
    from locate_amd._lib import lib
    return lib()


def call(name, *args):
    from locate_amd._lib import check
    check(getattr(L(), name)(*args), name)


def status(name, *args):
    """the raw status of an entry point (1 = refused argument) and the library's message"""
    st = getattr(L(), name)(*args)
    msg = L().locate_last_error()
    return st, (msg.decode() if msg else "")


class P:
    """Where an operand lies: behind c0 channels of a parent that has `extra` more channels after it and `pad` more words per
    image, the parent `off` words past a 16-byte boundary.  bs = (m, r): the batch stride must be = r mod m; at = (a, r): the address = r mod a
    bytes - the predicate the case is about, asserted by the helper."""

    def __init__(self, c0=0, extra=0, off=0, pad=0, bs=None, at=None):
        self.c0, self.extra, self.off, self.pad, self.bs, self.at = c0, extra, off, pad, bs, at

    def view(self, values):
        return slice_view(values, self.c0, self.c0 + values.shape[1] + self.extra, self.off, self.pad, self.bs, self.at)

    def out(self, shape):
        return slice_out(shape, self.c0, self.c0 + shape[1] + self.extra, self.off, self.pad, self.bs, self.at)


def _out_shape(kind, xshape, wshape, s, p, groups):
    B, _, H, W = xshape
    kh, kw = wshape[2], wshape[3]
    if kind == "convT":
        return (B, wshape[1] * groups, (H - 1) * s - 2 * p + kh, (W - 1) * s - 2 * p + kw)
    return (B, wshape[0], (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1)


@functools.lru_cache(maxsize=None)
def _operands(kind, cin, cout, k, s, p, B, H, W, form="bf16x3", groups=1):
    """Seeded operands of a layer and its float64 reference - computed once per geometry, shared by every placement, never changed.
    groups > 1: depthwise (groups = cin, cout = cin x multiplier) or, kind "full", a grouped conv whose kernel is the whole map."""
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + k + B)
    if groups == 1:
        wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    elif kind == "full":
        wshape = (cout, cin // cout, H, W)
    elif kind == "conv":
        wshape = (cout, 1, k, k)
    else:
        wshape = (cin, cout // cin, k, k)
    rk = "conv" if kind == "full" else kind
    fan = wshape[1] * wshape[2] * wshape[3] if rk == "conv" else (wshape[0] // groups) * k * k
    oshape = _out_shape(rk, (B, cin, H, W), wshape, s, p, groups)
    if form == "fp8":          # integers in [-15, 15]: e4m3 numbers, exact products and sums
        x = torch.randint(-15, 16, (B, cin, H, W), generator=gen).float()
        w = torch.randint(-15, 16, wshape, generator=gen).float()
        g = torch.randint(-15, 16, oshape, generator=gen).float()
    else:
        x = torch.randn(B, cin, H, W, generator=gen) * (3.0 if form == "f16x2" else 1.0)
        w = torch.randn(wshape, generator=gen) / float(max(fan, 1)) ** 0.5
        g = torch.randn(oshape, generator=gen) * (1e-4 if form == "f16x2" else 1.0)
    return x, w, g, conv_ref64(rk, s, p, x, w, g, groups)


class Tap:
    """ops.CONTRACTION_TAP: what every dense contraction was handed (address and batch stride of its operands)"""

    def __init__(self):
        self.seen = {}

    def __call__(self, role, w, a, b, forward_of_r):
        self.seen[role] = tuple((t.data_ptr(), t.stride(0)) for t in (a, b) if t is not None)


def _layer(ops, kind, k, s, p, x, w, g, out=None, precision=0, tag=False, mode="dense", defer=False, home=None):
    """Forward, input gradient and weight gradient through SNConvFn with sigma = 1 and u = v = 0 (no rank-1 term: dw is G), on the
    tensors AS GIVEN (views are not copied here).  Returns device tensors (y, dx, dw)."""
    rt = ops.Runtime()
    rt.precision = precision
    rt.defer_finalisers = defer
    wg = torch.nn.Parameter(w.to(dev())) if defer else w.to(dev()).requires_grad_(True)
    if home is not None:
        wg.__dict__["_locate_grad_buf"] = home
    if tag:
        ops.tag_amax(x)
        ops.tag_amax(g)
    xg = x.requires_grad_(True)
    h = w.shape[0]
    u, v = torch.zeros(h, device=dev()), torch.zeros(w.numel() // h, device=dev())
    sigma, wv = torch.tensor([1.0, 1.0], device=dev()), torch.zeros(h, device=dev())
    ops.reset_backward_state(rt)
    y = ops.SNConvFn.apply(xg, wg, u, v, None, sigma, wv, ops.ConvSpec(kind, k, k, s, p, p, mode), rt, None,
                           None if out is None else [out])
    y.backward(g)
    torch.cuda.synchronize()
    return y.detach(), xg.grad, wg.grad


def _check(got, ref, what):
    for name, tol, a, b in zip(("y", "dx", "dw"), (TOL_Y, TOL_DX, TOL_DW), got, ref):
        assert not bool(torch.isnan(a).any()), "%s: %s holds a NaN" % (what, name)
        assert_close(a.cpu().reshape(b.shape), b, tol, "%s: %s" % (what, name))


def _same(got, dense, names, what):
    for name, a, b in zip(("y", "dx", "dw"), got, dense):
        if name in names:
            assert torch.equal(bits(a), bits(b)), "%s: %s differs from the call on dense aligned copies" % (what, name)


# ====================================================================================================== forward and input gradient
# name: (geometry, x, gy, y placements, results that equal the dense call's bit for bit, form, counters)
DENSE_CASES = {
    # Gather kernels (conv_igemm_bx6_kernel<.., 3>), 32-row tile, split-K: no clause of launch_igemm mentions a pointer or a stride
    # once skinny_ok / pointwise_ok / the window form are out (H x W = 9 x 7, five taps), so y and dx equal the dense call's.  The
    # 63-word plane makes an odd batch stride (23 x 63) and a 4-byte start (63 words) reachable; the gather reads the whole strided
    # extent through one buffer descriptor (run_igemm: p.in_bytes), so only masks keep the neighbours out.  dw: pairs_ok
    # (convwgrad.hip, locate_conv_wgrad: gy 8-byte aligned, even gy_bs) is false for gy 84 bytes in - conv_wgrad_kernel, not the dense
    # call's conv_wgrad_bx6_kernel.
    "gather-odd-plane": (("conv", 20, 33, 5, 2, 2, 3, 9, 7), P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 2, 1, 0, (4, 0), (8, 4)),
                         P(2, 1, 3, 0, None, (8, 4)), ("y", "dx"), "bf16x3", True),
    # ... the same operands in the two-piece fp16 form (launch_bx6<2>, conv_wgrad_bx6_kernel<.., 2> / conv_wgrad_kernel)
    "gather-odd-plane-f16": (("conv", 20, 33, 5, 2, 2, 3, 9, 7), P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 2, 1, 0, (4, 0), (8, 4)),
                             P(2, 1, 3, 0, None, (8, 4)), ("y", "dx"), "f16x2", True),
    # Four-phase adjoint (conv_plan, adjoint: one phase per sub-pixel) on a 15-word plane: odd stride 43 x 15, start 15 words.  The
    # weight gradient's gout is x here (5 x 3 maps: (OH * OW) & 1 - pairs_ok false by geometry): the same kernel either way.
    "four-phase-adjoint": (("convT", 40, 24, 4, 2, 1, 2, 5, 3), P(1, 2, 0, 0, (2, 1), (8, 4)), P(2, 1, 1, 0, None, (8, 4)),
                           P(1, 2, 1, 0, None, (8, 4)), ("y", "dx", "dw"), "bf16x3", True),
    "four-phase-adjoint-f16": (("convT", 40, 24, 4, 2, 1, 2, 5, 3), P(1, 2, 0, 0, (2, 1), (8, 4)), P(2, 1, 1, 0, None, (8, 4)),
                               P(1, 2, 1, 0, None, (8, 4)), ("y", "dx", "dw"), "f16x2", True),
    # Split-K with the in-launch combine (igemm_split_plan: counters, ks x tile <= 512 KiB: K = 288, nine splits of a 96-row tile)
    # and the output in a slice; 49-word planes.  OW = 7: the weight gradient is conv_wgrad_kernel for every placement.
    "splitk-combine": (("conv", 32, 72, 3, 1, 1, 3, 7, 7), P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 1, 0, 0, (2, 0), (8, 4)),
                       P(3, 1, 0, 0, None, (8, 4)), ("y", "dx", "dw"), "bf16x3", True),
    # ... without counters: the partial tiles go to output-shaped slabs, igemm_slab_reduce_kernel writes the slice (out_bs)
    "splitk-reduce-kernel": (("conv", 32, 72, 3, 1, 1, 3, 7, 7), P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 1, 0, 0, (2, 0), (8, 4)),
                             P(3, 1, 0, 0, None, (8, 4)), ("y", "dx", "dw"), "bf16x3", False),
    # Split count capped at 64 (K = 2340): 64 x 32 KiB of partial tiles exceed the combine's 512 KiB, so the reduction kernel runs
    # with counters too.  gy is 16-byte aligned on an 8 x 8 map: pairs_ok holds as in the dense call (conv_wgrad_bx6_kernel, two slabs).
    "splitk-capped": (("conv", 260, 64, 3, 1, 1, 2, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)),
                      P(2, 1, 0, 0, None, (16, 0)), ("y", "dx", "dw"), "bf16x3", True),
    # 1x1 maps (skinny_ok: skinny_rows_kernel; skinny_wgrad_kernel): x is a column slice of a wider [B, 121] matrix - odd row
    # stride, start 3 words in; the ragged last chunk of the reduction (112 = 3.5 x 32) ends where the neighbour's columns begin
    "rows": (("conv", 112, 48, 1, 1, 0, 5, 1, 1), P(3, 5, 0, 1, (2, 1), (8, 4)), P(2, 3, 0, 0, (2, 1), (16, 8)),
             P(1, 2, 0, 0, (2, 1), (8, 4)), ("y", "dx", "dw"), "bf16x3", True),
    # Tall 192-row tile (igemm_bm: M % 192 == 0 and 512 column tiles of 128 = 16 x 64 x 64 pixels; M > 64 keeps it off the stream
    # kernel), K not split (workspace 0).  Every operand starts on an odd word.  dw: M = 192 but one tile (R = 8): not the 192-row
    # plan; gy is 8-byte aligned (2 words in): pairs_ok as in the dense call, 342 slabs under slab_reduce_kernel<16>.
    "tall-192": (("conv", 8, 192, 1, 1, 0, 16, 64, 64), P(1, 1, 1, 0, None, (8, 4)), P(0, 1, 2, 0, (2, 0), (16, 8)),
                 P(1, 1, 1, 0, None, (8, 4)), ("y", "dx", "dw"), "bf16x3", True),
    # fp8 operands (convfp8.hip: the same tiling and split plan, its own gathers) on integers in [-15, 15]: exact, compared with
    # torch.equal.  12 x 12 maps; x and y start on an odd word.
    "fp8-exact": (("conv", 32, 32, 5, 2, 2, 3, 12, 12), P(1, 1, 1, 0, None, (8, 4)), P(1, 2, 0, 0, None, (16, 0)),
                  P(2, 1, 1, 0, None, (8, 4)), ("y", "dx", "dw"), "fp8", True),
}


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_forward_and_gradients_on_channel_slices(name, monkeypatch):
    from locate_amd import ops
    geometry, px, pg, py, same, form, counters = DENSE_CASES[name]
    kind, cin, cout, k, s, p, B, H, W = geometry
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0 if form == "f16x2" else 1e30)
    if not counters:
        monkeypatch.setattr(ops, "_counters", lambda owner, adjoint: None)
    ops._WIN_CACHE.clear()
    x0, w0, g0, ref = _operands(*geometry, form=form)
    precision = 3 if form == "fp8" else 0
    # the split-K plan the case was written for (test_gpu_amax.py reads it the same way)
    garr = ops._geom(ops.ConvSpec(kind, k, k, s, p, p).geometry(tuple(x0.shape), tuple(w0.shape))[0])
    ws = (L().locate_conv_fwd_workspace_bytes if kind == "conv" else L().locate_conv_dgrad_workspace_bytes)(garr)
    if name.startswith("splitk-combine") or name == "splitk-reduce-kernel":
        assert ws > 0 and ws % (4 * ref[0].numel()) != 0, "not the in-launch combine's slab size"
    if name == "splitk-capped":
        assert ws == 64 * 4 * ref[0].numel(), "not 64 output-shaped slabs"
    if name in ("rows", "tall-192"):
        assert ws == 0
    xs, gs, ys = px.view(x0), pg.view(g0), py.out(tuple(ref[0].shape))
    tap = Tap()
    monkeypatch.setattr(ops, "CONTRACTION_TAP", tap)
    before = (dict(ops.F16_CALLS), ops.FP8_CALLS[0], ops.WIN_CALLS[0])
    got = _layer(ops, kind, k, s, p, xs, w0, gs, ys, precision, form == "f16x2")
    monkeypatch.setattr(ops, "CONTRACTION_TAP", None)
    # the views reached the launches as they are
    assert got[0].data_ptr() == ys.data_ptr() and got[0].stride() == ys.stride()
    assert tap.seen["fwd"] == ((xs.data_ptr(), xs.stride(0)),) and tap.seen["dgrad"] == ((gs.data_ptr(), gs.stride(0)),)
    assert tap.seen["wgrad"] == ((xs.data_ptr(), xs.stride(0)), (gs.data_ptr(), gs.stride(0)))
    if form == "f16x2":
        assert all(ops.F16_CALLS[kk] == before[0][kk] + 1 for kk in ("fwd", "dgrad", "wgrad")), (before[0], ops.F16_CALLS)
    else:
        assert ops.F16_CALLS == before[0]
    assert ops.FP8_CALLS[0] - before[1] == (2 if form == "fp8" else 0) and ops.WIN_CALLS[0] == before[2]
    intact(xs, gs, ys)
    written(ys)
    if form == "fp8":
        for what, a, b in zip(("y", "dx", "dw"), got, ref):
            assert torch.equal(a.cpu().double(), b), "%s: fp8 %s is not exact" % (name, what)
    else:
        _check(got, ref, name)
    dense = _layer(ops, kind, k, s, p, x0.to(dev()), w0, g0.to(dev()), None, precision, form == "f16x2")
    _same(got, dense, same, name)


# ---- pointwise stream --------------------------------------------------------------------------------------------------------
# conv 6 -> 3, 1x1, B 32, 64 x 64: B * HW = 131072, the threshold of pointwise_ok (conv.hip).  Its pointer clauses:
#   (p.in_bs & 1) == 0, (p.out_bs & 1) == 0, in 8-byte aligned, out 8-byte aligned
# (act_out / mul_pre are null here).  Forward: in = x, out = y; input gradient: in = gy, out = dx (a fresh allocation).
# A plane of 4096 words keeps every channel slice even and aligned, so the odd strides come from a row pad of one word and the
# 4-byte starts from the parent's offset.  The weight gradient of this geometry takes the narrow 1x1 route (pw_plan), which refuses
# such x / gy: ops._raw_weight_grad copies them (every placement below but the first).
POINTWISE = ("conv", 6, 3, 1, 1, 0, 32, 64, 64)
POINTWISE_PLACEMENTS = {
    # name: (x, gy, y, launches that fall back to the gather kernels)
    "all-true": (P(1, 1, 0, 0, (2, 0), (16, 0)), P(1, 1, 4, 0, (2, 0), (16, 0)), P(2, 2, 2, 0, (2, 0), (16, 8)), ()),
    "odd-in-stride": (P(1, 1, 0, 1, (2, 1), (16, 0)), P(1, 1, 0, 1, (2, 1), (16, 0)), P(2, 2, 0, 0, (2, 0), (16, 0)), ("y", "dx")),
    "odd-out-stride": (P(1, 1, 0, 0, (2, 0), (16, 0)), P(1, 1, 0, 0, (2, 0), (16, 0)), P(2, 2, 0, 1, (2, 1), (16, 0)), ("y",)),
    "in-4-byte": (P(1, 1, 1, 0, (2, 0), (8, 4)), P(1, 1, 3, 0, (2, 0), (8, 4)), P(2, 2, 0, 0, (2, 0), (16, 0)), ("y", "dx")),
    "out-4-byte": (P(1, 1, 0, 0, (2, 0), (16, 0)), P(1, 1, 0, 0, (2, 0), (16, 0)), P(2, 2, 1, 0, (2, 0), (8, 4)), ("y",)),
}


def test_pointwise_stream_clauses(monkeypatch):
    """Every clause of pointwise_ok true (conv_pointwise_kernel<16, 1>: equal to the dense call bit for bit), then one clause false
    per launch: the gather kernels take over, and since none of THEIR predicates mentions a pointer, all fall-back results of one
    direction are the same bits."""
    from locate_amd import ops
    kind, cin, cout, k, s, p, B, H, W = POINTWISE
    assert B * H * W == 131072
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 1e30)
    x0, w0, g0, ref = _operands(*POINTWISE)
    garr = ops._geom(ops.ConvSpec(kind, k, k, s, p, p).geometry(tuple(x0.shape), tuple(w0.shape))[0])
    assert L().locate_conv_wgrad_operand_align(garr, 0) == 16 and L().locate_conv_wgrad_operand_align(garr, 1) == 16
    dense = _layer(ops, kind, k, s, p, x0.to(dev()), w0, g0.to(dev()))
    _check(dense, ref, "pointwise, dense")
    fallback = {}
    for name, (px, pg, py, falls) in POINTWISE_PLACEMENTS.items():
        xs, gs, ys = px.view(x0), pg.view(g0), py.out(tuple(ref[0].shape))
        got = _layer(ops, kind, k, s, p, xs, w0, gs, ys)
        intact(xs, gs, ys)
        written(ys)
        _check(got, ref, "pointwise, " + name)
        stream = tuple(n for n in ("y", "dx") if n not in falls)
        _same(got, dense, stream, "pointwise, " + name)
        for n, t in zip(("y", "dx"), got):
            if n in falls:
                first = fallback.setdefault(n, (name, bits(t)))
                assert torch.equal(bits(t), first[1]), "pointwise fall-back %s: %s differs from %s" % (n, name, first[0])
    assert set(fallback) == {"y", "dx"}


# ---- window form ---------------------------------------------------------------------------------------------------------------
# locate_conv_win_ok (conv.hip): (x_bs & 1) || (x & 7) -> 0; run_igemm refuses the window flag for such a tensor, so ops._win_ok
# must not set it.  WIN_MODE = 2 as test_conv_window_form_vs_cpu sets it.  Per geometry: which launches (the layer's forward, its
# input gradient) have the form in the three-piece format when the operand is aligned.
WINDOW_GEOMS = {
    "convT4x4s2": (("convT", 64, 64, 4, 2, 1, 16, 4, 4), (1, 0)),        # 2x2-tap phases (adjoint panel); R's forward has no bf16x3 window
    "conv5x5s2": (("conv", 32, 32, 5, 2, 2, 6, 32, 32), (1, 1)),         # de-interleaved stride-2 window columns; both directions
    # single tap, THREE 8-channel groups under four per stage: the padded group's window chunks are read against zero weights -
    # with x as channels 1 .. 24 of a 28-channel parent those chunks are the parent's NaN channels (or the next image's)
    "convT1x1-3groups": (("convT", 24, 12, 1, 1, 0, 8, 16, 16), (1, 0)),
}
WINDOW_PLACEMENTS = {
    # name: (x, gy, expected window launches as a mask over (forward, input gradient))
    "aligned": (P(1, 3, 0, 0, (2, 0), (8, 0)), P(2, 1, 2, 0, (2, 0), (8, 0)), (1, 1)),
    "odd-word": (P(1, 3, 1, 0, (2, 0), (8, 4)), P(2, 1, 1, 0, (2, 0), (8, 4)), (0, 0)),
    "odd-stride": (P(1, 3, 0, 1, (2, 1), (8, 0)), P(2, 1, 0, 1, (2, 1), (8, 0)), (0, 0)),
}


@pytest.mark.parametrize("placement", list(WINDOW_PLACEMENTS))
@pytest.mark.parametrize("geom", list(WINDOW_GEOMS))
def test_window_form_on_channel_slices(geom, placement, monkeypatch):
    from locate_amd import ops
    geometry, has = WINDOW_GEOMS[geom]
    kind, cin, cout, k, s, p, B, H, W = geometry
    px, pg, takes = WINDOW_PLACEMENTS[placement]
    monkeypatch.setattr(ops, "WIN_MODE", 2)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 1e30)
    ops._WIN_CACHE.clear()
    x0, w0, g0, ref = _operands(*geometry)
    xs, gs = px.view(x0), pg.view(g0)
    ys = P(1, 1, 0, 0).out(tuple(ref[0].shape))
    garr = ops._geom(ops.ConvSpec(kind, k, k, s, p, p).geometry(tuple(x0.shape), tuple(w0.shape))[0])
    fwd_adj = 0 if kind == "conv" else 1
    expect = (has[0] * takes[0], has[1] * takes[1])
    answers = (int(L().locate_conv_win_ok(garr, fwd_adj, xs.stride(0), xs.data_ptr()) > 0),
               int(L().locate_conv_win_ok(garr, 1 - fwd_adj, gs.stride(0), gs.data_ptr()) > 0))
    assert answers == expect, "locate_conv_win_ok answers %s for this placement, the case expects %s" % (answers, expect)
    before = ops.WIN_CALLS[0]
    got = _layer(ops, kind, k, s, p, xs, w0, gs, ys)
    assert ops.WIN_CALLS[0] - before == sum(expect), "window launches: %d, expected %d" % (ops.WIN_CALLS[0] - before, sum(expect))
    intact(xs, gs, ys)
    written(ys)
    _check(got, ref, "%s, %s" % (geom, placement))
    if placement == "aligned":          # the same window kernels as on dense copies: no other clause looks at the operands
        dense = _layer(ops, kind, k, s, p, x0.to(dev()), w0, g0.to(dev()))
        _same(got, dense, ("y", "dx"), "%s, aligned" % geom)
    ops._WIN_CACHE.clear()


def test_window_form_f16_pieces_on_a_slice(monkeypatch):
    """The two-piece window of the transposed 4x4 stride-2 layer exists in BOTH directions (test_conv_window_form_vs_cpu): forward
    and input gradient through it on aligned slices, the tag riding on the views."""
    from locate_amd import ops
    geometry = WINDOW_GEOMS["convT4x4s2"][0]
    kind, cin, cout, k, s, p, B, H, W = geometry
    monkeypatch.setattr(ops, "WIN_MODE", 2)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    ops._WIN_CACHE.clear()
    x0, w0, g0, ref = _operands(*geometry, form="f16x2")
    px, pg, _ = WINDOW_PLACEMENTS["aligned"]
    xs, gs, ys = px.view(x0), pg.view(g0), P(1, 1, 0, 0).out(tuple(ref[0].shape))
    before = (ops.WIN_CALLS[0], dict(ops.F16_CALLS))
    got = _layer(ops, kind, k, s, p, xs, w0, gs, ys, 0, True)
    assert ops.WIN_CALLS[0] == before[0] + 2 and all(ops.F16_CALLS[kk] == before[1][kk] + 1 for kk in ("fwd", "dgrad"))
    intact(xs, gs, ys)
    written(ys)
    _check(got, ref, "convT4x4s2, f16 pieces")
    ops._WIN_CACHE.clear()


# ---- grouped -------------------------------------------------------------------------------------------------------------------
# dwconv_kernel / dw_wgrad_kernel (grouped.hip) are scalar throughout: no pointer clause, so every result equals the dense call's.
# groupdot_fwd_kernel: 16-byte loads where L % 4 == 0, x_bs % 4 == 0 and x, w are 16-byte aligned; locate_groupdot_dgrad and
# _wgrad are scalar (ops hands them a contiguous gy).
GROUPED_VIEW_CASES = {
    # name: ((kind, cin, cout, k, s, p, B, H, W), groups, mode, x, gy)
    "depthwise-mult2-odd": (("conv", 20, 40, 5, 2, 2, 2, 9, 7), 20, "depthwise", P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 2, 1, 0, None, (8, 4))),
    "depthwiseT-odd": (("convT", 10, 10, 4, 2, 1, 1, 5, 3), 10, "depthwise", P(1, 2, 0, 0, None, (8, 4)), P(1, 1, 1, 0, None, (8, 4))),
    "groupdot-L50": (("full", 6, 3, 5, 1, 0, 2, 5, 5), 3, "groupdot", P(1, 1, 0, 0, None, (8, 4)), P(1, 1, 0, 0, None, (8, 4))),
    # L = 64, batch stride 14 x 16: both multiples of 4 - and x 4 bytes past a 16-byte boundary
    "groupdot-L64-x-off": (("full", 12, 3, 4, 1, 0, 3, 4, 4), 3, "groupdot", P(1, 1, 1, 0, (4, 0), (16, 4)), P(0, 0, 1, 0, None, (8, 4))),
}


@pytest.mark.parametrize("name", list(GROUPED_VIEW_CASES))
def test_grouped_convs_on_channel_slices(name):
    from locate_amd import ops
    geometry, groups, mode, px, pg = GROUPED_VIEW_CASES[name]
    kind, cin, cout, k, s, p, B, H, W = geometry
    x0, w0, g0, ref = _operands(*geometry, groups=groups)
    xs, gs = px.view(x0), pg.view(g0)
    lk = "conv" if kind == "full" else kind
    got = _layer(ops, lk, k, s, p, xs, w0, gs, None, 0, False, mode)
    intact(xs, gs)
    _check(got, ref, name)
    dense = _layer(ops, lk, k, s, p, x0.to(dev()), w0, g0.to(dev()), None, 0, False, mode)
    # (the offset group dot runs the scalar body, the dense call the 16-byte one: y is held to float64 only)
    _same(got, dense, ("dx", "dw") if name == "groupdot-L64-x-off" else ("y", "dx", "dw"), name)


def test_groupdot_forward_bodies():
    """groupdot_fwd_kernel through the C ABI, L = 1024 (four channels of a 16 x 16 map per group): the 16-byte body for an aligned
    x with x_bs % 4 == 0 - bit for bit the call on a dense copy - and the scalar body for every x that fails ONE clause: x_bs % 4
    != 0, x 4 bytes off, x 8 bytes off.  The scalar runs see the same elements in the same order: equal bits, which a 16-byte load
    at a 4-byte aligned address (what the kernel issued before the pointer clause existed) would not give - the two bodies sum in
    different orders."""
    B, G, Ln = 3, 3, 1024
    gen = torch.Generator().manual_seed(77)
    x0 = torch.randn(B, G * Ln, 1, 1, generator=gen)
    w0 = torch.randn(G, Ln, generator=gen) / 32.0
    want = torch.einsum("bgl,gl->bg", x0.double().reshape(B, G, Ln), w0.double())
    w = w0.to(dev())

    def run(x):
        y = offset_out((B, G), 1)
        call("locate_groupdot_fwd", x.data_ptr(), x.stride(0), w.data_ptr(), None, 0, 0, y.data_ptr(), B, G, Ln, S())
        intact(x, y)
        written(y)
        assert_close(y.cpu(), want, TOL_Y, "group dot")
        return bits(y)
    dense = run(offset_view(x0, 0))
    assert torch.equal(run(slice_view(x0, 4, G * Ln + 8, 0, 0, (4, 0), (16, 0))), dense), "16-byte body on a slice"
    scalar = [run(slice_view(x0, 4, G * Ln + 8, 0, 1, (4, 1), (16, 0))),          # stride clause
              run(slice_view(x0, 4, G * Ln + 8, 1, 0, (4, 0), (16, 4))),          # pointer clause, 4 bytes off
              run(slice_view(x0, 4, G * Ln + 8, 2, 0, (4, 0), (16, 8)))]          # ... 8 bytes off
    assert torch.equal(scalar[1], scalar[0]) and torch.equal(scalar[2], scalar[0]), "a 4- or 8-byte aligned x did not take the scalar body"


# ====================================================================================================== weight gradient, C ABI
def _geom_of(ops, cin, cout, k, s, p, B, H, W):
    spec = ops.ConvSpec("conv", k, k, s, p, p)
    geom, out_shape = spec.geometry((B, cin, H, W), (cout, cin, k, k))
    return geom, (ctypes.c_int * 12)(*geom), out_shape


# name: (cin, cout, k, s, p, B, H, W), x, gy, (slabs, batch-record blocks > 0), why
# slabs: locate_conv_wgrad_workspace_bytes / (4 n); with n = M C KH KW it fixes the reduction form (wgrad_reduce_zp: 16 for >= 64
# slabs under n < 4096, 4 for >= 16 slabs, else 1) and, with n % 4 and the alignment of gw, its vector or scalar body
# (slab_reduce_body: (n & 3) == 0 && ((slab | out) & 15) == 0; ZP = 16 is always scalar).
WGRAD_CASES = {
    # WG_MAP1X1 (skinny_wgrad_ok): skinny_wgrad_body<8>, scalar stores; x a column slice with an odd row stride
    "map1x1": ((100, 7, 1, 1, 0, 5, 1, 1), P(3, 5, 0, 1, (2, 1), (8, 4)), P(1, 1, 0, 0, (2, 1), (8, 4)), (1, True)),
    # WG_ONEPIX (onepix_wgrad_ok), M >= 128: skinny_wgrad_wide.  2 x 2 input: 64 % hw == 0 and row lengths % 4 == 0, so the rows are
    # staged in LDS and streamed out with 16-byte stores IF gw is 16-byte aligned (`staged`), scattered 4-byte stores + skw_zero_taps
    # otherwise
    "onepix-staged": ((24, 160, 5, 2, 2, 6, 2, 2), P(1, 1, 1, 0, None, (8, 4)), P(1, 2, 0, 0, (2, 1), (8, 4)), (1, True)),
    # ... 3 x 3 input: 64 % 9 != 0 - scattered stores for every gw
    "onepix-scattered": ((16, 130, 4, 2, 1, 4, 3, 3), P(1, 1, 0, 0, None, (8, 4)), P(1, 2, 0, 0, (2, 1), (8, 4)), (1, True)),
    # WG_POINTWISE (pw_plan): 16-byte fragment loads - x, gy 16-byte aligned, strides % 4 == 0 (required: refusal test below);
    # 16 slabs, n = 4000: slab_reduce_kernel<4>, vector body for an aligned gw
    "pointwise": ((40, 100, 1, 1, 0, 8, 32, 32), P(1, 1, 0, 0, (4, 0), (16, 0)), P(2, 1, 4, 0, (4, 0), (16, 0)), (16, False)),
    # WG_TILED, direct launch (nsplit == 1): wgrad_epilogue's scalar stores into gw; odd maps: conv_wgrad_kernel
    "tiled-direct": ((20, 33, 5, 2, 2, 3, 9, 7), P(1, 2, 0, 0, (2, 1), (8, 4)), P(1, 2, 1, 0, None, (8, 4)), (1, False)),
    # WG_TILED through slabs: ZP = 1 with n % 4 == 0 (vector body for aligned gw) and n % 4 != 0 (scalar for every gw)
    "slabs-zp1-n4": ((16, 16, 3, 1, 1, 2, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (2, False)),
    "slabs-zp1-odd": ((5, 3, 3, 1, 1, 2, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (2, False)),
    # ... ZP = 4
    "slabs-zp4-n4": ((4, 4, 3, 1, 1, 16, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (16, False)),
    "slabs-zp4-odd": ((5, 3, 3, 1, 1, 16, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (16, False)),
    # ... ZP = 16
    "slabs-zp16-n4": ((2, 2, 3, 1, 1, 64, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (64, False)),
    "slabs-zp16-odd": ((3, 5, 3, 1, 1, 64, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 0, (2, 0), (16, 0)), (64, False)),
    # pairs_ok (locate_conv_wgrad: even map, even gy_bs, gy 8-byte aligned) true above - conv_wgrad_bx6_kernel - and false here purely
    # through gy's placement: the fp32-MFMA conv_wgrad_kernel on the same geometry and slabs
    "slabs-zp1-n4-unpaired": ((16, 16, 3, 1, 1, 2, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 1, 0, (2, 0), (8, 4)), (2, False)),
    "slabs-zp1-n4-odd-stride": ((16, 16, 3, 1, 1, 2, 8, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 0, 1, (2, 1), (16, 0)), (2, False)),
    # the 192-row plan (wgrad_plan: M % 192 == 0, even map, >= 24 tiles): paired loads required - gy 8-byte aligned (here: not
    # 16), even stride; x 4 bytes off
    "tall-192-plan": ((342, 192, 3, 1, 1, 3, 6, 8), P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 2, 0, (2, 0), (16, 8)), (2, False)),
}


@functools.lru_cache(maxsize=None)
def _wgrad_operands(cin, cout, k, s, p, B, H, W):
    gen = torch.Generator().manual_seed(7 * cin + 3 * cout + k + B)
    x = torch.randn(B, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen)
    import torch.nn.functional as F
    oh, ow = F.conv2d(torch.zeros(1, cin, H, W, device="meta"), torch.zeros(cout, cin, k, k, device="meta"), None, s, p).shape[2:]
    g = torch.randn(B, cout, oh, ow, generator=gen)
    _, _, dw = conv_ref64("conv", s, p, x, w, g)
    return x, w, g, dw


def _wgrad_launch(ops, garr, xs, gs, gw, w, inv, part, ws, rec=None):
    call("locate_conv_wgrad", garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), gw.data_ptr(), w.data_ptr(), inv.data_ptr(),
         0, 0, part.data_ptr(), ws.data_ptr(), 0, None, None, rec, S())


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_weight_gradient_into_offset_homes(name):
    """locate_conv_wgrad as test_small_weight_gradients_batched_equal_single_launches calls it, x and gy slice views, gw an
    offset_out 0, 1, 2 and 3 words past a 16-byte boundary (and once more at 0 with the WORKSPACE one word off: the other pointer of
    slab_reduce_body's clause), with w_ref and the <G, W_bar> partials.  Then the deferred forms on an offset gw - the batched
    small-map launch (locate_wgrad_batch) or the deferred split reduction (locate_slab_reduce_batch) - bit-equal to the immediate
    call on the same placement."""
    from locate_amd import ops
    shape, px, pg, (slabs, batched) = WGRAD_CASES[name]
    cin, cout, k, s, p, B, H, W = shape
    x0, w0, g0, dw_ref = _wgrad_operands(*shape)
    geom, garr, out_shape = _geom_of(ops, *shape)
    n = w0.numel()
    ws_bytes = L().locate_conv_wgrad_workspace_bytes(garr)
    assert ws_bytes == (slabs * n * 4 if slabs > 1 else 0), "the plan has %g slabs, the case was written for %d" % (ws_bytes / (4.0 * n), slabs)
    npart = L().locate_conv_wgrad_partials(garr)
    xs, gs = px.view(x0), pg.view(g0)
    w = w0.to(dev())
    inv = torch.full((1,), 0.5, device=dev())          # a power of two: gw = dw / 2 exactly
    rec0 = ctypes.create_string_buffer(L().locate_wgrad_batch_record_bytes())
    blocks = L().locate_wgrad_batch_record(garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), xs.data_ptr(), None, None, 0, 0, None, rec0)
    assert (blocks > 0) == batched
    want = dw_ref * 0.5
    dot_want = float((dw_ref * w0.double()).sum())
    dot_tol = TOL_DW * float(dw_ref.abs().max()) * float(w0.double().abs().sum())       # every element of gw within the dw bound
    first = None
    for gw_off, ws_off in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1)):
        gw = offset_out(tuple(w0.shape), gw_off)
        ws = offset_out((max(ws_bytes // 4, 4),), ws_off)
        part = torch.zeros(npart, dtype=torch.float64, device=dev())
        _wgrad_launch(ops, garr, xs, gs, gw, w, inv, part, ws)
        intact(xs, gs, gw, ws)
        written(gw)
        what = "%s, gw + %d, workspace + %d" % (name, gw_off, ws_off)
        assert_close(gw.cpu(), want, TOL_DW, what)
        assert abs(float(part.sum()) - dot_want) <= dot_tol, "%s: <G, W_bar> %.9g, expected %.9g +- %.3g" % (what, float(part.sum()), dot_want, dot_tol)
        if first is None:
            first = bits(gw)
        if slabs == 1 and name != "onepix-staged":          # no clause of these kernels mentions gw
            assert torch.equal(bits(gw), first), what + ": differs from the aligned gw"
    # the deferred forms, gw one word off
    gw_now, gw_later = offset_out(tuple(w0.shape), 1), offset_out(tuple(w0.shape), 1)
    p_now, p_later = (torch.zeros(npart, dtype=torch.float64, device=dev()) for _ in range(2))
    ws_now, ws_later = (offset_out((max(ws_bytes // 4, 4),), 0) for _ in range(2))
    _wgrad_launch(ops, garr, xs, gs, gw_now, w, inv, p_now, ws_now)
    if batched:
        rec = ctypes.create_string_buffer(L().locate_wgrad_batch_record_bytes())
        assert L().locate_wgrad_batch_record(garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), gw_later.data_ptr(), w.data_ptr(),
                                             inv.data_ptr(), 0, 0, p_later.data_ptr(), rec) > 0
        call("locate_wgrad_batch", rec.raw, 1, S())
    else:
        rec = ctypes.create_string_buffer(L().locate_slab_reduce_record_bytes())
        _wgrad_launch(ops, garr, xs, gs, gw_later, w, inv, p_later, ws_later, rec)
        assert (L().locate_slab_reduce_record_blocks(rec) > 0) == (slabs > 1)
        if slabs > 1:
            torch.cuda.synchronize()
            assert bool((gw_later.view(torch.int32) == UNWRITTEN).all()), "a deferred reduction wrote gw before its batch ran"
            call("locate_slab_reduce_batch", rec.raw, 1, S())
    intact(xs, gs, gw_now, gw_later, ws_now, ws_later)
    written(gw_later)
    assert torch.equal(bits(gw_later), bits(gw_now)) and torch.equal(p_later, p_now), name + ": deferred form differs from the immediate call"


def test_grouped_weight_gradients_into_offset_homes():
    """locate_dwconv_wgrad (dw_wgrad_final_kernel stores rows of k x k words) and locate_groupdot_wgrad (one thread per element)
    with slice-view operands and gw 0 ... 3 words off: scalar stores, no pointer clause - every gw equals the aligned one."""
    from locate_amd import ops
    # depthwise 20 -> 40 (multiplier 2), 5x5 s2 p2 on 9 x 7
    geometry = ("conv", 20, 40, 5, 2, 2, 2, 9, 7)
    x0, w0, g0, ref = _operands(*geometry, groups=20)
    spec = ops.ConvSpec("conv", 5, 5, 2, 2, 2, "depthwise")
    geom, _ = spec.geometry(tuple(x0.shape), tuple(w0.shape))
    garr = (ctypes.c_int * 12)(*geom)
    xs, gs = P(1, 2, 0, 0, (2, 1), (8, 4)).view(x0), P(1, 2, 1, 0, None, (8, 4)).view(g0)
    w = w0.to(dev())
    inv = torch.full((1,), 0.5, device=dev())
    nws = L().locate_dwconv_wgrad_workspace_bytes(garr) // 4
    first = None
    for off in range(4):
        gw, ws = offset_out(tuple(w0.shape), off), offset_out((nws,), 0)
        part = torch.zeros(L().locate_dwconv_wgrad_partials(garr), dtype=torch.float64, device=dev())
        call("locate_dwconv_wgrad", garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), gw.data_ptr(), w.data_ptr(), inv.data_ptr(),
             0, 0, part.data_ptr(), ws.data_ptr(), S())
        intact(xs, gs, gw, ws)
        written(gw)
        assert_close(gw.cpu(), ref[2] * 0.5, TOL_DW, "depthwise dw, gw + %d" % off)
        first = bits(gw) if first is None else first
        assert torch.equal(bits(gw), first)
    # group dot, L = 50 and L = 64
    for geometry, groups, off in ((("full", 6, 3, 5, 1, 0, 2, 5, 5), 3, 0), (("full", 12, 3, 4, 1, 0, 3, 4, 4), 3, 1)):
        x0, w0, g0, ref = _operands(*geometry, groups=groups)
        B, G, Ln = x0.shape[0], groups, w0[0].numel()
        xs = P(1, 1, off, 0, None, (8, 4)).view(x0)
        gy = offset_view(g0.reshape(B, G), 1)
        w = w0.to(dev())
        first = None
        for off in range(4):
            gw = offset_out(tuple(w0.shape), off)
            part = torch.zeros(L().locate_groupdot_wgrad_partials(G, Ln), dtype=torch.float64, device=dev())
            call("locate_groupdot_wgrad", xs.data_ptr(), xs.stride(0), gy.data_ptr(), gw.data_ptr(), w.data_ptr(), inv.data_ptr(), 0, 0,
                 part.data_ptr(), B, G, Ln, S())
            intact(xs, gy, gw)
            written(gw)
            assert_close(gw.cpu(), ref[2] * 0.5, TOL_DW, "group dot dw, L = %d, gw + %d" % (Ln, off))
            first = bits(gw) if first is None else first
            assert torch.equal(bits(gw), first)


# ====================================================================================================== weight gradient, operators
HOME_CASES = {
    # one layer per route of wgrad_route; the runtime defers its finalisers (small-map layers: locate_wgrad_batch; slabs:
    # locate_slab_reduce_batch; then locate_fin_sn_rank1 in place)
    "map1x1": ("conv", 100, 7, 1, 1, 0, 5, 1, 1),
    "onepix": ("conv", 24, 160, 5, 2, 2, 6, 2, 2),
    "pointwise": ("conv", 40, 100, 1, 1, 0, 8, 32, 32),
    "tiled-direct": ("conv", 20, 33, 5, 2, 2, 3, 9, 7),
    "tiled-slabs": ("conv", 16, 16, 3, 1, 1, 2, 8, 8),
}


@pytest.mark.parametrize("name", list(HOME_CASES))
def test_layer_gradient_lands_in_a_packed_home(name, monkeypatch):
    """The parameter's gradient home as GradAllReducer.make_homes lays it out - a 1-element tensor in front of it in one flat
    buffer, so the home is 4 bytes past a 16-byte boundary - through param.__dict__["_locate_grad_buf"], under a runtime that defers
    its finalisers: the gradient IS the home, within the float64 bound; the element in front and the guards are untouched."""
    from locate_amd import ops
    geometry = HOME_CASES[name]
    kind, cin, cout, k, s, p, B, H, W = geometry
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 1e30)
    x0, w0, g0, ref = _operands(*geometry)
    n = w0.numel()
    flat = offset_out((1 + n,), 0)
    home = flat[1:].view(w0.shape)
    assert home.data_ptr() % 16 == 4
    xs, gs = P(1, 1, 0, 0).view(x0), P(1, 1, 0, 0).view(g0)
    got = _layer(ops, kind, k, s, p, xs, w0, gs, None, 0, False, "dense", True, home)
    assert got[2].data_ptr() == home.data_ptr(), "the gradient was not written to the parameter's home"
    intact(xs, gs, flat)
    assert int(flat.view(torch.int32)[0]) == UNWRITTEN, "the element in front of the home (another parameter's gradient) was written"
    written(home)
    _check(got, ref, "home, " + name)


def test_layer_behind_a_real_concatenation(monkeypatch):
    """A stand-alone DEFAULT_RUNTIME layer whose output is the second input of ops.cat_channels: its gy is the view g[:, ca:] that
    CatChannelsFn.backward returns - 49 words into a 16-byte aligned gradient whose first channel (the other branch's gradient)
    is NaN here."""
    from locate_amd import ops
    geometry = ("conv", 32, 72, 3, 1, 1, 3, 7, 7)
    kind, cin, cout, k, s, p, B, H, W = geometry
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 1e30)
    x0, w0, g0, ref = _operands(*geometry)
    xg = x0.to(dev()).requires_grad_(True)
    wg = w0.to(dev()).requires_grad_(True)
    h = w0.shape[0]
    u, v = torch.zeros(h, device=dev()), torch.zeros(w0.numel() // h, device=dev())
    sigma, wv = torch.tensor([1.0, 1.0], device=dev()), torch.zeros(h, device=dev())
    a = torch.randn(B, 1, H, W, device=dev(), requires_grad=True)
    y = ops.SNConvFn.apply(xg, wg, u, v, None, sigma, wv, ops.ConvSpec(kind, k, k, s, p, p), None)
    out = ops.cat_channels(a, y)
    G = torch.full(tuple(out.shape), float("nan"), device=dev())
    G[:, 1:] = g0.to(dev())
    tap = Tap()
    monkeypatch.setattr(ops, "CONTRACTION_TAP", tap)
    ops.reset_backward_state()
    out.backward(G)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "CONTRACTION_TAP", None)
    assert tap.seen["dgrad"] == ((G[:, 1:].data_ptr(), G.stride(0)),) and G[:, 1:].data_ptr() % 8 == 4
    assert bool(torch.isnan(a.grad).all())
    _check((y.detach(), xg.grad, wg.grad), ref, "behind cat_channels")


# ====================================================================================================== refusals
def test_library_refuses_placements_a_route_cannot_take():
    """Status 1 with a message naming the requirement, nothing written: the narrow 1x1 route of locate_conv_wgrad (x / gy 16-byte
    aligned, strides % 4 == 0), its 192-row plan (gy 8-byte aligned, even stride) and the window flag of locate_conv_fwd on a tensor
    the window form cannot load in pixel pairs."""
    from locate_amd import ops
    # narrow 1x1 route
    shape = (40, 100, 1, 1, 0, 8, 32, 32)
    x0, w0, g0, _ = _wgrad_operands(*shape)
    geom, garr, _ = _geom_of(ops, *shape)
    w = w0.to(dev())
    inv = torch.full((1,), 0.5, device=dev())
    npart, nws = L().locate_conv_wgrad_partials(garr), L().locate_conv_wgrad_workspace_bytes(garr) // 4
    ok = P(1, 1, 0, 0, (4, 0), (16, 0))
    for what, px, pg in (("x 4 bytes off", P(1, 1, 1, 0, (4, 0), (16, 4)), ok), ("gy 8 bytes off", ok, P(1, 1, 2, 0, (4, 0), (16, 8))),
                         ("x stride = 2 mod 4", P(1, 1, 0, 2, (4, 2), (16, 0)), ok), ("gy stride odd", ok, P(1, 1, 0, 1, (4, 1), (16, 0)))):
        xs, gs, gw, ws = px.view(x0), pg.view(g0), offset_out(tuple(w0.shape), 0), offset_out((nws,), 0)
        part = torch.zeros(npart, dtype=torch.float64, device=dev())
        st, msg = status("locate_conv_wgrad", garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), gw.data_ptr(), w.data_ptr(),
                         inv.data_ptr(), 0, 0, part.data_ptr(), ws.data_ptr(), 0, None, None, None, S())
        assert st == 1 and "16-byte aligned" in msg and "multiples of 4" in msg, (what, st, msg)
        intact(xs, gs, gw, ws)
        assert bool((gw.view(torch.int32) == UNWRITTEN).all()) and bool((ws.view(torch.int32) == UNWRITTEN).all()), what
    # 192-row plan
    shape = (342, 192, 3, 1, 1, 3, 6, 8)
    x0, w0, g0, _ = _wgrad_operands(*shape)
    geom, garr, _ = _geom_of(ops, *shape)
    assert L().locate_conv_wgrad_operand_align(garr, 0) == 4 and L().locate_conv_wgrad_operand_align(garr, 1) == 8
    w = w0.to(dev())
    npart, nws = L().locate_conv_wgrad_partials(garr), L().locate_conv_wgrad_workspace_bytes(garr) // 4
    for what, pg in (("gy 4 bytes off", P(1, 1, 1, 0, (2, 0), (8, 4))), ("gy stride odd", P(1, 1, 0, 1, (2, 1), (8, 0)))):
        xs, gs, gw, ws = P(1, 1, 1, 0).view(x0), pg.view(g0), offset_out(tuple(w0.shape), 0), offset_out((nws,), 0)
        part = torch.zeros(npart, dtype=torch.float64, device=dev())
        st, msg = status("locate_conv_wgrad", garr, xs.data_ptr(), xs.stride(0), gs.data_ptr(), gs.stride(0), gw.data_ptr(), w.data_ptr(),
                         inv.data_ptr(), 0, 0, part.data_ptr(), ws.data_ptr(), 0, None, None, None, S())
        assert st == 1 and "8-byte aligned" in msg and "even batch stride" in msg, (what, st, msg)
        intact(xs, gs, gw, ws)
        assert bool((gw.view(torch.int32) == UNWRITTEN).all()) and bool((ws.view(torch.int32) == UNWRITTEN).all()), what
    # the window flag (precision | 16) on a tensor locate_conv_win_ok answers 0 for
    shape = (16, 16, 3, 1, 1, 2, 8, 8)
    x0, w0, g0, _ = _wgrad_operands(*shape)
    geom, garr, out_shape = _geom_of(ops, *shape)
    assert L().locate_conv_win_ok(garr, 0, 16 * 64, 16) > 0
    w = w0.to(dev())
    panel = torch.zeros(L().locate_conv_panel_bytes(garr, 4) // 4 + 4, device=dev())
    call("locate_conv_pack_panel", garr, 4, w.data_ptr(), panel.data_ptr(), S())
    wsb = max(L().locate_conv_win_workspace_bytes(garr, 0), 16)
    for what, px in (("x 4 bytes off", P(1, 1, 1, 0, (2, 0), (8, 4))), ("x stride odd", P(1, 1, 0, 1, (2, 1), (8, 0)))):
        xs, ys, ws = px.view(x0), P(1, 1, 0, 0).out(out_shape), offset_out((wsb // 4,), 0)
        assert L().locate_conv_win_ok(garr, 0, xs.stride(0), xs.data_ptr()) == 0
        st, msg = status("locate_conv_fwd", garr, xs.data_ptr(), xs.stride(0), panel.data_ptr(), None, 0, 0, None, ys.data_ptr(), ys.stride(0),
                         ws.data_ptr(), None, 16, None, None, S())
        assert st == 1 and "pixel pairs" in msg, (what, st, msg)
        intact(xs, ys, ws)
        assert int((ys.contiguous().view(torch.int32) == UNWRITTEN).sum()) == ys.numel(), what


@pytest.mark.parametrize("name", ["pointwise-route", "tall-192-plan"])
def test_operator_accepts_what_the_weight_gradient_routes_refuse(name, monkeypatch):
    """At the operator level there is no refusal: SNConvFn on float32 tensors with dense planes, however placed.  x and gy one word
    into their buffers (and gy with an odd batch stride) on the two geometries whose weight-gradient route refuses exactly that -
    ops._raw_weight_grad copies the operand the route cannot take (locate_conv_wgrad_operand_align) - forward and input gradient
    read the views in place."""
    from locate_amd import ops
    geometry = {"pointwise-route": ("conv", 40, 100, 1, 1, 0, 8, 32, 32), "tall-192-plan": ("conv", 342, 192, 3, 1, 1, 3, 6, 8)}[name]
    kind, cin, cout, k, s, p, B, H, W = geometry
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 1e30)
    x0, w0, g0, ref = _operands(*geometry)
    for what, px, pg in (("one word off", P(1, 1, 1, 0, None, (8, 4)), P(1, 1, 1, 0, None, (8, 4))),
                         ("odd strides", P(1, 1, 0, 1, (2, 1), (16, 0)), P(1, 1, 0, 1, (2, 1), (16, 0)))):
        xs, gs, ys = px.view(x0), pg.view(g0), P(1, 1, 1, 0).out(tuple(ref[0].shape))
        got = _layer(ops, kind, k, s, p, xs, w0, gs, ys)
        intact(xs, gs, ys)
        written(ys)
        _check(got, ref, "%s, %s" % (name, what))
    # and an operand the route takes is handed over as it is
    t = P(1, 1, 0, 0).view(g0)
    spec = ops.ConvSpec(kind, k, k, s, p, p)
    garr = ops._geom(spec.geometry(tuple(x0.shape), tuple(w0.shape))[0])
    assert ops._wgrad_operand(L(), garr, t, 1) is t
    moved = P(1, 1, 1, 0).view(g0)
    c = ops._wgrad_operand(L(), garr, moved, 1)
    assert c is not moved and c.data_ptr() % 16 == 0 and c.is_contiguous() and torch.equal(c, moved)
