"""The kernel variants that the stream kernels' host launchers pick from the POINTERS and the innermost extent they are handed
(csrc/softmax.hip, resample.hip, elementwise.hip, norm.hip, spectral.hip; the table is DESIGN.md, "Pointer alignment"), each clause
of each predicate made true and false on its own, one pointer at a time - tests/test_gpu_ops.py passes fresh allocations only, so
the alignment half of every predicate is always true there and a scalar / block fall-back runs only where the shape forces it.

Operands live in sentinel-filled flat buffers (offset_view): a contiguous view that starts `off` elements past a 16-byte (32-byte)
boundary with at least 8 guard words on either side, which must still hold the sentinel, bit for bit, after every launch.  Where
the output pointer is part of a predicate the call goes through the C ABI (ctypes), which lets the test place every pointer; the
operator-level cases (plane copies, the three operators that copy a misaligned tensor) go through locate_amd.ops.

Every case is compared with a float64 CPU reference (torch.softmax, F.interpolate, F.avg_pool2d, torch.cat, the oracle's
residual_gate / inplace_norm / root_tanh in double) at the bound tests/test_gpu_ops.py holds the same operator and quantity to:
  softmax 2e-6 on y, 2e-5 on dx (test_softmax_rows); upsample and avgpool 1e-6 (test_resampling_shapes_vs_aten); gate 1e-6 on dx,
  2e-5 on da and dgamma (test_residual_gate_large_vs_oracle); norm 1e-5 on out, 5e-5 on gradients
  (test_inplace_norm_fused_activation_and_big); RootTanh 2e-6 on y, 3e-6 on dx (test_roottanh_golden_and_large); tanh 2e-6 on y,
  5e-6 on dx (test_tanh); power iteration 1e-5 on u, v, sigma (test_spectral_norm_layers_golden); channel sums
  |got - want| <= 2e-6 sum |g| (derived in tests/test_gpu_finalisers.py for at most 32 additions per element; the shapes here
  have fewer).
Where the sources state that the variants share their roundings - the upsample forward kernels, the average pool, the plane
copies, add3, the unary kernels' 16-byte and tail bodies - the offset call must also equal the aligned call bit for bit.

Needs an MI355X: run with -m gpu."""
import functools
import os
import struct
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, assert_close

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

pytestmark = pytest.mark.gpu

# the sentinel-guarded buffers (offset_view, offset_out, guards_intact) are shared with tests/test_gpu_contraction_views.py
from placed_operands import GUARD, SENTINEL, bits, dev, guards_intact, offset_out, offset_view  # noqa: E402,F401


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


# ------------------------------------------------------------------------------------------------ softmax
SOFTMAX_ROWS = 5                # a partial last block of the one-wave-per-row kernels (four rows per block)
SOFTMAX_N = [64, 65, 256, 257, 1024, 1028, 2048, 2052, 3072, 3076, 4096, 4100]
SOFTMAX_OFFSET_N = [1028, 2048, 3076, 4096]          # the register-row kernels <2>, <2>, <4>, <4>: an offset pointer selects the block kernel


@functools.lru_cache(maxsize=None)
def _softmax_case(n):
    gen = torch.Generator().manual_seed(4000 + n)
    x = torch.randn(SOFTMAX_ROWS, n, generator=gen) * 3
    x[2] = (torch.rand(n, generator=gen) - 0.5) * 60          # one row: a 60-wide spread of logits ...
    x[2, n // 3] = 30.0 + 80.0                                # ... under a spike 80 above it
    g = torch.randn(SOFTMAX_ROWS, n, generator=gen)
    xd = x.double().requires_grad_(True)
    yd = torch.softmax(xd, -1)
    yd.backward(g.double())
    return x, g, yd.detach(), xd.grad


def _softmax_offsets(n, names):
    cases = [dict.fromkeys(names, 0)]
    if n in SOFTMAX_OFFSET_N:
        cases += [dict(cases[0], **{k: 1}) for k in names]
    return cases


@pytest.mark.parametrize("n", SOFTMAX_N)
def test_softmax_forward_variants(n):
    """softmax_fwd_wave_kernel<1 | 4 | 16> (n <= 64 | 256 | 1024), softmax_fwd_row_kernel<2 | 3 | 4> (n <= 2048 | 3072 | 4096,
    n % 4 == 0, x and y 16-byte aligned) and softmax_fwd_block_kernel (everything else: n % 4 != 0, n > 4096, or x or y offset)."""
    x, _, y_ref, _ = _softmax_case(n)
    for off in _softmax_offsets(n, ("x", "y")):
        xg, yg = offset_view(x, off["x"]), offset_out(x.shape, off["y"])
        call("locate_softmax_fwd", xg.data_ptr(), yg.data_ptr(), SOFTMAX_ROWS, n, S())
        guards_intact(xg, yg)
        assert_close(yg.cpu(), y_ref, 2e-6, "softmax y, n = %d, offsets %s" % (n, off))


@pytest.mark.parametrize("n", SOFTMAX_N)
def test_softmax_backward_variants(n):
    """The same table for softmax_bwd_*: y, gy and gx all enter the register-row kernels' predicate."""
    _, g, y_ref, dx_ref = _softmax_case(n)
    y = y_ref.float()
    for off in _softmax_offsets(n, ("y", "g", "gx")):
        yg, gg, gx = offset_view(y, off["y"]), offset_view(g, off["g"]), offset_out(y.shape, off["gx"])
        call("locate_softmax_bwd", yg.data_ptr(), gg.data_ptr(), gx.data_ptr(), SOFTMAX_ROWS, n, S())
        guards_intact(yg, gg, gx)
        assert_close(gx.cpu(), dx_ref, 2e-5, "softmax dx, n = %d, offsets %s" % (n, off))


# ------------------------------------------------------------------------------------------------ bilinear x2 upsample
PLANES = 5


def _pool_pairs(raw):
    """FeaturePooling(r = 2) of a flat tensor: the mean of adjacent elements"""
    return raw.reshape(-1, 2).mean(1)


def _upsample_ref(x, H, W):
    """float64 forward and the vector-Jacobian product of the bilinear x2 upsample of [PLANES, H, W]"""
    xd = x.double().reshape(1, PLANES, H, W).requires_grad_(True)
    yd = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)

    def vjp(gy):
        return torch.autograd.grad(yd, xd, gy.double().reshape(yd.shape), retain_graph=True)[0].reshape(PLANES, H, W)
    return yd.detach().reshape(PLANES, 2 * H, 2 * W), vjp


@pytest.mark.parametrize("W", [4, 6, 7, 8, 12])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pooled"])
def test_upsample_forward_variants(pool, H, W):
    """upsample2x_fwd_tile_kernel (W % 4 == 0, W >= 8, x 16-byte - pooled: 32-byte - and y 16-byte aligned), upsample2x_fwd_vec_kernel
    (W even, y 16-byte aligned; pooled: x 8-byte aligned, which the entry point requires anyway) and upsample2x_fwd_kernel (the
    rest).  W = 4 is a multiple of 4 below 8, 6 is even only, 7 scalar.  The three evaluate one expression with pinned roundings
    (bil_eval): every offset call equals the aligned call bit for bit."""
    torch.manual_seed(100 * H + W + int(pool))
    name = "locate_pool2_upsample2x_fwd" if pool else "locate_upsample2x_fwd"
    n_in = PLANES * H * W * (2 if pool else 1)
    x = torch.randn(n_in)
    y_ref, _ = _upsample_ref(_pool_pairs(x.double()) if pool else x, H, W)
    in_align = 32 if pool else 16
    in_offsets = (0, 2, 4) if pool else (0, 1, 2)          # pooled: 8 bytes off, then 16-byte but not 32-byte aligned
    first = None
    for in_off in in_offsets:
        for out_off in (0, 1):
            xg, yg = offset_view(x, in_off, in_align), offset_out((PLANES, 2 * H, 2 * W), out_off)
            call(name, xg.data_ptr(), yg.data_ptr(), PLANES, H, W, S())
            guards_intact(xg, yg)
            what = "%s H = %d W = %d, x + %d, y + %d" % (name, H, W, in_off, out_off)
            assert_close(yg.cpu(), y_ref, 1e-6, what)
            if first is None:
                first = bits(yg)
            assert torch.equal(bits(yg), first), what + ": differs from the aligned call"
    if pool:
        # 4 bytes off: the pooled form reads pairs with 8-byte loads in every kernel - refused, nothing launched
        xg, yg = offset_view(x, 1, in_align), offset_out((PLANES, 2 * H, 2 * W), 0)
        before = bits(yg)
        st, msg = status(name, xg.data_ptr(), yg.data_ptr(), PLANES, H, W, S())
        torch.cuda.synchronize()
        assert st == 1 and "unaligned" in msg, (st, msg)
        assert torch.equal(bits(yg), before)
        guards_intact(xg, yg)


@pytest.mark.parametrize("W", [4, 7, 8])
@pytest.mark.parametrize("H", [1, 3])
def test_upsample_backward_variants(H, W):
    """upsample2x_bwd_vec_kernel<false> (W % 4 == 0, W >= 8, gy and gx 16-byte aligned) against upsample2x_bwd_kernel<false>
    (this entry point has no accumulate argument: the plain upsample's input is never forked)."""
    torch.manual_seed(200 * H + W)
    x = torch.randn(PLANES * H * W)
    gy = torch.randn(PLANES, 2 * H, 2 * W)
    _, vjp = _upsample_ref(x, H, W)
    gx_ref = vjp(gy)
    for gy_off, gx_off in ((0, 0), (1, 0), (0, 1)):
        gg, gx = offset_view(gy, gy_off), offset_out((PLANES, H, W), gx_off)
        call("locate_upsample2x_bwd", gg.data_ptr(), gx.data_ptr(), PLANES, H, W, S())
        guards_intact(gg, gx)
        assert_close(gx.cpu(), gx_ref, 1e-6, "upsample dx H = %d W = %d, gy + %d, gx + %d" % (H, W, gy_off, gx_off))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("W", [4, 7, 8])
@pytest.mark.parametrize("H", [1, 3])
def test_pooled_upsample_backward_variants(H, W, accumulate):
    """upsample2x_bwd_vec_kernel<true> (W % 4 == 0, W >= 8, gy 16-byte and gx 32-byte aligned) against upsample2x_bwd_kernel<true>:
    gy 4 bytes off, gx 8 bytes off, gx 16-byte but not 32-byte aligned (the entry point's own clause in front of the shared
    launcher).  gx 4 bytes off is refused: the scalar kernel stores pairs."""
    torch.manual_seed(300 * H + W + accumulate)
    raw = torch.randn(2 * PLANES * H * W)
    gy = torch.randn(PLANES, 2 * H, 2 * W)
    gx0 = torch.randn(2 * PLANES * H * W)
    _, vjp = _upsample_ref(_pool_pairs(raw.double()), H, W)
    gx_ref = (vjp(gy).reshape(-1) * 0.5).repeat_interleave(2)
    if accumulate:
        gx_ref = gx_ref + gx0.double()
    for gy_off, gx_off in ((0, 0), (1, 0), (0, 2), (0, 4)):
        gg, gx = offset_view(gy, gy_off), offset_view(gx0 if accumulate else torch.full_like(gx0, float("nan")), gx_off, 32)
        call("locate_pool2_upsample2x_bwd", gg.data_ptr(), gx.data_ptr(), PLANES, H, W, accumulate, S())
        guards_intact(gg, gx)
        assert_close(gx.cpu(), gx_ref, 1e-6, "pooled upsample dx H = %d W = %d, gy + %d, gx + %d" % (H, W, gy_off, gx_off))
    gg, gx = offset_view(gy, 0), offset_view(gx0, 1, 32)
    st, msg = status("locate_pool2_upsample2x_bwd", gg.data_ptr(), gx.data_ptr(), PLANES, H, W, accumulate, S())
    torch.cuda.synchronize()
    assert st == 1 and "unaligned" in msg, (st, msg)
    assert torch.equal(bits(gx), bits(gx0))
    guards_intact(gg, gx)


# ------------------------------------------------------------------------------------------------ 2x2 average pool
AVGPOOL_SHAPES = [(2, 8), (4, 16), (2, 4), (2, 6), (5, 8), (4, 10)]


def _avgpool_ref(x, H, W):
    xd = x.double().reshape(1, PLANES, H, W).requires_grad_(True)
    yd = F.avg_pool2d(xd, 2, 2)

    def vjp(gy):
        return torch.autograd.grad(yd, xd, gy.double().reshape(yd.shape), retain_graph=True)[0].reshape(PLANES, H, W)
    return yd.detach().reshape(PLANES, H // 2, W // 2), vjp


@pytest.mark.parametrize("H,W", AVGPOOL_SHAPES)
def test_avgpool_forward_variants(H, W):
    """avgpool2_fwd_vec_kernel (W % 8 == 0, H even, x and y 16-byte aligned) against avgpool2_fwd_kernel: the same sum per output,
    bit for bit."""
    torch.manual_seed(400 + 16 * H + W)
    x = torch.randn(PLANES, H, W)
    y_ref, _ = _avgpool_ref(x, H, W)
    first = None
    for x_off, y_off in ((0, 0), (1, 0), (0, 1)):
        xg, yg = offset_view(x, x_off), offset_out(y_ref.shape, y_off)
        call("locate_avgpool2_fwd", xg.data_ptr(), yg.data_ptr(), PLANES, H, W, S())
        guards_intact(xg, yg)
        what = "avgpool %d x %d, x + %d, y + %d" % (H, W, x_off, y_off)
        assert_close(yg.cpu(), y_ref, 1e-6, what)
        if first is None:
            first = bits(yg)
        assert torch.equal(bits(yg), first), what + ": differs from the aligned call"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("H,W", AVGPOOL_SHAPES)
def test_avgpool_backward_variants(H, W, accumulate):
    """avgpool2_bwd_vec_kernel (W % 4 == 0, H even, gy 8-byte and gx 16-byte aligned) against avgpool2_bwd_kernel: gy 4 and 8 bytes
    off (the second keeps the vector kernel), gx 4 bytes off.  One exact product and at most one addition per element either way:
    bit for bit."""
    torch.manual_seed(500 + 16 * H + W + accumulate)
    x = torch.randn(PLANES, H, W)
    gy = torch.randn(PLANES, H // 2, W // 2)
    gx0 = torch.randn(PLANES, H, W)
    _, vjp = _avgpool_ref(x, H, W)
    gx_ref = vjp(gy) + (gx0.double() if accumulate else 0.0)
    first = None
    for gy_off, gx_off in ((0, 0), (1, 0), (2, 0), (0, 1)):
        gg, gx = offset_view(gy, gy_off), offset_view(gx0 if accumulate else torch.full_like(gx0, float("nan")), gx_off)
        call("locate_avgpool2_bwd", gg.data_ptr(), gx.data_ptr(), PLANES, H, W, accumulate, S())
        guards_intact(gg, gx)
        what = "avgpool dx %d x %d, gy + %d, gx + %d" % (H, W, gy_off, gx_off)
        assert_close(gx.cpu(), gx_ref, 1e-6, what)
        if first is None:
            first = bits(gx)
        assert torch.equal(bits(gx), first), what + ": differs from the aligned call"


# ------------------------------------------------------------------------------------------------ plane copies
# (B, Ca, Cb, H, W): every extent a multiple of 4 (16-byte copies both ways) | scalar by extent | a multiple-of-4 slice whose
# destination starts 8 bytes into the concatenation (and whose batch stride, 10, is no multiple of 4)
CAT_SHAPES = [(3, 4, 8, 2, 2), (3, 3, 5, 1, 3), (2, 1, 4, 1, 2)]


@pytest.mark.parametrize("src_off", [0, 1])
@pytest.mark.parametrize("B,Ca,Cb,H,W", CAT_SHAPES)
def test_plane_copies_through_cat_channels(B, Ca, Cb, H, W, src_off):
    """copy_planes_kernel's 16-byte body ((chw | src_bs | dst_bs) % 4 == 0, src and dst 16-byte aligned) and its scalar body through
    ops.cat_channels (forward: two copies into channel slices; backward: the slices themselves) and ops._copy_channels(accumulate =
    True), with fresh sources and with sources one element into a buffer: torch.cat and its slices, bit for bit."""
    from locate_amd import ops
    torch.manual_seed(600 + B * Ca * Cb + src_off)
    a0, b0 = torch.randn(B, Ca, H, W), torch.randn(B, Cb, H, W)
    a = offset_view(a0, src_off).requires_grad_(True)
    b = offset_view(b0, src_off).requires_grad_(True)
    out = ops.cat_channels(a, b)
    guards_intact(a, b)
    assert torch.equal(out.detach().cpu(), torch.cat([a0, b0], 1))
    g = torch.randn(out.shape, device=dev())
    out.backward(g)
    assert torch.equal(a.grad, g[:, :Ca]) and torch.equal(b.grad, g[:, Ca:])
    # dst[:, Ca:] += src: one fp32 addition per element, IEEE on both sides
    dst0 = torch.randn(B, Ca + Cb, H, W)
    dst = dst0.to(dev())
    ops._copy_channels(b.detach(), dst[:, Ca:], accumulate=True)
    want = dst0.clone()
    want[:, Ca:] += b0
    assert torch.equal(dst.cpu(), want)
    assert_close(dst.cpu(), torch.cat([dst0[:, :Ca].double(), dst0[:, Ca:].double() + b0.double()], 1), 1e-6, "accumulating copy")
    guards_intact(b)


# ------------------------------------------------------------------------------------------------ add3
@pytest.mark.parametrize("which", ["none", "a", "b", "c", "out"])
def test_add3_offset_operands(which):
    """add3_kernel<true> (per and the three batch strides multiples of 4, all four pointers 16-byte aligned) against
    add3_kernel<false>, one pointer off at a time (tests/test_gpu_ops.py::test_add3_strided_operands varies the strides): two
    fp32 additions in a fixed order, bit for bit the same two additions on the host."""
    torch.manual_seed(7)
    shape = (2, 3, 2, 2)
    a, b, c = (torch.randn(shape) for _ in range(3))
    per = a[0].numel()
    ag, bg, cg = (offset_view(t, int(which == k)) for t, k in ((a, "a"), (b, "b"), (c, "c")))
    out = offset_out(shape, int(which == "out"))
    call("locate_add3", ag.data_ptr(), per, bg.data_ptr(), per, cg.data_ptr(), per, out.data_ptr(), shape[0], per, S())
    guards_intact(ag, bg, cg, out)
    assert torch.equal(out.cpu(), (a + b) + c)
    assert_close(out.cpu(), (a.double() + b.double()) + c.double(), 1e-6, "add3, %s offset" % which)


# ------------------------------------------------------------------------------------------------ residual gate backward
@pytest.mark.parametrize("which", ["none", "x", "g", "dx", "a", "da"])
@pytest.mark.parametrize("per_plane", [1, 0], ids=["a_per_plane", "a_full"])
@pytest.mark.parametrize("hw", [4, 128, 132, 6])
def test_gate_backward_variants(hw, per_plane, which):
    """locate_gate_bwd: gate_bwd_small_kernel<1 | 32> (hw = 4 | 128: hw % 4 == 0, hw <= 128 - its upper bound - and x, g, dx and,
    with a full-map a, a and da 16-byte aligned) against gate_bwd_plane_kernel<1> with its 16-byte body (hw = 132) and its scalar
    body (hw = 6, or any of those pointers offset).  With one a per plane, a and da are read and written as scalars: their offset
    must change nothing.  (tests/test_gpu_gate_fold.py drives the term forms with EVERY operand one element off at hw = 64, 1024
    and 1; here one pointer at a time, without a term.)"""
    from oracle import locate_oracle as O
    B, C = 2, 3
    planes = B * C
    torch.manual_seed(700 + hw + per_plane)
    x = torch.randn(B, C, hw)
    a = torch.randn(B, C, 1) if per_plane else torch.randn(B, C, hw)
    gamma = torch.tensor([[0.7]])
    g = torch.randn(B, C, hw)
    xr, ar, gr = (t.double().requires_grad_(True) for t in (x, a, gamma))
    O.residual_gate(xr, ar.expand_as(xr), gr).backward(g.double())
    xg, gg, ag = offset_view(x, int(which == "x")), offset_view(g, int(which == "g")), offset_view(a, int(which == "a"))
    dx, da = offset_out(x.shape, int(which == "dx")), offset_out(a.shape, int(which == "da"))
    gm, dgamma = offset_view(gamma, 0), offset_out((1,), 0)
    ws = torch.empty(L().locate_gate_bwd_workspace_bytes(planes), dtype=torch.uint8, device=dev())
    call("locate_gate_bwd", xg.data_ptr(), ag.data_ptr(), per_plane, gm.data_ptr(), gg.data_ptr(), dx.data_ptr(), da.data_ptr(),
         dgamma.data_ptr(), planes, hw, ws.data_ptr(), 0, None, S())
    guards_intact(xg, gg, ag, dx, da, gm, dgamma)
    what = "gate hw = %d, %s, %s offset" % (hw, "a per plane" if per_plane else "full a", which)
    assert_close(dx.cpu(), xr.grad, 1e-6, what + ": dx")
    assert_close(da.cpu(), ar.grad, 2e-5, what + ": da")
    assert_close(dgamma.cpu(), gr.grad.reshape(1), 2e-5, what + ": dgamma")


# ------------------------------------------------------------------------------------------------ InPlaceNorm backward
def _norm_operands(B, C, hw, per_sample, seed):
    torch.manual_seed(seed)
    x = torch.randn(B, C, hw, 1) * 1.7 + 0.4
    y = torch.randn(B if per_sample else 1, C, 1, 1)
    b = torch.randn(1, C, 1, 1)
    g = torch.randn(B, C, hw, 1)
    return x, y, b, g


def _norm_ref(x, y, b, g, with_act):
    from oracle import locate_oracle as O
    xr, yr, br = (t.double().requires_grad_(True) for t in (x, y, b))
    ref = O.inplace_norm(xr, yr, br)
    if with_act:
        ref = O.root_tanh(ref)
    ref.backward(g.double())
    return ref.detach(), xr.grad, yr.grad, br.grad


@pytest.mark.parametrize("g_off", [0, 1])
@pytest.mark.parametrize("with_act", [0, 1], ids=["plain", "act"])
@pytest.mark.parametrize("per_sample", [0, 1], ids=["channel_scale", "sample_scale"])
@pytest.mark.parametrize("hw", [4, 128, 132, 6])
def test_norm_backward_variants(hw, per_sample, with_act, g_off):
    """locate_norm_bwd: norm_bwd_plane_small_kernel<., 1 | 32> (hw = 4 | 128: hw % 4 == 0, hw <= 128, x and g 16-byte aligned)
    against norm_bwd_plane_kernel (hw = 132, hw = 6, or g offset).  x stays aligned: the forward refuses any other x
    (test_norm_forward_refuses_an_offset_input)."""
    B, C = 2, 3
    x, y, b, g = _norm_operands(B, C, hw, per_sample, 800 + hw + 2 * per_sample + with_act)
    out_ref, dx_ref, dy_ref, db_ref = _norm_ref(x, y, b, g, with_act)
    xg, yg, bg, gg = offset_view(x, 0), offset_view(y, 0), offset_view(b, 0), offset_view(g, g_off)
    out, stats = offset_out(x.shape, 0), offset_out((2,), 0)
    ws = torch.empty(L().locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=dev())
    call("locate_norm_fwd", xg.data_ptr(), yg.data_ptr(), per_sample, bg.data_ptr(), out.data_ptr(), with_act, stats.data_ptr(), B, C, hw,
         1, ws.data_ptr(), None, None, S())
    dx, dy, db = offset_out(x.shape, 0), offset_out(y.shape, 0), offset_out(b.shape, 0)
    ws2 = torch.empty(L().locate_norm_bwd_workspace_bytes(B, C), dtype=torch.uint8, device=dev())
    call("locate_norm_bwd", xg.data_ptr(), gg.data_ptr(), stats.data_ptr(), yg.data_ptr(), per_sample, bg.data_ptr(), with_act,
         dx.data_ptr(), dy.data_ptr(), db.data_ptr(), B, C, hw, 1, ws2.data_ptr(), 0, S())
    guards_intact(xg, yg, bg, gg, out, stats, dx, dy, db)
    what = "norm hw = %d, per_sample = %d, act = %d, g + %d" % (hw, per_sample, with_act, g_off)
    assert_close(out.cpu(), out_ref, 1e-5, what + ": out")
    assert_close(dx.cpu(), dx_ref, 5e-5, what + ": dx")
    assert_close(dy.cpu(), dy_ref, 5e-5, what + ": dscale")
    assert_close(db.cpu(), db_ref, 5e-5, what + ": dbias")


def test_norm_forward_refuses_an_offset_input():
    """locate_norm_fwd and locate_norm_stats read x with 16-byte loads in every form: an x 4 bytes off is refused with the
    library's error status and nothing is written (ops.inplace_norm copies such a tensor first, see the operator tests below)."""
    B, C, hw = 2, 3, 4
    x, y, b, _ = _norm_operands(B, C, hw, 0, 5)
    xg, yg, bg = offset_view(x, 1), offset_view(y, 0), offset_view(b, 0)
    out, stats = offset_out(x.shape, 0), offset_out((2,), 0)
    before = bits(out), bits(stats)
    ws = torch.empty(L().locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=dev())
    st, msg = status("locate_norm_fwd", xg.data_ptr(), yg.data_ptr(), 0, bg.data_ptr(), out.data_ptr(), 0, stats.data_ptr(), B, C, hw, 1,
                     ws.data_ptr(), None, None, S())
    assert st == 1 and "16-byte aligned" in msg, (st, msg)
    st, msg = status("locate_norm_stats", xg.data_ptr(), x.numel(), stats.data_ptr(), ws.data_ptr(), S())
    assert st == 1 and "16-byte aligned" in msg, (st, msg)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), before[0]) and torch.equal(bits(stats), before[1])
    guards_intact(xg, yg, bg, out, stats)


@pytest.mark.parametrize("g_off", [0, 1])
@pytest.mark.parametrize("pad", [0, 4, 2])
@pytest.mark.parametrize("hw", [4, 6])
def test_channel_sum_variants(hw, pad, g_off):
    """locate_channel_sum: 16-byte loads where hw % 4 == 0, the batch stride % 4 == 0 and g is 16-byte aligned; each clause false
    in turn (hw = 6, a batch stride 2 elements wider than the slice, g one element off)."""
    B, C = 3, 5
    torch.manual_seed(900 + hw + pad)
    bs = C * hw + pad
    wide = torch.randn(B, bs)
    g = wide[:, :C * hw].reshape(B, C, hw)
    gg, out = offset_view(wide, g_off), offset_out((C,), 0)
    nbytes = L().locate_channel_sum_workspace_bytes(B, C, hw)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev())
    call("locate_channel_sum", gg.data_ptr(), out.data_ptr(), B, C, hw, bs, ws.data_ptr(), S())
    guards_intact(gg, out)
    want = g.double().sum((0, 2))
    err = ((out.cpu().double() - want).abs() / g.double().abs().sum((0, 2))).max().reshape(1)
    one = torch.ones(1, dtype=torch.float64)
    assert_close(torch.cat([err, one]), torch.cat([0 * one, one]), 2e-6, "channel sums hw = %d, stride + %d, g + %d" % (hw, pad, g_off))


# ------------------------------------------------------------------------------------------------ spectral-norm power iteration
# narrow row dot: 16-byte and scalar row bodies | wide row dot (wd >= 1024): the same two | two 64-row chunks, the second of one row |
# 71 rows: a 7-row remainder the unroll by 8 does not divide, two column strips | the finaliser's 4-way unrolled loop (wd > 3072)
# with a tail
SN_SHAPES = [(5, 12), (5, 13), (3, 1024), (3, 1027), (65, 8), (71, 260), (2, 4100)]
_SN_REC = struct.Struct("<8Q4i")


def _sn_operands(h, wd, seed):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(h, wd, generator=gen)
    u = torch.randn(h, generator=gen)
    v = torch.randn(wd, generator=gen)
    return w, u / u.norm(), v / v.norm()


def _sn_ref(w, u):
    """spectral_norm.py:26-31 in float64: v = l2n(W^T u), u = l2n(W v), sigma = u . (W v)"""
    w, u = w.double(), u.double()
    t = w.t().mv(u)
    v = t / (t.norm() + 1e-12)
    s = w.mv(v)
    u2 = s / (s.norm() + 1e-12)
    sigma = u2.dot(s)
    return u2, v, torch.stack([sigma, 1.0 / sigma]), s


def _sn_check(res, ref, what):
    for got, want, name in zip(res, ref, ("u", "v", "sigma", "wv")):
        assert_close(got.cpu(), want, 1e-5, "%s: %s" % (what, name))


@pytest.mark.parametrize("which", ["none", "w", "workspace"])
@pytest.mark.parametrize("h,wd", SN_SHAPES)
def test_power_iteration_variants(h, wd, which):
    """locate_sn_power_iter, one step from seeded u and v.  sn_row_partial reads a row of W with 16-byte loads where wd % 4 == 0 and
    the row pointer is 16-byte aligned (W one element off: every row scalar) and t with 16-byte loads where t is aligned (the
    workspace one element off: t scalar under 16-byte rows of W)."""
    w, u, v = _sn_operands(h, wd, 1000 + h + wd)
    ref = _sn_ref(w, u)
    wg, ug, vg = offset_view(w, int(which == "w")), offset_view(u, 0), offset_view(v, 0)
    sigma, wv = offset_out((2,), 0), offset_out((h,), 0)
    ws = offset_out((L().locate_sn_workspace_bytes(h, wd) // 4,), int(which == "workspace"))
    call("locate_sn_power_iter", wg.data_ptr(), ug.data_ptr(), vg.data_ptr(), sigma.data_ptr(), wv.data_ptr(), h, wd, ws.data_ptr(), S())
    guards_intact(wg, ug, vg, sigma, wv, ws)
    _sn_check((ug, vg, sigma, wv), ref, "power iteration %d x %d, %s offset" % (h, wd, which))


@pytest.mark.parametrize("w_off", [0, 1])
def test_power_iteration_batched_mixes_narrow_and_wide(w_off):
    """locate_sn_power_iter_batched over a table that mixes a narrow layer (9 x 40: a wave per row, three blocks of its own) with a
    wide one (2 x 1024: a block per row): the grid is sized by the maxima over the table, every layer takes its own form."""
    shapes = [(9, 40), (2, 1024)]
    layers, table = [], bytearray()
    for k, (h, wd) in enumerate(shapes):
        w, u, v = _sn_operands(h, wd, 1100 + k)
        nchunk = (h + 63) // 64
        wg, ug, vg = offset_view(w, w_off), offset_view(u, 0), offset_view(v, 0)
        sigma, wv = offset_out((2,), 0), offset_out((h,), 0)
        ws = offset_out((wd + h + nchunk * wd,), 0)
        assert ws.numel() * 4 == L().locate_sn_workspace_bytes(h, wd)
        base = ws.data_ptr()
        table += _SN_REC.pack(wg.data_ptr(), ug.data_ptr(), vg.data_ptr(), sigma.data_ptr(), wv.data_ptr(), base, base + 4 * wd,
                              base + 4 * (wd + h), h, wd, nchunk, 0)
        layers.append((w, u, (wg, ug, vg, sigma, wv, ws)))
    assert L().locate_sn_table_record_bytes() == _SN_REC.size
    tab = torch.frombuffer(table, dtype=torch.uint8).clone().to(dev())
    call("locate_sn_power_iter_batched", tab.data_ptr(), len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes), S())
    for (h, wd), (w, u, views) in zip(shapes, layers):
        guards_intact(*views)
        _sn_check((views[1], views[2], views[3], views[4]), _sn_ref(w, u), "batched power iteration %d x %d, W + %d" % (h, wd, w_off))


# ------------------------------------------------------------------------------------------------ operators on offset tensors
# (input, gradient) offsets in elements: the gradient alone first - the backward entry points refuse it on their own -, then both,
# then the aligned call the other two must equal bit for bit
OPERATOR_OFFSETS = ((0, 1), (1, 1), (0, 0))


def _unary(name):
    from locate_amd import ops
    from oracle import locate_oracle as O
    if name == "root_tanh":
        return ops.root_tanh, O.root_tanh, 2e-6, 3e-6
    return ops.tanh, torch.tanh, 2e-6, 5e-6


@pytest.mark.parametrize("n", [7, 1028])
@pytest.mark.parametrize("name", ["root_tanh", "tanh"])
def test_unary_operators_accept_offset_tensors(name, n):
    """ops.root_tanh / ops.tanh on an input one element into its buffer, with the gradient handed to backward() as such a view
    (what the second slice of a torch.cat(dim=0) backward with an odd element count is): locate_roottanh_* / locate_tanh_* have
    16-byte accesses only and refuse such pointers, so the operator copies them first.  n = 7: one 16-byte group and the scalar tail;
    1028: 16-byte groups only.  Against float64, and bit for bit the same call on aligned copies."""
    fn, ref_fn, tol_y, tol_dx = _unary(name)
    torch.manual_seed(n)
    x0, g0 = torch.randn(n) * 3, torch.randn(n)
    xr = x0.double().requires_grad_(True)
    yr = ref_fn(xr)
    yr.backward(g0.double())
    res = []
    for x_off, g_off in OPERATOR_OFFSETS:
        x = offset_view(x0, x_off).requires_grad_(True)
        g = offset_view(g0, g_off)
        y = fn(x)
        y.backward(g)
        guards_intact(x, g)
        assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(g), bits(g0)), "the operands are only read"
        assert_close(y.detach().cpu(), yr.detach(), tol_y, "%s n = %d, x + %d, g + %d: y" % (name, n, x_off, g_off))
        assert_close(x.grad.cpu(), xr.grad, tol_dx, "%s n = %d, x + %d, g + %d: dx" % (name, n, x_off, g_off))
        res.append((bits(y), bits(x.grad)))
    assert all(torch.equal(p, q) for r in res[:-1] for p, q in zip(r, res[-1])), "offset and aligned calls differ"


@pytest.mark.parametrize("shape", [(1, 7, 1, 1), (1, 257, 2, 2)], ids=["n7", "n1028"])
@pytest.mark.parametrize("with_act", [False, True], ids=["plain", "act"])
def test_inplace_norm_accepts_offset_tensors(with_act, shape):
    """ops.inplace_norm (with and without the fused activation) on an input one element into its buffer and a gradient handed to
    backward() as such a view; 7 and 1028 elements (2 x 2 planes: the small-plane backward, which needs x and g aligned)."""
    from locate_amd import ops
    torch.manual_seed(sum(shape))
    B, C = shape[:2]
    x0 = torch.randn(shape) * 1.7 + 0.4
    y0, b0, g0 = torch.randn(1, C, 1, 1), torch.randn(1, C, 1, 1), torch.randn(shape)
    out_ref, dx_ref, dy_ref, db_ref = _norm_ref(x0, y0, b0, g0, with_act)
    res = []
    for x_off, g_off in OPERATOR_OFFSETS:
        x = offset_view(x0, x_off).requires_grad_(True)
        g = offset_view(g0, g_off)
        y, b = (t.to(dev()).requires_grad_(True) for t in (y0, b0))
        out = ops.inplace_norm(x, y, b, with_act)
        out.backward(g)
        guards_intact(x, g)
        assert torch.equal(bits(x), bits(x0)) and torch.equal(bits(g), bits(g0)), "the operands are only read"
        what = "norm %s act = %d, x + %d, g + %d" % (shape, with_act, x_off, g_off)
        assert_close(out.detach().cpu(), out_ref, 1e-5, what + ": out")
        assert_close(x.grad.cpu(), dx_ref, 5e-5, what + ": dx")
        assert_close(y.grad.cpu(), dy_ref, 5e-5, what + ": dscale")
        assert_close(b.grad.cpu(), db_ref, 5e-5, what + ": dbias")
        res.append(tuple(bits(t) for t in (out, x.grad, y.grad, b.grad)))
    assert all(torch.equal(p, q) for r in res[:-1] for p, q in zip(r, res[-1])), "offset and aligned calls differ"


def test_aligned_tensors_pass_through_the_alignment_helper_untouched():
    """ops._c16 returns an aligned contiguous tensor as the object it is (no copy, no launch) and copies only an offset one."""
    from locate_amd import ops
    t = torch.randn(12, device=dev())
    assert ops._c16(t) is t
    v = offset_view(torch.randn(12), 1)
    c = ops._c16(v)
    assert c is not v and c.data_ptr() % 16 == 0 and torch.equal(c, v)
    v4 = offset_view(torch.randn(12), 4)
    assert ops._c16(v4) is v4
