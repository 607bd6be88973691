"""The deferred end-of-pass gradient kernels, through the C ABI, record by record: locate_fin_sn_rank1 / _sn_dots / _sums /
_channel_sums, locate_norm_bwd_fused + locate_fin_norm_channels, locate_sn_dv_batched and the power iteration - what a training
step and bench.py run (ops.Runtime with defer_finalisers), while tests/test_gpu_ops.py drives the per-layer entry points.

Every test compares with the float64 models of tests/helpers/finaliser_model.py and, where include/locate_hip.h promises "same
arithmetic and summation order as the per-layer entry points: bit-identical results", asserts torch.equal with that entry point
on the same inputs.  Needs an MI355X: run with -m gpu.

Tolerances (conftest's normalised max error unless said otherwise), each taken from what the immediate path is held to:
  norm dx / dscale / dbias 5e-5 (test_inplace_norm_fused_activation_and_big); dgamma 2e-5 (test_residual_gate_large_vs_oracle);
  dots 2e-5 of the sum of magnitudes (test_weight_side_group_dots); u, v, wv, sigma, 1/sigma 1e-5 and gw after the rank-1 term
  3e-5 (test_spectral_norm_layers_golden); du, dv, dsigma 1e-5 here, because the test supplies the partial sums itself: they are
  exact in double, only fp32 roundings of the result remain (the 5e-4 of test_spectral_norm_layers_golden is for a dsigma that
  comes out of a real weight gradient); the scalar dsigma_total as a fraction of sum_k |dsigma_k|, what its roundings scale with.
  Channel sums: |got - want| <= 2e-6 sum |g|.  Derived: an element passes through at most 2 additions inside its 16-byte load,
  ceil(B hw / 4096) <= 2 of its thread's running sum (the shapes below), 6 of the wave butterfly, 16 of the block's wave results
  and - sliced - 8 slices: under 32 additions, each with a relative rounding of 2^-24, on partial sums bounded by sum |g|:
  32 x 2^-24 = 1.9e-6."""
import os
import struct
import sys

import pytest
import torch

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import finaliser_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def S():
    return torch.cuda.current_stream().cuda_stream


def L():
    from locate_amd._lib import lib
    return lib()


def rec(ptrs, longs=(), ints=()):
    from locate_amd import ops
    return ops.Runtime._rec(ptrs, longs, ints)


def run(name, records):
    from locate_amd._lib import check
    assert L().locate_fin_record_bytes() == len(records[0]) == 112
    check(getattr(L(), name)(b"".join(records), len(records), S()), name)


def assert_within(got, want, magnitude, tol, what):
    """|got - want| <= tol * magnitude, element by element (a sum's error is a fraction of the sum of its terms' magnitudes)."""
    got, want, magnitude = (torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, want, magnitude))
    err = ((got - want).abs() / magnitude.clamp_min(1e-300)).max().reshape(1)
    one = torch.ones(1, dtype=torch.float64)
    assert_close(torch.cat([err, one]), torch.cat([0 * one, one]), tol, what)


# ------------------------------------------------------------------------------------------------ rank-1 term, du, dsigma
RANK1_SHAPES = [(1, 1), (3, 4), (7, 75), (6, 100), (33, 1028), (65, 1023), (768, 3072)]
# (npartial per call, sigma_stride, wv_stride - h, du wanted, dsigma_out wanted)
RANK1_VARIANTS = [(1, 2, 0, True, True), (255, 6, 3, True, False), (256, 2, 3, False, True), (257, 6, 0, True, True),
                  (1000, 2, 3, False, False)]


class Rank1Case:
    """One rank-1 record with its operands on the device and on the host.  The partial sums are positive (no cancellation in
    sum_k dsigma_k: the comparison of a scalar would otherwise be a comparison with the rounding of a difference) and differ by
    call, as do sigma_k and the rows of wv: a kernel that mixes the calls up is off by tens of percent."""

    def __init__(self, seed, h, wd, groups, variant, misalign=False):
        npartial, sigma_stride, wv_pad, want_du, want_dsig = variant
        gen = torch.Generator().manual_seed(seed)
        k = max(groups, 1)
        self.h, self.wd, self.groups, self.npartial, self.sigma_stride = h, wd, groups, npartial, sigma_stride
        self.gw_in = torch.randn(h, wd, generator=gen)
        self.u, self.v = torch.randn(h, generator=gen), torch.randn(wd, generator=gen)
        self.partial = (torch.rand(k, npartial, generator=gen, dtype=torch.float64) + 0.25) * \
            torch.arange(1, k + 1, dtype=torch.float64)[:, None] / npartial
        sig = torch.rand(k, generator=gen) + 0.5
        self.tab = torch.full((k, sigma_stride), 7.0)          # (the filler would show in dsigma if the stride were ignored)
        self.tab[:, 0], self.tab[:, 1] = sig, 1.0 / sig
        self.wv = torch.randn(k, h + wv_pad, generator=gen)
        d = dev()
        self.d_partial, self.d_tab, self.d_u, self.d_v, self.d_wv = (t.to(d) for t in (self.partial, self.tab, self.u, self.v, self.wv))
        if misalign:          # gw starts 4 bytes into its buffer: no 16-byte accesses, whatever wd is
            self.buf = torch.full((h * wd + 1,), 123.0, device=d)
            self.d_gw = self.buf[1:].view(h, wd)
            self.d_gw.copy_(self.gw_in)
            assert self.d_gw.data_ptr() % 16 == 4
        else:
            self.d_gw = self.gw_in.to(d)
        self.d_du = torch.full((h,), float("nan"), device=d) if want_du else None
        self.d_dsig = torch.full((1,), float("nan"), device=d) if want_dsig else None

    def record(self):
        return rec([self.d_partial, self.d_tab, self.d_u, self.d_v, self.d_wv, self.d_gw, self.d_du, self.d_dsig],
                   [self.wv.shape[1]], [self.npartial, self.groups, self.sigma_stride, self.h, self.wd])

    def verify(self, what):
        gw, du, total = M.sn_rank1(self.gw_in, self.partial, self.u, self.v, self.tab, self.wv, self.groups)
        assert_close(self.d_gw.cpu(), gw, 3e-5, what + " gw")
        if self.d_du is not None:
            assert_close(self.d_du.cpu(), du, 1e-5, what + " du")
        if self.d_dsig is not None:
            # the sum of the fp32-rounded dsigma_k: its error is a fraction of sum_k |dsigma_k| (dots of real data may cancel)
            sums, sig = self.partial.reshape(max(self.groups, 1), -1).sum(1), self.tab[:, 0].double()
            magnitude = (sums.abs() / (sig * sig if self.groups == 0 else sig)).sum()
            assert_within(self.d_dsig.cpu(), total, magnitude, 1e-5, what + " dsigma")

    def verify_immediate(self, what):
        """groups = 0: locate_sn_weight_bwd on the same inputs gives the same bits."""
        from locate_amd._lib import check
        assert self.groups == 0
        d = dev()
        gw = self.gw_in.to(d)
        du, dsig = torch.empty(self.h, device=d), torch.empty(1, device=d)
        check(L().locate_sn_weight_bwd(self.d_partial.data_ptr(), self.npartial, self.d_u.data_ptr(), self.d_v.data_ptr(),
                                       self.d_tab.data_ptr(), self.d_wv.data_ptr(), gw.data_ptr(), du.data_ptr(), dsig.data_ptr(),
                                       self.h, self.wd, S()), "locate_sn_weight_bwd")
        assert torch.equal(gw, self.d_gw), what + " gw bits"
        assert self.d_du is None or torch.equal(du, self.d_du), what + " du bits"
        assert self.d_dsig is None or torch.equal(dsig, self.d_dsig), what + " dsigma bits"


@pytest.mark.parametrize("groups", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("h,wd", RANK1_SHAPES)
def test_fin_sn_rank1_single_records(h, wd, groups):
    """Both meanings of the record (groups 0: one call, dsigma from the weight-side partials; k >= 1: stacked calls), partial
    counts around the block size, both table strides, padded wv rows, du / dsigma_out present and absent; 16-byte and scalar
    bodies by shape; (768, 3072) needs more blocks than the grid's cap."""
    for i, variant in enumerate(RANK1_VARIANTS):
        c = Rank1Case(1000 * h + 10 * groups + i, h, wd, groups, variant)
        run("locate_fin_sn_rank1", [c.record()])
        what = "rank1 %dx%d groups %d variant %d" % (h, wd, groups, i)
        c.verify(what)
        if groups == 0:
            c.verify_immediate(what)


@pytest.mark.parametrize("groups", [0, 3])
def test_fin_sn_rank1_unaligned_gw_takes_the_scalar_body(groups):
    for h, wd in ((6, 100), (33, 1028)):
        assert wd % 4 == 0
        c = Rank1Case(77 + groups, h, wd, groups, RANK1_VARIANTS[3], misalign=True)
        run("locate_fin_sn_rank1", [c.record()])
        assert float(c.buf[0]) == 123.0          # (the word in front of the view is not gw's)
        c.verify("rank1 unaligned %dx%d groups %d" % (h, wd, groups))
        if groups == 0:
            c.verify_immediate("rank1 unaligned %dx%d" % (h, wd))


@pytest.mark.parametrize("n_records", [1, 32, 33, 70])
def test_fin_sn_rank1_many_records_in_one_call(n_records):
    """Records of mixed sizes and meanings in one call, below, at and above the 32 a launch takes: every block finds its record
    by the first-block table, every record is checked.  Several records have tens of blocks, one has the capped 2048."""
    small = RANK1_SHAPES[:6]
    cases = []
    for i in range(n_records):
        h, wd = small[(i * 5 + 4) % 6] if n_records > 1 else (33, 1028)
        if n_records == 70 and i == 35:
            h, wd = RANK1_SHAPES[6]
        cases.append(Rank1Case(31 * n_records + i, h, wd, i % 5, RANK1_VARIANTS[(i // 5) % 5], misalign=(i % 11 == 7)))
    run("locate_fin_sn_rank1", [c.record() for c in cases])
    for i, c in enumerate(cases):
        what = "rank1 record %d of %d (%dx%d groups %d)" % (i, n_records, c.h, c.wd, c.groups)
        c.verify(what)
        if c.groups == 0:
            c.verify_immediate(what)


# ------------------------------------------------------------------------------------------------ dots of stacked calls
DOT_SHAPES = [(1, 1, 1), (3, 5, 7), (4, 16, 64), (2, 33, 128), (5, 96, 1024), (3, 1025, 4), (130, 3, 2048)]
#   (3, 5, 7): scalar body; (2, 33, 128) and (3, 1025, 4): M * plane = 4224 / 4100, a short last chunk (of 4 elements in the second);
#   Bg * chunks = 120 blocks for (5, 96, 1024), 260 > 256 for (130, 3, 2048): blocks that take a second piece of work


def _strided(shape, layout, gen):
    """A [B, M, plane] operand: dense, a channel slice of a wider tensor (its own batch stride), or rows an odd number of
    elements apart (batch stride % 4 != 0: no 16-byte accesses)."""
    B, Mn, plane = shape
    if layout == "dense":
        host = torch.randn(B, Mn, plane, generator=gen)
        return host, host.to(dev())
    if layout == "slice":
        wide = torch.randn(B, Mn + 5, plane, generator=gen).to(dev())
        view = wide[:, 2:2 + Mn]
    else:
        flat = torch.randn(B * (Mn * plane + 3), generator=gen).to(dev())
        view = flat.as_strided((B, Mn, plane), (Mn * plane + 3, plane, 1))
        assert view.stride(0) % 4 != 0 or plane % 4 != 0
    assert not view.is_contiguous() or B == 1
    return view.cpu().contiguous(), view


class DotCase:
    def __init__(self, seed, Bg, Mn, plane, groups, with_bias, gy_layout="dense", y_layout="dense"):
        gen = torch.Generator().manual_seed(seed)
        self.Bg, self.M, self.plane, self.groups = Bg, Mn, plane, groups
        shape = (Bg * groups, Mn, plane)
        self.gy, self.d_gy = _strided(shape, gy_layout, gen)
        self.y, self.d_y = _strided(shape, y_layout, gen)
        self.bias = torch.randn(Mn, generator=gen) if with_bias else None
        self.d_bias = self.bias.to(dev()) if with_bias else None
        self.np = L().locate_fin_sn_dot_partials(Bg, Mn, plane)
        chunks = Bg * ((Mn * plane + 4095) // 4096)
        assert self.np == min(chunks, 256)
        self.d_partial = torch.full((groups, self.np), float("nan"), dtype=torch.float64, device=dev())

    def record(self):
        return rec([self.d_gy, self.d_y, self.d_bias, self.d_partial], [self.d_gy.stride(0), self.d_y.stride(0)],
                   [self.groups, self.Bg, self.M, self.plane])

    def verify(self, what):
        dots, mags = M.sn_dots(self.gy, self.y, self.bias, self.groups)
        got = self.d_partial.cpu()
        assert torch.isfinite(got).all(), what + ": a partial sum was not written"
        assert_within(got.sum(1), dots, mags, 2e-5, what)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
@pytest.mark.parametrize("Bg,Mn,plane", DOT_SHAPES)
def test_fin_sn_dots_vs_float64(Bg, Mn, plane, groups, with_bias):
    c = DotCase(Bg * 1000 + Mn + groups, Bg, Mn, plane, groups, with_bias)
    run("locate_fin_sn_dots", [c.record()])
    c.verify("dots %s groups %d bias %d" % ((Bg, Mn, plane), groups, with_bias))


DOT_LAYOUTS = [((4, 16, 64), "dense", "slice"), ((4, 16, 64), "odd", "dense"), ((2, 33, 128), "slice", "slice"),
               ((3, 5, 7), "dense", "slice"), ((3, 5, 7), "odd", "odd"), ((3, 1025, 4), "dense", "odd")]


def test_fin_sn_dots_strided_operands_and_many_records():
    """y as a channel-slice view with its own batch stride, batch strides that rule the 16-byte body out, and 33 records of mixed
    shape in one call (two launches)."""
    cases = [DotCase(50 + i, *shape, groups=1 + i % 4, with_bias=i % 2 == 0, gy_layout=gl, y_layout=yl)
             for i, (shape, gl, yl) in enumerate(DOT_LAYOUTS)]
    for c in cases:
        run("locate_fin_sn_dots", [c.record()])
    small = DOT_SHAPES[:4] + [DOT_SHAPES[5]]
    many = [DotCase(500 + i, *small[i % 5], groups=1 + (i * 3) % 4, with_bias=i % 3 != 0) for i in range(33)]
    run("locate_fin_sn_dots", [c.record() for c in many])
    for i, c in enumerate(cases + many):
        c.verify("dots case %d %s groups %d" % (i, (c.Bg, c.M, c.plane), c.groups))


@pytest.mark.parametrize("shape,gy_layout,y_layout,h,wd", [((4, 16, 64), "dense", "dense", 16, 36), ((3, 5, 7), "dense", "slice", 5, 9),
                                                           ((2, 33, 128), "slice", "dense", 33, 1028), ((130, 3, 2048), "dense", "dense", 3, 27),
                                                           ((4, 16, 64), "odd", "dense", 65, 1023)])
@pytest.mark.parametrize("groups", [1, 2, 3, 4])
def test_dots_then_rank1_equal_the_grouped_entry_point_bit_for_bit(shape, gy_layout, y_layout, h, wd, groups):
    """locate_fin_sn_dots feeding locate_fin_sn_rank1 (stacked meaning) against locate_sn_weight_bwd_grouped on the same inputs:
    gw, du, dsigma bit for bit.  Against float64 the rank-1 term is checked from the dots the kernel left (the dots themselves:
    test_fin_sn_dots_vs_float64)."""
    from locate_amd._lib import check
    d = dev()
    dot = DotCase(groups * 10 + h, *shape, groups=groups, with_bias=True, gy_layout=gy_layout, y_layout=y_layout)
    r1 = Rank1Case(groups * 13 + wd, h, wd, groups, (dot.np, 6, 3, True, True))
    r1.d_partial = dot.d_partial
    run("locate_fin_sn_dots", [dot.record()])
    run("locate_fin_sn_rank1", [r1.record()])
    gw = r1.gw_in.to(d)
    du, dsig = torch.empty(h, device=d), torch.empty(1, device=d)
    ws = torch.empty(L().locate_sn_group_workspace_bytes(), dtype=torch.uint8, device=d)
    check(L().locate_sn_weight_bwd_grouped(dot.d_gy.data_ptr(), dot.d_gy.stride(0), dot.d_y.data_ptr(), dot.d_y.stride(0),
                                           dot.d_bias.data_ptr(), groups, dot.Bg, dot.M, dot.plane, r1.d_tab.data_ptr(), 6,
                                           r1.d_u.data_ptr(), r1.d_v.data_ptr(), r1.d_wv.data_ptr(), r1.wv.shape[1], gw.data_ptr(),
                                           du.data_ptr(), dsig.data_ptr(), h, wd, ws.data_ptr(), S()), "locate_sn_weight_bwd_grouped")
    what = "dots %s + rank1 %dx%d groups %d" % (shape, h, wd, groups)
    assert torch.equal(ws.view(torch.float64)[:groups * dot.np].view(groups, dot.np), dot.d_partial), what + " dot bits"
    assert torch.equal(gw, r1.d_gw), what + " gw bits"
    assert torch.equal(du, r1.d_du), what + " du bits"
    assert torch.equal(dsig, r1.d_dsig), what + " dsigma bits"
    r1.partial = dot.d_partial.cpu()
    r1.verify(what)


# ------------------------------------------------------------------------------------------------ the gates' dgamma
GATE_SHAPES = [(5, 7, 2, 2), (6, 33, 4, 4), (3, 64, 1, 1), (8, 48, 64, 64)]


class GateCase:
    def __init__(self, seed, shape, per_plane):
        from locate_amd._lib import check
        gen = torch.Generator().manual_seed(seed)
        d = dev()
        B, C = shape[:2]
        planes, hw = B * C, shape[2] * shape[3]
        self.x, self.g = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
        a = torch.randn((B, C, 1, 1) if per_plane else shape, generator=gen)
        gamma = torch.tensor([[3.0]])
        dx, dg, da, dgam = self.x.to(d), self.g.to(d), a.to(d), gamma.to(d)
        self.count = L().locate_gate_bwd_partials(planes, hw)
        self.ws = torch.full((L().locate_gate_bwd_workspace_bytes(planes) // 8,), float("nan"), dtype=torch.float64, device=d)
        ws2 = torch.empty_like(self.ws)
        self.immediate = torch.empty(1, device=d)
        self.out = torch.full((1,), float("nan"), device=d)
        for w, dgamma in ((self.ws, None), (ws2, self.immediate.data_ptr())):
            gx, ga = torch.empty_like(dx), torch.empty_like(da)
            check(L().locate_gate_bwd(dx.data_ptr(), da.data_ptr(), int(per_plane), dgam.data_ptr(), dg.data_ptr(), gx.data_ptr(),
                                      ga.data_ptr(), dgamma, planes, hw, w.data_ptr(), 0, None, S()), "locate_gate_bwd")
        self.what = "dgamma %s per_plane %d" % (shape, per_plane)

    def record(self):
        return rec([self.ws, self.out], [], [self.count])

    def verify(self):
        assert torch.equal(self.out, self.immediate), self.what + " bits"
        want = (self.x.double() ** 2 * self.g.double()).sum().reshape(1)          # x^2 g, as the reference codes it (libs/merge.py:33-38)
        assert_close(self.out.cpu(), want, 2e-5, self.what)


@pytest.mark.parametrize("per_plane", [False, True])
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_fin_sums_of_gate_workspaces(shape, per_plane):
    """locate_gate_bwd(dgamma = NULL) leaves its block sums, locate_fin_sums adds them: bit for bit locate_gate_bwd(dgamma)."""
    c = GateCase(shape[1] + per_plane, shape, per_plane)
    run("locate_fin_sums", [c.record()])
    c.verify()


def test_fin_sums_forty_records_in_one_call():
    combos = [(s, p) for s in GATE_SHAPES[:3] for p in (False, True)]
    cases = [GateCase(900 + i, *combos[i % 6]) for i in range(38)]
    cases[13:13] = [GateCase(950, GATE_SHAPES[3], False)]
    cases[31:31] = [GateCase(951, GATE_SHAPES[3], True)]
    assert len(cases) == 40
    run("locate_fin_sums", [c.record() for c in cases])
    for c in cases:
        c.verify()


# ------------------------------------------------------------------------------------------------ bias gradients
#   (B, C, hw, channel-slice view): scalar bodies; sixteen (channel, slice) pairs per block; slices > 1 (partial buffer + final
#   kernel); C >= 512 (never sliced); views with a batch stride of their own, one of them sliced, one unaligned
#   (40, 3, 35) and (8, 300, 2400): slices of more than 1024 (16-byte) elements - a block per (channel, slice), scalar and sliced
CHANNEL_CASES = [(5, 7, 1, False), (3, 20, 35, False), (6, 40, 64, False), (8, 6, 1024, False), (4, 512, 2048, False),
                 (6, 40, 64, True), (8, 6, 1024, True), (3, 20, 35, True), (40, 3, 35, False), (8, 300, 2400, False)]


class ChannelCase:
    def __init__(self, seed, B, C, hw, view):
        gen = torch.Generator().manual_seed(seed)
        d = dev()
        self.B, self.C, self.hw = B, C, hw
        if view:
            self.d_g = torch.randn(B, C + 3, hw, generator=gen).to(d)[:, 1:1 + C]
        else:
            self.d_g = torch.randn(B, C, hw, generator=gen).to(d)
        self.g = self.d_g.cpu().contiguous()
        self.slices = L().locate_fin_channel_slices(B, C, hw)
        self.part = torch.full((self.slices * C,), float("nan"), device=d) if self.slices > 1 else None
        self.out = torch.full((C,), float("nan"), device=d)
        self.what = "channel sums %s view %d" % ((B, C, hw), view)

    def record(self):
        return rec([self.d_g, self.out, self.part], [self.d_g.stride(0)], [self.B, self.C, self.hw])

    def verify(self):
        from locate_amd._lib import check
        d = dev()
        nbytes = L().locate_channel_sum_workspace_bytes(self.B, self.C, self.hw)
        assert (nbytes > 0) == (self.slices > 1)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=d)
        imm = torch.empty(self.C, device=d)
        check(L().locate_channel_sum(self.d_g.data_ptr(), imm.data_ptr(), self.B, self.C, self.hw, self.d_g.stride(0), ws.data_ptr(), S()),
              "locate_channel_sum")
        assert torch.equal(self.out, imm), self.what + " bits"
        sums, mags = M.channel_sums(self.g)
        assert_within(self.out, sums, mags, 2e-6, self.what)


@pytest.mark.parametrize("B,C,hw,view", CHANNEL_CASES)
def test_fin_channel_sums_single_records(B, C, hw, view):
    c = ChannelCase(B * 100 + C, B, C, hw, view)
    assert (c.slices > 1) == ((B, C, hw) in ((8, 6, 1024), (8, 300, 2400)))
    run("locate_fin_channel_sums", [c.record()])
    c.verify()


def test_fin_channel_sums_mixed_and_33_records_in_one_call():
    """All forms in one call (sliced and unsliced records side by side: the final kernel skips the unsliced ones), then 33 records:
    two launches, the second with one record."""
    mixed = [ChannelCase(300 + i, *case) for i, case in enumerate(CHANNEL_CASES)]
    run("locate_fin_channel_sums", [c.record() for c in mixed])
    light = [c for c in CHANNEL_CASES if c[0] * c[1] * c[2] < 100000]
    assert len(light) == 8
    many = [ChannelCase(400 + i, *light[(i * 3) % 8]) for i in range(32)] + [ChannelCase(433, *CHANNEL_CASES[4])]
    run("locate_fin_channel_sums", [c.record() for c in many])
    for c in mixed + many:
        c.verify()


# ------------------------------------------------------------------------------------------------ InPlaceNorm, two-launch backward
# ((B, C, H, W), per-sample scale, groups): the rows of tests/test_gpu_deferred_layers.py
NORM_ROWS = [((6, 34, 1, 1), False, 3), ((12, 20, 2, 2), True, 3), ((8, 17, 4, 4), False, 4), ((3, 5, 5, 7), False, 1),
             ((9, 40, 6, 6), True, 3), ((6, 48, 8, 16), True, 3), ((6, 18, 12, 12), False, 3), ((34, 10, 2, 2), False, 2),
             ((192, 768, 1, 1), True, 3), ((6, 96, 32, 32), False, 3)]


class NormCase:
    """Forward (for the statistics), the three-launch backward, and the two-launch backward whose plane sums wait in its workspace
    for locate_fin_norm_channels."""

    def __init__(self, seed, shape, per_sample, groups, with_act):
        from locate_amd._lib import check
        gen = torch.Generator().manual_seed(seed)
        d = dev()
        B, C = shape[:2]
        hw = shape[2] * shape[3]
        assert groups == 1 or (B // groups) * C * hw % 4 == 0          # what the entry points require of stacked calls
        self.args = (per_sample, groups, with_act)
        self.x = torch.randn(shape, generator=gen) * 1.7 + 0.4
        self.scale = torch.randn(B if per_sample else 1, C, 1, 1, generator=gen)
        self.bias = torch.randn(1, C, 1, 1, generator=gen)
        self.g = torch.randn(shape, generator=gen)
        x, scale, bias, g = (t.to(d) for t in (self.x, self.scale, self.bias, self.g))
        self.stats = torch.empty(2 * groups, device=d)
        out = torch.empty_like(x)
        ws = torch.empty(L().locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=d)
        check(L().locate_norm_fwd(x.data_ptr(), scale.data_ptr(), int(per_sample), bias.data_ptr(), out.data_ptr(), int(with_act),
                                  self.stats.data_ptr(), B, C, hw, groups, ws.data_ptr(), None, None, S()), "locate_norm_fwd")
        self.dx1, self.dscale1, self.dbias1 = torch.empty_like(x), torch.empty_like(scale), torch.empty_like(bias)
        ws1 = torch.empty(L().locate_norm_bwd_workspace_bytes(B, C), dtype=torch.uint8, device=d)
        check(L().locate_norm_bwd(x.data_ptr(), g.data_ptr(), self.stats.data_ptr(), scale.data_ptr(), int(per_sample), bias.data_ptr(),
                                  int(with_act), self.dx1.data_ptr(), self.dscale1.data_ptr(), self.dbias1.data_ptr(), B, C, hw, groups,
                                  ws1.data_ptr(), 0, S()), "locate_norm_bwd")
        self.dx2 = torch.full_like(x, float("nan"))
        self.dscale2 = torch.full_like(scale, float("nan"))
        self.dbias2 = torch.full_like(bias, float("nan"))
        self.ws2 = torch.empty(L().locate_norm_bwd_fused_workspace_bytes(B, C), dtype=torch.uint8, device=d)
        check(L().locate_norm_bwd_fused(x.data_ptr(), g.data_ptr(), self.stats.data_ptr(), scale.data_ptr(), int(per_sample),
                                        bias.data_ptr(), int(with_act), self.dx2.data_ptr(), self.dscale2.data_ptr() if per_sample else None,
                                        B, C, hw, groups, self.ws2.data_ptr(), 0, S()), "locate_norm_bwd_fused")
        s1 = self.ws2.data_ptr() + L().locate_norm_bwd_fused_plane_offset()
        self.rec = rec([s1, s1 + 4 * B * C, self.stats, None if per_sample else self.dscale2, self.dbias2], [], [B, C, groups])
        self.what = "norm %s per_sample %d groups %d act %d" % (shape, per_sample, groups, with_act)

    def verify(self):
        per_sample, groups, with_act = self.args
        # the header's promise: the channel finaliser repeats norm_bwd_final_kernel's arithmetic on the same plane sums (the
        # per-sample scale gradient is the same quotient S2 / std, written by the plane kernel instead)
        assert torch.equal(self.dbias2, self.dbias1), self.what + " dbias bits"
        assert torch.equal(self.dscale2, self.dscale1), self.what + " dscale bits"
        dx, dscale, dbias, _ = M.norm_bwd(self.x, self.g, self.scale, self.bias, per_sample, groups, with_act)
        assert_close(self.dx2.cpu(), dx, 5e-5, self.what + " dx")
        assert_close(self.dx1.cpu(), dx, 5e-5, self.what + " dx (three launches)")
        assert_close(self.dscale2.cpu(), dscale, 5e-5, self.what + " dscale")
        assert_close(self.dbias2.cpu(), dbias, 5e-5, self.what + " dbias")


@pytest.mark.parametrize("with_act", [False, True])
@pytest.mark.parametrize("shape,per_sample,groups", NORM_ROWS)
def test_norm_bwd_fused_and_fin_norm_channels(shape, per_sample, groups, with_act):
    c = NormCase(shape[0] * 31 + shape[1] + with_act, shape, per_sample, groups, with_act)
    run("locate_fin_norm_channels", [c.rec])
    c.verify()


def test_fin_norm_channels_forty_records_in_one_call():
    small = [r for r in NORM_ROWS if r[0][0] * r[0][1] * r[0][2] * r[0][3] < 100000]
    cases = [NormCase(700 + i, *small[i % len(small)], with_act=bool((i // len(small)) % 2)) for i in range(40)]
    run("locate_fin_norm_channels", [c.rec for c in cases])
    for c in cases:
        c.verify()


# ------------------------------------------------------------------------------------------------ spectral norm tables
SN_TABLE = [(1, 5), (65, 300), (130, 1028), (8, 1)]
_SN_REC = struct.Struct("<8Q4i")          # SnLayer of csrc/spectral.hip: eight pointers, h, wd, nchunk, pad


class SnLayerCase:
    def __init__(self, seed, h, wd):
        gen = torch.Generator().manual_seed(seed)
        d = dev()
        self.h, self.wd = h, wd
        self.W = torch.randn(h, wd, generator=gen)
        u = torch.randn(h, generator=gen)
        self.u0 = u / u.norm()
        self.d_W, self.d_u = self.W.to(d), self.u0.to(d)
        self.d_v = torch.full((wd,), float("nan"), device=d)
        self.d_sigma = torch.full((4,), float("nan"), device=d)
        self.d_wv = torch.full((h,), float("nan"), device=d)
        self.nchunk = (h + 63) // 64
        self.scratch = torch.empty(wd + h + self.nchunk * wd, device=d)
        assert L().locate_sn_workspace_bytes(h, wd) == 4 * self.scratch.numel()

    def table_record(self):
        base = self.scratch.data_ptr()
        return _SN_REC.pack(self.d_W.data_ptr(), self.d_u.data_ptr(), self.d_v.data_ptr(), self.d_sigma.data_ptr(), self.d_wv.data_ptr(),
                            base, base + 4 * self.wd, base + 4 * (self.wd + self.h), self.h, self.wd, self.nchunk, 0)

    def verify_iteration(self, state, what):
        """state: the float64 model's (u, v, sigma, wv) after the same number of iterations."""
        u, v, sigma, wv = state
        assert_close(self.d_u.cpu(), u, 1e-5, what + " u")
        assert_close(self.d_v.cpu(), v, 1e-5, what + " v")
        assert_close(self.d_wv.cpu(), wv, 1e-5, what + " wv")
        assert_close(self.d_sigma[:1].cpu(), sigma.reshape(1), 1e-5, what + " sigma")
        assert_close(self.d_sigma[1:2].cpu(), 1 / sigma.reshape(1), 1e-5, what + " 1/sigma")


def _table(cases):
    assert L().locate_sn_table_record_bytes() == _SN_REC.size == 80
    host = torch.frombuffer(bytearray(b"".join(c.table_record() for c in cases)), dtype=torch.uint8).clone()
    return host.to(dev()), max(c.h for c in cases), max(c.wd for c in cases)


POWER_SHAPES = SN_TABLE + [(64, 1024), (768, 768)]
#   (65, 300), (130, 1028): two and three 64-row chunks; (130, 1028), (64, 1024): the block-per-row body (wd >= 1024) beside
#   wave-per-row layers under one padded grid; (1, 5), (8, 1): one row, one column


@pytest.mark.parametrize("batched", [False, True])
def test_power_iteration_two_rounds_vs_float64(batched):
    from locate_amd._lib import check
    cases = [SnLayerCase(60 + i, h, wd) for i, (h, wd) in enumerate(POWER_SHAPES)]
    states = [(c.u0.double(), None, None, None) for c in cases]
    if batched:
        table, max_h, max_wd = _table(cases)
    for it in range(2):
        if batched:
            check(L().locate_sn_power_iter_batched(table.data_ptr(), len(cases), max_h, max_wd, S()), "locate_sn_power_iter_batched")
        else:
            for c in cases:
                check(L().locate_sn_power_iter(c.d_W.data_ptr(), c.d_u.data_ptr(), c.d_v.data_ptr(), c.d_sigma.data_ptr(), c.d_wv.data_ptr(),
                                               c.h, c.wd, c.scratch.data_ptr(), S()), "locate_sn_power_iter")
        states = [M.power_iteration(c.W, s[0]) for c, s in zip(cases, states)]
        for c, s in zip(cases, states):
            c.verify_iteration((s[0], s[1], s[2], s[3]), "power iteration %d of %dx%d batched %d" % (it + 1, c.h, c.wd, batched))


def test_sn_dv_batched_vs_float64():
    """One table of four layers of mixed size under one padded grid: dv = (sum of the four slots) W^T u, slots cleared."""
    from locate_amd._lib import check
    cases = [SnLayerCase(80 + i, h, wd) for i, (h, wd) in enumerate(SN_TABLE)]
    slots = []
    for i, c in enumerate(cases):
        s = torch.tensor([0.75, -1.5, 0.375, 2.0]) * (i + 1)          # exact in fp32, any order of the four additions
        c.d_sigma.copy_(s)
        slots.append(s)
    table, max_h, max_wd = _table(cases)
    assert (max_h, max_wd) == (130, 1028)
    check(L().locate_sn_dv_batched(table.data_ptr(), len(cases), max_h, max_wd, S()), "locate_sn_dv_batched")
    for c, s in zip(cases, slots):
        assert_close(c.d_v.cpu(), M.dv(c.W, c.u0, s), 1e-5, "dv %dx%d" % (c.h, c.wd))
        assert torch.equal(c.d_sigma.cpu(), torch.zeros(4)), "slots of %dx%d not cleared" % (c.h, c.wd)
        assert torch.equal(c.d_u.cpu(), c.u0)
