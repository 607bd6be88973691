"""The largest-magnitude side channel of the scaled contractions (two fp16 pieces per operand, fp8), pinned bit for bit.

Every kernel that produces a contraction operand folds the largest magnitude of what it STORED into a set of device words
(absmax_publish / absmax_publish_wave, csrc/common.h); the consumer derives a power-of-two scale from them (f16_scale_exp /
f8_scale_exp, csrc/igemm.h).  The scaled maximum sits one binade below fp16's largest finite value, so a producer that loses a
corner of its tensor (scalar tail, last chunk, masked row tile, ragged plane group) or counts something it did not store (a padded
row, a neighbour's words, stale words) goes unseen by every normalised-error bound.  The assertions here are identities:

    A  word_bits(words) == bits(stored.abs().max())   for every producer, with the maximum steered into each such corner and the
       word sets on either side of the kernel's own left untouched (the kernel gets the middle third of a zeroed tensor);
    B  the host plumbing of the tag (version stamp, views, the arena's hand-outs);
    C  y(2^s x, w) == ldexp(y(x, w), s) for every piece form: the scale arithmetic (exponent from the word bits, pow2f, the two
       un-scales after the K loop) is exact, from s = -96 to s = +116 for the scaled forms;
    D  the edges of the scale (a maximum that is a power of two, the value just below one, all-zero operands, one non-zero element).

No assertion of A, B, C or of the zero cases of D carries a tolerance.  The only tolerances in the file are those of
test_conv_fp16_pieces_vs_cpu in test_gpu_ops.py (2e-5 for y and dx, 5e-5 for dw, normalised max error against a float64 CPU conv),
used in D where the issue is "finite and as accurate as ever", not an identity.

Producer table (grep -n absmax_publish locate_amd/csrc):

    kernel                            path                                         case id
    absmax_kernel                     one block ... several grid-stride wraps       test_locate_absmax[n]
    unary_fwd_kernel<0>               vector loop / scalar tail / both / grid cap   test_roottanh_fwd_words[n]
    unary_bwd_kernel<0>               the same, accumulate 0 and 1                  test_roottanh_bwd_words[n-acc]
    norm_apply_fused_kernel<ACT>      hw % 4 == 0 and scalar, groups 1 / 3, cap     test_norm_fwd_words[...]
    gate_bwd_small_kernel<1..32>      hw 4 ... 128, ragged last plane group         test_gate_bwd_words[5-4 ... 67-128, 128-1]
    gate_bwd_plane_kernel<1>          vector (hw 36, 576), scalar (35), > 16384     test_gate_bwd_words[5-36, 7-576, 5-35, 16421-36]
    gate_bwd_plane_kernel<4>          hw 1024                                       test_gate_bwd_words[3-1024]
    igemm_epilogue, general           act_out, ragged M and N, K not split          test_epilogue_words[general-fwd-*] (bf16x3, f16x2, fp8)
                                      mul_pre, the same                             test_epilogue_words[general-dgrad-*] (bf16x3, f16x2, fp8)
    igemm_epilogue, staged            act_out (rolled loop), 96- and 64-row tiles   test_epilogue_words[staged-fwd-*, staged-fwd-w8-*, staged-s2-*]
                                      mul_pre, eight-wave small tiles               test_epilogue_words[staged-w8-*]
                                      mul_pre, rolled loop (96-row tiles)           test_epilogue_words[staged-rolled-*]
                                      (unfused: not a producer)
    in-launch split-K combine         the general epilogue behind the combine       test_epilogue_words[combine-fwd-*, combine-dgrad-*]
    igemm_slab_reduce_kernel          split-K, reduction launch (no counters)       test_epilogue_words[splitk-reduce-*]
    conv_pointwise_kernel<MT, 1>      131072 <= B * HW < 524288                     test_epilogue_words[pointwise-px1-*]
    conv_pointwise_kernel<MT, 2>      B * HW >= 524288                              test_epilogue_words[pointwise-px2-*]
    skinny_rows_kernel                128 -> 64 at B 16, ragged 100 -> 7 at B 5     test_epilogue_words[rows-*]
    window kernels (shared epilogue)  WIN_MODE 2                                    test_epilogue_words[window-*]
    fp8 kernels (shared epilogue)     precision 3                                   test_epilogue_words[general-*-fp8-*]
    nadam_update_kernel               1 ... 40000 elements, chunk edges             test_nadam_words_*

Which path a shape takes is asserted, not assumed.  The fused epilogue of the tile kernels runs only where K is not split or the
split is combined inside the launch; every contraction of K = C_in x taps >= 128 on a small map is split, and without the
in-launch combine its words come from igemm_slab_reduce_kernel, whatever the tile.  So the tile-kernel cases have K <= 96 (8 or 3
input channels forward, 8 output channels for the input gradient) and assert a split-K workspace of zero bytes; the combine cases
(K = 288, nine splits of 96-row tiles) assert the combine's slab size.  The pointwise stream needs B * H * W >= 131072 pixels and an
even pixel count, and takes two pixels per thread from 524288 pixels up: PX = 1 is 8 -> 20 channels at B 32, 64 x 64; PX = 2 is
4 -> 4 at B 128, 64 x 64; no odd pixel count or unaligned stride reaches conv_pointwise_kernel.  (The C 96, 8 x 8, B 2 shape of
test_split_k_combined_in_launch_... does not combine: 12 splits x 96 rows exceed the combine's 512 KiB limit.)

Beyond the old clamp: f16_scale_exp / f8_scale_exp clamped k to +-100, so an operand whose largest magnitude was >= 2^115
scaled to >= 2^15 and its high pieces overflowed; the clamp now sits at pow2f's own limit (+-126), which binds only for tensors
below 2^-112 (they lose low bits, nothing overflows).  Behind the clamp sat a second overflow: the two inverse factors were
applied as (acc * 2^-ka) * 2^-kb, and for a weight gradient whose output gradient is ~2^118 the first product is inf although the
result (2^125) is finite - they are now two halves of the total exponent (unscale_pair, csrc/igemm.h).  Red before the two fixes:
test_pow2_equivariance[tile-splitk-f16x2, tile-splitk-fp8, transposed-s2-f16x2, transposed-s2-fp8, pointwise-f16x2], all at s = +116.

What the file is sensitive to (one-line faults built into a scratch copy of the library; the rest of the GPU suite passed on each):
    scalar tail of unary_fwd_kernel without its `am` update    test_roottanh_fwd_words[1, 3, 5, 1023, 1025, 4194311],
                                                               test_autograd_root_tanh_and_norm_tags
    nadam_update_kernel's last block does not publish          test_nadam_words_equal_the_updated_weights, test_nadam_words_drop_...,
                                                               test_repack_from_nadam_words_equals_two_pass_repack[0, 2]
    nadam_schedule_kernel does not clear the words             test_nadam_words_equal_the_updated_weights, test_nadam_words_drop_...
    igemm_epilogue publishes nothing (general and staged)      every general-*, staged-*, combine-* case of test_epilogue_words, the
                                                               window cases that have the form, test_autograd_linked_convs_tags
                                                               (this one the rest of the suite notices too: it is here to show
                                                               that those cases run the fused paths of the tile kernels)
    padded rows m >= M counted in igemm_epilogue's act_out     nothing - with general-fwd-* running exactly that code: the panel's
                                                               columns beyond M are zero and so is their bias, so what the padded
                                                               rows would store is RootTanh(0) = 0 and the maximum is unchanged
"""

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def word_bits(words):
    """The consumer's view of a word set: non-negative floats order like their bit patterns."""
    return int(words.max())


def bits(t):
    """Bit pattern of the largest magnitude of the tensor the kernel stored."""
    return int(t.detach().abs().max().reshape(1).view(torch.int32))


def S():
    return torch.cuda.current_stream().cuda_stream


class Words:
    """A word set the test owns: the middle third of a zeroed tensor; the outer thirds must stay zero."""

    def __init__(self):
        from locate_amd._lib import lib
        self.nw = lib().locate_absmax_words()
        self.all = torch.zeros(3 * self.nw, dtype=torch.int32, device=dev())
        self.mid = self.all[self.nw:2 * self.nw]

    def ptr(self):
        return self.mid.data_ptr()

    def check(self, stored, what=""):
        torch.cuda.synchronize()
        assert int(self.all[:self.nw].abs().max()) == 0 and int(self.all[2 * self.nw:].abs().max()) == 0, "%s: neighbouring word sets touched" % (what,)
        assert int(self.mid.min()) >= 0
        got, want = word_bits(self.mid), bits(stored)
        assert got == want, "%s: words %#010x, stored maximum %#010x" % (what, got, want)

    def check_untouched(self, what=""):
        torch.cuda.synchronize()
        assert int(self.all.abs().max()) == 0, "%s: words written" % (what,)


def positions(n):
    """First float4, last float4, scalar tail - where each exists."""
    pos = {0}
    if n >= 4:
        pos.add(4 * (n // 4) - 1)
    if n % 4:
        pos.add(n - 1)
    pos.add(n // 2)
    return sorted(pos)


# ====================================================================================================================== A
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 524288 + 1, 4194304 + 5])
def test_locate_absmax(n):
    """The separate pass: one block, block edges, the first grid-stride wrap (2048 blocks x 256 threads) and several wraps;
    maximum at index 0, n / 2 and n - 1, both signs."""
    from locate_amd._lib import check, lib
    torch.manual_seed(n)
    base = torch.randn(n, device=dev())
    for k, pos in enumerate(sorted({0, n // 2, n - 1})):
        x = base.clone()
        x[pos] = 37.5 if k % 2 == 0 else -37.5
        assert int(x.abs().argmax()) == pos
        w = Words()
        check(lib().locate_absmax(x.data_ptr(), n, w.ptr(), S()), "locate_absmax")
        w.check(x, "n %d pos %d" % (n, pos))


ROOTTANH_N = [1, 3, 4, 5, 1023, 1024, 1025, 4194304 + 7]


@pytest.mark.parametrize("n", ROOTTANH_N)
def test_roottanh_fwd_words(n):
    """unary_fwd_kernel<0>: the vector loop alone (n % 4 == 0), the scalar tail alone (n < 4), both, and the capped grid wrapping
    (2048 blocks x 1024 elements < n); the largest output in the first float4, the last float4, the tail."""
    from locate_amd._lib import check, lib
    torch.manual_seed(n)
    base = torch.randn(1, 1, n, device=dev())
    for k, pos in enumerate(positions(n)):
        x = base.clone()
        x.view(-1)[pos] = 30.0 if k % 2 == 0 else -30.0
        y = torch.empty_like(x)
        w = Words()
        check(lib().locate_roottanh_fwd(x.data_ptr(), y.data_ptr(), n, w.ptr(), S()), "locate_roottanh_fwd")
        assert int(y.abs().argmax()) == pos
        w.check(y, "n %d pos %d" % (n, pos))


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", ROOTTANH_N)
def test_roottanh_bwd_words(n, acc):
    """unary_bwd_kernel<0>, same walk.  accumulate = 1: the largest value AFTER the accumulation is the one already in gx (the new
    term there is small) - the words are those of the stored sum, not of the term."""
    from locate_amd._lib import check, lib
    torch.manual_seed(n + acc)
    x = torch.randn(1, 1, n, device=dev())
    g0 = torch.randn(1, 1, n, device=dev())
    for k, pos in enumerate(positions(n)):
        sign = 1.0 if k % 2 == 0 else -1.0
        g = g0.clone()
        gx = torch.randn(1, 1, n, device=dev()) if acc else torch.empty(1, 1, n, device=dev())
        if acc:
            gx.view(-1)[pos] = sign * 1.0e4
        else:
            g.view(-1)[pos] = sign * 1.0e3
        w = Words()
        check(lib().locate_roottanh_bwd(x.data_ptr(), g.data_ptr(), gx.data_ptr(), n, acc, w.ptr(), S()), "locate_roottanh_bwd")
        assert int(gx.abs().argmax()) == pos
        w.check(gx, "n %d pos %d acc %d" % (n, pos, acc))


# (16 channels on the smallest maps: the largest normalised value of a group of n elements is bounded by (n - 1) / sqrt(n), so one
# outlier only stands out of a group that is not tiny)
NORM_CASES = [(B, 16 if hw <= 4 else 4, hw, groups, per_sample) for hw in (1, 2, 4, 35, 64) for groups in (1, 3) for (B, per_sample) in ((3, 0), (6, 1))]
NORM_CASES += [(2, 16, 65544, 1, 0), (2, 16, 65541, 1, 1)]          # n_g > 2097152: the capped grid wraps, vector and scalar path


@pytest.mark.parametrize("with_act", [0, 1])
@pytest.mark.parametrize("B,C,hw,groups,per_sample", NORM_CASES, ids=lambda v: str(v))
def test_norm_fwd_words(B, C, hw, groups, per_sample, with_act):
    """norm_apply_fused_kernel<ACT>: the 16-byte path (hw % 4 == 0) and the scalar one, per-channel and per-sample scale, one group
    and three (blockIdx.y = group); the largest output in the last group's last plane's last element, and in the very first."""
    from locate_amd._lib import check, lib
    L = lib()
    torch.manual_seed(B * 1000 + C * 100 + hw + groups)
    base = torch.randn(B, C, hw).to(dev())
    scale = (1.0 + 0.05 * torch.rand(B * C if per_sample else C)).to(dev())
    bias = (0.01 * torch.randn(C)).to(dev())
    n = base.numel()
    for k, pos in enumerate((n - 1, 0)):
        x = base.clone()
        x.view(-1)[pos] = 50.0 if k == 0 else -50.0
        out = torch.empty_like(x)
        stats = torch.empty(2 * groups, device=dev())
        ws = torch.empty(L.locate_norm_stats_workspace_bytes(), dtype=torch.uint8, device=dev())
        w = Words()
        check(L.locate_norm_fwd(x.data_ptr(), scale.data_ptr(), per_sample, bias.data_ptr(), out.data_ptr(), with_act, stats.data_ptr(),
                                B, C, hw, groups, ws.data_ptr(), None, w.ptr(), S()), "locate_norm_fwd")
        assert int(out.abs().argmax()) == pos
        w.check(out, "pos %d" % pos)


GATE_CASES = [(5, 4), (67, 8), (5, 16), (67, 32), (5, 64), (67, 128),          # gate_bwd_small_kernel<1 ... 32>, ragged last plane group
              (5, 36), (7, 576), (5, 35),                                        # gate_bwd_plane_kernel<1>: vector, vector, scalar
              (3, 1024),                                                         # gate_bwd_plane_kernel<4>
              (128, 1),                                                          # 1x1 maps: remapped to 64-element planes
              (16384 + 37, 36)]                                                  # 4096 blocks x 4 waves walk several planes


@pytest.mark.parametrize("planes,hw", GATE_CASES, ids=lambda v: str(v))
def test_gate_bwd_words(planes, hw):
    """da = gamma * x * g of the residual gate's backward, full-map form: the largest value in the last live plane's last element
    and in the first; the per-plane form of `a` stores no full map and must leave the words alone."""
    from locate_amd._lib import check, lib
    L = lib()
    torch.manual_seed(planes + hw)
    n = planes * hw
    x0 = torch.randn(planes, hw, device=dev())
    g = torch.randn(planes, hw, device=dev())
    gamma = torch.tensor([0.7], device=dev())
    ws = torch.empty(L.locate_gate_bwd_workspace_bytes(planes), dtype=torch.uint8, device=dev())
    dgamma = torch.empty(1, device=dev())
    for k, pos in enumerate((n - 1, 0)):
        x = x0.clone()
        x.view(-1)[pos] = 1000.0 if k == 0 else -1000.0
        gg = g.clone()
        gg.view(-1)[pos] = 3.0
        a = torch.randn(planes, hw, device=dev())
        dx, da = torch.empty_like(x), torch.empty_like(x)
        w = Words()
        check(L.locate_gate_bwd(x.data_ptr(), a.data_ptr(), 0, gamma.data_ptr(), gg.data_ptr(), dx.data_ptr(), da.data_ptr(), dgamma.data_ptr(),
                                planes, hw, ws.data_ptr(), 0, w.ptr(), S()), "locate_gate_bwd")
        assert int(da.abs().argmax()) == pos
        w.check(da, "full map, pos %d" % pos)
    a_pl, da_pl = torch.randn(planes, device=dev()), torch.empty(planes, device=dev())
    w = Words()
    check(L.locate_gate_bwd(x0.data_ptr(), a_pl.data_ptr(), 1, gamma.data_ptr(), g.data_ptr(), dx.data_ptr(), da_pl.data_ptr(), dgamma.data_ptr(),
                            planes, hw, ws.data_ptr(), 0, w.ptr(), S()), "locate_gate_bwd")
    assert float(da_pl.abs().max()) > 0
    w.check_untouched("per-plane form")


# ---- contraction epilogues ---------------------------------------------------------------------------------------------
# How a launch gets its split-K plan is visible from the host: locate_conv_{fwd,dgrad}_workspace_bytes is 0 when K is not split (then
# igemm_epilogue itself stores and publishes), a multiple of the output size when the partial tiles go to output-shaped slabs for
# igemm_slab_reduce_kernel (igemm_epilogue then runs its UNFUSED store and publishes nothing), and ks x tiles x tile size - here no
# multiple of the output - when the tile's last block combines them inside the launch and runs the fused epilogue.  Un-split: fewer
# than 8 K steps of 16, i.e. K = C_in x taps <= 96.
EPI_CASES = {
    # name: (kind, cin, cout, k, s, p, B, H, W, directions, path)
    "general-fwd": ("conv", 8, 72, 3, 1, 1, 3, 7, 7, ("fwd",), "unsplit"),          # ragged M (72 of a 96-row tile), ragged N (147): act_out
    "general-dgrad": ("conv", 72, 8, 3, 1, 1, 3, 7, 7, ("dgrad",), "unsplit"),      # the same tile the other way round: mul_pre
    "staged-fwd": ("conv", 8, 72, 3, 1, 1, 3, 4, 4, ("fwd",), "unsplit"),           # 4x4 planes: staged store, act_out in the rolled loop (96-row tile)
    "staged-fwd-w8": ("conv", 8, 64, 3, 1, 1, 3, 4, 4, ("fwd",), "unsplit"),        # ... on the eight-wave 64-row tile (act_out: rolled loop as well)
    "staged-s2": ("conv", 3, 72, 5, 2, 2, 6, 4, 4, ("fwd",), "unsplit"),            # stride 2 onto 2x2 planes, ragged N (24 of 32)
    "staged-w8": ("conv", 40, 8, 3, 1, 1, 3, 4, 4, ("dgrad",), "unsplit"),          # input gradient on the eight-wave 64-row tile: mul_pre, loads batched
    "staged-rolled": ("conv", 96, 8, 3, 1, 1, 3, 4, 4, ("dgrad",), "unsplit"),      # ... on the four-wave 96-row tile: mul_pre in the rolled loop
    "combine-fwd": ("conv", 32, 72, 3, 1, 1, 3, 7, 7, ("fwd",), "combine"),         # K = 288: 9 splits x 96 rows, combined in the launch
    "combine-dgrad": ("conv", 72, 32, 3, 1, 1, 3, 7, 7, ("dgrad",), "combine"),
    "splitk-reduce": ("conv", 256, 256, 5, 2, 2, 6, 4, 4, ("fwd", "dgrad"), "reduce"),   # run without counters: igemm_slab_reduce_kernel
    "pointwise-px1": ("conv", 8, 20, 1, 1, 0, 32, 64, 64, ("fwd", "dgrad"), None),  # 131072 pixels
    "pointwise-px2": ("conv", 4, 4, 1, 1, 0, 128, 64, 64, ("fwd", "dgrad"), None),  # 524288 pixels
    "rows": ("conv", 128, 64, 1, 1, 0, 16, 1, 1, ("fwd", "dgrad"), None),
    "rows-ragged": ("conv", 100, 7, 1, 1, 0, 5, 1, 1, ("fwd", "dgrad"), None),
    "window": ("conv", 64, 48, 5, 2, 2, 24, 8, 8, ("fwd", "dgrad"), None),
    "window-T": ("convT", 128, 96, 4, 2, 1, 3, 8, 8, ("fwd", "dgrad"), None),
}
EPI_PARAMS = [(name, form, direction, where)
              for name, case in EPI_CASES.items()
              for form in (("bf16x3", "f16x2", "fp8") if name.startswith("general") else ("bf16x3", "f16x2"))
              for direction in case[9]
              for where in ("row", "col")]


@pytest.mark.parametrize("name,form,direction,where", EPI_PARAMS, ids=lambda v: str(v))
def test_epilogue_words(name, form, direction, where, monkeypatch):
    """The fused epilogues of the contractions: act_out = RootTanh(y) as a second output (forward) and gx = RootTanh'(pre) *
    contraction (input gradient, mul_pre), each with the largest magnitude of what it stored.  `row`: the largest value sits in
    the last output channel (the last, ragged row tile) - steered by a bias on that channel, or by the weights that feed it;
    `col`: in the last batch element (the last column tile) - steered by the gathered operand's last batch element."""
    from locate_amd import ops
    kind, cin, cout, k, s, p, B, H, W, _, path = EPI_CASES[name]
    window = name.startswith("window")
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", 2 if window else 0)
    ops._WIN_CACHE.clear()
    if name == "splitk-reduce":
        monkeypatch.setattr(ops, "_counters", lambda owner, adjoint: None)
    torch.manual_seed(len(name) * 100 + cin + cout)
    spec = ops.ConvSpec(kind, k, k, s, p, p)
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    w = torch.randn(wshape, device=dev()) / float(cin * k * k) ** 0.5
    x = torch.randn(B, cin, H, W, device=dev())
    geom, out_shape = spec.geometry(tuple(x.shape), wshape)
    garr = ops._geom(geom)
    sigma = torch.tensor([2.0, 0.5], device=dev())
    precision = 3 if form == "fp8" else 0
    sign = 1.0 if (where == "row") == (direction == "fwd") else -1.0
    words = Words()
    before = (dict(ops.F16_CALLS), ops.WIN_CALLS[0], ops.FP8_CALLS[0])
    if direction == "fwd":
        bias = 0.1 * torch.randn(cout, device=dev())
        if where == "row":
            bias[cout - 1] = sign * 40.0
        else:
            x[B - 1] *= sign * 32.0
        gathered = ops.tag_amax(x) if form == "f16x2" else x
        stored = torch.empty(out_shape, device=dev())
        epi = ops._ActEpilogue(stored.data_ptr(), stored.stride(0), None, 0, 0, 0, None, 0, words.ptr())
        y = ops._conv_apply(gathered, w, w, spec, geom, garr, sigma, bias, out_shape, precision, ops._amax_of(gathered), None, epi)
        adj = 0 if kind == "conv" else 1
        assert float(y.abs().max()) > 0
    else:
        gy = torch.randn(out_shape, device=dev())
        pre = torch.randn(B, cin, H, W, device=dev())
        if where == "row":
            (w[:, cin - 1] if kind == "conv" else w[cin - 1]).mul_(sign * 64.0)
        else:
            gy[B - 1] *= sign * 64.0
        gathered = ops.tag_amax(gy) if form == "f16x2" else gy
        stored = torch.empty_like(x)
        epi = ops._ActEpilogue(None, 0, None, 0, 0, 0, pre.data_ptr(), pre.stride(0), words.ptr())
        ops._contract(kind != "conv", gathered, w, w, spec, geom, garr, sigma, None, stored, precision, ops._amax_of(gathered), epi)
        adj = 1 if kind == "conv" else 0
    torch.cuda.synchronize()
    # the intended form ran, with the intended split-K plan
    which = "fwd" if direction == "fwd" else "dgrad"
    L = ops.lib()
    ws_bytes = (L.locate_conv_fwd_workspace_bytes if adj == 0 else L.locate_conv_dgrad_workspace_bytes)(garr)
    if path == "unsplit":
        assert ws_bytes == 0, "K is split: the fused epilogue does not run"
    elif path == "combine":
        assert ws_bytes > 0 and ws_bytes % (4 * stored.numel()) != 0, "not the in-launch combine's slab"
    elif path == "reduce":
        assert ws_bytes > 0 and ws_bytes % (4 * stored.numel()) == 0, "not the reduction kernel's output-shaped slabs"
    assert ops.F16_CALLS[which] - before[0][which] == int(form == "f16x2")
    assert ops.FP8_CALLS[0] - before[2] == int(form == "fp8")
    if window:
        fmt = 2 if form == "f16x2" else 0
        has = int(ops.lib().locate_conv_win_ok(garr, adj | fmt, gathered.stride(0), gathered.data_ptr()) > 0)
        assert ops.WIN_CALLS[0] - before[1] == has
        # (the three-piece window of the 5x5 stride-2 forward exceeds the LDS budget: that one case runs the gather kernel; the
        # transposed geometry has the form in both directions and both piece formats)
        assert has == 1 or (name, form, direction) == ("window", "bf16x3", "fwd"), "the window form of this geometry is gone"
    else:
        assert ops.WIN_CALLS[0] == before[1]
    # the precondition: the largest stored value lies where it was steered
    at = int(stored.abs().argmax())
    per_b = stored.numel() // B
    plane = stored.shape[2] * stored.shape[3]
    if where == "row":
        assert (at % per_b) // plane == stored.shape[1] - 1, "largest value not in the last channel"
    else:
        assert at // per_b == B - 1, "largest value not in the last batch element"
    assert torch.isfinite(stored).all()
    words.check(stored, "%s %s %s %s" % (name, form, direction, where))
    ops._WIN_CACHE.clear()


# ---- through the autograd layer, once per producer -----------------------------------------------------------------------
class _Probe(torch.autograd.Function):
    """Identity whose backward records what the next contraction would see of the arriving gradient."""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        from locate_amd import ops
        a = ops._amax_of(g)
        _Probe.seen.append((None if a is None else a.clone(), g.detach().clone()))
        return g


def _assert_tagged(t, what):
    from locate_amd import ops
    a = ops._amax_of(t)
    assert a is not None, "%s: no largest-magnitude words on the tensor" % what
    torch.cuda.synchronize()
    assert word_bits(a) == bits(t), "%s: words %#010x, stored maximum %#010x" % (what, word_bits(a), bits(t))


def _assert_probe(what):
    assert len(_Probe.seen) == 1, what
    a, g = _Probe.seen.pop()
    assert a is not None, "%s: the gradient arrived without words" % what
    assert word_bits(a) == bits(g), "%s: words %#010x, gradient maximum %#010x" % (what, word_bits(a), bits(g))


def test_autograd_root_tanh_and_norm_tags(monkeypatch):
    """ops.root_tanh (output and input gradient) and ops.inplace_norm (output, both with_act): the words that ride on the tensor
    the next contraction receives are those of that tensor."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "AMAX_MIN_NUMEL", [1])
    torch.manual_seed(1)
    _Probe.seen.clear()
    x = torch.randn(2, 3, 37, device=dev())
    x[1, 2, 36] = -25.0          # the scalar tail
    x.requires_grad_(True)
    y = ops.root_tanh(_Probe.apply(x))
    _assert_tagged(y, "root_tanh output")
    g = torch.randn_like(y)
    g[1, 2, 36] = 500.0
    ops.reset_backward_state()
    y.backward(g)
    _assert_probe("root_tanh input gradient")
    for with_act in (False, True):
        xn = torch.randn(3, 4, 5, 7, device=dev())
        xn[2, 3, 4, 6] = 60.0
        out = ops.inplace_norm(xn, 1.0 + 0.05 * torch.rand(4, device=dev()), 0.01 * torch.randn(4, device=dev()), with_act)
        assert int(out.abs().argmax()) == out.numel() - 1
        _assert_tagged(out, "inplace_norm output, with_act %s" % with_act)


def test_autograd_residual_gate_backward_tag(monkeypatch):
    """ops.residual_gate: the gradient of a full-map gate value arrives at its producer with the words of the stored map."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "AMAX_MIN_NUMEL", [1])
    torch.manual_seed(2)
    _Probe.seen.clear()
    x = torch.randn(2, 5, 6, 6, device=dev())
    x[1, 4, 5, 5] = -800.0
    a = torch.randn(2, 5, 6, 6, device=dev(), requires_grad=True)
    gamma = torch.tensor([0.3], device=dev())
    out = ops.residual_gate(x, _Probe.apply(a), gamma)
    g = torch.randn_like(out)
    g[1, 4, 5, 5] = 2.0
    ops.reset_backward_state()
    out.backward(g)
    _assert_probe("gate value gradient")
    assert int(a.grad.abs().argmax()) == a.numel() - 1


@pytest.mark.parametrize("form", ["bf16x3", "f16x2"])
def test_autograd_linked_convs_tags(form, monkeypatch):
    """SNConvFn with act = {"link": ...} (second output RootTanh(y), tagged) feeding SNConvFn with in_link (its input-gradient
    launch multiplies by RootTanh'(y) and tags the result): the words equal the stored tensors, and the producer's backward
    receives them with the gradient (what its own input- and weight-gradient contractions are scaled by)."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "AMAX_MIN_NUMEL", [1])
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0 if form == "f16x2" else 1e30)
    torch.manual_seed(3)
    rt = ops.Runtime()
    rt.defer_finalisers = False
    B, cin, mid, cout, H = 3, 40, 72, 24, 7
    w0 = (torch.randn(mid, cin, 3, 3, device=dev()) * 0.05).requires_grad_(True)
    w1 = (torch.randn(cout, mid, 1, 1, device=dev()) * 0.1).requires_grad_(True)
    sigma = torch.tensor([1.0, 1.0], device=dev())

    def uvw(w):
        return torch.zeros(w.shape[0], device=dev()), torch.zeros(w.numel() // w.shape[0], device=dev()), torch.zeros(w.shape[0], device=dev())
    u0, v0, wv0 = uvw(w0)
    u1, v1, wv1 = uvw(w1)
    x = ops.tag_amax(torch.randn(B, cin, H, H, device=dev())).requires_grad_(True)
    link = ops.ActLink()
    y, second = ops.SNConvFn.apply(x, w0, u0, v0, None, sigma, wv0, ops.ConvSpec("conv", 3, 3, 1, 1, 1), rt, None, None, {"link": link}, None)
    _assert_tagged(second, "linked activation")
    seen = []
    real = ops._conv_weight_grad

    import inspect
    signature = inspect.signature(real)

    def spy(*args, **kw):
        bound = signature.bind(*args, **kw).arguments
        seen.append((bound["gy"], bound["amax_gy"]))
        return real(*args, **kw)
    monkeypatch.setattr(ops, "_conv_weight_grad", spy)
    y2 = ops.SNConvFn.apply(second, w1, u1, v1, None, sigma, wv1, ops.ConvSpec("conv", 1, 1, 1, 0, 0), rt, None, None, None, link)
    gy = ops.tag_amax(torch.randn(y2.shape, device=dev()))
    ops.reset_backward_state()
    y2.backward(gy)
    torch.cuda.synchronize()
    assert len(seen) == 2          # conv_1's weight gradient, then conv_0's: the latter with the premultiplied gradient
    g_pre, a_pre = seen[1]
    assert tuple(g_pre.shape) == tuple(y.shape)
    assert a_pre is not None, "the premultiplied input gradient arrived at conv_0 without words"
    assert word_bits(a_pre) == bits(g_pre)
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


# ---- Nadam ---------------------------------------------------------------------------------------------------------------
NADAM_SIZES = [1, 255, 4095, 4096, 4097, 8193, 40000]


def _nadam_params():
    from locate_amd._lib import lib
    assert lib().locate_nadam_chunk_elems() == 4096          # the sizes above straddle one and two chunk edges
    params = []
    for i, n in enumerate(NADAM_SIZES + [777]):
        p = torch.randn(n, device=dev())
        p[n - 1] = 50.0 if i % 2 == 0 else -50.0          # an lr-sized update cannot move the argmax
        p = p.reshape(n, 1) if n != 777 else p               # ... plus one 1-D parameter, the last of the launch
        params.append(torch.nn.Parameter(p.contiguous()))
    return params


def _assert_nadam_words(p, what):
    hold = p.__dict__["_locate_wmax"]
    assert hold[1] == p._version, "%s: stamp %d, version %d" % (what, hold[1], p._version)
    assert int(hold[0].min()) >= 0
    assert word_bits(hold[0]) == bits(p), "%s (%d elements): words %#010x, weights %#010x" % (what, p.numel(), word_bits(hold[0]), bits(p))


def test_nadam_words_equal_the_updated_weights():
    """nadam_update_kernel: after every step each parameter's words hold the largest magnitude of the weights it stored - tensors of
    one element, one chunk minus one, exactly one, one plus one, two plus one, ten - and the stamp equals the parameter version.  A
    parameter whose .grad is None in a step keeps words and stamp."""
    from locate_amd.optim import Nadam
    torch.manual_seed(4)
    params = _nadam_params()
    opt = Nadam(params, lr=2e-3)
    for step in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        skipped = params[3] if step == 1 else None
        if skipped is not None:
            skipped.grad = None
            kept = (skipped.__dict__["_locate_wmax"][0].clone(), skipped.__dict__["_locate_wmax"][1], skipped._version)
        opt.step()
        torch.cuda.synchronize()
        for p in params:
            if p is skipped:
                hold = p.__dict__["_locate_wmax"]
                assert torch.equal(hold[0], kept[0]) and hold[1] == kept[1] and p._version == kept[2]
            _assert_nadam_words(p, "step %d" % step)
            assert int(p.detach().abs().argmax()) == p.numel() - 1


def test_nadam_words_drop_with_the_largest_weight():
    """The schedule kernel clears the words before the update folds the new maximum in: after the largest weight is overwritten with
    zero, the words of the next step are those of the new, smaller maximum."""
    from locate_amd.optim import Nadam
    torch.manual_seed(5)
    params = _nadam_params()
    opt = Nadam(params, lr=2e-3)
    for step in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        if step == 2:
            with torch.no_grad():
                for p in params:
                    p.view(-1)[p.numel() - 1] = 0.0
        opt.step()
        torch.cuda.synchronize()
        for p in params:
            _assert_nadam_words(p, "step %d" % step)
    assert all(float(p.detach().abs().max()) < 10.0 for p in params)


@pytest.mark.parametrize("win_mode", [0, 2])
def test_repack_from_nadam_words_equals_two_pass_repack(win_mode, monkeypatch):
    """After an optimizer step, refresh_panels re-packs the fp16-piece panel directly from the optimizer's words; with
    DIRECT_REPACK off it takes the two-pass form with a maximum of its own.  The contraction's output is the same, bit for bit
    (the weight shape of test_conv_window_form_stacked_calls_and_repack)."""
    from locate_amd import ops
    from locate_amd.optim import Nadam
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", win_mode)
    ops._WIN_CACHE.clear()
    torch.manual_seed(6)
    B, C, M, H = 24, 64, 48, 8
    spec = ops.ConvSpec("conv", 5, 5, 2, 2, 2)
    x = ops.tag_amax((torch.randn(B, C, H, H) * 2).to(dev()))
    w = torch.nn.Parameter((torch.randn(M, C, 5, 5) * 0.05).to(dev()))
    w.data.view(-1)[-1] = 3.0          # the largest weight is the last element of the last chunk
    sigma = torch.tensor([2.0, 0.5], device=dev())
    geom, out_shape = spec.geometry(tuple(x.shape), tuple(w.shape))
    garr = ops._geom(geom)

    def run():
        before = ops.F16_CALLS["fwd"]
        y = ops._conv_apply(x, w.detach(), w, spec, geom, garr, sigma, None, out_shape, 0, ops._amax_of(x)).clone()
        assert ops.F16_CALLS["fwd"] == before + 1
        return y
    y_old = run()
    opt = Nadam([w], lr=2e-3)
    w.grad = torch.randn_like(w)
    opt.step()
    hold = w.__dict__["_locate_wmax"]
    assert hold[1] == w._version and ops.DIRECT_REPACK
    ops.refresh_panels([w])
    y_direct = run()
    with torch.no_grad():
        w.add_(0.0)                     # same weights, new version: the panel is stale again and the optimizer's words no longer apply
    monkeypatch.setattr(ops, "DIRECT_REPACK", False)
    ops.refresh_panels([w])
    y_two_pass = run()
    assert torch.isfinite(y_direct).all() and not torch.equal(y_old, y_direct)
    assert torch.equal(y_direct, y_two_pass)
    ops._WIN_CACHE.clear()


# ====================================================================================================================== B
def test_tag_plumbing(monkeypatch):
    """_amax_of through a full view and through carry_amax; None after an in-place change, for a partial view, with the arena off."""
    from locate_amd import ops
    torch.manual_seed(7)
    t = ops.tag_amax(torch.randn(4, 6, 5, 5, device=dev()))
    a = ops._amax_of(t)
    assert a is not None and word_bits(a) == bits(t)
    full = t.view(4, 6, 25)
    assert ops._amax_of(full) is a, "a full view finds the words on its base"
    carried = ops.carry_amax(t, t.reshape(24, 25))
    assert ops._amax_of(carried) is a
    assert ops._amax_of(t[:, 2:4]) is None, "a channel slice shows other elements"
    assert ops._amax_of(t[1:]) is None
    monkeypatch.setattr(ops.AMAX, "enabled", False)
    assert ops._amax_of(t) is None and ops._amax_of(full) is None
    monkeypatch.setattr(ops.AMAX, "enabled", True)
    assert ops._amax_of(t) is a
    t.mul_(2.0)
    assert ops._amax_of(t) is None and ops._amax_of(full) is None and ops._amax_of(carried) is None, "an in-place change invalidates the tag"


def test_arena_hand_outs_are_disjoint_and_zero(monkeypatch):
    """Word sets handed out inside one new_step / end_step bracket - more of them than the iteration's block holds - are pairwise
    disjoint and zero on hand-out; after end_step the next iteration's block covers what this one took."""
    from locate_amd import ops
    arena = ops._AmaxArena()
    monkeypatch.setattr(ops, "AMAX", arena)
    arena.new_step(dev())
    take = arena.STEP_SLOTS + 23
    sets = []
    for i in range(take):
        s = arena.slot(dev())
        assert int(s.abs().max()) == 0, "hand-out %d is not zero" % i
        s.fill_(i + 1)                  # a producer publishes
        sets.append(s)
    spans = sorted((s.data_ptr(), s.data_ptr() + 4 * s.numel()) for s in sets)
    assert all(s.numel() == arena.words for s in sets)
    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)), "word sets overlap"
    assert all(int(s.min()) == i + 1 and int(s.max()) == i + 1 for i, s in enumerate(sets))
    arena.end_step()
    assert arena.STEP_SLOTS >= take
    arena.new_step(dev())
    assert arena.cap >= take and int(arena.block.abs().max()) == 0
    arena.end_step()


# ====================================================================================================================== C
GEOMS = {
    # name: (kind, cin, cout, k, s, p, B, H, W)
    "tile-splitk": ("conv", 128, 128, 1, 1, 0, 4, 8, 8),
    "transposed-s2": ("convT", 96, 96, 4, 2, 1, 2, 8, 8),
    "rows": ("conv", 256, 192, 1, 1, 0, 64, 1, 1),
    "pointwise": ("conv", 8, 20, 1, 1, 0, 32, 64, 64),
}


class _Contraction:
    """The three bias-free contractions of one layer in one piece form, on raw operands (no spectral-norm term: _raw_weight_grad)."""

    def __init__(self, name, form):
        from locate_amd import ops
        self.ops = ops
        self.kind, cin, cout, k, s, p, B, H, W = GEOMS[name]
        self.form = form
        self.spec = ops.ConvSpec(self.kind, k, k, s, p, p)
        self.wshape = (cout, cin, k, k) if self.kind == "conv" else (cin, cout, k, k)
        self.xshape = (B, cin, H, W)
        self.geom, self.out_shape = self.spec.geometry(self.xshape, self.wshape)
        self.garr = ops._geom(self.geom)
        self.sigma = torch.tensor([2.0, 0.5], device=dev())
        self.precision = 3 if form == "fp8" else 0

    def _am(self, t):
        return self.ops._amax_of(self.ops.tag_amax(t)) if self.form == "f16x2" else None

    def fwd(self, x, w):
        return self.ops._conv_apply(x, w, w, self.spec, self.geom, self.garr, self.sigma, None, self.out_shape, self.precision, self._am(x))

    def dgrad(self, gy, w):
        x_like = torch.empty(self.xshape, device=dev())
        return self.ops._conv_input_grad(gy, x_like, w, w, self.spec, self.geom, self.garr, self.sigma, self.precision, self._am(gy))

    def wgrad(self, x, gy, w):
        ops = self.ops
        xin, gout = (x, gy) if self.kind == "conv" else (gy, x)
        gw = torch.empty(self.wshape, device=dev())
        part = torch.zeros(ops._weight_grad_partials(self.spec, self.geom, self.garr), dtype=torch.float64, device=dev())
        ops._raw_weight_grad(self.spec, self.geom, self.garr, xin, gout, gw, w, self.sigma[1:], 0, 0, part, self.precision,
                             self._am(xin), self._am(gout))
        return gw


def _normal_or_zero(t):
    a = t.abs()
    return bool((torch.isfinite(t) & ((a == 0) | (a >= 2.0 ** -126))).all())


def _ldexp(t, s):
    """t * 2^s, exact where the result is a normal number or zero (asserted)."""
    r = (t.double() * 2.0 ** s).float()
    assert _normal_or_zero(r), "the expected result leaves the normal range: wrong test input"
    assert torch.equal(r.double(), t.double() * 2.0 ** s)
    return r


def _scaled(t, s):
    r = _ldexp(t, s)
    return r.contiguous()


# (s on the gathered operand, s on the other): +-13 and +-40 in every form; at |s| = 40 the two un-scales cannot be one factor.
SWEEP = [(-40, 0), (-13, 0), (13, 0), (40, 0), (0, -40), (0, 40), (-40, 40)]
# the scaled forms beyond the old clamp of the scale exponent at +-100: largest magnitudes of 2^118 and 2^-94.  (Not the three-piece
# bf16 form: it has no scale to clamp, and the low bf16 pieces of elements near 2^-115 are subnormal bf16 numbers - the split
# is no longer the same split of the same significand there.)
SWEEP_WIDE = [(116, 0), (-96, 0)]


@pytest.mark.parametrize("form", ["bf16x3", "f16x2", "fp8"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_pow2_equivariance(name, form, monkeypatch):
    """Scaling an operand by 2^s is exact in fp32, and every form splits or quantises after an exact power-of-two scale (or splits
    exactly): y(2^s x, w) == ldexp(y(x, w), s) bit for bit; the same for scaling w, for dx under scaling of gy, and for the raw
    weight gradient under scaling of either operand."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", 0)
    c = _Contraction(name, form)
    torch.manual_seed(len(name))
    x = torch.randn(c.xshape, device=dev())
    w = torch.randn(c.wshape, device=dev()) * 0.05
    gy = torch.randn(c.out_shape, device=dev())
    before = (dict(ops.F16_CALLS), ops.FP8_CALLS[0])
    y0, dx0, dw0 = c.fwd(x, w), c.dgrad(gy, w), c.wgrad(x, gy, w)
    torch.cuda.synchronize()
    if form == "f16x2":
        assert all(ops.F16_CALLS[k] == before[0][k] + 1 for k in ("fwd", "dgrad"))
        assert ops.F16_CALLS["wgrad"] == before[0]["wgrad"] + 1
    else:
        assert ops.F16_CALLS == before[0]
    assert ops.FP8_CALLS[0] - before[1] == (2 if form == "fp8" else 0)
    assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in (y0, dx0, dw0))
    for sa, sb in SWEEP + (SWEEP_WIDE if form != "bf16x3" else []):
        what = "%s %s s = (%d, %d)" % (name, form, sa, sb)
        xs, gs, ws = _scaled(x, sa), _scaled(gy, sa), _scaled(w, sb)
        assert torch.equal(c.fwd(xs, ws), _ldexp(y0, sa + sb)), "y: " + what
        assert torch.equal(c.dgrad(gs, ws), _ldexp(dx0, sa + sb)), "dx: " + what
        if sb == 0:
            assert torch.equal(c.wgrad(xs, gy, w), _ldexp(dw0, sa)), "dw under x: " + what
            assert torch.equal(c.wgrad(x, gs, w), _ldexp(dw0, sa)), "dw under gy: " + what
    if form != "bf16x3":
        # both operands of the weight gradient at once, at the two ends
        assert torch.equal(c.wgrad(_scaled(x, -96), _scaled(gy, 116), w), _ldexp(dw0, 20)), "dw: x 2^-96, gy 2^116"


# ====================================================================================================================== D
EDGE_GEOMS = {
    "3x3": ("conv", 40, 72, 3, 1, 1, 3, 7, 7),
    "convT": ("convT", 64, 64, 4, 2, 1, 4, 4, 4),
    "window": ("conv", 64, 48, 5, 2, 2, 24, 8, 8),
}


def _sn_run(kind, k, s, p, x, w, g, precision=0, tag=True):
    """Forward, input gradient and weight gradient through SNConvFn with sigma = 1 and u = v = 0 (no rank-1 term: dw is G)."""
    from locate_amd import ops
    rt = ops.Runtime()
    rt.precision = precision
    rt.defer_finalisers = False
    wg = w.to(dev()).requires_grad_(True)
    xg = x.to(dev())
    xg = (ops.tag_amax(xg) if tag else xg).requires_grad_(True)
    u, v = torch.zeros(w.shape[0], device=dev()), torch.zeros(w.numel() // w.shape[0], device=dev())
    sigma, wv = torch.tensor([1.0, 1.0], device=dev()), torch.zeros(w.shape[0], device=dev())
    y = ops.SNConvFn.apply(xg, wg, u, v, None, sigma, wv, ops.ConvSpec(kind, k, k, s, p, p), rt)
    gg = g.to(dev())
    y.backward(ops.tag_amax(gg) if tag else gg)
    torch.cuda.synchronize()
    return y.detach().cpu(), xg.grad.cpu(), wg.grad.cpu()


def _ref64(kind, s, p, x, w, g):
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, s, p) if kind == "conv" else F.conv_transpose2d(xr, wr, None, s, p)
    yr.backward(g.double())
    return yr.detach(), xr.grad, wr.grad


def _edge_operands(name, seed):
    kind, cin, cout, k, s, p, B, H, W = EDGE_GEOMS[name]
    torch.manual_seed(seed)
    wshape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
    w = torch.randn(wshape) * 0.05
    x = torch.randn(B, cin, H, W)
    y = F.conv2d(x, w, None, s, p) if kind == "conv" else F.conv_transpose2d(x, w, None, s, p)
    g = torch.randn(y.shape)
    return (kind, k, s, p), x, w, g


@pytest.mark.parametrize("edge", ["pow2", "below-pow2"])
@pytest.mark.parametrize("name", list(EDGE_GEOMS))
def test_scale_edges_of_the_fp16_piece_form(name, edge, monkeypatch):
    """The operand's largest magnitude is exactly 2^e (zero mantissa: scaled to 2^14, the bottom of the target binade), or the value
    just below 2^(e+1) (whose high piece rounds up to 2^15 after scaling): finite, and within the bounds of
    test_conv_fp16_pieces_vs_cpu (2e-5 / 2e-5 / 5e-5) against a float64 CPU conv.  x at e = 3, gy at e = -13, w at e = -2."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", 2 if name == "window" else 0)
    ops._WIN_CACHE.clear()
    (kind, k, s, p), x, w, g = _edge_operands(name, 8)

    def plant(t, e):
        top = 2.0 ** e if edge == "pow2" else float(torch.nextafter(torch.tensor(2.0 ** (e + 1)), torch.tensor(0.0)))
        t = t * (2.0 ** e / float(t.abs().max())) * 0.9          # everything else below 2^e
        t.view(-1)[-1] = -top
        t.view(-1)[0] = top
        assert float(t.abs().max()) == top
        return t
    x, g, w = plant(x, 3), plant(g, -13), plant(w, -2)
    before = dict(ops.F16_CALLS)
    got = _sn_run(kind, k, s, p, x, w, g)
    assert all(ops.F16_CALLS[kk] == before[kk] + 1 for kk in ("fwd", "dgrad", "wgrad"))
    want = _ref64(kind, s, p, x, w, g)
    for what, tol, a, b in zip(("y", "dx", "dw"), (2e-5, 2e-5, 5e-5), got, want):
        assert torch.isfinite(a).all(), what
        assert_close(a, b, tol, what)
    ops._WIN_CACHE.clear()


@pytest.mark.parametrize("form", ["bf16x3", "f16x2", "fp8"])
@pytest.mark.parametrize("name", list(EDGE_GEOMS))
def test_zero_operands_give_exact_zeros(name, form, monkeypatch):
    """An all-zero x gives y == 0, an all-zero gy gives dx == 0 and dw == 0, exactly, in every form and in the window kernels: the
    words are 0, so k = 0, and nothing un-scaled (padding, cleared LDS) may turn into a NaN."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", 2 if name == "window" else 0)
    ops._WIN_CACHE.clear()
    (kind, k, s, p), x, w, g = _edge_operands(name, 9)
    precision = 3 if form == "fp8" else 0
    tag = form == "f16x2"
    before = (dict(ops.F16_CALLS), ops.FP8_CALLS[0])
    y, dx, dw = _sn_run(kind, k, s, p, torch.zeros_like(x), w, g, precision, tag)
    assert bool((y == 0).all()), "y of a zero input"
    assert bool((dw == 0).all()), "dw of a zero input"
    assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
    y, dx, dw = _sn_run(kind, k, s, p, x, w, torch.zeros_like(g), precision, tag)
    assert bool((dx == 0).all()), "dx of a zero gradient"
    assert bool((dw == 0).all()), "dw of a zero gradient"
    assert torch.isfinite(y).all() and float(y.abs().max()) > 0
    if form == "f16x2":
        assert all(ops.F16_CALLS[kk] == before[0][kk] + 2 for kk in ("fwd", "dgrad", "wgrad"))
    if form == "fp8":
        assert ops.FP8_CALLS[0] == before[1] + 4
    ops._WIN_CACHE.clear()


@pytest.mark.parametrize("name", list(EDGE_GEOMS))
def test_single_nonzero_element(name, monkeypatch):
    """One non-zero element in x: the tensor's maximum IS that element, every other gathered value is an exact zero, and the output
    is the corresponding slice of w / sigma times it - within the bounds of test_conv_fp16_pieces_vs_cpu against float64."""
    from locate_amd import ops
    monkeypatch.setattr(ops, "F16_MIN_FLOPS", 0.0)
    monkeypatch.setattr(ops, "WIN_MODE", 2 if name == "window" else 0)
    ops._WIN_CACHE.clear()
    (kind, k, s, p), x, w, g = _edge_operands(name, 10)
    one = torch.zeros_like(x)
    B, C, H, W = x.shape
    one[B - 1, C - 1, H // 2, W // 2] = -1.7
    got = _sn_run(kind, k, s, p, one, w, g)
    want = _ref64(kind, s, p, one, w, g)
    for what, tol, a, b in zip(("y", "dx", "dw"), (2e-5, 2e-5, 5e-5), got, want):
        assert torch.isfinite(a).all(), what
        assert_close(a, b, tol, what)
    assert int((got[0] != 0).sum()) <= w.numel() // (w.shape[1] if kind == "conv" else w.shape[0])
    ops._WIN_CACHE.clear()
