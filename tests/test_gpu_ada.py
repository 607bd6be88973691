"""The adaptive augmentation's kernels on the MI355X: the per-image op mask of csrc/diffaug.hip against the static instantiations it
must equal bit for bit, and csrc/ada.hip's gate and observer against the numpy definition (tests/helpers/ada_model.py) with ==.

Shapes as in tests/test_gpu_diffaug.py - S = 32, n = 5 | S = 64, n = 3 | S = 128, n = 2 | S = 256, n = 2 - with a batch of 8 images
that carry the masks 0 .. 7 (image k is source image k % n)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ada_model as A  # noqa: E402
import diffaug_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(32, 5), (64, 3), (128, 2), (256, 2)]
SENTINEL = 0x7FC0DEAD
SNAN, NEG_INF = 0x7F800001, 0xFF800000          # a signalling NaN (a multiplication by 1.0f would quiet it) and -Inf
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def offset_views(values, words):
    """`values` (int32 bit patterns) inside a larger allocation, `words` words past a 16-byte boundary, between sentinel guards"""
    flat = torch.full((values.size + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[32 + words:32 + words + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values).to(DEV))
    return flat, view


def guards_intact(flat, words, size):
    host = flat.cpu().numpy()
    return bool((host[:32 + words] == SENTINEL).all() and (host[32 + words + size:] == SENTINEL).all())


# ---- 1. the mask ---------------------------------------------------------------------------------------------------------------------
def rows_for(S):
    D, cut = M.shift_bound(S), M.cut_size(S)
    h = cut // 2
    rows = [
        M.make_row(b=0.25, s=0.0, c=0.5, ty=0, tx=0, y0=0, y1=0, x0=0, x1=0),
        M.make_row(b=-0.5, s=2.0, c=1.5, ty=D, tx=D, y0=0, y1=h, x0=0, x1=h),
        M.make_row(b=0.1, s=0.7, c=0.5, ty=-D, tx=-D, y0=S - h, y1=S, x0=S - h, x1=S),
        M.make_row(b=0.0, s=1.3, c=0.9, ty=D, tx=-D, y0=0, y1=h, x0=S - h, x1=S),
        M.make_row(b=-0.2, s=1.9, c=0.6, ty=1, tx=-3, y0=5, y1=5 + cut, x0=3, x1=3 + cut),
    ]
    drawn = M.rows_from_uniform(np.random.default_rng(200 + S).uniform(0.0, 1.0, size=(3, 7)), S)
    rows = np.concatenate([np.stack(rows), drawn]).astype(np.float32)
    assert rows.shape == (8, 12) and not rows[:, 9:].any()
    return rows


_BATCH, _REFERENCE = {}, {}


def batch(S, n):
    """(x, g, rows): 8 images, image k being source image k % n; made once per size.  Bit patterns (int32), on the device."""
    if S not in _BATCH:
        rng = np.random.default_rng(S + 1)
        idx = np.arange(8) % n
        x = rng.uniform(-1.0, 1.0, size=(n, 3, S, S)).astype(np.float32)[idx]
        g = rng.uniform(-1.0, 1.0, size=(n, 3, S, S)).astype(np.float32)[idx]
        _BATCH[S] = (torch.from_numpy(bits(x)).to(DEV), torch.from_numpy(bits(g)).to(DEV), rows_for(S))
    return _BATCH[S]


def launch(src, rows, S, policy, backward, dst=None):
    """the raw entry over int32 bit patterns on the device; returns the output's bit patterns (a device tensor)"""
    from locate_amd._lib import check, lib
    n = src.shape[0]
    dst = torch.empty_like(src) if dst is None else dst
    p = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(DEV)
    ws = torch.empty(max(int(lib().locate_diffaug_workspace_bytes(n, S)), 16), dtype=torch.uint8, device=DEV)
    entry = lib().locate_diffaug_bwd if backward else lib().locate_diffaug_fwd
    check(entry(src.data_ptr(), p.data_ptr(), dst.data_ptr(), n, S, policy, ws.data_ptr(), stream()), "locate_diffaug")
    return dst


def reference(S, n, ops, backward):
    """what the instantiation `ops` writes for the batch with word 9 zero: computed once, kept on the host, read-only"""
    key = (S, ops, backward)
    if key not in _REFERENCE:
        x, g, rows = batch(S, n)
        out = launch(g if backward else x, rows, S, ops, backward).cpu().numpy()
        out.setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]


@pytest.mark.parametrize("S,n", SHAPES)
def test_mask_equals_the_instantiation_without_the_masked_ops(S, n):
    """forward and backward of image k under static policy P and mask k == the instantiation P & ~k on the same row, bit for bit;
    again with source and destination one word past a 16-byte boundary, the guards around the destination intact"""
    x, g, rows = batch(S, n)
    masked = rows.copy()
    masked[:, 9] = np.arange(8, dtype=np.float32)
    for backward, src in ((False, x), (True, g)):
        src_flat, src_off = offset_views(src.cpu().numpy(), 1)
        for policy in range(1, 8):
            got = launch(src, masked, S, policy, backward).cpu().numpy()
            dst_flat, dst_off = offset_views(np.zeros(tuple(src.shape), np.int32), 1)
            assert src_off.data_ptr() % 16 == 4 and dst_off.data_ptr() % 16 == 4
            got_off = launch(src_off, masked, S, policy, backward, dst=dst_off).cpu().numpy()
            assert guards_intact(dst_flat, 1, src.numel()), "policy %d: a word outside the output was written" % policy
            for k in range(8):
                want = reference(S, n, policy & ~k, backward)[k]
                assert np.array_equal(got[k], want), "%s policy %d mask %d: %d words differ from instantiation %d" % (
                    "backward" if backward else "forward", policy, k, int((got[k] != want).sum()), policy & ~k)
                assert np.array_equal(got_off[k], want), "policy %d mask %d: the buffers' alignment shows" % (policy, k)
    # the comparison is not vacuous: masks change the result, and a fully masked image is its source
    full = reference(S, n, 7, False)
    assert not np.array_equal(full[0], x[0].cpu().numpy()) and np.array_equal(reference(S, n, 0, False), x.cpu().numpy())


@pytest.mark.parametrize("S,n", SHAPES)
def test_non_finite_values_pass_a_masked_op_with_their_bits(S, n):
    """a signalling NaN and -Inf under a masked cutout and under a masked colour: the rows have no shift, so the whole image, the two
    words included, comes out as it went in - no 1.0f * x, no colour chain - while the same rows unmasked do change them"""
    x, g, _ = batch(S, n)
    cut = M.cut_size(S)
    row = M.make_row(b=0.1, s=0.8, c=1.1, ty=0, tx=0, y0=8, y1=8 + cut, x0=8, x1=8 + cut).astype(np.float32)
    for backward, clean in ((False, x), (True, g)):
        src = clean[:4].clone()
        src[:, 1, 12, 12] = SNAN          # int32 bit patterns: under the cut
        src[:, 2, 9, 20] = NEG_INF - (1 << 32)          # the same 32 bits as an int32
        want = src.cpu().numpy()
        for policy, mask in ((M.FULL, 5), (M.FULL, 7), (M.CUTOUT, 4), (M.COLOR, 1), (M.COLOR | M.CUTOUT, 5), (M.TRANSLATION | M.CUTOUT, 4)):
            rows = np.tile(row, (4, 1))
            rows[:, 9] = mask
            got = launch(src, rows, S, policy, backward).cpu().numpy()
            assert np.array_equal(got, want), "policy %d mask %d: %d words changed" % (policy, mask, int((got != want).sum()))
        rows = np.tile(row, (4, 1))
        unmasked = launch(src, rows, S, M.CUTOUT, backward).cpu().numpy()
        assert unmasked[0, 1, 12, 12] != SNAN and np.isnan(unmasked.view(np.float32)[0, 1, 12, 12])          # 0.0f * sNaN: quiet


# ---- 2. the gate ---------------------------------------------------------------------------------------------------------------------
def gate_rows(n, p, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, 12)).astype(np.float32)
    raw[:, 9:] = A.gate_uniforms(rng.random((n, 3)))
    special = [0.0, f32(p), A.GATE_CAP, np.nextafter(f32(p), f32(0)), np.nextafter(f32(p), f32(1))]
    for k, value in enumerate(special):          # exactly 0, exactly p, the cap, p's neighbours: in every column
        raw[k % n, 9 + k % 3] = value
        raw[(k + 1) % n, 9 + (k + 1) % 3] = value
    words = raw.view(np.uint32)
    words[0, 0], words[0, 1], words[n - 1, 8] = SNAN, NEG_INF, 0x7FC12345          # words 0 .. 8 are copied as bits
    return raw


@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("p", [0.0, 2.0 ** -24, 0.5, 1.0])
def test_gate_equals_the_model(n, p):
    from locate_amd._lib import check, lib
    raw = gate_rows(n, p, seed=n)
    state = torch.from_numpy(A.new_state(p).view(np.int32).copy()).to(DEV)
    src = torch.from_numpy(raw).to(DEV)
    for policy in range(8):
        flat, out = offset_views(np.full((n, 12), 0x55555555, np.int32), 0)
        check(lib().locate_ada_gate(src.data_ptr(), state.data_ptr(), out.data_ptr(), n, policy, stream()), "locate_ada_gate")
        got = out.cpu().numpy().view(np.uint32)
        want = A.gate(raw, p, policy).view(np.uint32)
        assert np.array_equal(got, want), "policy %d: %d words differ" % (policy, int((got != want).sum()))
        assert np.array_equal(got[:, :9], raw.view(np.uint32)[:, :9]) and not got[:, 10:].any()
        assert guards_intact(flat, 0, n * 12)
    assert np.array_equal(state.cpu().numpy().view(np.uint32), A.new_state(p))          # the gate only reads the record


# ---- 3. the observer -----------------------------------------------------------------------------------------------------------------
def both(batches, interval, target, step, p_max, p0, capacity=8, first_iteration=1):
    """the sequence through the kernel and through the model: (device state, device ring, model state, model ring) as uint32"""
    from locate_amd._lib import check, lib
    state_m, ring_m = A.new_state(p0), A.new_ring(capacity)
    state_flat, state = offset_views(state_m.view(np.int32).copy(), 0)
    ring_flat, ring = offset_views(ring_m.view(np.int32).copy(), 0)
    for k, x in enumerate(batches):
        x = np.ascontiguousarray(x, np.float32)
        d = torch.from_numpy(x).to(DEV)
        check(lib().locate_ada_observe(d.data_ptr(), x.size, first_iteration + k, state.data_ptr(), ring.data_ptr(), capacity, interval, target,
                                       float(step), p_max, stream()), "locate_ada_observe")
        A.observe(x, first_iteration + k, state_m, ring_m, interval, target, step, p_max)
    torch.cuda.synchronize()
    assert guards_intact(state_flat, 0, 16) and guards_intact(ring_flat, 0, capacity * 4)
    return state.cpu().numpy().view(np.uint32), ring.cpu().numpy().view(np.uint32), state_m, ring_m


SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("interval", [1, 3])
def test_observe_equals_the_model_on_mixed_logits(B, interval):
    rng = np.random.default_rng(B)
    batches = []
    for k in range(3 * interval + 1):
        x = (rng.standard_normal(B) + 0.4).astype(np.float32)
        if B == 1:
            x[0] = [np.nan, 1.0, -0.0, np.inf, -np.inf, 0.0, -2.0, 0.5, np.nan, 3.0][k]
        else:
            x[rng.choice(B, size=min(5, B), replace=False)] = SPECIALS[:min(5, B)]
        batches.append(x)
    state, ring, state_m, ring_m = both(batches, interval, 0.1, f32(0.03125), 1.0, 0.25)
    assert np.array_equal(state, state_m), (A.fields(state), A.fields(state_m))
    assert np.array_equal(ring, ring_m)
    assert A.fields(state)["closed"] == (3 * interval + 1) // interval and A.fields(state)["nan"] > 0


UP, DOWN, MEET = np.ones(5, np.float32), -np.ones(5, np.float32), np.array([1.0, 1.0, 1.0, 1.0, -1.0], np.float32)


@pytest.mark.parametrize("name, batches, p0, p_max, ps", [
    ("up", [UP], 0.25, 1.0, [0.375, 0.5, 0.625]),
    ("down", [DOWN], 0.5, 1.0, [0.375, 0.25, 0.125]),
    ("sticks at 0", [DOWN], 0.125, 1.0, [0.0, 0.0, 0.0]),
    ("sticks at p_max", [UP], 0.5, 0.6, [float(f32(0.6))] * 3),
    ("meets the target", [MEET], 0.5, 1.0, [0.5, 0.5, 0.5]),
    ("up, meets, down", [UP, UP, MEET, MEET, DOWN, DOWN, UP], 0.5, 1.0, [0.625, 0.625, 0.5]),
])
def test_observe_sequences(name, batches, p0, p_max, ps):
    interval = 2
    seq = [batches[k % len(batches)] for k in range(3 * interval + 1)]
    state, ring, state_m, ring_m = both(seq, interval, 0.6, f32(0.125), p_max, p0, first_iteration=100)
    assert np.array_equal(state, state_m) and np.array_equal(ring, ring_m), name
    assert [row["p"] for row in A.curve(ring, 0, 3)] == ps and [row["iteration"] for row in A.curve(ring, 0, 3)] == [101, 103, 105]
    assert A.fields(state)["seen"] == 1 and A.fields(state)["counted"] == 5          # the seventh observation waits in the open window
    if name == "meets the target":
        assert A.fields(state)["r"] == f32(0.6) and A.fields(state)["ups"] == A.fields(state)["downs"] == 0


def test_observe_ring_wraps():
    rng = np.random.default_rng(5)
    seq = [rng.standard_normal(65).astype(np.float32) for _ in range(11)]
    state, ring, state_m, ring_m = both(seq, 1, 0.0, f32(0.01), 1.0, 0.3, capacity=4)
    assert np.array_equal(state, state_m) and np.array_equal(ring, ring_m)
    assert A.fields(state)["rows"] == 11 and [row["iteration"] for row in A.curve(ring, 7, 11)] == [8, 9, 10, 11]


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    ok = (t.data_ptr(), 4, 1, t.data_ptr(), t.data_ptr(), 4, 2, 0.6, 0.1, 1.0, None)
    for k, bad in ((1, 0), (5, 0), (6, 0), (7, float("nan")), (8, -0.1), (9, 0.0), (9, 1.5), (0, None), (3, None)):
        args = list(ok)
        args[k] = bad
        assert lib().locate_ada_observe(*args) != 0, (k, bad)
    assert lib().locate_ada_observe(t.data_ptr(), 1 << 30, 1, t.data_ptr(), t.data_ptr(), 4, 4, 0.6, 0.1, 1.0, None) != 0          # the window's int32
    for args in ((t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 7, None), (t.data_ptr(), t.data_ptr(), t[16:].data_ptr(), 0, 7, None),
                 (t.data_ptr(), t.data_ptr(), t[16:].data_ptr(), 1, 8, None), (None, t.data_ptr(), t[16:].data_ptr(), 1, 7, None)):
        assert lib().locate_ada_gate(*args) != 0, args
    torch.cuda.synchronize()
    assert not t.any()


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------
def test_two_identical_call_sequences_give_identical_bytes():
    from locate_amd import AdaptiveDiffAugment, diff_augment
    rng = np.random.default_rng(9)
    logits = [torch.from_numpy((rng.standard_normal(8) + 0.5).astype(np.float32)).to(DEV) for _ in range(9)]
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(8, 3, 32, 32)).astype(np.float32)).to(DEV)
    runs = []
    for _ in range(2):
        a = AdaptiveDiffAugment(S=32, batch=8, seed=3, device=DEV, target=0.2, interval=2, kimg=0.1, initial_p=0.5)
        seen = []
        for d in logits:
            a.draw()
            seen.append(diff_augment(x, a.params[:8], a.bits).cpu().numpy().view(np.int32))
            seen.append(a.params.cpu().numpy().view(np.int32))
            a.observe(d)
        a.flush()
        runs.append((seen, a.state.cpu().numpy(), a._ring.cpu().numpy(), a.curve(), a.status()))
    for one, two in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(one, two)
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2]) and runs[0][3:] == runs[1][3:]
    status = runs[0][4]
    assert status["updates"] == 4 and len(runs[0][3]) == 4 and status["ups"] + status["downs"] > 0 and status["p"] != 0.5
