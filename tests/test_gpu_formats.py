"""The format audit on the MI355X: the kernels through the raw C ABI against the model (tests/helpers/formats_model.py) - both block
axes, partial blocks, several tiles, a batch stride with slack, a base that is only 4-byte aligned, ties, denormals, NaN and Inf,
guards around every buffer, the same bits from call to call and whatever else the call holds - and `FormatAudit` around a running
training: the tap sees every dense contraction, the rows are what the model says of the operands, and the trajectory stays where a
run without it would be."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import formats_model as M  # noqa: E402
import stats_model as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = torch.as_tensor
GUARD = 32
SENTINEL = 0x7FC0DEAD                # as int32: a NaN with a payload of its own - a read outside a view would be counted
SENTINEL64 = 0x5EAD5EAD5EAD5EAD
WORDS = 58                           # int64 words of a 464-byte slot


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def family():
    """[(what, x, {axis: the model's record})], computed once"""
    return [(what, x, {axis: M.audit(x, axis) for axis in (1, 2)}) for what, x in M.fixtures()]


class Placed:
    """views inside ONE allocation, each between sentinel guards, at a chosen offset (in elements) from a 16-byte boundary and
    with `slack` sentinel words behind every batch element; the allocation is compared afterwards: nothing may be written"""

    def __init__(self):
        self.words, self.views, self.size = [], [], 0

    def add(self, x, axis, offset=0, slack=0):
        B, C, P = x.shape
        stride = C * P + slack
        body = np.full((B, stride), SENTINEL, dtype=np.int32)
        body[:, :C * P] = np.ascontiguousarray(x, dtype=np.float32).reshape(B, C * P).view(np.int32)
        total = -(-(GUARD + offset + body.size + GUARD) // 4) * 4
        piece = np.full(total, SENTINEL, dtype=np.int32)
        piece[GUARD + offset:GUARD + offset + body.size] = body.reshape(-1)
        self.views.append((self.size + GUARD + offset, B, C, P, stride, axis))
        self.words.append(piece)
        self.size += total
        return len(self.views) - 1

    def upload(self):
        self.host = np.concatenate(self.words)
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def records(self, which=None):
        which = range(len(self.views)) if which is None else which
        return [(self.dev.data_ptr() + 4 * self.views[i][0],) + self.views[i][1:] for i in which]

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def pack(records):
    return b"".join(struct.pack("<Qiii4xqi4x", *r) for r in records)


def audit_raw(records, slots, n_slots, rows=None):
    """One call of locate_formats_audit with guarded rows and a guarded workspace; returns (host int64 [n_slots, 58], device rows)."""
    from locate_amd._lib import check, lib
    L = lib()
    assert L.locate_formats_view_record_bytes() == 40 and L.locate_formats_base_record_bytes() == 304
    assert L.locate_formats_format_record_bytes() == 32 and L.locate_formats_count() == 5 and L.locate_formats_max_views() == 8
    rec = pack(records)
    need = L.locate_formats_workspace_bytes(rec, len(records))
    assert need > 0 and need % 8 == 0
    if rows is None:
        rows = torch.full((GUARD + n_slots * WORDS + GUARD,), SENTINEL64, dtype=torch.int64, device=DEV)
        rows[GUARD:GUARD + n_slots * WORDS] = 0
    ws = torch.full((GUARD + need // 8 + GUARD,), SENTINEL64, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    check(L.locate_formats_audit(rec, len(records), (ctypes.c_int * len(slots))(*slots), p(rows[GUARD:]), p(ws[GUARD:]),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "locate_formats_audit")
    torch.cuda.synchronize()
    host, wsh = rows.cpu().numpy(), ws.cpu().numpy()
    assert (host[:GUARD] == SENTINEL64).all() and (host[GUARD + n_slots * WORDS:] == SENTINEL64).all(), "a guard around the rows was written"
    assert (wsh[:GUARD] == SENTINEL64).all() and (wsh[GUARD + need // 8:] == SENTINEL64).all(), "a guard around the workspace was written"
    return host[GUARD:GUARD + n_slots * WORDS].reshape(n_slots, WORDS).copy(), rows


def decode(words):
    from locate_amd.formats import decode as d
    return d(words)


def assert_record(d, i, want, what):
    """slot i of decoded rows against a model record: counts, absmax and histogram exactly, the two kinds of sums within the bound
    of a float64 sum of n exactly known non-negative terms (stats_model.sumsq_tolerance)"""
    for key in ("n", "zeros", "nonfinite", "calls"):
        assert int(d[key][i]) == want[key], (what, key, int(d[key][i]), want[key])
    assert int(d["absmax"][i:i + 1].view(np.uint32)[0]) == want["absmax"], (what, "absmax")
    assert [int(v) for v in d["hist"][i]] == want["hist"], (what, "hist", d["hist"][i].tolist(), want["hist"])
    n = want["n"]
    assert S.sumsq_close(float(d["sumsq"][i]), want["sumsq"], n), (what, "sumsq", float(d["sumsq"][i]), want["sumsq"])
    for f, fr in enumerate(want["formats"]):
        for key in ("flushed", "subnormal", "clamped"):
            assert int(d[key][i, f]) == fr[key], (what, M.NAMES[f], key, int(d[key][i, f]), fr[key])
        assert S.sumsq_close(float(d["err_sumsq"][i, f]), fr["err_sumsq"], n), (what, M.NAMES[f], float(d["err_sumsq"][i, f]), fr["err_sumsq"])


def test_names_and_sizes():
    from locate_amd.formats import FormatAudit, format_names
    assert format_names() == M.NAMES == FormatAudit.FORMAT_NAMES
    from locate_amd._lib import lib
    assert lib().locate_formats_name(5) is None and lib().locate_formats_name(-1) is None


def test_kernel_against_the_model(family):
    placed, expect = Placed(), []
    for what, x, model in family:
        for axis in (1, 2):
            variants = [(0, 0)]
            if x.shape == (2, 33, 5):
                variants += [(0, 7), (1, 3)]          # a channel slice of a wider tensor; and only 4-byte aligned
            if x.shape in ((1, 64, 67), (2, 40, 150)):
                variants += [(1, 0), (3, 0)]
            for offset, slack in variants:
                placed.add(x, axis, offset, slack)
                expect.append(("%s axis %d offset %d slack %d" % (what, axis, offset, slack), model[axis]))
    placed.upload()
    records = placed.records()
    for at in range(0, len(records), 8):
        part = records[at:at + 8]
        host, _ = audit_raw(part, list(range(len(part))), len(part))
        d = decode(host)
        for i in range(len(part)):
            assert_record(d, i, *reversed(expect[at + i]))
    assert placed.untouched()
    tiles = [(-(-B * -(-C // 32) * P // 256), -(-B * C * -(-P // 32) // 128)) for B, C, P in M.SHAPES]
    assert max(t[0] for t in tiles) > 1 and max(t[1] for t in tiles) > 1          # a view that spans several tiles, on either axis


def test_a_view_does_not_depend_on_its_surroundings(family):
    by_what = {what: x for what, x, _ in family}
    x, other = by_what["[2, 40, 150] plain"], by_what["[1, 64, 67] max"]
    for axis in (1, 2):
        placed = Placed()
        a0 = placed.add(x, axis, 0, 0)
        a1 = placed.add(x, axis, 1, 0)          # another alignment
        a2 = placed.add(x, axis, 2, 5)          # and slack in the batch stride
        rest = [placed.add(other, 1 + k % 2, k % 4, k) for k in range(7)]
        placed.upload()
        alone, _ = audit_raw(placed.records([a0]), [0], 1)
        again, _ = audit_raw(placed.records([a0]), [0], 1)
        assert alone.tobytes() == again.tobytes(), "two calls, two results"
        crowd, _ = audit_raw(placed.records(rest[:3] + [a0] + rest[3:]), [4, 2, 7, 5, 0, 1, 3, 6], 8)
        assert crowd[5].tobytes() == alone[0].tobytes(), "the record changed beside seven other views"
        for i in (a1, a2):
            moved, _ = audit_raw(placed.records([i]), [0], 1)
            assert moved.tobytes() == alone.tobytes(), "the record depends on alignment or batch stride"
        assert placed.untouched()


def test_two_calls_into_one_row_add_up(family):
    by_what = {what: (x, model) for what, x, model in family}
    (xa, ma), (xb, mb) = by_what["[1, 64, 67] plain"], by_what["[2, 33, 5] max"]
    placed = Placed()
    ia, ib = placed.add(xa, 2), placed.add(xb, 1, 1, 3)
    placed.upload()
    first, rows = audit_raw(placed.records([ia]), [1], 3)
    both, _ = audit_raw(placed.records([ib]), [1], 3, rows=rows)
    assert not both[0].any() and not both[2].any(), "a slot no view names was written"
    assert_record(decode(first), 1, ma[2], "first call")
    assert_record(decode(both), 1, M.accumulate(ma[2], mb[1]), "both calls")


def test_bad_arguments_are_refused():
    from locate_amd._lib import lib
    L = lib()
    x = torch.ones(2 * 3 * 4 + 8, dtype=torch.float32, device=DEV)
    rows = torch.full((2 * WORDS,), SENTINEL64, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 12, dtype=torch.int64, device=DEV)
    good = (x.data_ptr(), 2, 3, 4, 12, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    slots = (ctypes.c_int * 8)(0, 1, 0, 0, 0, 0, 0, 0)

    def call(records, n=None, slots=slots, rows_p=p(rows), ws_p=p(ws)):
        return L.locate_formats_audit(pack(records), len(records) if n is None else n, slots, rows_p, ws_p, None)
    bad = [[good[:5] + (0,)], [good[:5] + (3,)], [(x.data_ptr(), 0, 3, 4, 12, 1)], [(x.data_ptr(), 2, -3, 4, 12, 2)],
           [(x.data_ptr(), 2, 3, 0, 12, 2)], [good[:4] + (11, 1)], [(0, 2, 3, 4, 12, 1)], [(x.data_ptr() + 2, 2, 3, 4, 12, 1)],
           [good, good[:5] + (7,)]]
    for records in bad:
        assert call(records) == 1, records
        assert b"locate_formats" in L.locate_last_error()
        assert L.locate_formats_workspace_bytes(pack(records), len(records)) == 0
    assert call([good], n=0) == 1 and call([good] * 8, n=9) == 1 and call([good], n=-1) == 1
    assert call([good, good], slots=(ctypes.c_int * 2)(1, 1)) == 1 and call([good], slots=(ctypes.c_int * 1)(-1)) == 1
    assert call([good], rows_p=None) == 1 and call([good], ws_p=None) == 1 and call([good], slots=None) == 1
    assert call([good], rows_p=ctypes.c_void_p(rows.data_ptr() + 4)) == 1
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == SENTINEL64).all(), "a refused call wrote its rows"
    rows.zero_()
    assert call([good, good[:5] + (2,)]) == 0          # and the same arguments, undamaged, are taken
    torch.cuda.synchronize()
    d = decode(rows.cpu().numpy())
    assert d["n"].tolist() == [24, 24] and d["calls"].tolist() == [1, 1] and d["sumsq"].tolist() == [24.0, 24.0]


def test_format_errors_maps_tensors_to_views(family):
    from locate_amd import format_errors
    x = next(x for what, x, _ in family if what == "[2, 40, 150] plain")
    wide = torch.full((2, 50, 15, 10), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, 6:46] = T(x).to(DEV).view(2, 40, 15, 10)
    piece = wide[:, 6:46]          # dense planes, a batch stride with slack: read in place
    rows = T(x[0]).to(DEV)          # [40, 150] as [1, 40, 150]
    flat = T(x[1, 3]).to(DEV)          # [150] as [1, 1, 150]
    strided = T(np.ascontiguousarray(x.transpose(0, 2, 1))).to(DEV).transpose(1, 2)          # [2, 40, 150], planes not dense: copied
    out = format_errors([piece, rows, flat, strided, piece], axis=[1, 2, 2, 1, 2])
    want = [M.audit(x, 1), M.audit(x[:1], 2), M.audit(x[1:, 3:4], 2), M.audit(x, 1), M.audit(x, 2)]
    for got, model in zip(out, want):
        assert (got["n"], got["zeros"], got["nonfinite"]) == (model["n"], model["zeros"], model["nonfinite"])
        assert got["hist"].tolist() == model["hist"] and S.sumsq_close(got["sumsq"], model["sumsq"], model["n"])
        for name, fr in zip(M.NAMES, model["formats"]):
            assert {k: got[name][k] for k in ("flushed", "subnormal", "clamped")} == {k: fr[k] for k in ("flushed", "subnormal", "clamped")}
            assert S.sumsq_close(got[name]["err_sumsq"], fr["err_sumsq"], model["n"])
            assert got[name]["snr_db"] == pytest.approx(10 * np.log10(model["sumsq"] / fr["err_sumsq"]), rel=1e-9)
    assert bool(torch.isnan(wide[:, :6]).all()) and bool(torch.isnan(wide[:, 46:]).all())
    with pytest.raises(TypeError):
        format_errors([torch.ones(4)])
    with pytest.raises(TypeError):
        format_errors([torch.ones(4, dtype=torch.float64, device=DEV)])
    with pytest.raises(ValueError):
        format_errors([torch.ones(4, device=DEV)], axis=3)


# ---- beside a training run: the tiny fixture network of tests/test_gpu_stats.py (32 x 32, base width 1, batch 8) ------------------------
def build_tiny():
    from locate_amd import Discriminator, Generator, Nadam, NetConfig, TrainStep
    z = load_golden("g8_tiny_e2e")
    cfg = NetConfig(image_size=32, base_feature_factor=1)
    G, D = Generator(cfg), Discriminator(cfg)
    G.load_state_dict({k[len("G/sd0/"):]: T(z[k]) for k in z.files if k.startswith("G/sd0/")})
    D.load_state_dict({k[len("D/sd0/"):]: T(z[k]) for k in z.files if k.startswith("D/sd0/")})
    G.noise = T(z["G/noise"])
    G, D = G.to(DEV), D.to(DEV)
    G.batched_spectral_norm = D.batched_spectral_norm = True
    step = TrainStep(G, D, Nadam(G.parameters(), lr=cfg.glr, betas=(cfg.beta1, cfg.beta2)),
                     Nadam(D.parameters(), lr=cfg.dlr, betas=(cfg.beta1, cfg.beta2)), stacked_d=True, minibatches=1)
    inputs = tuple(T(z["step1/" + k]).to(DEV) for k in ("latent", "real", "aug"))
    return G, D, step, inputs


def training_state(G, D, step):
    """every parameter (u and v included) and every Nadam state tensor, by name"""
    torch.cuda.synchronize()
    state = {"G/" + k: v.detach().clone() for k, v in G.state_dict().items()}
    state.update({"D/" + k: v.detach().clone() for k, v in D.state_dict().items()})
    for tag, net, opt in (("G", G, step.gen_opt), ("D", D, step.dis_opt)):
        for name, q in net.named_parameters():
            for k, v in opt.state.get(q, {}).items():
                if torch.is_tensor(v):
                    state["%s/opt/%s/%s" % (tag, name, k)] = v.detach().clone()
    return state


def as_view(t):
    """a cloned operand as the [B, C, P] array the audit saw"""
    a = t.cpu().numpy()
    return a.reshape(a.shape[0], a.shape[1], -1)


def test_the_tap_sees_every_dense_contraction():
    from locate_amd import FormatAudit, ops
    from locate_amd.formats import ROLES
    from locate_amd.nn import SpectralNorm
    G, D, step, (lat, real, aug) = build_tiny()
    step(lat, real, aug)          # one plain iteration first: the audited one is an ordinary one
    audit = FormatAudit(G, D, capacity=2)
    names = [n for n, _ in audit.layers]

    def layer_of(net, tag, pick):
        name_of = {id(p): n for n, p in net.named_parameters()}
        found = [(m.module.weight_bar.numel(), "%s/%s" % (tag, name_of[id(m.module.weight_bar)])) for m in net.modules()
                 if isinstance(m, SpectralNorm) and pick(m.module)]
        return min(found)[1]
    chosen = {"convT": layer_of(G, "G", lambda m: isinstance(m, torch.nn.ConvTranspose2d) and m.groups == 1),
              "linear": layer_of(G, "G", lambda m: isinstance(m, torch.nn.Linear)),          # a 1x1 map: its weight gradient is only queued
              "D conv": layer_of(D, "D", lambda m: isinstance(m, torch.nn.Conv2d) and m.groups == 1 and m.kernel_size != (1, 1))}
    keys = audit.key_map()
    wanted = {w.data_ptr(): name for name, w in audit.layers if name in chosen.values()}
    assert len(wanted) == 3 and set(wanted) <= set(keys)
    seen = []

    def chained(role, w, a, b, forward_of_r):
        if w is not None and w.data_ptr() in wanted:
            seen.append((wanted[w.data_ptr()], role, a.detach().clone(), None if b is None else b.detach().clone(), w.detach().clone(), forward_of_r))
        inner(role, w, a, b, forward_of_r)
    with audit.iteration(2):
        inner = ops.CONTRACTION_TAP
        assert inner is not None
        ops.CONTRACTION_TAP = chained
        step(lat, real, aug)
    assert ops.CONTRACTION_TAP is None
    with pytest.raises(RuntimeError, match="stop here"):
        with audit.iteration(3):
            assert ops.CONTRACTION_TAP is not None
            raise RuntimeError("stop here")
    assert ops.CONTRACTION_TAP is None
    rows = audit.flush()
    assert [r["iteration"] for r in rows] == [2] and audit.unmatched == 0
    row = rows[0]
    entries = audit.entries()
    assert len(entries) == 6 * len(names) == row["calls"].size and [r for _, r in entries[:6]] == list(ROLES)
    calls = row["calls"].reshape(len(names), 6)
    for j, role in enumerate(ROLES):
        if calls[:, j].any():
            idle = [names[i] for i in np.flatnonzero(calls[:, j] == 0)]
            # a layer without an input gradient (the first of a network) has no dgrad; every other role reaches every layer
            assert not idle or (role.startswith("dgrad") and len(idle) <= 2), (role, idle)
    assert calls[:, [0, 1, 4, 5]].all() and (calls[:, 0] == calls[:, 1]).all() and (calls[:, 4] == calls[:, 5]).all()
    assert not row["nonfinite"].any()
    assert calls[names.index(chosen["D conv"]), 0] > 1, "the discriminator runs more than once per iteration"
    # the three layers: the model on the cloned operands, call by call, reproduces the rows
    want = {}
    for name, role, a, b, w, forward_of_r in seen:
        wm = w.cpu().numpy().reshape(1, w.shape[0], -1)
        if role == "wgrad":
            parts = [("wgrad.x", M.audit(as_view(a), 2)), ("wgrad.gy", M.audit(as_view(b), 2))]
        else:
            parts = [("fwd.x" if role == "fwd" else "dgrad.gy", M.audit(as_view(a), 1)), (role + ".w", M.audit(wm, 2 if forward_of_r else 1))]
        for full, rec in parts:
            want[name, full] = M.accumulate(want[name, full], rec) if (name, full) in want else rec
    kinds = {what: {role for name, role in want if name == chosen[what]} for what in chosen}
    assert all(k >= {"fwd.x", "fwd.w", "wgrad.x", "wgrad.gy"} for k in kinds.values()), kinds
    assert {"dgrad.gy", "dgrad.w"} <= kinds["convT"]
    for (name, role), rec in want.items():
        assert_record(row, audit.slot(name, role), rec, (name, role))
    convT = [s for s in seen if s[0] == chosen["convT"] and s[1] == "fwd"][0]
    assert convT[5] is False, "a ConvTranspose's forward is the adjoint contraction"
    report = audit.report()[0]
    assert report["snr_db"].shape == (len(entries), 5) and np.isfinite(report["snr_db"][row["calls"] > 0][:, 4]).all()
    assert (report["snr_db"][row["calls"] > 0][:, 4] > 40).all()          # bf16 keeps 8 significant bits: 6 dB each, less the rounding's share
    assert np.isnan(report["snr_db"][row["calls"] == 0]).all()
    assert audit.clear().rows == []


def test_an_audited_run_is_the_plain_run_bit_for_bit():
    from locate_amd import FormatAudit

    def run(audited):
        G, D, step, (lat, real, aug) = build_tiny()
        audit = FormatAudit(G, D) if audited else None
        losses = []
        for i in range(1, 4):
            if audited and i == 2:
                with audit.iteration(i):
                    out = step(lat, real, aug)
            else:
                out = step(lat, real, aug)
            losses.append({k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)})
        return training_state(G, D, step), losses, audit
    plain, plain_losses, _ = run(False)
    followed, losses, audit = run(True)
    assert sorted(plain) == sorted(followed)
    bad = [k for k in plain if not torch.equal(plain[k], followed[k])]
    assert not bad, "%d of %d tensors differ, first %s" % (len(bad), len(plain), bad[:4])
    assert any(k.endswith("weight_u") for k in plain) and any("/opt/" in k for k in plain)
    for a, b in zip(plain_losses, losses):
        assert sorted(a) == sorted(b) and len(a) >= 2 and all(torch.equal(a[k], b[k]) for k in a)
    assert audit.flush()[0]["calls"].sum() > 0 and audit.unmatched == 0


KEYS = ["absmax", "calls", "clamped", "err_sumsq", "flushed", "formats", "hist", "iterations", "n", "names", "nonfinite", "roles", "snr_db",
        "subnormal", "sumsq", "zeros"]


def test_trainer_writes_the_file_and_nothing_else(tmp_path):
    from locate_amd import DeviceImageStore, FormatAudit, InputPipeline, Trainer
    images = np.random.default_rng(6).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8)
    store = DeviceImageStore(images, DEV)

    def trainer(out, audited, **more):
        G, D, step, _ = build_tiny()
        pipeline = InputPipeline(store, 32, 8, seed=11)
        extra = dict(formats=FormatAudit(G, D), formats_every=2) if audited else {}
        extra.update(more)
        return Trainer(step, pipeline, str(out), epochs=2, max_iterations=4, images=13, seed=3, miniter_function=lambda e: 1,
                       subepoch_function=lambda e: 1, image_interval_function=lambda batch: 2, **extra)

    def files(out):
        return sorted(os.path.relpath(os.path.join(d, f), str(out)) for d, _, fs in os.walk(str(out)) for f in fs)
    t = trainer(tmp_path / "on", True)
    assert t.run() == 4 and t.formats.last_iteration == 4 and t.formats.rows == [] and t.formats.unmatched == 0
    path = os.path.join(str(tmp_path / "on"), "error", "1-formats.npz")
    assert path in t.written
    with np.load(path) as z:
        assert sorted(z.files) == KEYS and z["iterations"].tolist() == [2, 4] and z["formats"].tolist() == list(M.NAMES)
        e = len(z["names"])
        assert e == len(t.formats.entries()) and z["err_sumsq"].shape == (2, e, 5) and z["hist"].shape == (2, e, 32) and z["calls"].any()
        assert [tuple(p) for p in zip(z["names"].tolist(), z["roles"].tolist())] == t.formats.entries()
    plain = trainer(tmp_path / "off", False)
    assert plain.run() == 4
    assert [f for f in files(tmp_path / "on") if f != os.path.join("error", "1-formats.npz")] == files(tmp_path / "off")
    for name in ("netG.torch", "netD.torch"):
        a, b = (torch.load(str(folder / name), map_location="cpu", weights_only=True) for folder in (tmp_path / "on", tmp_path / "off"))
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a), name
    a, b = (torch.load(str(folder / "trainer.torch"), map_location="cpu", weights_only=True) for folder in (tmp_path / "on", tmp_path / "off"))
    assert sorted(a) == sorted(b)
    with pytest.raises(ValueError, match="graph"):
        trainer(tmp_path / "graphed", True, graphed=True)


def test_command_line_flag(tmp_path):
    store = str(tmp_path / "store.npy")
    np.save(store, np.random.default_rng(8).integers(0, 256, size=(32, 78, 64, 3), dtype=np.uint8))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "locate_amd.run", "--store", store, "--image-size", "32", "--batch", "8", "--out", out, "--epochs", "1",
           "--minibatches", "1", "--images", "16", "--formats-every", "2", "--max-iterations", "4"]          # 32 images in batches of 8: the epoch ends, its file is written
    refused = subprocess.run(cmd + ["--graph"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert refused.returncode == 2 and "--formats-every" in refused.stderr and not os.path.exists(out)
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    with np.load(os.path.join(out, "error", "1-formats.npz")) as z:
        assert sorted(z.files) == KEYS and z["iterations"].tolist() == [2, 4] and len(z["names"]) > 100 and z["calls"].any()
        assert set(z["roles"].tolist()) == {"fwd.x", "fwd.w", "dgrad.gy", "dgrad.w", "wgrad.x", "wgrad.gy"}
