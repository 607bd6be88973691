"""The numpy model of the nearest-neighbour search (tests/helpers/neighbours_model.py) against plainer spellings of the same
definitions, and the property the whole construction rests on: the encoder inverts `data.output_lut()` for all 256 bytes."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import neighbours_model as M  # noqa: E402


def test_the_encoder_inverts_the_output_table_for_every_byte():
    from locate_amd.data import output_lut
    lut = output_lut().numpy()
    assert lut.dtype == np.float32 and lut.shape == (256,)
    t = (lut + np.float32(1)) * np.float32(127.5)
    assert t.dtype == np.float32
    assert np.array_equal(np.rint(t), np.arange(256, dtype=np.float32))
    assert float(np.abs(t.astype(np.float64) - np.arange(256)).max()) <= 4e-6          # nowhere near a half-way point
    x = np.zeros((1, 3, 16, 16), dtype=np.float32)
    x.reshape(-1)[:256] = lut
    x.reshape(-1)[256:512] = lut[::-1]
    codes, norms, flags = M.encode(x)
    want = np.concatenate([np.arange(256), np.arange(256)[::-1]]) - 128
    assert np.array_equal(codes[0, :512], want) and flags[0] == 0
    assert norms[0] == int((codes[0].astype(np.int64) ** 2).sum())


def test_encoder_model_edge_cases():
    S = 4
    x = np.zeros((2, 3, S, S), dtype=np.float32)
    flat = x.reshape(2, -1)
    flat[0, :8] = [-1.0, 1.0, -0.0, 1e-40, -1.5, 1.5, -1.0 - 1e-3, 1.0 + 1e-3]
    flat[1, :4] = [np.nan, np.inf, -np.inf, 0.25]
    codes, norms, flags = M.encode(x)
    assert codes.shape == (2, 64) and not codes[:, 48:].any()
    assert codes[0, :8].tolist() == [-128, 127, 0, 0, -128, 127, -128, 127]          # 127.5 is a tie: to the even 128
    assert flags.tolist() == [0, 3] and codes[1, :3].tolist() == [0, 0, 0]
    assert codes[1, 3] == int(np.rint(np.float32(1.25) * np.float32(127.5))) - 128
    # every half-way point (n + 0.5) / 127.5 - 1 the float32 grid can hold: wherever t lands on n + 0.5 exactly, the even one
    n = np.arange(255)
    half = ((n + 0.5) / 127.5 - 1).astype(np.float32)
    t = (half + np.float32(1)) * np.float32(127.5)
    y = np.zeros((1, 3, 12, 12), dtype=np.float32)
    y.reshape(-1)[:255] = half
    got = M.encode(y)[0][0, :255].astype(np.int64) + 128
    exact = t == (n + 0.5).astype(np.float32)
    assert exact.any()
    assert np.array_equal(got[exact], (n + (n % 2))[exact])
    assert np.array_equal(got, np.rint(t).astype(np.int64))


def plain_topk(d2, k, qflags, rflags, skip):
    out = []
    for i in range(d2.shape[0]):
        cand = [] if qflags[i] else sorted((int(d2[i, j]), j) for j in range(d2.shape[1]) if not rflags[j] and j != skip[i])
        cand = (cand + [(-1, -1)] * k)[:k]
        out.append(cand)
    return np.array(out)[:, :, 0], np.array(out)[:, :, 1]


def test_topk_against_a_plain_sort():
    rng = np.random.default_rng(3)
    q = rng.integers(-128, 128, size=(9, 64), dtype=np.int8)
    r = rng.integers(-128, 128, size=(21, 64), dtype=np.int8)
    r[7] = r[2]
    r[20] = r[2]          # ties
    q[4] = r[2]          # distance 0, three times
    d2 = M.distances(q, r)
    assert np.array_equal(d2, ((q.astype(np.int64)[:, None] - r.astype(np.int64)[None]) ** 2).sum(-1))
    assert np.array_equal(d2, M.norms(q)[:, None] + M.norms(r)[None] - 2 * (q.astype(np.int64) @ r.astype(np.int64).T))          # the Gram form
    qflags, rflags = np.zeros(9, np.int32), np.zeros(21, np.int32)
    qflags[1], rflags[5], rflags[7] = 2, 1, 4
    skip = np.full(9, -1)
    skip[4], skip[0] = 2, 11
    for k in (1, 3, 8):
        got = M.topk(d2, k, qflags, rflags, skip)
        want = plain_topk(d2, k, qflags, rflags, skip)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    d, i = M.topk(d2, 3, qflags, rflags, skip)
    assert i[4].tolist()[0] == 20 and d[4, 0] == 0 and (i[1] == -1).all() and (d[1] == -1).all()          # 2 skipped, 7 flagged
    d, i = M.topk(d2[:, :2], 3)
    assert (i[:, 2] == -1).all() and (d[:, 2] == -1).all() and (i[:, :2] >= 0).all()          # k > candidates


def test_canonical_view_and_summary():
    rng = np.random.default_rng(4)
    store = rng.integers(0, 256, size=(3, 10, 14, 3), dtype=np.uint8)
    codes = M.bank_codes(store, 8)
    assert codes.shape == (3, 192) and codes.dtype == np.int8
    # a square image at its own size is its own canonical view
    square = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    assert np.array_equal(M.canonical_u8(square, 8), square)
    assert M.rms(-1, 8) is None and M.rms(0, 8) == 0.0 and abs(M.rms(255 * 255 * 192, 8) - 2.0) < 1e-12
    assert M.summary([None, None]) == {"min": None, "median": None}
    assert M.summary([3.0, None, 1.0, 2.0]) == {"min": 1.0, "median": 2.0}
