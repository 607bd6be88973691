"""Numpy model of locate_amd/neighbours.py and csrc/neighbours.hip: the encoder in float32 with its three roundings, brute-force
int64 distances, the top-k by np.lexsort with the -1 rules, the canonical view through input_model.transform_u8, and the record
that `NearestNeighbours.search` returns.  Integers throughout: the GPU tests compare with ==."""
import numpy as np

import input_model

PLAIN = (3, 3, 3, 3)          # data.PLAIN_ORDER unpacked: four no-ops


def row_bytes(S):
    return (3 * S * S + 63) // 64 * 64


def encode(x):
    """x: float32 [n, 3, S, S] -> (codes int8 [n, row_bytes], norms int64 [n], nonfinite int32 [n])"""
    x = np.asarray(x, dtype=np.float32)
    n, S = x.shape[0], x.shape[-1]
    flat = x.reshape(n, -1)
    bad = ~np.isfinite(flat)
    with np.errstate(all="ignore"):
        t = (np.where(bad, np.float32(0), flat) + np.float32(1)) * np.float32(127.5)          # two fp32 roundings
        assert t.dtype == np.float32
        u = np.where(t < 0, np.float32(0), np.where(t > 255, np.float32(255), np.rint(t)))          # ties to even
    code = np.where(bad, 0, u.astype(np.int64) - 128)
    codes = np.zeros((n, row_bytes(S)), dtype=np.int8)
    codes[:, :flat.shape[1]] = code
    return codes, (code * code).sum(1).astype(np.int64), bad.sum(1).astype(np.int32)


def norms(codes):
    c = codes.astype(np.int64)
    return (c * c).sum(1)


def distances(qcodes, rcodes):
    """int64 [Q, N]: sum (code_q - code_r)^2, one query at a time"""
    r = rcodes.astype(np.int32)
    out = np.empty((qcodes.shape[0], rcodes.shape[0]), dtype=np.int64)
    for i, q in enumerate(qcodes.astype(np.int32)):
        d = r - q
        out[i] = (d * d).sum(1, dtype=np.int64)
    return out


def topk(d2, k, qflags=None, rflags=None, skip=None):
    """(d2 int64 [Q, k], index int32 [Q, k]): per query the k candidates with the smallest (d2, index); -1 in empty slots and in every
    slot of a flagged query; flagged references and reference skip[i] are no candidates"""
    Q, N = d2.shape
    out_d, out_i = np.full((Q, k), -1, dtype=np.int64), np.full((Q, k), -1, dtype=np.int32)
    for i in range(Q):
        if qflags is not None and qflags[i] != 0:
            continue
        ok = np.ones(N, dtype=bool) if rflags is None else np.asarray(rflags) == 0
        if skip is not None and skip[i] >= 0:
            ok[skip[i]] = False
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, d2[i, cand]))][:k]
        out_d[i, :order.size], out_i[i, :order.size] = d2[i, order], order
    return out_d, out_i


def nearest(q, r, k, skip=None):
    """the triples' form of locate_amd.nearest"""
    return topk(distances(q[0], r[0]), k, q[2], r[2], skip)


def canonical_u8(img, S):
    """uint8 [S, S, 3]: the centred square of side min(H, W) of img uint8 [H, W, 3], no flip, no jitter, resized to S"""
    H, W = img.shape[:2]
    side = min(H, W)
    return input_model.transform_u8(img, S, False, PLAIN, (1.0, 1.0, 1.0), (H - side) // 2, (W - side) // 2, side)


def bank_codes(store, S):
    """int8 [N, row_bytes]: the canonical views' bytes minus 128 in c, y, x order, zero pad"""
    codes = np.zeros((store.shape[0], row_bytes(S)), dtype=np.int8)
    for i, img in enumerate(store):
        codes[i, :3 * S * S] = (canonical_u8(img, S).transpose(2, 0, 1).astype(np.int64) - 128).reshape(-1)
    return codes


def rms(d2, S):
    return None if d2 < 0 else float(np.sqrt(d2 / (3.0 * S * S)) / 127.5)


def summary(values):
    v = np.asarray([x for x in values if x is not None], dtype=np.float64)
    return {"min": None, "median": None} if v.size == 0 else {"min": float(v.min()), "median": float(np.median(v))}


def baselines(bank, drawn, S):
    """(real_to_real, real_among_themselves) of the bank triple for the drawn indices"""
    sub = tuple(a[drawn] for a in bank)
    to_bank, _ = nearest(sub, bank, 1, skip=np.asarray(drawn))
    among, _ = nearest(sub, sub, 1, skip=np.arange(len(drawn)))
    return summary([rms(v, S) for v in to_bank[:, 0]]), summary([rms(v, S) for v in among[:, 0]])


def record(images, bank, k, S, real_to_real, real_among_themselves):
    """what NearestNeighbours.search returns for float32 images [Q, 3, S, S]"""
    q = encode(images)
    Q = len(q[1])
    d2, index = nearest(q, bank, k)
    own, _ = nearest(q, q, 1, skip=np.arange(Q))
    value = {"images": Q, "k": k, "index": index.tolist(), "d2": d2.tolist(), "rms": [rms(v, S) for v in d2[:, 0]]}
    value["generated_to_real"] = summary(value["rms"])
    value["generated_to_generated"] = summary([rms(v, S) for v in own[:, 0]])
    value["real_to_real"], value["real_among_themselves"] = dict(real_to_real), dict(real_among_themselves)
    value["nonfinite"] = int((q[2] != 0).sum())
    return value
