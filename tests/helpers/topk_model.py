"""The definition of top-k training of the generator (Sinha et al. 2020, "Top-k Training of GANs: Improving GAN Performance by
Throwing Away Bad Samples") as this project runs it, in numpy: the order of the logits, the G-step's loss over the k that stand first,
the record and the ring, the schedule of k.  csrc/topk.hip and locate_amd/topk.py (TopK) are held to it with ==, bytes included.

Raw logits f = D(G(z)); the hinge is relu(1 - f).  `before(j, i)`: f_j is a NaN and f_i is not; or both are NaNs and j < i; or neither
is and f_j > f_i; or neither is, f_j == f_i (-0 == +0) and j < i.  rank_i = #{j : before(j, i)}; element i is kept iff rank_i < k_used,
k_used = k if 1 <= k <= B else B.

The record: 16 32-bit words, FIELDS names words 0 .. 7 (threshold and the two means are fp32 bit patterns, k an int32, the rest unsigned
counters mod 2^32), words 8 .. 15 are zero.  A ring row: 8 words {launch ordinal (1-based), k_used, active, threshold, mean_all,
mean_kept, 1 if the logits held a NaN or an Inf else 0, 0} at slot (ordinal - 1) % capacity.

Every fp32 operation below is one numpy float32 operation (rounded once); the float64 sums run in the order of the kernel's block
reduction (lecam_model.block_sum): thread t holds elements t, t + 256, ...; an element that is not kept adds nothing."""
import math

import numpy as np

from lecam_model import block_sum, clamp0

STATE_WORDS = 16
RING_WORDS = 8
MAX_BATCH = 4096
FIELDS = ("k", "launches", "nonfinite", "k_used", "active", "threshold", "mean_all", "mean_kept")
_FLOAT_WORDS = (5, 6, 7)

f32 = np.float32
f64 = np.float64


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


def _float(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def new_state(k=0):
    state = np.zeros(STATE_WORDS, np.uint32)
    state[0] = np.array([k], np.int32).view(np.uint32)[0]
    return state


def new_ring(capacity):
    return np.zeros((int(capacity), RING_WORDS), np.uint32)


def fields(state):
    out = {name: int(state[k]) for k, name in enumerate(FIELDS)}
    out["k"] = int(np.array([state[0]], np.uint32).view(np.int32)[0])
    for k in _FLOAT_WORDS:
        out[FIELDS[k]] = _float(state[k])
    return out


def k_used(k, B):
    return int(k) if 1 <= int(k) <= B else B


# ---- the order -----------------------------------------------------------------------------------------------------------------------------
def before(f, j, i):
    """whether element j stands before element i"""
    fj, fi = f[j], f[i]
    nj, ni = bool(np.isnan(fj)), bool(np.isnan(fi))
    if nj or ni:
        return (nj and not ni) or (nj and ni and j < i)
    return bool(fj > fi) or (bool(fj == fi) and j < i)


def ranks(f):
    """rank_i = #{j : before(j, i)}, the definition as it stands, pair by pair, vectorised over j"""
    f = np.asarray(f, np.float32).reshape(-1)
    B = len(f)
    nan = np.isnan(f)
    index = np.arange(B)
    out = np.zeros(B, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(B):
            if nan[i]:
                first = nan & (index < i)
            else:
                first = nan | (~nan & ((f > f[i]) | ((f == f[i]) & (index < i))))
            out[i] = int(first.sum())
    return out


def kept(f, k):
    f = np.asarray(f, np.float32).reshape(-1)
    return ranks(f) < k_used(k, len(f))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def plain_g_loss(f):
    """locate_g_loss: (loss, g_fake)"""
    f = np.asarray(f, np.float32).reshape(-1)
    B = len(f)
    with np.errstate(all="ignore"):
        loss = f32(block_sum(clamp0(f32(1) - f).astype(np.float64)) / B)
        g = np.where((f32(1) - f) >= 0, -(f32(1) / f32(B)), f32(0)).astype(np.float32)
    return loss, g


def g_loss(f, state, ring, rank=None):
    """locate_g_loss_topk, in place on `state` (uint32 [16]) and `ring` (uint32 [capacity, 8]):
    (losses[2] = {loss_topk, loss_all}, g_fake).  rank: ranks(f) where the caller has them already (they do not depend on k)."""
    f = np.asarray(f, np.float32).reshape(-1)
    B = len(f)
    assert 1 <= B <= MAX_BATCH
    ku = k_used(fields(state)["k"], B)
    rank = ranks(f) if rank is None else np.asarray(rank)
    keep = rank < ku
    with np.errstate(all="ignore"):
        hinge = clamp0(f32(1) - f).astype(np.float64)
        passes = (f32(1) - f) >= 0
        zero = np.zeros(B, np.float64)
        loss_topk = f32(block_sum(np.where(keep, hinge, zero)) / ku)
        loss_all = f32(block_sum(hinge) / B)
        mean_all = f32(block_sum(f.astype(np.float64)) / B)
        mean_kept = f32(block_sum(np.where(keep, f.astype(np.float64), zero)) / ku)
        g = np.where(keep & passes, -(f32(1) / f32(ku)), f32(0)).astype(np.float32)
    active = int((keep & passes).sum())
    bad = int(not np.isfinite(f).all())
    threshold = _bits(f[int(np.nonzero(rank == ku - 1)[0][0])])
    launches = int(state[1])
    ordinal = (launches + 1) & 0xFFFFFFFF
    ring[launches % len(ring)] = (ordinal, ku, active, threshold, _bits(mean_all), _bits(mean_kept), bad, 0)
    state[1] = ordinal
    state[2] = (int(state[2]) + bad) & 0xFFFFFFFF
    state[3], state[4], state[5] = ku, active, threshold
    state[6], state[7] = _bits(mean_all), _bits(mean_kept)
    return np.array([loss_topk, loss_all], np.float32), g


def curve(ring, first, last):
    """ring rows first .. last - 1 (counted over the whole run) as TopK.curve() returns them"""
    out = []
    for n in range(first, last):
        row = ring[n % len(ring)]
        out.append({"launch": int(row[0]), "k": int(row[1]), "active": int(row[2]), "threshold": float(_float(row[3])),
                    "mean_all": float(_float(row[4])), "mean_kept": float(_float(row[5])), "nonfinite": int(row[6])})
    return out


# ---- the schedule --------------------------------------------------------------------------------------------------------------------------
def topk_k(batch, gamma, floor, periods):
    """k after `periods` annealing periods: max(k_min, min(B, int(floor(B * gamma ** periods + 0.5)))), k_min = max(1, ceil(floor * B)),
    in float64"""
    B = int(batch)
    k_min = max(1, int(math.ceil(float(floor) * B)))
    return max(k_min, min(B, int(math.floor(B * float(gamma) ** int(periods) + 0.5))))
