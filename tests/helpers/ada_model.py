"""The definition of adaptive discriminator augmentation (Karras et al. 2020) as this project runs it, in numpy: the gate that turns
uniforms into the per-image op mask of a DiffAugment parameter row, the observer with its state record and ring, and the controller's
step constant.  csrc/ada.hip and locate_amd/augment.py (AdaptiveDiffAugment) are held to it with ==, bytes included.

The state record: 16 32-bit words, FIELDS names words 0 .. 9 (p and r are fp32 bit patterns, sum is an int32, the rest unsigned),
words 10 .. 15 are zero.  A ring row: 4 words {iteration, r, p, logits counted in the closed window}."""
import numpy as np

STATE_WORDS = 16
RING_WORDS = 4
ROW_WORDS = 12
GATE_WORD = 9          # raw row: uniforms of op 0, 1, 2 in words 9, 10, 11; gated row: the mask in word 9, zeros behind it
FIELDS = ("p", "r", "sum", "counted", "seen", "closed", "ups", "downs", "nan", "rows")
GATE_CAP = np.nextafter(np.float32(1.0), np.float32(0.0))          # the largest fp32 below 1

f32 = np.float32


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


def _float(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def new_state(p=0.0):
    state = np.zeros(STATE_WORDS, np.uint32)
    state[0] = _bits(p)
    return state


def new_ring(capacity):
    return np.zeros((int(capacity), RING_WORDS), np.uint32)


def fields(state):
    """the record by name: p and r as fp32, sum as a signed integer"""
    out = {name: int(state[k]) for k, name in enumerate(FIELDS)}
    out["p"], out["r"] = _float(state[0]), _float(state[1])
    out["sum"] = int(np.array([state[2]], np.uint32).view(np.int32)[0])
    return out


def step_constant(batch, interval, kimg):
    """p's move per closed window: batch * interval / (kimg * 1000) in float64, rounded once to fp32 (kimg = inf: 0)"""
    return f32(float(batch) * float(interval) / (float(kimg) * 1000.0))


def gate_uniforms(r64):
    """float64 uniforms in [0, 1) -> fp32 below 1 (rounding alone can reach 1.0)"""
    return np.minimum(np.asarray(r64, np.float64).astype(np.float32), GATE_CAP)


def gate(raw, p, policy):
    """raw float32 [n, 12] -> the gated rows.  Op k of the policy is applied iff g_k < p, strictly."""
    raw = np.ascontiguousarray(raw, np.float32)
    out = raw.copy()
    g = raw[:, GATE_WORD:GATE_WORD + 3]
    mask = np.zeros(len(raw), np.int64)
    for k in range(3):
        if policy >> k & 1:
            mask |= np.where(g[:, k] < f32(p), 0, 1 << k)
    out[:, GATE_WORD] = mask.astype(np.float32)
    out[:, GATE_WORD + 1:] = 0.0
    return out


def observe(logits, iteration, state, ring, interval, target, step, p_max):
    """One observation, in place on `state` (uint32 [16]) and `ring` (uint32 [capacity, 4])."""
    x = np.asarray(logits, np.float32).reshape(-1)
    s = fields(state)
    nans = int(np.isnan(x).sum())
    total = s["sum"] + int((x > 0).sum()) - int((x < 0).sum())
    counted = s["counted"] + len(x) - nans
    seen = s["seen"] + 1
    p, r = f32(s["p"]), f32(s["r"])
    closed, ups, downs, rows = s["closed"], s["ups"], s["downs"], s["rows"]
    target, step, p_max = f32(target), f32(step), f32(p_max)
    if seen >= interval:
        if counted > 0:
            r = f32(np.float64(total) / np.float64(counted))
            if r > target:
                p = np.minimum(np.maximum(f32(p + step), f32(0)), p_max)
                ups += 1
            elif r < target:
                p = np.minimum(np.maximum(f32(p - step), f32(0)), p_max)
                downs += 1
        ring[rows % len(ring)] = (np.uint32(iteration & 0xFFFFFFFF), _bits(r), _bits(p), np.uint32(counted))
        rows = (rows + 1) & 0xFFFFFFFF
        closed = (closed + 1) & 0xFFFFFFFF
        total = counted = seen = 0
    state[0], state[1] = _bits(p), _bits(r)
    state[2] = np.array([total], np.int32).view(np.uint32)[0]
    state[3:10] = (counted, seen, closed, ups, downs, (s["nan"] + nans) & 0xFFFFFFFF, rows)
    return state


def curve(ring, first, last):
    """ring rows first .. last - 1 (counted over the whole run) as [{"iteration", "r_t", "p"}]"""
    out = []
    for k in range(first, last):
        row = ring[k % len(ring)]
        out.append({"iteration": int(np.array([row[0]], np.uint32).view(np.int32)[0]), "r_t": float(_float(row[1])), "p": float(_float(row[2]))})
    return out
