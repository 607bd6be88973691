"""The sample grid on the host, in numpy: torchvision's make_grid(normalize=True) followed by matplotlib's imsave, restated from
their documented behaviour as single fp32 operations.  tools/gen_grid_golden.py asserts that this model equals both a torch-CPU
spelling of make_grid and the bytes the real imsave writes before it records them (tests/golden/g23_sample_grid.npz), so the
model is a yardstick of its own for sizes that are too big to store."""
import numpy as np


def geometry(n, S, nrow=8, padding=2):
    xm = min(nrow, n)
    ym = -(-n // xm)
    return xm, ym, (S + padding) * ym + padding, (S + padding) * xm + padding


def model(x, nrow=8, padding=2, value_range=None, pad_value=0.0):
    """x: float32 [n, 3, S, S].  Returns (grid fp32 [3, GH, GW], RGBA bytes [GH, GW, 4])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if value_range is None:
        lo, hi = x.min(), x.max()
        d = np.float32(max(float(hi) - float(lo), 1e-5))
    else:
        lo, hi = np.float32(value_range[0]), np.float32(value_range[1])
        d = np.float32(max(float(value_range[1]) - float(value_range[0]), 1e-5))      # from the caller's doubles, as torchvision does
        x = np.minimum(np.maximum(x, lo), hi)
    v = (x - lo) / d
    assert v.dtype == np.float32
    n, _, S, _ = x.shape
    xm, ym, GH, GW = geometry(n, S, nrow, padding)
    g = np.full((3, GH, GW), np.float32(pad_value), np.float32)
    for k in range(n):
        r, c = divmod(k, xm)
        g[:, r * (S + padding) + padding:][:, :S, c * (S + padding) + padding:][:, :, :S] = v[k]
    rgba = np.full((GH, GW, 4), 255, np.uint8)
    rgba[:, :, :3] = (g * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
    return g, rgba
