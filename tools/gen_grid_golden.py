"""Writes tests/golden/g23_sample_grid.npz: image batches and the picture the reference's monitoring chain makes of them
(main.py:203-209: torchvision's make_grid(padding, normalize=True), then matplotlib's imsave).

torchvision is not needed: make_grid's documented steps are spelled in torch CPU ops below (clone, clamp to the range, subtract
the lower bound, divide by max(high - low, 1e-5) - min and max taken over the whole batch as Python floats - then tile into a
pad_value canvas).  The PNG is written by the real matplotlib.pyplot.imsave and decoded with Pillow.  Before anything is
written, the numpy model of tests/helpers/grid_model.py must equal both records on every case.

    python tools/gen_grid_golden.py [--check]       (needs matplotlib and Pillow; --check compares with the committed file)
"""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "g23_sample_grid.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import grid_model as M  # noqa: E402


def make_grid_cpu(x, nrow, padding, value_range, pad_value=0.0):
    t = x.clone()
    if value_range is not None:
        low, high = value_range
    else:
        low, high = float(t.min()), float(t.max())
    t.clamp_(min=low, max=high)
    t.sub_(low).div_(max(high - low, 1e-5))
    n, _, S, _ = t.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    h, w = S + padding, S + padding
    grid = t.new_full((3, h * ymaps + padding, w * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for xx in range(xmaps):
            if k >= n:
                break
            grid.narrow(1, y * h + padding, h - padding).narrow(2, xx * w + padding, w - padding).copy_(t[k])
            k += 1
    return grid


def imsave_bytes(grid):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, arr=np.transpose(grid.numpy(), (1, 2, 0)), format="png")
    buf.seek(0)
    im = Image.open(buf)
    assert im.mode == "RGBA", im.mode
    return np.asarray(im).copy()


def cases():
    """(name, x, nrow, padding, value_range or None, keep the fp32 grid)"""
    g = torch.Generator().manual_seed(23)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return [
        ("tanh13", torch.tanh(1.5 * r(13, 3, 32, 32)), 8, 8, None, False),           # the sampler's form, ragged last row
        ("randn16", r(16, 3, 32, 32).clamp(-1, 1), 8, 2, None, False),               # plot_images' form (libs/utils.py:75-77)
        ("tiny5", r(5, 3, 16, 16) * 1e-7, 8, 2, None, True),                         # a range far below the 1e-5 floor
        ("const4", torch.full((4, 3, 16, 16), 0.25), 8, 2, None, True),              # hi == lo: the floor gives all zeros
        ("nrow5", torch.tanh(r(7, 3, 16, 16)), 5, 3, None, True),
        ("range6", r(6, 3, 16, 16), 8, 2, (-1.0, 1.0), True),                        # data beyond the range: the clamp works
    ]


def build():
    import matplotlib
    import PIL
    out = {"names": np.array([c[0] for c in cases()]), "matplotlib_version": np.array(matplotlib.__version__),
           "pillow_version": np.array(PIL.__version__), "torch_version": np.array(torch.__version__)}
    for name, x, nrow, padding, vr, keep in cases():
        grid = make_grid_cpu(x, nrow, padding, vr)
        rgba = imsave_bytes(grid)
        want_grid, want_rgba = M.model(x.numpy(), nrow, padding, vr)
        assert grid.numpy().shape == want_grid.shape and np.array_equal(grid.numpy(), want_grid), name
        assert rgba.shape == want_rgba.shape and np.array_equal(rgba, want_rgba), name
        if vr is not None:
            assert float(x.min()) < vr[0] and float(x.max()) > vr[1], name
        out["x_" + name] = x.numpy()
        out["rgba_" + name] = rgba
        out["args_" + name] = np.array([nrow, padding], dtype=np.int64)
        out["range_" + name] = np.array(vr if vr is not None else [], dtype=np.float64)
        if keep:
            out["grid_" + name] = grid.numpy()
    return out


if __name__ == "__main__":
    new = build()
    if "--check" in sys.argv:
        old = np.load(PATH, allow_pickle=False)
        skip = {"matplotlib_version", "pillow_version", "torch_version"}
        assert sorted(old.files) == sorted(new), "different entries"
        for k in new:
            assert k in skip or np.array_equal(old[k], new[k]), k
        print("matches", PATH)
    else:
        np.savez_compressed(PATH, **new)
        print(PATH, os.path.getsize(PATH), "bytes")
