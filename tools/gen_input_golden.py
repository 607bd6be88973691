"""Writes tests/golden/g22_input_pipeline.npz: synthetic uint8 sources, transform records and what Pillow itself makes of them
(transpose(FLIP_LEFT_RIGHT), ImageEnhance.Brightness / Contrast / Color in the record's order, crop, resize(BILINEAR)) - the
wiring of torchvision's PIL backend for RandomHorizontalFlip, ColorJitter(hue = 0), RandomResizedCrop(ratio = (1, 1)).

    python tools/gen_input_golden.py [--check]       (needs Pillow; --check compares with the committed file instead of writing)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "g22_input_pipeline.npz")
HUE = 3


def sources(H, W, n_smooth, n_noise, seed):
    rng = np.random.default_rng(seed)
    out = []
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for k in range(n_smooth):
        ph = rng.uniform(0, 2 * np.pi, size=(3, 3))
        fr = rng.uniform(0.02, 0.15, size=(3, 2))
        amp = (60.0, 110.0, 127.0)[k % 3]                  # the widest one reaches 0 and 255, so the 1.2 factors clip
        img = np.stack([127.5 + amp * np.sin(fr[c, 0] * xx + ph[c, 0]) * np.cos(fr[c, 1] * yy + ph[c, 1])
                        + 20.0 * np.sin(0.9 * xx + 1.3 * yy + ph[c, 2]) for c in range(3)], axis=2)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    for _ in range(n_noise):
        out.append(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    return np.stack(out)


def records():
    """(source set, source index, S, flip, order, (brightness, contrast, saturation), top, left, side); order is padded with HUE.
    Large: 157 x 128 at S = 64 (sources 0-2 smooth, 3-5 noise); small: 78 x 64 at S = 32 (0 smooth, 1 noise)."""
    H, W, h, w = 157, 128, 78, 64
    orders = [(1, 0, 2, 3), (0, 1, 2, 3), (0, 2, 1, 3), (3, 0, 2, 1), (2, 1, 3, 0), (1, 3, 2, 0), (2, 0, 3, 1), (3, 2, 1, 0)]
    lo, hi = 0.8, 1.2
    recs = [
        ("large", 0, 64, 0, orders[0], (hi, hi, hi), 0, 0, 128),              # side = min(H, W), top-left corner
        ("large", 1, 64, 1, orders[1], (lo, lo, lo), 29, 0, 128),             # bottom edge
        ("large", 2, 64, 0, orders[2], (hi, lo, hi), 0, 0, 64),               # side = S: identity resize, corner
        ("large", 3, 64, 1, orders[3], (lo, hi, lo), 93, 64, 64),             # bottom-right corner
        ("large", 4, 64, 0, orders[4], (hi, hi, lo), 0, 17, 111),             # top-right corner
        ("large", 5, 64, 1, orders[5], (lo, lo, hi), 46, 0, 111),             # bottom-left corner
        ("large", 0, 64, 1, orders[6], (1.2, 0.8, 1.2), 12, 5, 123),
        ("large", 1, 64, 0, orders[7], (0.8, 1.2, 0.8), 30, 1, 127),
        ("large", 2, 64, 1, orders[0], (1.0371, 0.9122, 1.1693), 7, 9, 97),
        ("large", 3, 64, 0, orders[1], (0.8514, 1.1907, 0.9336), 20, 30, 65),
        ("large", 4, 64, 1, orders[2], (1.1999, 1.0001, 0.8001), 33, 3, 124),
        ("large", 5, 64, 0, orders[3], (0.9, 1.1, 1.0), 50, 20, 100),
        ("large", 0, 64, 0, orders[4], (1.2, 1.2, 1.2), 3, 2, 126),
        ("large", 2, 64, 1, orders[5], (1.2, 1.2, 1.2), 10, 0, 128),
        ("large", 1, 64, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 14, 0, 128),       # plain chain
        ("large", 3, 64, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 31, 2, 125),
        ("large", 4, 64, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 0, 0, 64),
        ("large", 5, 64, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 44, 15, 113),
        ("small", 0, 32, 0, orders[6], (hi, lo, hi), 0, 0, 64),
        ("small", 1, 32, 1, orders[7], (lo, hi, lo), 14, 0, 64),
        ("small", 0, 32, 1, orders[0], (1.13, 0.87, 1.2), 46, 32, 32),        # side = S in the bottom-right corner
        ("small", 1, 32, 0, orders[1], (0.8, 1.2, 1.05), 9, 3, 61),
        ("small", 0, 32, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 23, 0, 55),
        ("small", 1, 32, 0, (3, 3, 3, 3), (1.0, 1.0, 1.0), 0, 9, 55),
    ]
    for r in recs:
        hh, ww = (H, W) if r[0] == "large" else (h, w)
        assert 0 <= r[6] and r[6] + r[8] <= hh and 0 <= r[7] and r[7] + r[8] <= ww, r
    return recs


def pillow_transform(src, S, flip, order, factors, top, left, side):
    from PIL import Image, ImageEnhance
    img = Image.fromarray(src, "RGB")
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    enhancers = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    for op in order:
        if op != HUE:
            img = enhancers[op](img).enhance(float(factors[op]))
    img = img.crop((left, top, left + side, top + side))
    return np.asarray(img.resize((S, S), Image.BILINEAR))


def generate():
    import PIL
    large = sources(157, 128, 3, 3, seed=22)
    small = sources(78, 64, 1, 1, seed=23)
    recs = records()
    out = {"src_large": large, "src_small": small, "pillow_version": np.array(PIL.__version__)}
    for name in ("large", "small"):
        rs = [r for r in recs if r[0] == name]
        src = large if name == "large" else small
        out["rec_%s_source" % name] = np.array([r[1] for r in rs], dtype=np.int32)
        out["rec_%s_size" % name] = np.array([r[2] for r in rs], dtype=np.int32)
        out["rec_%s_flip" % name] = np.array([r[3] for r in rs], dtype=np.int32)
        out["rec_%s_order" % name] = np.array([r[4] for r in rs], dtype=np.int32)
        out["rec_%s_factors" % name] = np.array([r[5] for r in rs], dtype=np.float64)
        out["rec_%s_crop" % name] = np.array([r[6:9] for r in rs], dtype=np.int32)          # top, left, side
        out["out_%s" % name] = np.stack([pillow_transform(src[r[1]], r[2], r[3], r[4], r[5], r[6], r[7], r[8]) for r in rs])
    return out


def main():
    try:
        import PIL  # noqa: F401
    except ImportError:
        sys.exit("tools/gen_input_golden.py needs Pillow: the fixture holds Pillow's own outputs")
    out = generate()
    if "--check" in sys.argv:
        z = np.load(PATH, allow_pickle=False)
        bad = [k for k in out if k != "pillow_version" and not np.array_equal(out[k], z[k])]
        print("Pillow %s against the fixture's %s: %s" % (out["pillow_version"], z["pillow_version"], bad or "equal"))
        sys.exit(1 if bad else 0)
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
