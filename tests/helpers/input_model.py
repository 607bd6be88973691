"""Integer model (numpy) of the input pipeline's arithmetic: what Pillow computes for
transpose(FLIP_LEFT_RIGHT) -> ImageEnhance.{Brightness, Contrast, Color} in a given order -> crop -> resize(BILINEAR) on an
RGB uint8 image, followed by ToTensor / Normalize(0.5, 0.5).  It is the yardstick of tests/test_input_golden.py (against real
Pillow outputs in tests/golden/g22_input_pipeline.npz) and of the GPU tests where no Pillow output is stored."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
PRECISION_BITS = 22


def luma(img):
    """Pillow's RGB -> L: (19595 R + 38470 G + 7471 B + 32768) >> 16"""
    p = img.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(degenerate, img, factor):
    """Image.blend(degenerate, img, factor): fp32, separate multiply and add, clip, truncate"""
    d = degenerate.astype(np.float32)
    p = img.astype(np.float32)
    t = d + np.float32(factor) * (p - d)            # numpy rounds each operation to fp32: no fused multiply-add
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def contrast_mean(img):
    n = img.shape[0] * img.shape[1]
    return int((2 * int(luma(img).astype(np.int64).sum()) + n) // (2 * n))


def jitter(img, order, factors):
    """order: sequence of op codes; factors: (brightness, contrast, saturation).  Every op quantises to uint8."""
    for op in order:
        if op == BRIGHTNESS:
            img = blend(np.zeros_like(img), img, factors[0])
        elif op == CONTRAST:
            img = blend(np.full_like(img, contrast_mean(img)), img, factors[1])
        elif op == SATURATION:
            img = blend(np.repeat(luma(img)[..., None], 3, axis=2), img, factors[2])
    return img


def resize_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter: [(first tap, int32 weights)] per output"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    out = []
    for i in range(out_size):
        c = (i + 0.5) * scale
        x0 = max(int(c - fs + 0.5), 0)
        x1 = min(int(c + fs + 0.5), in_size)
        w = np.array([max(0.0, 1.0 - abs((x - c + 0.5) / fs)) for x in range(x0, x1)], dtype=np.float64)
        w = w / w.sum()
        out.append((x0, np.floor(0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)))
    return out


def _resize_axis0(img, out_size):
    res = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    for i, (x0, k) in enumerate(resize_coeffs(img.shape[0], out_size)):
        acc = np.tensordot(k, img[x0:x0 + len(k)].astype(np.int64), axes=(0, 0))
        res[i] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return res


def resize_bilinear(img, S):
    """Image.resize((S, S), BILINEAR): horizontal pass, uint8, vertical pass"""
    h = _resize_axis0(img.transpose(1, 0, 2), S).transpose(1, 0, 2)
    return _resize_axis0(h, S)


def transform_u8(src, S, flip, order, factors, top, left, side):
    img = src[:, ::-1] if flip else src
    img = jitter(np.ascontiguousarray(img), order, factors)
    return resize_bilinear(img[top:top + side, left:left + side], S)


def to_float(u8):
    """ToTensor + Normalize(0.5, 0.5): HWC uint8 -> CHW fp32"""
    x = u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((x - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))
