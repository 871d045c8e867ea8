"""Pillow's 8-bit resize (ImagingResample, modes "L" and "RGB") restated in numpy: the coefficient tables and both passes -- the reference of
mx_resize_coeffs / mx_resize_u8, and the case list their tests share.  Integer arithmetic on integer tables; only the tables need ``sin``, and
they take it from ``math`` (the C library's, as Pillow and the library do), one value at a time in Pillow's order of operations."""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3}                 # MX_RESIZE_* = PIL.Image.Resampling
SUPPORT = {"lanczos": 3.0, "bilinear": 1.0, "bicubic": 2.0}

# (in_h, in_w, out_h, out_w): what each is there for stands in tests/test_image_resize_gpu.py
CASES = ((37, 53, 16, 24), (9, 11, 40, 44), (64, 48, 64, 40), (128, 96, 17, 96), (7, 5, 7, 5), (400, 24, 8, 24), (20, 300, 24, 200), (33, 65, 32, 64))
# beyond those, one case per further path of the kernel; their inputs are not stored with Pillow's outputs but made by case_input(seed 200 + index):
#   6x700 -> 6x20: 211 horizontal lanczos taps, the tile's horizontal coefficients are read from memory (bilinear: 71 taps, from LDS);
#   400x700 -> 8x20: neither table fits LDS;  3x6000 -> 3x2: a row segment so long that the chunk shrinks to two rows and the tile to four bytes
EXTRA_CASES = ((6, 700, 6, 20), (400, 700, 8, 20), (3, 6000, 3, 2))
OVERSHOOT_CASE = (37, 53, 16, 24)                                     # the checkerboard and the stripe image, lanczos


def axis_pairs():
    """every (in, out) of the case list, both axes, in order of first appearance"""
    seen = []
    for ih, iw, oh, ow in CASES:
        for p in ((ih, oh), (iw, ow)):
            if p not in seen:
                seen.append(p)
    return seen


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {"lanczos": _lanczos, "bilinear": _bilinear, "bicubic": _bicubic}


def coeffs(n_in: int, n_out: int, resample: str):
    """(bounds int32 [out, 2] = (xmin, n), k int32 [out, ksize], ksize) of one axis: precompute_coeffs + normalize_coeffs_8bpc"""
    fn = _FILTER[resample]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    k = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = [fn((j + xmin - center + 0.5) * ss) for j in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for j in range(n):
            v = w[j] / ww if ww != 0.0 else w[j]
            k[xx, j] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return bounds, k, ksize


def pass_unclipped(x: np.ndarray, axis: int, n_out: int, resample: str) -> np.ndarray:
    """one pass along ``axis`` of a uint8 array before the clip: ((1 << 21) + sum) >> 22 as int64"""
    bounds, k, _ = coeffs(x.shape[axis], n_out, resample)
    x = np.moveaxis(x, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + x.shape[1:], dtype=np.int64)
    for xx in range(n_out):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        kk = k[xx, :n].astype(np.int64).reshape((n,) + (1,) * (x.ndim - 1))
        s = (1 << (PRECISION_BITS - 1)) + (x[xmin:xmin + n] * kk).sum(axis=0)
        assert s.size == 0 or (abs(s).max() < 2 ** 31)             # Pillow sums in int32
        out[xx] = s >> PRECISION_BITS
    return np.moveaxis(out, 0, axis)


def _pass(x: np.ndarray, axis: int, n_out: int, resample: str) -> np.ndarray:
    """one pass along ``axis`` of a uint8 array, into bytes"""
    return np.clip(pass_unclipped(x, axis, n_out, resample), 0, 255).astype(np.uint8)


def resize(x: np.ndarray, size, resample: str = "lanczos") -> np.ndarray:
    """x uint8 [B, H, W] or [B, H, W, C] -> [B, size[0], size[1](, C)]: horizontal pass into bytes, then vertical; a pass whose sizes agree is skipped"""
    assert x.dtype == np.uint8 and x.ndim in (3, 4)
    oh, ow = size
    if x.shape[2] != ow:
        x = _pass(x, 2, ow, resample)
    if x.shape[1] != oh:
        x = _pass(x, 1, oh, resample)
    return np.ascontiguousarray(x)


def case_input(ih: int, iw: int, seed: int) -> np.ndarray:
    """uint8 [2, ih, iw, 3]: two different images; noise over a gradient, with runs of 0 and 255 so that the filters overshoot into the clip"""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, size=(2, ih, iw, 3)).astype(np.uint8)
    x[0, : ih // 2, : iw // 3] = 255
    x[0, : ih // 2, iw // 3: 2 * iw // 3] = 0
    x[1, ih // 3:, ::2] = 0
    x[1, ih // 3:, 1::2] = 255
    return x


def overshoot_inputs():
    """uint8 [2, 37, 53, 3]: a 0 / 255 checkerboard and an image of 1-pixel stripes (0 on 255, 255 on 0)"""
    ih, iw = OVERSHOOT_CASE[:2]
    yy, xx = np.mgrid[0:ih, 0:iw]
    checker = (((yy // 3 + xx // 3) % 2) * 255).astype(np.uint8)
    stripe = np.where(xx % 7 == 3, 0, 255).astype(np.uint8)
    stripe[ih // 2:] = 255 - stripe[ih // 2:]
    stripe[5::9] = 255 - stripe[5::9]
    return np.stack([np.repeat(checker[..., None], 3, axis=2), np.repeat(stripe[..., None], 3, axis=2)])
