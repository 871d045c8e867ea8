"""Numpy restatements of the pieces of inpainting only the masked region: Pillow's GaussianBlur on mode "L" (three box passes per axis), the
bounding box of a mask, diffusers' crop rule (VaeImageProcessor.get_crop_region after the box) and its apply_overlay on bytes -- the references of
mx_blur_box_params / mx_gaussian_blur_u8 / mx_mask_bbox_u8 / mx_crop_region / mx_rgb8_overlay, and the case lists their tests share.  Integer
arithmetic throughout; only the blur's three box parameters are floating point, single precision in the order include/mxdenoise.h gives."""
import numpy as np

RADII = (0.3, 0.5, 1.0, 2.0, 3.3, 4.0, 8.0, 12.5, 33.0, 40.0)
SHAPES = ((37, 53), (64, 64), (5, 200), (129, 17))
KINDS = ("random", "binary", "rect")
LARGE = ((300, 520), (4.0, 33.0))                  # one larger plane at two radii: rows and columns across several thread segments
OVERLAY_SAMPLE = 1 << 16


def case_mask(h: int, w: int, kind: str, seed: int) -> np.ndarray:
    """uint8 [h, w]: uniform random bytes, 0 / 255 noise, or a 255 rectangle off the centre that touches no edge (where the planes are large enough)"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w), dtype=np.uint8) * 255).astype(np.uint8)
    m = np.zeros((h, w), dtype=np.uint8)
    m[h // 4:max(h // 4 + 1, (2 * h) // 3), w // 3:max(w // 3 + 1, (3 * w) // 4)] = 255
    return m


def blur_cases():
    """(key, h, w, kind, seed) of every stored input plane"""
    out = []
    for si, (h, w) in enumerate(SHAPES):
        for ki, kind in enumerate(KINDS):
            out.append((f"{h}x{w}_{kind}", h, w, kind, 300 + 10 * si + ki))
    out.append(("%dx%d_random" % LARGE[0], LARGE[0][0], LARGE[0][1], "random", 399))
    return out


def radii_of(key: str):
    return LARGE[1] if key == "%dx%d_random" % LARGE[0] else RADII


def box_params(radius: float):
    """(r, ww, fw) of one box pass of GaussianBlur(radius): every operation rounded to single precision"""
    f = np.float32
    radius = f(radius)
    sigma2 = radius * radius / f(3)
    big_l = np.sqrt(f(12) * sigma2 + f(1), dtype=np.float32)
    l = np.floor((big_l - f(1)) / f(2))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * sigma2) / (f(6) * (sigma2 - (l + f(1)) * (l + f(1))))
    fr = l + a
    assert fr.dtype == np.float32
    r = int(fr)
    ww = int(f(1 << 24) / (fr * f(2) + f(1)))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(x: np.ndarray, axis: int, r: int, ww: int, fw: int) -> np.ndarray:
    """one box pass along ``axis`` of a uint8 array, rounded to bytes"""
    x = np.moveaxis(x, axis, -1).astype(np.int64)
    n = x.shape[-1]
    # clamping the index is padding the line with its end pixels: xp[j] = x[clamp(j - r - 1)], and the window sum is a difference of prefix sums
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(r + 1, r + 1)], mode="edge")
    cs = np.concatenate([np.zeros(x.shape[:-1] + (1,), dtype=np.int64), np.cumsum(xp, axis=-1)], axis=-1)
    acc = cs[..., 2 * r + 2:2 * r + 2 + n] - cs[..., 1:1 + n]                  # x[clamp(i - r)] .. x[clamp(i + r)]
    far = xp[..., :n] + xp[..., 2 * r + 2:]
    out = (ww * acc + fw * far + (1 << 23)) >> 24
    assert out.min() >= 0 and out.max() <= 255
    return np.moveaxis(out.astype(np.uint8), -1, axis)


def gaussian_blur(x: np.ndarray, radius: float) -> np.ndarray:
    """uint8 [..., H, W] -> the same shape: ImageFilter.GaussianBlur(radius) of every plane"""
    if radius <= 0:
        return x.copy()
    r, ww, fw = box_params(radius)
    for axis in (-1, -2):
        for _ in range(3):
            x = box_pass(x, axis, r, ww, fw)
    return x


def bbox(mask: np.ndarray) -> np.ndarray:
    """uint8 [B, H, W] -> int32 [B, 4]: (x_min, y_min, x_max + 1, y_max + 1) over the non-zero bytes, (W, H, 0, 0) for an empty plane"""
    b, h, w = mask.shape
    out = np.zeros((b, 4), dtype=np.int32)
    for i in range(b):
        ys, xs = np.nonzero(mask[i])
        out[i] = (w, h, 0, 0) if ys.size == 0 else (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return out


def crop_region(box, mask_w: int, mask_h: int, width: int, height: int, pad: int):
    """diffusers' VaeImageProcessor.get_crop_region from its step 2 on, the box (x1, y1, x2, y2) being what its step 1 finds"""
    x1, y1, x2, y2 = (int(v) for v in box)
    x1, y1, x2, y2 = int(max(x1 - pad, 0)), int(max(y1 - pad, 0)), int(min(x2 + pad, mask_w)), int(min(y2 + pad, mask_h))
    ratio_crop_region = (x2 - x1) / (y2 - y1)
    ratio_processing = width / height
    if ratio_crop_region > ratio_processing:
        desired_height = (x2 - x1) / ratio_processing
        desired_height_diff = int(desired_height - (y2 - y1))
        y1 -= desired_height_diff // 2
        y2 += desired_height_diff - desired_height_diff // 2
        if y2 >= mask_h:
            diff = y2 - mask_h
            y2 -= diff
            y1 -= diff
        if y1 < 0:
            y2 -= y1
            y1 -= y1
        if y2 >= mask_h:
            y2 = mask_h
    else:
        desired_width = (y2 - y1) * ratio_processing
        desired_width_diff = int(desired_width - (x2 - x1))
        x1 -= desired_width_diff // 2
        x2 += desired_width_diff - desired_width_diff // 2
        if x2 >= mask_w:
            diff = x2 - mask_w
            x2 -= diff
            x1 -= diff
        if x1 < 0:
            x2 -= x1
            x1 -= x1
        if x2 >= mask_w:
            x2 = mask_w
    return x1, y1, x2, y2


def overlay_bytes(d: np.ndarray, o: np.ndarray, m: np.ndarray) -> np.ndarray:
    """apply_overlay per channel byte: d decoded, o original, m the soft mask (255 = repaint), broadcast against each other"""
    d, o, m = (np.asarray(v).astype(np.int64) for v in (d, o, m))
    big_a = 255 - m
    t = o * big_a + 128
    p = ((t >> 8) + t) >> 8
    c = np.minimum(255, (255 * p) // np.maximum(big_a, 1))
    u = c * (big_a * 128) + d * (255 * 128 - big_a * 128) + (0x80 << 7)
    out = (((u >> 8) + u) >> 8) >> 7
    return np.where(big_a == 0, d, out).astype(np.uint8)


def overlay(decoded: np.ndarray, original: np.ndarray, mask: np.ndarray, x: int, y: int) -> np.ndarray:
    """decoded [B, h, w, 3] blended into original [B, H, W, 3] at (x, y) under mask [B, H, W]; the original's bytes outside the box"""
    out = original.copy()
    h, w = decoded.shape[1:3]
    out[:, y:y + h, x:x + w] = overlay_bytes(decoded, original[:, y:y + h, x:x + w], mask[:, y:y + h, x:x + w, None])
    return out


def triple_image():
    """every (d, o, m) once as a 4096 x 4096 problem: decoded, original uint8 [1, 4096, 4096, 3] and mask [1, 4096, 4096].  Pixel i has m = i >> 16,
    o = (i >> 8) & 255, d = i & 255 in channel 0; channels 1 and 2 carry other data (rotations of the same bytes), so a channel mix-up shows."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(1, 4096, 4096)
    m = (i >> 16).astype(np.uint8)
    o0, d0 = ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)
    orig = np.stack([o0, d0, (o0 + np.uint8(101)).astype(np.uint8)], axis=-1)
    dec = np.stack([d0, (o0 ^ np.uint8(0x5a)).astype(np.uint8), (d0 * np.uint8(7)).astype(np.uint8)], axis=-1)
    return dec, orig, m


def sample_triples(n: int = OVERLAY_SAMPLE, seed: int = 77) -> np.ndarray:
    """uint8 [n, 3] random (d, o, m), the ends of the mask over-represented"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    t[: n // 16, 2] = rng.choice(np.array([0, 1, 2, 127, 128, 253, 254, 255], dtype=np.uint8), n // 16)
    return t
