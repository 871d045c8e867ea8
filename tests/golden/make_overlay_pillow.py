"""Writes overlay_pillow.npz next to this file: the mask planes of tests/overlay_ref.py's case list with what Pillow's ImageFilter.GaussianBlur makes
of them, and what the literal Pillow sequence of diffusers' apply_overlay makes of a random sample of (decoded, original, mask) bytes, so that a
machine without Pillow still checks against Pillow's bytes.  Needs Pillow; run from the repository root:  python tests/golden/make_overlay_pillow.py

Keys: ``in_<h>x<w>_<kind>`` uint8 [h, w] for the small shapes (the larger plane is overlay_ref.case_mask of its seed and is not stored),
``blur_<h>x<w>_<kind>_r<radius>`` Pillow's blurred plane, ``overlay_out`` uint8 [65536]: the overlay of overlay_ref.sample_triples() (channel 0 of a
65536 x 1 image whose other channels carry other data), ``pillow_version``."""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageFilter, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import overlay_ref as O  # noqa: E402


def pillow_blur(m: np.ndarray, radius: float) -> np.ndarray:
    return np.asarray(Image.fromarray(m, "L").filter(ImageFilter.GaussianBlur(radius)))


def pillow_overlay(decoded: np.ndarray, original: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """diffusers' VaeImageProcessor.apply_overlay without crop_coords, call for call: decoded, original uint8 [H, W, 3], mask uint8 [H, W] -> [H, W, 3]"""
    init_image, image, mask = Image.fromarray(original, "RGB"), Image.fromarray(decoded, "RGB"), Image.fromarray(mask, "L")
    init_image_masked = Image.new("RGBa", (init_image.width, init_image.height))
    init_image_masked.paste(init_image.convert("RGBA").convert("RGBa"), mask=ImageOps.invert(mask.convert("L")))
    init_image_masked = init_image_masked.convert("RGBA")
    image = image.convert("RGBA")
    image.alpha_composite(init_image_masked)
    return np.asarray(image.convert("RGB"))


def sample_images():
    """the sample triples as a 65536 x 1 image: (decoded, original, mask) with the triple in channel 0"""
    t = O.sample_triples()
    d, o, m = t[:, 0], t[:, 1], t[:, 2]
    dec = np.stack([d, o ^ np.uint8(0x33), m], axis=-1)[:, None, :]
    orig = np.stack([o, m, d], axis=-1)[:, None, :]
    return np.ascontiguousarray(dec), np.ascontiguousarray(orig), np.ascontiguousarray(m[:, None])


def main() -> None:
    out = {"pillow_version": np.array(PIL.__version__)}
    for key, h, w, kind, seed in O.blur_cases():
        m = O.case_mask(h, w, kind, seed)
        if (h, w) != O.LARGE[0]:
            out[f"in_{key}"] = m
        for radius in O.radii_of(key):
            out[f"blur_{key}_r{radius:g}"] = pillow_blur(m, radius)
    dec, orig, m = sample_images()
    out["overlay_out"] = np.ascontiguousarray(pillow_overlay(dec, orig, m)[:, 0, 0])
    path = os.path.join(HERE, "overlay_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
