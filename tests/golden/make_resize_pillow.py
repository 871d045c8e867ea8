"""Writes resize_pillow.npz next to this file: the inputs of tests/resize_ref.py's case list and what Pillow's Image.resize makes of them, so
that a machine without Pillow still checks against Pillow's bytes.  Needs Pillow; run from the repository root:  python tests/golden/make_resize_pillow.py

Keys: ``in_<case>`` uint8 [2, ih, iw, 3] (the one-channel input of a case is channel 0 of it), ``out_<case>_<filter>_c<C>`` Pillow's result
[2, oh, ow(, 3)], ``out_x<case>_<filter>_c<C>`` the same for resize_ref.EXTRA_CASES (inputs: case_input(seed 200 + case)), ``in_overshoot`` / ``out_overshoot_lanczos_c<C>`` for the checkerboard and the stripe image, ``pillow_version``."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_ref as R  # noqa: E402

RESAMPLE = {"lanczos": Image.Resampling.LANCZOS, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}


def pillow_resize(x: np.ndarray, size, resample: str) -> np.ndarray:
    """x uint8 [B, H, W] (mode "L") or [B, H, W, 3] (mode "RGB") through Image.resize((width, height), resample)"""
    return np.stack([np.asarray(Image.fromarray(im).resize((size[1], size[0]), resample=RESAMPLE[resample])) for im in x])


def main() -> None:
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (ih, iw, oh, ow) in enumerate(R.CASES):
        x = R.case_input(ih, iw, seed=100 + i)
        out[f"in_{i}"] = x
        for f in R.FILTERS:
            out[f"out_{i}_{f}_c3"] = pillow_resize(x, (oh, ow), f)
            out[f"out_{i}_{f}_c1"] = pillow_resize(np.ascontiguousarray(x[..., 0]), (oh, ow), f)
    for i, (ih, iw, oh, ow) in enumerate(R.EXTRA_CASES):
        x = R.case_input(ih, iw, seed=200 + i)
        for f in R.FILTERS:
            out[f"out_x{i}_{f}_c3"] = pillow_resize(x, (oh, ow), f)
            out[f"out_x{i}_{f}_c1"] = pillow_resize(np.ascontiguousarray(x[..., 0]), (oh, ow), f)
    x = R.overshoot_inputs()
    oh, ow = R.OVERSHOOT_CASE[2:]
    out["in_overshoot"] = x
    out["out_overshoot_lanczos_c3"] = pillow_resize(x, (oh, ow), "lanczos")
    out["out_overshoot_lanczos_c1"] = pillow_resize(np.ascontiguousarray(x[..., 0]), (oh, ow), "lanczos")
    path = os.path.join(HERE, "resize_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
