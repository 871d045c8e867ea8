"""Host-side checks of inpainting only the masked region: the five entries of csrc/inpaint_overlay.hip and csrc/inpaint_region.cpp are declared,
exported and bound; each refuses bad arguments before any launch; the library's box parameters and crop rule equal the restatements
(tests/overlay_ref.py); the restatements equal Pillow's bytes, stored (tests/golden/overlay_pillow.npz) and live, the overlay over all 2^24 byte
triples; the wrappers refuse CPU tensors; InpaintState constructs as before.  No GPU: the library loads without a device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import overlay_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mx_blur_box_params", "mx_gaussian_blur_u8", "mx_mask_bbox_u8", "mx_crop_region", "mx_rgb8_overlay")
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal
FAR = 1 << 30                # buffers this far apart do not overlap at the sizes used here


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "overlay_pillow.npz"))


def test_entries_are_declared_exported_and_bound():
    from sduss_amd import lib, ops
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in lib.SYMBOLS and hasattr(l, name)
        assert getattr(l, name).argtypes == lib.SYMBOLS[name][1]
    for name in ("gaussian_blur_u8", "mask_bbox", "crop_region", "rgb8_overlay", "blur_box_params"):
        assert callable(getattr(ops, name))
    mk = open(os.path.join(ROOT, "sduss_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS_HIP = .*\binpaint_overlay\.hip\b", mk, re.M) and re.search(r"^SRCS_CPP = .*\binpaint_region\.cpp\b", mk, re.M)
    assert "-ffast-math" not in mk
    assert l.mx_version() == 1


def _params(radius):
    from sduss_amd import lib
    r, ww, fw = C.c_int(-7), C.c_uint32(7), C.c_uint32(7)
    status = lib.load().mx_blur_box_params(radius, C.byref(r), C.byref(ww), C.byref(fw))
    return status, (r.value, ww.value, fw.value)


def test_box_params_equal_the_restatement():
    from sduss_amd import lib, ops
    for radius in O.RADII + (0.01, 7.77, 100.0, 1024.0):
        status, got = _params(radius)
        r, ww, fw = O.box_params(radius)
        assert status == 0 and got == (r, ww, fw) == ops.blur_box_params(radius), (radius, got)
        assert r >= 0 and (2 * r + 1) * ww + 2 * fw in ((1 << 24) - 1, 1 << 24) and 0 <= fw <= ww       # the weights of a line sum to 2^24 (less the halving)
    assert O.box_params(0.3)[0] == 0 and O.box_params(40.0)[0] == 39                                      # r = 0 and the widest box of the case list
    l = lib.load()
    for radius, msg in ((0.0, b"positive"), (-1.0, b"positive"), (1025.0, b"MX_BLUR_MAX_RADIUS"), (float("nan"), b"positive")):
        status, got = _params(radius)
        assert status != 0 and msg in l.mx_last_error() and got == (-7, 7, 7), (radius, l.mx_last_error())
    assert l.mx_blur_box_params(2.0, None, None, None) != 0 and b"null" in l.mx_last_error()


def test_restatement_equals_the_stored_pillow_bytes(golden):
    n = 0
    for key, h, w, kind, seed in O.blur_cases():
        m = O.case_mask(h, w, kind, seed)
        if (h, w) != O.LARGE[0]:
            assert np.array_equal(golden[f"in_{key}"], m)                      # the stored inputs are the generator's
        assert m.shape == (h, w) and m.any()
        for radius in O.radii_of(key):
            want = golden[f"blur_{key}_r{radius:g}"]
            assert np.array_equal(O.gaussian_blur(m, radius), want), (key, radius)
            n += 1
    assert n == len(O.SHAPES) * len(O.KINDS) * len(O.RADII) + len(O.LARGE[1])
    assert np.array_equal(O.gaussian_blur(m, 0.0), m) and np.array_equal(O.gaussian_blur(m, -2.0), m)
    t = O.sample_triples()
    assert t.shape == (O.OVERLAY_SAMPLE, 3) and np.array_equal(O.overlay_bytes(t[:, 0], t[:, 1], t[:, 2]), golden["overlay_out"])


def test_every_tap_clamps_where_the_box_is_wider_than_the_line():
    """r + 1 >= n: 5 and 17 pixel lines under radius 40 (r = 39), and a one-pixel line, whose blur is the pixel itself"""
    r, ww, fw = O.box_params(40.0)
    for n in (5, 17, 1):
        x = O.case_mask(1, n, "random", 50 + n)
        assert r + 1 >= n
        out = O.box_pass(x, -1, r, ww, fw)
        edge = (np.arange(n) - r - 1 < 0).all() and (np.arange(n) + r + 1 > n - 1).all()
        assert edge and out.shape == x.shape
    one = np.array([[201]], dtype=np.uint8)
    assert O.gaussian_blur(one, 40.0)[0, 0] in (200, 201)                        # (2^24 less the halving of fw: the pixel, or one below)


def test_restatements_equal_live_pillow():
    pytest.importorskip("PIL.Image")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_overlay_pillow as M
    for key, h, w, kind, seed in O.blur_cases():
        m = O.case_mask(h, w, kind, seed)
        for radius in O.radii_of(key):
            assert np.array_equal(O.gaussian_blur(m, radius), M.pillow_blur(m, radius)), (key, radius)
    dec, orig, mask = O.triple_image()                                           # every (d, o, m), other data in the other channels
    assert np.array_equal(O.overlay(dec, orig, mask, 0, 0)[0], M.pillow_overlay(dec[0], orig[0], mask[0]))
    from PIL import Image
    for kind in O.KINDS:
        m = O.case_mask(37, 53, kind, 7)
        assert tuple(O.bbox(m[None])[0]) == Image.fromarray(m, "L").getbbox()
    assert tuple(O.bbox(np.zeros((1, 5, 9), dtype=np.uint8))[0]) == (9, 5, 0, 0) and Image.fromarray(np.zeros((5, 9), dtype=np.uint8), "L").getbbox() is None


def test_overlay_of_a_hard_mask_is_the_paste():
    """m = 0 gives the original's byte and m = 255 the decoded one, for every pair: on a 0 / 255 mask the overlay is mx_rgb8_paste's selection"""
    o, d = np.arange(256)[:, None], np.arange(256)[None, :]
    assert (O.overlay_bytes(d, o, 0) == o).all() and (O.overlay_bytes(d, o, 255) == d).all()
    mid = O.overlay_bytes(d, o, 128)
    assert (mid >= np.minimum(o, d)).all() and (mid <= np.maximum(o, d)).all() and not (mid == o).all() and not (mid == d).all()


CROP_CASES = [
    # (box, mask_w, mask_h, width, height, pad): what it is there for
    ((0, 0, 10, 10, ), 200, 120, 64, 64, 8),              # the top left corner: the pad clips on two sides
    ((190, 0, 200, 10), 200, 120, 64, 64, 8),             # top right
    ((0, 110, 10, 120), 200, 120, 64, 64, 8),             # bottom left
    ((190, 110, 200, 120), 200, 120, 64, 64, 8),          # bottom right
    ((0, 50, 200, 60), 200, 120, 64, 64, 0),              # full width, a short height: grows past both ends of the mask, y2 is clipped
    ((90, 40, 110, 60), 200, 120, 64, 64, 500),           # pad larger than every margin: the whole mask
    ((60, 40, 140, 50), 200, 120, 64, 64, 3),             # wider than the request's aspect: the height grows
    ((60, 20, 70, 100), 200, 120, 64, 64, 3),             # narrower: the width grows
    ((60, 40, 101, 50), 200, 120, 96, 64, 0),             # a non-square request, an odd difference: the halves differ by one
    ((20, 100, 120, 118), 200, 120, 64, 64, 0),           # grows past the bottom: shifted back up (y2 >= mask_h)
    ((20, 2, 120, 20), 200, 120, 64, 64, 0),              # grows past the top: shifted back down (y1 < 0)
    ((20, 30, 199, 90), 200, 120, 64, 64, 0),             # shifted up, then down, then y2 clipped: taller than the mask allows
    ((150, 20, 198, 110), 200, 120, 64, 64, 0),           # the same three on x: past the right edge
    ((2, 20, 50, 110), 200, 120, 64, 64, 0),              # past the left edge
    ((5, 0, 195, 120), 200, 120, 128, 64, 0),             # full height under a 2:1 request: x grows, is shifted, and x2 clipped
    ((7, 9, 8, 10), 11, 13, 1024, 768, 1),                # a single pixel
]


@pytest.mark.parametrize("case", range(len(CROP_CASES)))
def test_crop_region_equals_the_python_rule(case):
    from sduss_amd import lib, ops
    box, mw, mh, width, height, pad = CROP_CASES[case]
    want = O.crop_region(box, mw, mh, width, height, pad)
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert lib.load().mx_crop_region(*box, mw, mh, width, height, pad, out) == 0, lib.load().mx_last_error()
    assert tuple(out) == want == ops.crop_region(box, (mh, mw), (height, width), pad)
    x1, y1, x2, y2 = want
    assert 0 <= x1 < x2 <= mw and 0 <= y1 < y2 <= mh
    assert x1 <= max(box[0] - pad, 0) and y1 <= max(box[1] - pad, 0) and x2 >= min(box[2] + pad, mw) and y2 >= min(box[3] + pad, mh)   # it only grows


def test_crop_cases_take_every_branch():
    """the case list reaches both aspect branches and the three shift-back steps of each: found by instrumenting the restatement's inputs"""
    seen = set()
    for box, mw, mh, width, height, pad in CROP_CASES:
        x1, y1, x2, y2 = max(box[0] - pad, 0), max(box[1] - pad, 0), min(box[2] + pad, mw), min(box[3] + pad, mh)
        tall = (x2 - x1) / (y2 - y1) > width / height
        lo, hi, n = (y1, y2, mh) if tall else (x1, x2, mw)
        other = (x2 - x1) if tall else (y2 - y1)
        diff = int(other / (width / height) - (hi - lo)) if tall else int(other * (width / height) - (hi - lo))
        lo, hi = lo - diff // 2, hi + diff - diff // 2
        seen.add(("y" if tall else "x", "grow"))
        if hi >= n:
            seen.add(("y" if tall else "x", "past the end"))
            lo, hi = lo - (hi - n), n
        if lo < 0:
            seen.add(("y" if tall else "x", "past the start"))
            hi, lo = hi - lo, 0
        if hi > n:
            seen.add(("y" if tall else "x", "clipped"))
    assert seen == {(a, s) for a in "xy" for s in ("grow", "past the end", "past the start", "clipped")}, seen


def test_crop_region_on_random_boxes():
    from sduss_amd import lib
    l = lib.load()
    rng = np.random.default_rng(5)
    out = (C.c_int32 * 4)()
    for _ in range(3000):
        mw, mh = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        x1, y1 = int(rng.integers(0, mw)), int(rng.integers(0, mh))
        box = (x1, y1, int(rng.integers(x1 + 1, mw + 1)), int(rng.integers(y1 + 1, mh + 1)))
        width, height, pad = int(rng.integers(1, 200)), int(rng.integers(1, 200)), int(rng.integers(0, 40))
        assert l.mx_crop_region(*box, mw, mh, width, height, pad, out) == 0
        assert tuple(out) == O.crop_region(box, mw, mh, width, height, pad), (box, mw, mh, width, height, pad)
        assert 0 <= out[0] < out[2] <= mw and 0 <= out[1] < out[3] <= mh


def test_entries_refuse_without_a_launch():
    from sduss_amd import lib
    l = lib.load()
    src, dst, tmp = OK, OK + FAR, OK + 2 * FAR
    for args, msg in (((None, dst, tmp, 1, 8, 8, 2.0), b"null"), ((src, None, tmp, 1, 8, 8, 2.0), b"null"), ((src, dst, None, 1, 8, 8, 2.0), b"null scratch"),
                      ((src, dst, tmp, 0, 8, 8, 2.0), b"positive"), ((src, dst, tmp, 1, -1, 8, 2.0), b"positive"), ((src, dst, tmp, 1, 8, 0, 2.0), b"positive"),
                      ((src, dst, tmp, 1, 8, 16385, 2.0), b"MX_BLUR_MAX_WIDTH"), ((src, dst, tmp, 1, 8, 8, 1025.0), b"MX_BLUR_MAX_RADIUS"),
                      ((src, dst, tmp, 1, 8, 8, float("nan")), b"must be a number"),
                      ((src, src, tmp, 1, 8, 8, 2.0), b"alias"), ((src, src + 63, tmp, 1, 8, 8, 2.0), b"alias"), ((src, src, None, 1, 8, 8, 0.0), b"alias"),
                      ((src, dst, src + 8, 1, 8, 8, 2.0), b"scratch may alias"), ((src, dst, dst, 1, 8, 8, 2.0), b"scratch may alias")):
        assert l.mx_gaussian_blur_u8(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((None, OK, 1, 8, 8), b"null"), ((OK, None, 1, 8, 8), b"null"), ((OK, OK + FAR, 0, 8, 8), b"positive"),
                      ((OK, OK + FAR, 1, 0, 8), b"positive"), ((OK, OK + FAR, 1, 8, -3), b"positive"), ((OK, OK + FAR + 2, 1, 8, 8), b"aligned")):
        assert l.mx_mask_bbox_u8(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    dec, orig, mask, out = OK, OK + FAR, OK + 2 * FAR, OK + 3 * FAR
    good = (1, 50, 70, 3, 5, 20, 10)                          # B, H, W, x, y, w, h
    for args, msg in (((None, orig, mask, out) + good, b"null"), ((dec, None, mask, out) + good, b"null"), ((dec, orig, None, out) + good, b"null"),
                      ((dec, orig, mask, None) + good, b"null"),
                      ((dec, orig, mask, out, 0, 50, 70, 3, 5, 20, 10), b"positive"), ((dec, orig, mask, out, 1, 50, 70, 3, 5, 0, 10), b"positive"),
                      ((dec, orig, mask, out, 1, 50, 70, 3, 5, 20, -1), b"positive"), ((dec, orig, mask, out, 1, 0, 70, 3, 5, 20, 10), b"positive"),
                      ((dec, orig, mask, out, 1, 50, 70, -1, 5, 20, 10), b"inside the image"), ((dec, orig, mask, out, 1, 50, 70, 3, -2, 20, 10), b"inside the image"),
                      ((dec, orig, mask, out, 1, 50, 70, 51, 5, 20, 10), b"inside the image"), ((dec, orig, mask, out, 1, 50, 70, 3, 41, 20, 10), b"inside the image"),
                      ((dec, orig, mask, out, 1, 50, 70, 3, 5, 2147483647, 10), b"inside the image"),
                      ((dec, orig, mask, orig) + good, b"alias"), ((dec, orig, mask, orig + 100) + good, b"alias"), ((dec, orig, mask, mask) + good, b"alias"),
                      ((dec, orig, mask, dec) + good, b"alias"), ((dec, orig, mask, dec + 599) + good, b"alias")):
        assert l.mx_rgb8_overlay(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    out4 = (C.c_int32 * 4)(-7, -7, -7, -7)
    for args, msg in (((0, 0, 4, 4, 8, 8, 64, 64, 0, None), b"null"), ((0, 0, 4, 4, 0, 8, 64, 64, 0, out4), b"positive"), ((0, 0, 4, 4, 8, 8, 64, 0, 0, out4), b"positive"),
                      ((0, 0, 4, 4, 8, 8, 64, 64, -1, out4), b"pad"), ((8, 8, 0, 0, 8, 8, 64, 64, 0, out4), b"empty"), ((2, 2, 2, 5, 8, 8, 64, 64, 0, out4), b"empty"),
                      ((2, 5, 6, 5, 8, 8, 64, 64, 4, out4), b"empty"), ((-1, 0, 4, 4, 8, 8, 64, 64, 0, out4), b"inside the mask"),
                      ((0, 0, 9, 4, 8, 8, 64, 64, 0, out4), b"inside the mask"), ((0, 0, 4, 9, 8, 8, 64, 64, 0, out4), b"inside the mask")):
        assert l.mx_crop_region(*args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    assert tuple(out4) == (-7, -7, -7, -7)                   # refused: nothing written


def test_wrappers_refuse_cpu_tensors():
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    m = torch.zeros(1, 8, 8, dtype=torch.uint8)
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(MxError, match="contiguous CUDA uint8"):
        ops.gaussian_blur_u8(m, 2.0)
    with pytest.raises(MxError, match="contiguous CUDA uint8"):
        ops.mask_bbox(m)
    with pytest.raises(MxError, match="contiguous CUDA uint8"):
        ops.rgb8_overlay(img, img.clone(), m)
    with pytest.raises(MxError, match="empty"):
        ops.crop_region((8, 8, 0, 0), (8, 8), (64, 64), 4)                      # what mask_bbox gives for an empty mask


def test_inpaint_state_constructs_as_before():
    from sduss_amd.pipeline import InpaintState
    t = torch.zeros(1)
    s = InpaintState(t, t, t, None, t, False)                                  # the six fields of the parent, positionally
    assert s.full_image_u8 is None and s.full_mask_u8 is None and s.region is None and s.overlay is False
    s = InpaintState(t, t, t, None, t, True, t, t, (1, 2, 3, 4), True)
    assert s.paste and s.region == (1, 2, 3, 4) and s.overlay


def test_new_arguments_need_the_uint8_image_and_finish_cropped_a_region():
    from sduss_amd.lib import MxError
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    from sduss_amd.vae import OUTPUT_TYPES, finish_cropped
    enc = SimpleNamespace(device="cpu")
    img, mask = torch.zeros(1, 3, 24, 24), torch.zeros(1, 24, 24, dtype=torch.uint8)
    for den in (SDXLDenoiser(SimpleNamespace(device="cpu")), SD3Denoiser(SimpleNamespace(device="cpu"))):
        for kw in ({"blur": 2.0}, {"crop_pad": 4}, {"overlay": True}):
            req = SimpleNamespace(num_inference_steps=10)
            with pytest.raises(MxError, match="work on the client's uint8"):
                den.start_inpaint(req, enc, img, mask, **kw)
            assert not hasattr(req, "latents") and not hasattr(req, "sigmas")
        with pytest.raises(MxError, match="expected a uint8 mask"):
            den.start_inpaint(SimpleNamespace(num_inference_steps=10), enc, torch.zeros(1, 24, 24, 3, dtype=torch.uint8), mask[:, :20], overlay=True)
    with pytest.raises(MxError, match="not started with crop_pad"):
        finish_cropped(SimpleNamespace(inpaint=None), torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    assert OUTPUT_TYPES == ("pt", "uint8", "pil")
