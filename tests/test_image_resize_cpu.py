"""Host-side checks of the image resize: the entries of csrc/image_resize.hip and csrc/resize_coeffs.cpp are declared, exported and bound; the
library's coefficient tables equal the numpy restatement (tests/resize_ref.py) entry by entry; the restatement equals Pillow's bytes, stored
(tests/golden/resize_pillow.npz) and live; every refusal comes before a launch; ``size=`` with a float image raises.  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mx_resize_coeffs", "mx_resize_create", "mx_resize_destroy", "mx_resize_u8")
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow.npz"))


def test_entries_are_declared_exported_and_bound():
    from sduss_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in lib.SYMBOLS and hasattr(l, name)
        assert getattr(l, name).argtypes == lib.SYMBOLS[name][1]
    assert "typedef struct mx_resize mx_resize;" in hdr
    for name, code in R.FILTERS.items():
        assert re.search(rf"#define MX_RESIZE_{name.upper()} {code}\b", hdr) and lib.RESIZE_FILTERS[name] == code
    assert f"#define MX_RESIZE_PRECISION_BITS {R.PRECISION_BITS}" in hdr
    assert l.mx_version() == 1


@pytest.mark.parametrize("resample", list(R.FILTERS))
def test_library_tables_equal_the_restatement(resample):
    """mx_resize_coeffs against resize_ref.coeffs for every (in, out) of the case list, both axes, plus the edge sizes of the sanitizer walk"""
    from sduss_amd import lib
    l = lib.load()
    code = R.FILTERS[resample]
    for n_in, n_out in R.axis_pairs() + [(1, 1), (1, 7), (7, 1), (4096, 1), (2, 3), (3, 2)]:
        bounds, k, ksize = R.coeffs(n_in, n_out, resample)
        assert l.mx_resize_coeffs(n_in, n_out, code, None, None, 0) == ksize
        got_b = np.full((n_out, 2), -7, dtype=np.int32)
        got_k = np.full((n_out, ksize), -7, dtype=np.int32)                 # the tail entries must come back as zeros
        assert l.mx_resize_coeffs(n_in, n_out, code, got_b.ctypes.data, got_k.ctypes.data, n_out * ksize) == ksize, l.mx_last_error()
        assert np.array_equal(got_b, bounds) and np.array_equal(got_k, k), (n_in, n_out, resample)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] <= ksize).all()


def _inputs(golden, case, channels):
    x = golden[f"in_{case}"]
    return x if channels == 3 else np.ascontiguousarray(x[..., 0])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("resample", list(R.FILTERS))
def test_restatement_equals_the_stored_pillow_bytes(golden, resample, channels):
    for i, (ih, iw, oh, ow) in enumerate(R.CASES):
        assert np.array_equal(golden[f"in_{i}"], R.case_input(ih, iw, seed=100 + i))          # the stored inputs are the generator's
        x = _inputs(golden, i, channels)
        want = golden[f"out_{i}_{resample}_c{channels}"]
        got = R.resize(x, (oh, ow), resample)
        assert got.shape == want.shape == (2, oh, ow) + x.shape[3:] and np.array_equal(got, want), (i, resample, channels)
        if (ih, iw) == (oh, ow):
            assert np.array_equal(got, x)                                                      # equal sizes on both axes: a copy
    for i, (ih, iw, oh, ow) in enumerate(R.EXTRA_CASES):
        x = R.case_input(ih, iw, seed=200 + i)
        x = x if channels == 3 else np.ascontiguousarray(x[..., 0])
        assert np.array_equal(R.resize(x, (oh, ow), resample), golden[f"out_x{i}_{resample}_c{channels}"]), (i, resample, channels)


def test_overshoot_images_reach_both_ends_of_the_clip(golden):
    """the checkerboard and the stripe image: lanczos overshoots below 0 and above 255 in both passes, and Pillow's bytes are what the clip leaves"""
    x = R.overshoot_inputs()
    oh, ow = R.OVERSHOOT_CASE[2:]
    assert np.array_equal(golden["in_overshoot"], x)
    h = R.pass_unclipped(x, 2, ow, "lanczos")
    assert h.min() < 0 and h.max() > 255
    v = R.pass_unclipped(np.clip(h, 0, 255).astype(np.uint8), 1, oh, "lanczos")
    assert v.min() < 0 and v.max() > 255
    for c in (1, 3):
        want = golden[f"out_overshoot_lanczos_c{c}"]
        assert np.array_equal(R.resize(_inputs(golden, "overshoot", c), (oh, ow), "lanczos"), want)
        assert (want == 0).any() and (want == 255).any()


def test_restatement_equals_live_pillow(golden):
    Image = pytest.importorskip("PIL.Image")
    resample = {"lanczos": Image.Resampling.LANCZOS, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC}
    for i, (ih, iw, oh, ow) in enumerate(R.CASES):
        for f in R.FILTERS:
            for c in (1, 3):
                x = _inputs(golden, i, c)
                live = np.stack([np.asarray(Image.fromarray(im).resize((ow, oh), resample=resample[f])) for im in x])
                assert np.array_equal(R.resize(x, (oh, ow), f), live), (i, f, c)


def test_refusals_come_before_any_launch():
    from sduss_amd import lib
    l = lib.load()
    for args, msg in (((0, 8, 8, 8, 1), b"positive"), ((8, -1, 8, 8, 1), b"positive"), ((8, 8, 0, 8, 1), b"positive"), ((8, 8, 8, 0, 1), b"positive"),
                      ((8, 8, 4, 4, 0), b"unknown filter"), ((8, 8, 4, 4, 4), b"unknown filter"), ((8, 8, 8, 8, 9), b"unknown filter"),
                      (((1 << 24) + 1, 8, 4, 4, 1), b"2^24")):
        assert l.mx_resize_create(*args) is None and msg in l.mx_last_error(), (args, l.mx_last_error())
    l.mx_resize_destroy(None)                                                # as free(NULL)
    for args, msg in (((None, None, OK, OK + 64, 1, 3), b"null"), ((OK, None, None, OK + 64, 1, 3), b"null"), ((OK, None, OK + 64, None, 1, 3), b"null"),
                      ((OK, None, OK, OK + 64, 0, 3), b"positive"), ((OK, None, OK, OK + 64, -2, 1), b"positive"),
                      ((OK, None, OK, OK + 64, 1, 2), b"C must be 1 or 3"), ((OK, None, OK, OK + 64, 1, 4), b"C must be 1 or 3"),
                      ((OK, None, OK, OK + 64, 1, 0), b"C must be 1 or 3"), ((OK, None, OK + 64, OK + 64, 1, 3), b"alias")):
        assert l.mx_resize_u8(*args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((0, 8, 1, None, None, 0), b"positive"), ((8, 0, 1, None, None, 0), b"positive"), ((8, 4, 5, None, None, 0), b"unknown filter")):
        assert l.mx_resize_coeffs(*args) == -1 and msg in l.mx_last_error(), (args, l.mx_last_error())
    bounds, k = np.zeros((4, 2), dtype=np.int32), np.full(4 * 13 + 1, -7, dtype=np.int32)
    assert l.mx_resize_coeffs(8, 4, 1, bounds.ctypes.data, k.ctypes.data, 4 * 13 - 1) == -1 and b"fewer than" in l.mx_last_error()
    assert (k == -7).all()                                                   # refused: nothing written
    assert l.mx_resize_coeffs(8, 4, 1, bounds.ctypes.data, None, 4 * 13) == -1 and b"null" in l.mx_last_error()


def test_wrapper_checks_before_the_library():
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    with pytest.raises(MxError, match="contiguous CUDA uint8"):
        ops.resize_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (4, 4))                      # not on the device
    with pytest.raises(MxError, match="contiguous CUDA uint8"):
        ops.resize_u8(torch.zeros(1, 8, 8, 3), (4, 4))


def test_size_with_a_float_image_raises():
    """``size=`` resizes the client's bytes: a float image has no Pillow resize to be equal to, and is refused before anything else happens"""
    from sduss_amd.lib import MxError
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    enc = SimpleNamespace(device="cpu")
    img = torch.zeros(1, 3, 24, 24)
    for den in (SDXLDenoiser(SimpleNamespace(device="cpu")), SD3Denoiser(SimpleNamespace(device="cpu"))):
        req = SimpleNamespace(num_inference_steps=10)
        with pytest.raises(MxError, match="start_from_image: size= resizes the client's uint8 image"):
            den.start_from_image(req, enc, img, 0.5, size=(16, 16))
        with pytest.raises(MxError, match="start_inpaint: size= resizes the client's uint8 image"):
            den.start_inpaint(req, enc, img, torch.zeros(1, 24, 24, dtype=torch.uint8), size=(16, 16))
        assert not hasattr(req, "latents") and not hasattr(req, "sigmas")


def test_tables_under_address_and_ub_sanitizers():
    """tests/resize_coeffs_walk.cpp: a program of its own over csrc/resize_coeffs.cpp, compiled with -fsanitize=address,undefined and run on the CPU.
    It builds the tables of the case list and of the edge sizes (in = 1, out = 1, 4096 -> 1) into exactly sized arrays and checks xmin >= 0,
    xmin + n <= in and n <= ksize for every entry."""
    import subprocess
    csrc = os.path.join(ROOT, "sduss_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "resize_walk"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESIZE_COEFFS_WALK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
