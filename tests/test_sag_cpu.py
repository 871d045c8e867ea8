"""Self-attention guidance without a GPU: every refusal of the new entry points and of the capture on the paths that do not serve it arrives before
a launch, the host's blur taps, and set_sag's own refusals."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from sduss_amd import lib, ops
from sduss_amd.config import UNetConfig
from sduss_amd.unet import config_c

A = 0x10000          # an aligned address that no refused call may touch


def _call(name, **changed):
    l = lib.load()
    rows, coef, taps = (C.c_int * 2)(0, 1), (C.c_float * 2)(0.1, 0.1), (C.c_float * 9)()
    base = {
        "mx_attention_colmass": dict(stream=None, q=A, ldq=128, k=A + 128, ldk=128, B=1, H=1, L=60, scale=0.125, prescaled=0, ws=A, ws_bytes=1 << 20,
                                     mass=A, mask=A),
        "mx_sag_degrade": dict(stream=None, lat=A, eps=A, sigma=A, mask=A, hm=2, wm=2, rows=rows, n_out=2, n=2, C=4, h=8, w=8, blur=1.0, out=A, dtype=2),
        "mx_sag_fold": dict(stream=None, noise=A, eps_d=A, coef=coef, rows=rows, n_out=2, n=2, elems=64, dtype=2),
        "mx_sag_blur_taps": dict(blur=1.0, taps=taps),
    }[name]
    assert set(changed) <= set(base)
    rc = getattr(l, name)(*{**base, **changed}.values())
    return rc, l.mx_last_error().decode()


@pytest.mark.parametrize("name,changed,message", [
    ("mx_attention_colmass", dict(q=None), "null operand"), ("mx_attention_colmass", dict(mask=None), "null operand"),
    ("mx_attention_colmass", dict(L=0), "empty problem"), ("mx_attention_colmass", dict(k=A + 8), "16-byte aligned"),
    ("mx_attention_colmass", dict(mass=A + 2), "4-byte aligned"), ("mx_attention_colmass", dict(ldq=60), "multiples of 8"),
    ("mx_attention_colmass", dict(H=3), "covering H*64"), ("mx_attention_colmass", dict(scale=0.0), "positive and finite"),
    ("mx_attention_colmass", dict(ws_bytes=239), "workspace too small"),
    ("mx_sag_degrade", dict(eps=None), "null operand"), ("mx_sag_degrade", dict(h=4), "more than 4 x 4"), ("mx_sag_degrade", dict(w=3), "more than 4 x 4"),
    ("mx_sag_degrade", dict(blur=0.0), "blur_sigma"), ("mx_sag_degrade", dict(blur=-1.0), "blur_sigma"), ("mx_sag_degrade", dict(out=A + 1), "misaligned"),
    ("mx_sag_degrade", dict(sigma=A + 2), "misaligned"), ("mx_sag_degrade", dict(dtype=9), "bad dtype"), ("mx_sag_degrade", dict(n=1), "output rows"),
    ("mx_sag_degrade", dict(rows=(C.c_int * 2)(0, 2)), "outside [0, n)"), ("mx_sag_degrade", dict(n_out=65, n=65), "output rows"),
    ("mx_sag_fold", dict(noise=None), "null operand"), ("mx_sag_fold", dict(eps_d=A + 1), "misaligned"), ("mx_sag_fold", dict(n=1), "SAG rows"),
    ("mx_sag_fold", dict(rows=(C.c_int * 2)(-1, 0)), "outside [0, n)"), ("mx_sag_fold", dict(rows=(C.c_int * 2)(1, 1)), "twice"), ("mx_sag_fold", dict(coef=(C.c_float * 2)(float("nan"), 0.0)), "NaN"),
    ("mx_sag_fold", dict(dtype=-1), "bad dtype"), ("mx_sag_blur_taps", dict(blur=0.0), "positive"), ("mx_sag_blur_taps", dict(taps=None), "null operand"),
])
def test_entry_point_refusals(name, changed, message):
    rc, said = _call(name, **changed)
    assert rc == 1 and message in said, said


def test_workspace_bytes():
    l = lib.load()
    assert l.mx_attention_colmass_workspace_bytes(1, 1, 60) == 240 and l.mx_attention_colmass_workspace_bytes(4, 20, 1024) == 4 * 20 * 8 * 1024 * 4
    assert l.mx_attention_colmass_workspace_bytes(2, 3, 129) == 2 * 3 * 2 * 129 * 4 and l.mx_attention_colmass_workspace_bytes(0, 1, 8) == 0


@pytest.mark.parametrize("blur_sigma", [1.0, 0.5, 3.0])
def test_blur_taps(blur_sigma):
    t = ops.sag_blur_taps(blur_sigma)
    want = np.exp(-0.5 * (np.arange(-4, 5) / blur_sigma) ** 2)
    assert t.dtype == np.float32 and np.array_equal(t, (want / want.sum()).astype(np.float32))
    assert np.array_equal(t, t[::-1]) and abs(float(t.astype(np.float64).sum()) - 1.0) <= 9 * 2.0 ** -25 and t.argmax() == 4


def _forward(l, u, name):
    args = [u] + [0 if a in (C.c_int, C.c_size_t) else None for a in lib.SYMBOLS[name][1][1:]]
    if name == "mx_unet_forward":
        args[9:13] = 4, 128, 128, 77           # batch, H, W, ctx_len: the mid grid is 32 x 32
    if name == "mx_unet_forward_mixed":        # two resolution groups
        args[2:4] = (lib.UNetGroup * 2)(lib.UNetGroup(None, None, 2, 32, 32), lib.UNetGroup(None, None, 2, 16, 16)), 2
        args[9] = 77
    return getattr(l, name)(*args)


def test_capture_refusals():
    """announced, the paths that do not capture refuse with their own message ahead of every other complaint (the operands are NULL: nothing can
    launch), and the announcement is used up"""
    l = lib.load()
    cc = config_c(UNetConfig.tiny())
    u = l.mx_unet_create(C.byref(cc))
    try:
        for mass, mask, rows, message in [(A, None, 2, b"come together"), (None, None, 2, b"come together"), (A, A, 0, b"come together"), (A + 2, A, 2, b"misaligned")]:
            assert l.mx_unet_set_attn_mass(u, mass, mask, rows) == 1 and message in l.mx_last_error()
        assert l.mx_unet_set_attn_mass(None, A, A, 2) == 1 and b"null handle" in l.mx_last_error()
        for name, how in [("mx_unet_forward_cached", b"block-skip cache"), ("mx_unet_forward_cached_mixed", b"block-skip cache"), ("mx_unet_forward_pp", b"patch-parallel"),
                          ("mx_unet_forward_pp_stale", b"patch-parallel"), ("mx_unet_forward_mixed", b"more than one resolution group")]:
            assert l.mx_unet_set_attn_mass(u, A, A, 2) == 0
            assert _forward(l, u, name) != 0 and b"attention mass" in l.mx_last_error() and how in l.mx_last_error()
            assert _forward(l, u, name) != 0 and b"attention mass" not in l.mx_last_error()
        for turn_on, turn_off, message in [(lambda: l.mx_unet_set_tome(u, 0.5, 2, 2, 2), lambda: l.mx_unet_set_tome(u, 0.0, 2, 2, 2), b"ToMe"),
                                           (lambda: l.mx_unet_set_hypertile(u, 16, 2), lambda: l.mx_unet_set_hypertile(u, 0, 2), b"HyperTile")]:
            assert turn_on() == 0 and l.mx_unet_set_attn_mass(u, A, A, 2) == 0
            assert _forward(l, u, "mx_unet_forward") != 0 and b"attention mass" in l.mx_last_error() and message in l.mx_last_error()
            assert turn_off() == 0
        assert l.mx_unet_set_hypertile(u, 16, 1) == 0 and l.mx_unet_set_attn_mass(u, A, A, 2) == 0      # HyperTile above the mid level: served
        assert _forward(l, u, "mx_unet_forward") != 0 and b"attention mass" not in l.mx_last_error()
        assert l.mx_unet_set_attn_mass(u, A, A, 5) == 0
        assert _forward(l, u, "mx_unet_forward") != 0 and b"more rows than the forward" in l.mx_last_error()
        assert l.mx_unet_set_attn_mass(u, A, A, 2) == 0 and l.mx_unet_set_attn_mass(u, None, None, 0) == 0
    finally:
        l.mx_unet_destroy(u)


def test_set_sag_refusals():
    import torch
    from sduss_amd.pipeline import Denoiser, SDXLDenoiser
    den = object.__new__(SDXLDenoiser)
    den.guidance_scale, den.unet = 5.0, SimpleNamespace(_block_caches=None, _tome=None)
    req = SimpleNamespace(sag_scale=0.0, sag_blur_sigma=1.0)
    for scale, blur in [(-0.1, 1.0), (float("nan"), 1.0), (0.75, 0.0), (0.75, float("inf"))]:
        with pytest.raises(lib.MxError, match="set_sag"):
            den.set_sag(req, scale, blur)
    assert req.sag_scale == 0.0 and den._sag_begin([SimpleNamespace(reqs=[req])], False) is None
    den.set_sag(req)
    assert (req.sag_scale, req.sag_blur_sigma) == (0.75, 1.0)
    part = SimpleNamespace(reqs=[req])
    with pytest.raises(lib.MxError, match="classifier-free guidance"):
        den._sag_begin([part], False)
    with pytest.raises(lib.MxError, match="several resolutions"):
        den._sag_begin([part, part], True)
    den.unet._tome = (0.5, 2, 2, 2)
    with pytest.raises(lib.MxError, match="ToMe"):
        den._sag_begin([part], True)
    den.unet._tome, den.unet._block_caches = None, {}
    with pytest.raises(lib.MxError, match="block-skip cache"):
        den._sag_begin([part], True)
    den.unet._block_caches, den.unet.hypertile_windows = None, lambda h, w: [None, (h // 4, w // 4, 16, 16) if h >= 128 else None]
    stub = lambda h, image=None: SimpleNamespace(reqs=[req], entry=SimpleNamespace(image=image, uid=1), latents=torch.zeros(1, 4, h, h))      # noqa: E731
    for case, message in [(stub(16, image=(None, None)), "image prompt"), (stub(128), "HyperTile"), (stub(4), "more than 4 x 4")]:
        with pytest.raises(lib.MxError, match=message):
            den._sag_begin([case], True)
    flow = object.__new__(Denoiser)
    with pytest.raises(lib.MxError, match="SDXL model only"):
        flow._sag_begin([part], True)
