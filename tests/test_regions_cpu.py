"""Regional prompts without a GPU: the mask-to-weights rule on a hand case, and the Python-level refusals."""
from types import SimpleNamespace

import pytest
import torch

from sduss_amd import lib
from sduss_amd.regions import mask_weights


def test_mask_weights_hand_case():
    """4 x 4 masks on a 2 x 2 token grid (cells of 2 x 2): area means, normalised over the prompts; the bottom-right token is covered by no mask"""
    m = torch.zeros(2, 4, 4)
    m[0, :2, :] = 1.0               # prompt 0: the top half -> tokens 0, 1 fully
    m[1, :2, 2:] = 1.0              # prompt 1: the top-right cell as well -> token 1 shared half and half
    m[1, 2, 0] = 2.0                # and one pixel of weight 2 in the bottom-left cell: mean 0.5, alone there
    w = mask_weights(m, (2, 2))
    assert torch.equal(w, torch.tensor([[1.0, 0.5, 0.0, 1.0], [0.0, 0.5, 1.0, 0.0]]))
    assert torch.equal(mask_weights(m > 0, (4, 4)).sum(0), torch.ones(16))


def test_library_refusals():
    """announced, the entry points that do not serve regions refuse with their own message before anything can launch (NULL operands); one-shot"""
    import ctypes as C
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import config_c
    from test_sag_cpu import A, _forward
    l, cc = lib.load(), config_c(UNetConfig.tiny())
    u, two = l.mx_unet_create(C.byref(cc)), (C.c_void_p * 2)(A, A)
    try:
        assert l.mx_unet_set_regions(u, 5, 77, A, two, 2) == 1 and b"n_sets" in l.mx_last_error()
        for name, how in [("mx_unet_forward_cached", b"block-skip cache"), ("mx_unet_forward_pp", b"patch-parallel"), ("mx_unet_forward_mixed", b"more than one resolution group"),
                          ("mx_unet_forward", b"ctx_len == n_sets")]:
            assert l.mx_unet_set_regions(u, 2, 77, A, two, 2) == 0
            assert _forward(l, u, name) != 0 and b"regional" in l.mx_last_error() and how in l.mx_last_error(), l.mx_last_error()
            assert _forward(l, u, name) != 0 and b"regional" not in l.mx_last_error()
    finally:
        l.mx_unet_destroy(u)


def test_python_refusals():
    from sduss_amd.pipeline import Denoiser, SDXLDenoiser
    den = object.__new__(SDXLDenoiser)
    den.unet, den._region_comp = SimpleNamespace(_block_caches=None), {}
    req = SimpleNamespace(latents=torch.zeros(1, 4, 16, 16), regions=None, sag_scale=0.0)
    emb = lambda r: torch.zeros(r, 77, 64)      # noqa: E731
    for embeds, masks, message in [(emb(5), torch.ones(5, 16, 16), "R in 1..4"), (emb(2), torch.ones(2, 16, 8), "masks must be"),
                                   (emb(2), torch.ones(3, 16, 16), "masks must be"), (emb(2), -torch.ones(2, 16, 16), "negative"), (emb(2), None, "masks")]:
        with pytest.raises(lib.MxError, match=message):
            den.set_regions(req, embeds, masks)
    assert req.regions is None and den._regions_begin([SimpleNamespace(reqs=[req])], None, True) is None
    den.set_regions(req, emb(2), torch.ones(2, 16, 16, dtype=torch.bool))
    part = SimpleNamespace(reqs=[req], entry=SimpleNamespace(uid=1))
    with pytest.raises(lib.MxError, match="image prompt"):
        den._regions_begin([part], (None, None), True)
    req.sag_scale = 0.75
    with pytest.raises(lib.MxError, match="self-attention guidance"):
        den._regions_begin([part], None, True)
    with pytest.raises(lib.MxError, match="SDXL model only"):
        object.__new__(Denoiser)._regions_begin([part], None, True)
