"""HyperTile without a GPU: the windows a geometry gets against HyperTile's random_divisor rule written out, and mx_unet_set_hypertile's argument
refusals."""
import ctypes as C

import pytest

from sduss_amd.config import UNetConfig
from sduss_amd.unet import config_c, hypertile_windows


def random_divisor_swap1(value, min_value):
    """tfernd/HyperTile ``random_divisor(value, min_value, max_options=1)``: the divisors of ``value`` that are >= min(min_value, value), ascending; the
    first ``max_options`` are the candidates, so with one option the choice is the first"""
    min_value = min(min_value, value)
    divisors = [i for i in range(min_value, value + 1) if value % i == 0]
    return divisors[:1][0]


@pytest.mark.parametrize("tile_size", [128, 256])
@pytest.mark.parametrize("H_lat,W_lat", [(128, 128), (128, 96), (64, 64), (96, 72)])
def test_windows_follow_random_divisor(H_lat, W_lat, tile_size):
    tokens = max(tile_size // 8, 4)
    got = hypertile_windows(UNetConfig.sdxl_base(), (tokens, 2), H_lat, W_lat)
    assert len(got) == 2
    for depth, win in zip((1, 2), got):
        gh, gw = H_lat >> depth, W_lat >> depth
        wh, ww = random_divisor_swap1(gh, tokens), random_divisor_swap1(gw, tokens)
        assert win == ((gh, gw, wh, ww) if (wh, ww) != (gh, gw) and ww % 16 == 0 else None), (depth, win, wh, ww)
    if (H_lat, W_lat) == (128, 128):            # the headline geometry: 16 x 16 windows at both levels, or 32 x 32 at the first alone
        assert got == ([(64, 64, 16, 16), (32, 32, 16, 16)] if tile_size == 128 else [(64, 64, 32, 32), None])
    assert hypertile_windows(UNetConfig.sdxl_base(), None, H_lat, W_lat) == [None, None]
    assert hypertile_windows(UNetConfig.sdxl_base(), (tokens, 1), H_lat, W_lat) == [got[0], None]


def test_setter_refusals():
    from sduss_amd import lib
    l = lib.load()
    cc = config_c(UNetConfig.tiny())
    u = l.mx_unet_create(C.byref(cc))
    assert u
    try:
        for tokens, depth in [(16, 2), (0, 2), (4, 0), (4096, 3)]:
            assert l.mx_unet_set_hypertile(u, tokens, depth) == 0
        for tokens, depth, message in [(3, 2, b"tile_tokens"), (-1, 2, b"tile_tokens"), (4097, 2, b"tile_tokens"), (16, -1, b"max_depth"), (16, 4, b"max_depth")]:
            assert l.mx_unet_set_hypertile(u, tokens, depth) == 1 and message in l.mx_last_error()
        assert l.mx_unet_set_hypertile(None, 16, 2) == 1 and b"null handle" in l.mx_last_error()
    finally:
        l.mx_unet_destroy(u)
