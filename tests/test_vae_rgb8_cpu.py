"""Host half of the 8-bit image path (mx_conv3x3_rgb8, mx_vae_decode_rgb8, post_inference's output_type): the symbols are exported and bound,
and every bad argument is refused with a message before any HIP call -- none of this needs a GPU."""
import ctypes as C

import pytest

from sduss_amd import lib as L

PTR = 0x10000          # a non-null, 16-byte aligned placeholder: an argument check that passed it on would fault, a refusal never reads it


def _err():
    return L.load().mx_last_error().decode()


def test_rgb8_symbols_are_exported_and_bound():
    l = L.load()
    for name in ("mx_conv3x3_rgb8", "mx_vae_decode_rgb8"):
        assert name in L.SYMBOLS
        fn = getattr(l, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == L.SYMBOLS[name][1]
    assert len(L.SYMBOLS["mx_conv3x3_rgb8"][1]) == 9 and len(L.SYMBOLS["mx_vae_decode_rgb8"][1]) == 10
    assert l.mx_version() == 1


@pytest.mark.parametrize("which", ["x", "w", "bias", "out"])
def test_conv3x3_rgb8_refuses_null_pointers(which):
    p = {"x": PTR, "w": PTR, "bias": PTR, "out": PTR}
    p[which] = None
    assert L.load().mx_conv3x3_rgb8(None, p["x"], p["w"], p["bias"], p["out"], 1, 4, 16, 64) != 0
    assert "null" in _err()


@pytest.mark.parametrize("cin", [3, 32, 96, 100])
def test_conv3x3_rgb8_refuses_channel_counts_off_the_chunk(cin):
    assert L.load().mx_conv3x3_rgb8(None, PTR, PTR, PTR, PTR, 1, 4, 16, cin) != 0
    assert "multiple of 64" in _err()


@pytest.mark.parametrize("shape", [(0, 4, 16, 64), (1, 0, 16, 64), (1, 4, 0, 64), (1, 4, 16, 0), (-1, 4, 16, 64), (1, -4, 16, 64), (1, 4, -16, 64),
                                   (1, 4, 16, -64)])
def test_conv3x3_rgb8_refuses_non_positive_sizes(shape):
    assert L.load().mx_conv3x3_rgb8(None, PTR, PTR, PTR, PTR, *shape) != 0
    assert "positive" in _err()


def test_conv3x3_rgb8_refuses_what_the_kernel_cannot_index():
    """32-bit source offsets (as conv_small_n_serves) and the LDS the launch would request: errors, not launches"""
    l = L.load()
    assert l.mx_conv3x3_rgb8(None, PTR, PTR, PTR, PTR, 8, 2048, 2048, 64) != 0          # B H W Cin = 2^31
    assert "32-bit" in _err()
    assert l.mx_conv3x3_rgb8(None, PTR, PTR, PTR, PTR, 1, 4, 16, 1024) != 0             # 3 x 9 x 1024 bf16 weights + the stage > 64 KB
    assert "LDS" in _err()
    assert l.mx_conv3x3_rgb8(None, PTR + 2, PTR, PTR, PTR, 1, 4, 16, 64) != 0
    assert "aligned" in _err()


def _handle(out_channels):
    l = L.load()
    cc = L.VAEConfigC()
    cc.latent_channels, cc.out_channels, cc.n_levels = 4, out_channels, 3
    for i, v in enumerate((64, 64, 128)):
        cc.block_out_channels[i] = v
    cc.layers_per_block, cc.norm_num_groups, cc.norm_eps = 1, 32, 1e-6
    h = l.mx_vae_create(C.byref(cc))
    assert h, _err()
    return h


def test_vae_decode_rgb8_refuses_bad_arguments():
    l = L.load()
    assert l.mx_vae_decode_rgb8(None, None, PTR, L.MX_BF16, PTR, 1, 16, 16, PTR, 1 << 20) != 0
    assert "null handle" in _err()
    h4 = _handle(4)
    try:
        assert l.mx_vae_decode_rgb8(h4, None, PTR, L.MX_BF16, PTR, 1, 16, 16, PTR, 1 << 20) != 0
        assert "out_channels == 3" in _err()
    finally:
        l.mx_vae_destroy(h4)
    h3 = _handle(3)
    try:
        for shape in ((0, 16, 16), (1, 0, 16), (1, 16, -1)):
            assert l.mx_vae_decode_rgb8(h3, None, PTR, L.MX_BF16, PTR, *shape, PTR, 1 << 20) != 0
            assert "bad shape" in _err()
        for lat, out, ws in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
            assert l.mx_vae_decode_rgb8(h3, None, lat, L.MX_BF16, out, 1, 16, 16, ws, 1 << 20) != 0
            assert "null operand" in _err()
        assert l.mx_vae_decode_rgb8(h3, None, PTR, L.MX_BF16, PTR, 1, 16, 16, PTR, 1 << 20) != 0      # no weights set
        assert "weights not set" in _err()
        # the float entry point does not reach the 8-bit path through its dtype code
        assert l.mx_vae_decode(h3, None, PTR, L.MX_BF16, PTR, -1, 1, 16, 16, PTR, 1 << 20) != 0
        assert "bad dtype" in _err()
    finally:
        l.mx_vae_destroy(h3)


def test_post_inference_refuses_an_unknown_output_type():
    from sduss_amd.vae import OUTPUT_TYPES, post_inference
    assert OUTPUT_TYPES == ("pt", "uint8", "pil")
    with pytest.raises(ValueError, match="output_type"):
        post_inference(None, {"64": []}, output_type="bogus")
