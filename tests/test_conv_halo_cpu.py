"""Host half of mx_conv3x3_halo (csrc/conv_halo.hip): mx_conv3x3_halo_serves over a table of descriptors (fake 16-byte-aligned pointers, no device),
the LDS bytes it reports, and the entry's refusal of a descriptor it does not serve."""
import ctypes as C

import pytest

from sduss_amd import lib as L

PTR = 0x10000
LDS_LIMIT = 160 * 1024


def _desc(B=8, H=32, W=32, Cin=1280, N=1280, **over):
    d = L.GemmDesc()
    d.a, d.w, d.c, d.bias = PTR, PTR, PTR, PTR
    d.M, d.N, d.K, d.ldc, d.ldr = B * H * W, N, 9 * Cin, N, N
    d.rows_per_batch = H * W
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = B, H, W, Cin, H, W, 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _strided(**kw):
    d = _desc(**kw)
    d.stride, d.Hout, d.Wout = 2, d.Hin // 2, d.Win // 2
    d.M = d.B * d.Hout * d.Wout
    d.rows_per_batch = d.Hout * d.Wout
    return d


def _upsampled(**kw):
    d = _desc(**kw)
    d.up, d.Hout, d.Wout = 1, 2 * d.Hin, 2 * d.Win
    d.M = d.B * d.Hout * d.Wout
    d.rows_per_batch = d.Hout * d.Wout
    return d


def _grouped():
    d = _desc()
    segs = (L.GemmSeg * 2)()
    d.segs, d.n_segs = C.cast(segs, C.POINTER(L.GemmSeg)), 2
    return d, segs


ACCEPTED = {
    "width32_1280": _desc(),                                            # the 8192-row convs of the headline step
    "width64_640": _desc(H=64, W=64, Cin=640, N=640),                   # its stride-1 32768-row convs
    "width64_cin1920": _desc(H=64, W=64, Cin=1920, N=640),
    "one_tile": _desc(B=1, H=8, W=32, Cin=64, N=160),                   # H W == 256, Cin == 64, N == 160: the smallest of each
    "one_tile_w64": _desc(B=1, H=4, W=64, Cin=64, N=160),
    "rowbias": _desc(rowbias=PTR, ldrb=1280),
    "residual": _desc(residual=PTR),
    "gn_partials": _desc(gn_part_out=PTR),
}
REFUSED = {
    "stride2": _strided(),
    "upsampled": _upsampled(H=32, W=32, Cin=1280, N=1280),
    "vhalo": _desc(vhalo=1),
    "corner_patch": _desc(corner_patch=8),
    "cin_mod_64": _desc(Cin=96, N=160),
    "n_mod_160": _desc(N=1024),
    "cin_valid": _desc(Cin=64, N=320, cin_valid=4),
    "width128": _desc(H=128, W=128, Cin=320, N=320),
    "width16": _desc(H=16, W=16, Cin=1280, N=1280),
    "hw_mod_256": _desc(B=1, H=12, W=32, Cin=64, N=160),
    "activation": _desc(flags=L.EPI_SILU),
    "forced_splitk": _desc(splitk=2),
    "ldc_mod_8": _desc(ldc=1284),
    # the two shapes of the SDXL step that did not count as faster in the per-shape A/B (profiles/conv_halo_ab.txt)
    "ab_width32_cin640": _desc(Cin=640, N=1280),
    "ab_width64_cin320": _desc(H=64, W=64, Cin=320, N=640),
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_serves_accepts(name):
    lds = L.load().mx_conv3x3_halo_serves(C.byref(ACCEPTED[name]))
    assert 0 < lds <= LDS_LIMIT, (name, lds)


@pytest.mark.parametrize("name", list(REFUSED))
def test_serves_refuses(name):
    assert L.load().mx_conv3x3_halo_serves(C.byref(REFUSED[name])) == 0, name


def test_serves_refuses_a_grouped_launch():
    d, segs = _grouped()
    assert L.load().mx_conv3x3_halo_serves(C.byref(d)) == 0
    assert L.load().mx_conv3x3_halo_serves(None) == 0


def test_lds_bytes_are_the_staged_buffers_the_weight_ring_and_the_zero_lines():
    l = L.load()
    for W, H in ((32, 32), (64, 64)):
        lines = (256 // W + 2) * W
        assert l.mx_conv3x3_halo_serves(C.byref(_desc(H=H, W=W, Cin=640, N=640))) == 2 * lines * 128 + 3 * 160 * 128 + 256


def test_entry_refuses_what_serves_refuses():
    """no device is touched: the refusal comes before anything is launched"""
    l = L.load()
    for name, d in REFUSED.items():
        assert l.mx_conv3x3_halo(None, C.byref(d)) != 0, name
        assert b"mx_conv3x3_halo_serves" in l.mx_last_error(), name


def test_served_descriptors_keep_their_route():
    """the entry stands beside mx_conv3x3: a served descriptor still resolves to the 256 x 160 conv tile there"""
    for name in ("width32_1280", "width64_640", "rowbias"):
        assert L.gemm_kernels_of(ACCEPTED[name], True)[0].startswith("gemm_v5_kernel<160, 4, true"), name
