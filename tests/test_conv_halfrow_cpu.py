"""Host half of mx_conv3x3_halfrow (csrc/conv_halo.hip, the half-row form for 128-wide images): mx_conv3x3_halfrow_serves over a table of
descriptors (fake 16-byte-aligned pointers, no device), the LDS bytes it reports, and the entry's refusal of a descriptor it does not serve."""
import ctypes as C

import pytest

from sduss_amd import lib as L

PTR = 0x10000
LDS_LIMIT = 160 * 1024


def _desc(B=8, H=128, W=128, Cin=320, N=320, **over):
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
    "step_320": _desc(),                                                # the three 128-wide stride-1 shapes of the headline step, 8 images
    "step_cin640": _desc(Cin=640),
    "step_cin960": _desc(Cin=960),
    "one_row_block": _desc(B=1, H=4, Cin=64, N=160),                    # H == 4, Cin == 64, N == 160: the smallest of each
    "rowbias": _desc(rowbias=PTR, ldrb=320),
    "residual": _desc(residual=PTR),
    "gn_partials": _desc(gn_part_out=PTR),
}
REFUSED = {
    "width32": _desc(H=32, W=32, Cin=1280, N=1280),
    "width64": _desc(H=64, W=64, Cin=640, N=640),
    "width256": _desc(H=256, W=256),
    "h_mod_4": _desc(B=1, H=6, Cin=64, N=160),
    "stride2": _strided(),
    "upsampled": _upsampled(H=64, W=64, Cin=640, N=640),               # (the output is 128 wide)
    "upsampled_in128": _upsampled(),
    "vhalo": _desc(vhalo=1),
    "corner_patch": _desc(corner_patch=32),
    "cin_mod_64": _desc(Cin=96, N=160),
    "n_mod_160": _desc(N=256),
    "cin_valid": _desc(Cin=64, cin_valid=4),
    "activation": _desc(flags=L.EPI_SILU),
    "forced_splitk": _desc(splitk=2),
    "ldc_mod_8": _desc(ldc=324),
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_serves_accepts(name):
    lds = L.load().mx_conv3x3_halfrow_serves(C.byref(ACCEPTED[name]))
    assert 0 < lds <= LDS_LIMIT, (name, lds)


@pytest.mark.parametrize("name", list(REFUSED))
def test_serves_refuses(name):
    assert L.load().mx_conv3x3_halfrow_serves(C.byref(REFUSED[name])) == 0, name


def test_serves_refuses_a_grouped_launch_and_null():
    d, segs = _grouped()
    assert L.load().mx_conv3x3_halfrow_serves(C.byref(d)) == 0
    assert L.load().mx_conv3x3_halfrow_serves(None) == 0


def test_lds_bytes_are_the_staged_buffers_their_side_columns_the_weight_ring_and_the_zero_lines():
    """a staged buffer is 6 rows x 64 pixel lines and 6 side lines, padded to the 8 lines one wave-wide DMA writes"""
    side = 8
    want = 2 * (384 + side) * 128 + 3 * 160 * 128 + 256
    assert want == 162048 and want <= LDS_LIMIT
    for name in ("step_320", "step_cin960", "one_row_block"):
        assert L.load().mx_conv3x3_halfrow_serves(C.byref(ACCEPTED[name])) == want, name


def test_entry_refuses_what_serves_refuses():
    """no device is touched: the refusal comes before anything is launched"""
    l = L.load()
    for name, d in REFUSED.items():
        assert l.mx_conv3x3_halfrow(None, C.byref(d)) != 0, name
        assert b"mx_conv3x3_halfrow_serves" in l.mx_last_error(), name


def test_the_two_entries_do_not_overlap():
    """a descriptor is served by at most one of the staged entries: the plan's order of asking decides nothing"""
    l = L.load()
    for d in list(ACCEPTED.values()) + list(REFUSED.values()):
        assert not (l.mx_conv3x3_halo_serves(C.byref(d)) and l.mx_conv3x3_halfrow_serves(C.byref(d)))


def test_served_descriptors_keep_their_route():
    """the entry stands beside mx_conv3x3: a served descriptor still resolves to the 256 x 160 conv tile there"""
    for name in ("step_320", "step_cin640", "step_cin960", "rowbias"):
        assert L.gemm_kernels_of(ACCEPTED[name], True)[0].startswith("gemm_v5_kernel<160, 4, true"), name
