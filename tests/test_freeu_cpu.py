"""Host side of FreeU: the argument checks of mx_freeu, the slab route with its addition chain, and the all-four-non-zero rule of mx_unet_set_freeu
seen through the sizing walk.  No GPU: every call returns before a launch."""
import ctypes as C

import pytest

from oracle import sdxl_unet_ref as ref  # (parameters only)
from sduss_amd import lib, ops, weights
from sduss_amd.config import UNetConfig
from sduss_amd.unet import config_c


def _problems(n=1, H=4, W=6, skip=1 << 20, hidden=3 << 20):
    arr = (lib.FreeUProblem * n)()
    for a in arr:
        a.skip, a.skip_out, a.hidden, a.B, a.H, a.W = skip, 2 << 20, hidden, 2, H, W
    return arr


@pytest.mark.parametrize("what,kw,c_skip,c_hidden", [
    ("H, W >= 2", dict(H=1), 64, 64), ("H, W >= 2", dict(W=1), 64, 64), ("multiple of 16", {}, 72, 64), ("multiple of 16", {}, 64, 40),
    ("16-byte aligned", dict(skip=(1 << 20) + 8), 64, 64), ("MX_MAX_SEGS", dict(n=lib.MAX_SEGS + 1), 64, 64),
    ("not overlap", dict(hidden=(2 << 20) + 4096), 64, 64)])
def test_bad_arguments_are_refused_by_name(what, kw, c_skip, c_hidden):
    l = lib.load()
    assert l.mx_freeu(None, _problems(**kw), kw.get("n", 1), c_skip, c_hidden, 0.9, 1.2) != 0 and what.encode() in l.mx_last_error(), l.mx_last_error()


# the seven test shapes at batch 3 (16-channel slabs: too few workgroups for a wider one), the other side of the staging switch, and a wide SDXL-base
# launch at 8 x 1024 px: (B, H, W, C) -> (slab, staged, wseg + items per lane + 6)
@pytest.mark.parametrize("B,H,W,C,slab,staged,chain", [
    (3, 2, 2, 64, 16, 1, 8), (3, 2, 8, 64, 16, 1, 8), (3, 3, 5, 320, 16, 1, 9), (3, 4, 6, 64, 16, 1, 9), (3, 24, 24, 320, 16, 1, 19),
    (3, 32, 32, 64, 16, 1, 23), (3, 64, 64, 64, 16, 1, 71), (3, 64, 66, 64, 16, 0, 73), (8, 32, 32, 1280, 32, 1, 23)])
def test_route(B, H, W, C, slab, staged, chain):
    got = ops.freeu_route([(B, H, W)], C)
    assert (got[0], got[1][0], got[2][0]) == (slab, staged, chain)


def test_set_freeu_needs_all_four_and_the_walks_count_it():
    cfg = UNetConfig.tiny()
    l, pw = lib.load(), weights.PackedWeights(weights.pack(cfg, ref.init_params(ref.UNetConfig.tiny())), "cpu")
    h = l.mx_unet_create(C.byref(config_c(cfg)))
    assert h and l.mx_unet_set_weights(h, pw.blob.data_ptr(), pw.blob.numel(), pw.table, len(pw.names)) == 0
    plain = l.mx_unet_workspace_bytes(h, 2, 16, 16, 77)
    for zero in range(4):                          # any zero: off, as in diffusers
        f = [0.9, 0.2, 1.3, 1.4]
        f[zero] = 0.0
        assert l.mx_unet_set_freeu(h, *f) == 0 and l.mx_unet_workspace_bytes(h, 2, 16, 16, 77) == plain
    assert l.mx_unet_set_freeu(h, 0.9, 0.2, 1.3, 1.4) == 0
    assert l.mx_unet_validate(h, 2, 16, 16, 77) == 0, l.mx_last_error()
    # up block 0: 2 x 4 x 4 x 256 and up block 1: 2 x 8 x 8 x 128 bf16 (the widest skip of each)
    assert l.mx_unet_workspace_bytes(h, 2, 16, 16, 77) >= plain + 2 * (16 * 256 + 64 * 128) * 2
    l.mx_unet_destroy(h)
