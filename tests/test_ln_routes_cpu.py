"""By which route each of the SDXL transformer block's three folded LayerNorms reaches its consuming GEMM (sduss_amd/csrc/ln_route.h: a normalisation
pass, the producer's statistics slabs, or its finalised (mean, rstd)): mx_unet_ln_routes, the function the step plan itself asks, answers over a sweep
what the plan's nine booleans answered before the decision had a place of its own (tests/golden/ln_routes.json, recorded by running that block of
Plan::transformer(), lifted unchanged, against the library of the commit before).  Host only: without a device cu_count() is the MI355X's 256 CUs,
which is what the table was recorded with."""
import ctypes as C
import itertools
import json
import os

import pytest

from sduss_amd import lib as L

PASS, SLABS, FINAL = 0, 1, 2
PLAIN, PATCH_PARALLEL, PATCH_CACHE = 0, 1, 2          # the table's modes = the query's flag bits 0, 1, 2
TICKETS = 4
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_routes.json")


@pytest.fixture(scope="module")
def table():
    """{(C, M, layers, n_groups, mode, tickets): (norm1, norm2, norm3, norm3_from_merge)}"""
    with open(TABLE) as f:
        t = json.load(f)
    keys = list(itertools.product(t["C"], t["M"], t["layers"], t["n_groups"], range(len(t["modes"])), t["tickets"]))
    assert len(keys) == len(t["routes"])
    return dict(zip(keys, map(tuple, t["routes"])))


def test_sweep_is_the_stated_one(table):
    Cs, Ms, layers, groups, modes, tickets = (sorted(set(k[i] for k in table)) for i in range(6))
    assert Cs == [64, 128, 256, 320, 640, 1280]
    assert Ms == sorted([256 << i for i in range(9)] + [1728, 2304, 8000])
    assert (layers, groups, modes, tickets) == ([1, 2, 10], [1, 3], [PLAIN, PATCH_PARALLEL, PATCH_CACHE], [0, 1])


def test_sweep_reaches_every_route(table):
    """conditions on the sweep itself, checked on the recorded answers"""
    rows = table.items()
    assert {v[0] for _, v in rows} == {PASS, SLABS, FINAL}
    assert {v[1] for _, v in rows} == {PASS, SLABS}                                   # norm2 never finalises
    assert {v[2] for _, v in rows} == {PASS, SLABS, FINAL}
    assert {v[2:] for k, v in rows if k[4] == PATCH_CACHE} == {(PASS, 0), (SLABS, 0), (FINAL, 1)}     # under the patch cache Final comes from the merge kernel
    assert all(v[3] == 0 for k, v in rows if k[4] != PATCH_CACHE)
    assert all(v[0] != FINAL for k, v in rows if k[3] > 1)                            # a grouped launch never finalises norm1
    assert any(v[2] == FINAL for k, v in rows if k[3] > 1)                            # ... norm3's consumer is one launch whatever the mix
    assert all(FINAL not in v[:3] for k, v in rows if k[4] == PATCH_PARALLEL)         # patch-parallel never finalises anything
    assert all(FINAL not in v[:3] for k, v in rows if k[5] == 0)                      # nor does a plan without tickets


def test_plain_grid_reaches_each_region(table):
    """one request mix, one group, tickets: the regions of (C, M) the plan's routes fall into"""
    at = lambda Cw, M, layers=2: table[(Cw, M, layers, 1, PLAIN, 1)][:3]
    assert at(1280, 4096) == (PASS, SLABS, PASS)                 # the consumers prefer a pass, the producers cannot finalise
    assert at(1280, 8192) == (FINAL, SLABS, FINAL)
    assert at(1280, 32768) == (FINAL, PASS, FINAL)               # norm2 as a pass: only here and at C = 256, M = 65536
    assert {k[:2] for k, v in table.items() if v[1] == PASS and k[3:] == (1, PLAIN, 1)} == {(1280, 32768), (1280, 65536), (256, 65536)}
    for M in (2048, 4096, 8192):
        assert at(640, M) == (SLABS, SLABS, PASS)
    assert at(640, 16384) == (SLABS, SLABS, FINAL)
    for Cw in (64, 128, 256):
        for M in (256, 512, 1024, 1728, 2048, 2304, 4096):
            assert at(Cw, M) == (SLABS, SLABS, SLABS)


def test_routes_the_gpu_tests_reach(table):
    """SDXL-base on a 32 x 32 latent holds 256 tokens an image at its 640-wide level (2 layers) and 64 at the 1280-wide one (10 layers), four times as
    many on a 64 x 64 latent.  tests/test_unet_gpu.py: test_unet_full_width_sdxl_batch8 (8 x 32 x 32) takes Pass and Slabs;
    test_unet_full_width_sdxl_finalised_statistics (32 x 64 x 64) takes Final for norm3 at both widths and for norm1 at the 1280-wide level (the
    640-wide q|k|v projection, N = 1920, never runs on the 256 x 256 kernel: its norm1 stays on the slabs)."""
    at = lambda Cw, M, layers: table[(Cw, M, layers, 1, PLAIN, 1)][:3]
    assert at(640, 8 * 256, 2) == (SLABS, SLABS, PASS) and at(1280, 8 * 64, 10) == (SLABS, SLABS, SLABS)
    assert at(640, 32 * 1024, 2) == (SLABS, SLABS, FINAL) and at(1280, 32 * 256, 10) == (FINAL, SLABS, FINAL)


def test_routes_match_the_recorded_table(table):
    lib = L.load()
    out = (C.c_int * 4)()
    wrong = []
    for (Cw, M, layers, groups, mode, tickets), want in table.items():
        flags = (mode and 1 << (mode - 1)) | (TICKETS if tickets else 0)
        assert lib.mx_unet_ln_routes(M, Cw, layers, groups, flags, out) == 0
        if tuple(out) != want:
            wrong.append(((Cw, M, layers, groups, mode, tickets), tuple(out), want))
    assert not wrong, f"{len(wrong)} of {len(table)} shapes take another route, first: {wrong[:5]}"


def test_bad_arguments_are_refused():
    lib = L.load()
    out = (C.c_int * 4)()
    for M, Cw, layers, groups in ((0, 640, 2, 1), (2048, 100, 2, 1), (2048, 640, 0, 1), (2048, 640, 2, 0), (2048, 640, 2, 5)):
        assert lib.mx_unet_ln_routes(M, Cw, layers, groups, 0, out) != 0
        assert lib.mx_last_error().decode() == "unet_ln_routes: bad arguments"
    assert lib.mx_unet_ln_routes(2048, 640, 2, 1, 0, None) != 0
