"""Host half of the block-skip cache's kernel tests (tests/test_cache_move_gpu.py): the references of tests/cache_move_ref.py against the literal
patch pipeline of oracle/patch_ref.py, the cases of tests/cache_move_cases.py against a list of deliberately wrong references (each must be
told apart from the true one by at least one case), and the ctypes tables of sduss_amd/lib.py against the structs include/mxdenoise.h declares."""
import ctypes as C
import os
import re
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import cache_move_cases as K
import cache_move_ref as R
from oracle import patch_ref as pr
from sduss_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [K.TABLE_A[0], K.TABLE_A[2]]             # the square samples: what split_sample takes
ALL = lambda table: [(b, py, px) for b, (h, w, _s) in enumerate(table) for py in range(h // K.P0) for px in range(w // K.P0)]


def _pipeline(src, Cc, level, up):
    """split_sample -> (interpolate) -> mock_groupnorm on the square samples: [N, P, P, C] fp32, every patch in (sample, row, column) order"""
    geo = R.geometry(SQUARE, level, K.P0)
    samples = {str(8 * g.h): R.batch_image(src, g, Cc).float().permute(2, 0, 1)[None] for g in geo}
    pidx, _lat, _res, patches, _map = pr.split_sample(samples, 8 * geo[0].p)
    inner = patches[:, :, 1:-1, 1:-1]
    if up:
        inner = F.interpolate(inner, scale_factor=2.0, mode="nearest")           # as cache_patch_ref._sampler does
    return pr.mock_groupnorm(inner, pidx).permute(0, 2, 3, 1)


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("up", [0, 1])
def test_gather_ref_is_the_literal_patch_pipeline(level, up):
    Cc = 8
    gen = torch.Generator().manual_seed(11 + level + 7 * up)
    src = K.rand_bf16(gen, (K.level0_rows(SQUARE) >> (2 * level), Cc))
    geo = R.geometry(SQUARE, level, K.P0)
    p = geo[0].p << up
    got = R.gather_ref(src, Cc, geo, ALL(SQUARE), p, 1, 1, up)
    want = _pipeline(src, Cc, level, up)
    assert got.shape == want.shape
    assert torch.equal(R.bits(got), R.bits(want.to(torch.bfloat16))) and torch.equal(got.float(), want)
    bare = R.gather_ref(src, Cc, geo, ALL(SQUARE), p, 0, 0, up)
    assert torch.equal(bare.float(), want[:, 1:-1, 1:-1])


# ---- deliberately wrong references ----

def _wrong_halo_patch(kind, img, py, px, p):
    H, W, Cc = img.shape
    y0, x0 = py * p, px * p
    out = R.halo_patch(img, py, px, p)
    if kind == "border":                          # a border halo that is not zero: the patch's own edge pixels repeated outwards
        if y0 == 0:
            out[0] = out[1]
        if y0 + p == H:
            out[p + 1] = out[p]
        if x0 == 0:
            out[:, 0] = out[:, 1]
        if x0 + p == W:
            out[:, p + 1] = out[:, p]
    elif kind == "diag":                          # corners from the diagonal neighbour's pixel
        for yo, ys in ((0, y0 - 1), (p + 1, y0 + p)):
            for xo, xs in ((0, x0 - 1), (p + 1, x0 + p)):
                out[yo, xo] = img[ys, xs] if 0 <= ys < H and 0 <= xs < W else 0
    elif kind == "swap":                          # top and bottom neighbours swapped
        top, bottom = out[0, 1:p + 1].clone(), out[p + 1, 1:p + 1].clone()
        out[0, 1:p + 1], out[p + 1, 1:p + 1] = bottom, top
    return out


def _wrong_gather(kind, src, Cc, geo, patches, p, lo, hi, up):
    out = []
    for b, py, px in patches:
        img = R.batch_image(src, geo[b], Cc)
        if up:
            if kind == "up_round_up":             # source pixel (i + 1) >> 1 instead of i >> 1
                iy = ((torch.arange(2 * img.shape[0]) + 1) >> 1).clamp_max(img.shape[0] - 1)
                ix = ((torch.arange(2 * img.shape[1]) + 1) >> 1).clamp_max(img.shape[1] - 1)
                img = img[iy][:, ix]
            else:
                img = R.nearest_2x(img)
        h11 = _wrong_halo_patch(kind, img, py, px, p) if kind in ("border", "diag", "swap") else R.halo_patch(img, py, px, p)
        if lo == 2 and kind == "ring_behind":     # the zero ring behind instead of in front
            o = torch.zeros_like(h11)
            o[:-1, :-1] = h11[1:, 1:]
        else:
            o = h11[1:-1, 1:-1] if lo == 0 else h11 if lo == 1 else R.ring_in_front(h11)
        out.append(o)
    return torch.stack(out)


@pytest.mark.parametrize("kind", ["diag", "swap", "border", "ring_behind", "up_round_up"])
def test_gather_cases_reject_a_wrong_gather(kind):
    told = []
    for c in K.GATHER_CASES:
        o = K.build_gather(c)
        geo = R.geometry(K.TABLE_A, c["level"], K.P0)
        args = (o["src"], c["C"], geo, K.PATCHES_A, o["p"], *c["mode"])
        if not torch.equal(R.bits(R.gather_ref(*args)), R.bits(_wrong_gather(kind, *args))):
            told.append(c["name"])
    print(f"{kind}: told apart by {len(told)} of {len(K.GATHER_CASES)} cases")
    assert told, f"no gather case tells the '{kind}' mistake from the reference"


def _slot_is_position(geo):
    for i, g in enumerate(geo):
        g.slot = i
    return geo


def test_cases_reject_the_slot_taken_as_batch_index():
    """pc_scatter, pc_patch_store, pc_image_copy (both directions): a reference that takes state row b for sample b differs in some case"""
    n = {"scatter": 0, "patch_store": 0, "store": 0, "load": 0}
    for c in K.SCATTER_CASES:
        o = K.build_scatter(c)
        args = lambda geo: (o["state"], o["src"], o["Ps"], o["o0"], c["C"], geo, K.PATCHES_A, o["p"])
        n["scatter"] += not torch.equal(R.bits(R.scatter_ref(*args(R.geometry(K.TABLE_A, c["level"], K.P0)))),
                                        R.bits(R.scatter_ref(*args(_slot_is_position(R.geometry(K.TABLE_A, c["level"], K.P0))))))
    for c in K.PATCH_CASES:
        o = K.build_patch(c)
        args = lambda geo: (o["state"], o["x"], c["C"], geo, K.PATCHES_A, o["p"])
        n["patch_store"] += not torch.equal(R.bits(R.patch_store_ref(*args(R.geometry(K.TABLE_A, c["level"], K.P0)))),
                                            R.bits(R.patch_store_ref(*args(_slot_is_position(R.geometry(K.TABLE_A, c["level"], K.P0))))))
    for c in K.IMAGE_COPY_CASES:
        o = K.build_image_copy(c)
        run = lambda geo: R.image_copy_ref(o["batch"], o["state"], c["C"], geo, c["to_batch"], o["vec"], o["residual"], c.get("gate", 0))
        a, b = run(R.geometry(c["table"], c["level"], K.P0)), run(_slot_is_position(R.geometry(c["table"], c["level"], K.P0)))
        if c["to_batch"]:
            n["load"] += not (torch.equal(R.bits(a[0]), R.bits(b[0])) or torch.equal(R.bits(a[1]), R.bits(b[0])))
        else:
            n["store"] += not torch.equal(R.bits(a), R.bits(b))
    print(n)
    assert all(v > 0 for v in n.values()), n


def test_cases_reject_the_vector_indexed_by_slot():
    """pc_image_copy with a time-embedding / gate row: a reference that reads vec[slot] instead of vec[batch position] differs"""
    told = 0
    for c in K.IMAGE_COPY_CASES:
        if not c.get("vec"):
            continue
        o = K.build_image_copy(c)
        geo = R.geometry(c["table"], c["level"], K.P0)
        by_slot = o["vec"][[g.slot for g in geo]]
        a = R.image_copy_ref(o["batch"], o["state"], c["C"], geo, 1, o["vec"], o["residual"], c.get("gate", 0))
        b = R.image_copy_ref(o["batch"], o["state"], c["C"], geo, 1, by_slot, o["residual"], c.get("gate", 0))
        told += not (torch.equal(R.bits(a[0]), R.bits(b[0])) or torch.equal(R.bits(a[1]), R.bits(b[0])))
    assert told > 0


def _round_f32(q):
    """a Fraction rounded to fp32, to nearest, ties to even, in integer arithmetic (normal range)"""
    if q == 0:
        return 0.0
    s, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    m = q / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    n, r = divmod(m.numerator, m.denominator)
    if 2 * r > m.denominator or (2 * r == m.denominator and n & 1):
        n += 1
    return s * float(n) * 2.0 ** (e - 23)


def test_the_fused_candidate_of_the_gate_path_is_one_exact_rounding():
    """state * vec + residual with ONE rounding (cache_move_ref._fma_f32) against exact rational arithmetic, operands as the cases draw them and a
    few built to land on an fp32 tie after the fp64 sum; the unfused candidate differs from it somewhere, by no more than the product's own rounding and one step of the sum"""
    gen = torch.Generator().manual_seed(5)
    n = 4000
    a, c = K.rand_bf16(gen, (n,)).double(), K.rand_bf16(gen, (n,)).double()
    b = (torch.randn(n, generator=gen) * 1.5).double()
    # exact ties: a * b = 2^12 + 2^-11 (one fp32 step above 2^12), c = +-2^-12 (half a step)
    a[:2], b[:2], c[:2] = 2.0 ** 12, 1.0 + 2.0 ** -23, torch.tensor([2.0 ** -12, -2.0 ** -12], dtype=torch.float64)
    fused = R._fma_f32(a, b, c)
    exact = torch.tensor([_round_f32(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=torch.float64)
    assert torch.equal(fused.double(), exact)
    unfused = (a.float() * b.float()) + c.float()
    differ = fused != unfused
    assert 0 < int(differ.sum()) < n // 2
    # the product's own rounding (which a cancelling residual can magnify relative to the sum) and one step of the sum
    assert torch.all((fused.double() - unfused.double()).abs() <= 2.0 ** -24 * (a * b).abs() + 2.0 ** -23 * fused.double().abs())


def test_sq_diff_references_partition_and_terms():
    """the partial sums of a unit add up to the unit's whole sum; k comes from the shape: 8 per 16-byte vector one of the 256 threads visits"""
    assert R.sq_terms(1) == 8 and R.sq_terms(256) == 8 and R.sq_terms(257) == 16 and R.sq_terms(8 * 40) == 16
    o = K.build_ranges("small", equal=True)
    ref, bound = R.range_sq_diff_ref(o["batch"], o["state"], o["C"], o["ranges"])
    for i, (row0, rows, slot, srow0) in enumerate(o["ranges"]):
        d = o["batch"][row0:row0 + rows].double().reshape(-1) - o["state"][slot, srow0 * o["C"]:(srow0 + rows) * o["C"]].double()
        assert abs(float(ref[i].sum()) - float((d * d).sum())) <= 1e-12 * float((d * d).sum())
    eq = K.RANGE_SETS["small"]["eq"]
    assert float(ref[eq].sum()) == 0.0 and float(ref.sum()) > 0.0
    assert int((ref[1] != 0).sum()) == 15                       # 15 vectors: one per chunk, 49 empty chunks
    assert torch.all(bound == (8 + 3) * R.U32 * ref)


# ---- the tables ----

def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    body = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (name, name), hdr).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.match(r"(long long|int)\s+(.*)", decl).groups()
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("name,struct", [("mx_pc_sample", L.PcSample), ("mx_pc_patch", L.PcPatch), ("mx_pc_range", L.PcRange)])
def test_tables_match_the_header(name, struct):
    fields = _header_struct(name)
    ctypes_of = {"long long": C.c_longlong, "int": C.c_int}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(struct._fields_)
    size, align = 0, 1
    for _n, t in fields:                              # natural alignment, as the C ABI lays the struct out
        a = C.sizeof(ctypes_of[t])
        size = (size + a - 1) // a * a + a
        align = max(align, a)
    assert C.sizeof(struct) == (size + align - 1) // align * align
    assert C.sizeof(L.PcSample) == 24 and C.sizeof(L.PcPatch) == 16 and C.sizeof(L.PcRange) == 24


def test_entry_points_refuse_null_operands():
    """the one-launch entry points are bound and refuse null operands before anything is launched (no GPU needed)"""
    l = L.load()
    for name in ("mx_pc_image_copy", "mx_pc_rows_load_stats", "mx_pc_gather", "mx_pc_scatter", "mx_pc_patch_store", "mx_pc_patch_sq_diff", "mx_pc_range_copy",
                 "mx_pc_range_sq_diff", "mx_sq_diff_partial", "mx_copy_rows"):
        args = [0 if a in (C.c_int, C.c_int64, C.c_size_t) else 0.0 if a is C.c_float else None for a in L.SYMBOLS[name][1]]
        assert getattr(l, name)(*args) != 0 and l.mx_last_error(), name
