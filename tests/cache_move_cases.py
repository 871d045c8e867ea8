"""The cases of the block-skip cache's data kernels (tests/test_cache_move_cpu.py, tests/test_cache_move_gpu.py): plain data and the operand
builder, shared by the CPU and the GPU tests.  The smallest shapes at which each kernel can still go wrong.

Inputs are random bf16 BIT PATTERNS: finite, exponents spread over 2^-12 .. 2^12, so that a value read from a wrong place is a wrong value.

Sample table A (patch edge P0 = 8 at level 0): (24, 24) -- a 3 x 3 patch grid, with an interior patch; (16, 24) -- not square, 2 x 3; (8, 8) -- one
patch, every halo is the image border.  Slots [3, 0, 4] of 5 state rows: not the identity, with gaps.  Levels 0, 1, 2: patch edge 8, 4, 2.
The patch list is unsorted and incomplete: the four corner patches, one edge patch and the interior patch of the 3 x 3 grid, two patches of the
non-square image, the single patch.
Channels: 8 (one 16-byte vector), 24 (three: not a power of two), 320 at level 0 (a patch row of 10 x 40 or 8 x 40 vectors: more than the 256
threads of a block, so the inner loops take a second trip)."""
import numpy as np
import torch

P0 = 8
TABLE_A = [(24, 24, 3), (16, 24, 0), (8, 8, 4)]          # (h, w, slot) at level 0
SLOTS_A = 5
PATCHES_A = [(0, 2, 2), (1, 0, 1), (0, 0, 0), (0, 1, 1), (2, 0, 0), (0, 0, 2), (1, 1, 2), (0, 2, 0), (0, 1, 0)]      # (sample, py, px)
# grid-stride tails: the largest image has 32 * 32 * 320 / 8 = 40960 vectors > 128 blocks x 256 threads; the (8, 8) sample leaves blocks idle
TABLE_BIG = [(32, 32, 1), (8, 8, 0)]
# more than 256 blocks x 4 rows = 1024 token rows in one image
TABLE_ROWS = [(40, 32, 1), (8, 8, 0)]
TABLE_WIDE = [(8, 8, 2), (8, 16, 0)]                     # for C = 520: 65 vectors a row, only lane 0 takes a second trip
# MMDiT (mmdit_sd3.cpp, the chunk cache's sample tables): a sample is a token sequence {row0, L, 1, slot, 1}; image streams of two lengths, context rows
MMDIT_IMG = [(36, 1, 2), (16, 1, 0), (36, 1, 1)]
MMDIT_CTX = [(5, 1, 2), (5, 1, 0), (5, 1, 1)]
MMDIT_SLOTS = 3

GATHER_MODES = [(0, 0, 0), (1, 1, 0), (2, 0, 0), (1, 1, 1)]          # (halo_lo, halo_hi, up): the four the plan uses


def _gather_cases():
    out = []
    for C in (8, 24):
        for level in (0, 1, 2):
            for mode in GATHER_MODES:
                out.append(dict(name=f"c{C}_l{level}_h{mode[0]}{mode[1]}_u{mode[2]}", C=C, level=level, mode=mode, ld_pad=0))
    out += [dict(name=f"c320_l0_h{m[0]}{m[1]}_u{m[2]}", C=320, level=0, mode=m, ld_pad=0) for m in GATHER_MODES]
    out.append(dict(name="c24_l0_h11_u0_ld32", C=24, level=0, mode=(1, 1, 0), ld_pad=8))
    out.append(dict(name="c24_l1_h11_u1_ld32", C=24, level=1, mode=(1, 1, 1), ld_pad=8))
    return out


GATHER_CASES = _gather_cases()
# pc_scatter: (Ps, o0) = (p, 0) the bare patch; (p + 2, 1) the stride-1 conv's halo'd output; (p + 1, 1) the stride-2 conv's: its input patch of 2p
# pixels carries halo (2, 0), P = 2p + 2, and pc_conv computes Po = (P + 1) / 2 = (2p + 3) / 2
SCATTER_KINDS = {"bare": lambda p: (p, 0), "halo": lambda p: (p + 2, 1), "stride2": lambda p: ((2 * p + 3) // 2, 1)}
SCATTER_CASES = [dict(name=f"c{C}_l{level}_{k}", C=C, level=level, kind=k) for C in (8, 24) for level in (0, 1, 2) for k in SCATTER_KINDS] + \
                [dict(name=f"c320_l0_{k}", C=320, level=0, kind=k) for k in SCATTER_KINDS]
PATCH_CASES = [dict(name=f"c{C}_l{level}", C=C, level=level) for C in (8, 24) for level in (0, 1, 2)] + [dict(name="c320_l0", C=320, level=0)]


def _image_copy_cases():
    A = dict(table=TABLE_A, slots=SLOTS_A)
    out = [dict(name=f"store_c{C}_l{level}", C=C, level=level, to_batch=0, **A) for C in (8, 24) for level in (0, 1, 2)]
    for C, level in ((8, 0), (24, 1), (24, 2)):
        out += [dict(name=f"load_c{C}_l{level}", C=C, level=level, to_batch=1, **A),
                dict(name=f"load_res_c{C}_l{level}", C=C, level=level, to_batch=1, residual=True, **A),
                dict(name=f"load_vec_c{C}_l{level}", C=C, level=level, to_batch=1, vec=True, **A),
                dict(name=f"load_vec_res_c{C}_l{level}", C=C, level=level, to_batch=1, vec=True, residual=True, **A),
                dict(name=f"load_gate_c{C}_l{level}", C=C, level=level, to_batch=1, vec=True, gate=1, **A),
                dict(name=f"load_gate_res_c{C}_l{level}", C=C, level=level, to_batch=1, vec=True, residual=True, gate=1, **A)]
    out.append(dict(name="load_gate_cancel_c24_l0", C=24, level=0, to_batch=1, vec=True, residual=True, gate=1, cancel=True, **A))
    big = dict(table=TABLE_BIG, slots=2, C=320, level=0)
    out += [dict(name="store_tail", to_batch=0, **big), dict(name="load_tail_vec_res", to_batch=1, vec=True, residual=True, **big),
            dict(name="load_tail_gate_res", to_batch=1, vec=True, residual=True, gate=1, **big)]     # 330 000 cells through the gate
    for nm, tab in (("img", MMDIT_IMG), ("ctx", MMDIT_CTX)):
        m = dict(table=tab, slots=MMDIT_SLOTS, C=24, level=0, ldvec=6 * 24 + 8)
        out += [dict(name=f"mmdit_{nm}_store", to_batch=0, **m), dict(name=f"mmdit_{nm}_load", to_batch=1, **m),
                dict(name=f"mmdit_{nm}_gate_res", to_batch=1, vec=True, residual=True, gate=1, **m)]
    return out


IMAGE_COPY_CASES = _image_copy_cases()
ROWS_STATS_CASES = [dict(name="a_c24_l0", table=TABLE_A, slots=SLOTS_A, C=24, level=0, stats=True, fin=True),
                    dict(name="a_c8_l1", table=TABLE_A, slots=SLOTS_A, C=8, level=1, stats=True, fin=True),
                    dict(name="rows1280_c8", table=TABLE_ROWS, slots=2, C=8, level=0, stats=True, fin=True),
                    dict(name="c520_stats", table=TABLE_WIDE, slots=3, C=520, level=0, stats=True, fin=False),
                    dict(name="c520_fin", table=TABLE_WIDE, slots=3, C=520, level=0, stats=False, fin=True),
                    dict(name="c520_both", table=TABLE_WIDE, slots=3, C=520, level=0, stats=True, fin=True)]
# token ranges (row0, rows, slot, srow0) over a batch of `rows` rows and `slots` state rows of `srows` rows.  small: 15 vectors (below the 64 chunks),
# 111 (not a multiple of 64), two ranges in one slot, srow0 != 0, one range equal to its cached rows (eq).  big: 40960 vectors beside 15
RANGE_SETS = {
    "small": dict(C=24, rows=120, slots=3, srows=64, ranges=[(70, 37, 2, 11), (3, 5, 0, 40), (20, 5, 2, 55), (30, 32, 1, 0)], eq=3),
    "mid": dict(C=64, rows=260, slots=2, srows=230, ranges=[(50, 200, 1, 30), (0, 8, 0, 1)], eq=1),
    "big": dict(C=320, rows=1040, slots=2, srows=1030, ranges=[(10, 1024, 1, 6), (1034, 5, 0, 3)], eq=1),
}
RANGE_COPY_CASES = [dict(name=f"{s}_{'load' if t else 'store'}", set=s, to_batch=t) for s in RANGE_SETS for t in (0, 1)]
RANGE_SQ_CASES = [dict(name=s, set=s) for s in RANGE_SETS]
# per-request pair: sample i against row slot[i]; 100 vectors (per = 2: chunks 50.. are empty), 20000 (per = 313: a second trip)
SQ_PARTIAL_CASES = [dict(name=f"v{v}_{'slots' if s else 'direct'}", vectors=v, slot=[3, 0, 4] if s else None, slots=5 if s else 3, eq=1)
                    for v in (100, 20000) for s in (True, False)]
# rows of 3 vectors, and of 66000 (more than 256 blocks x 256 threads); the middle sample has slot < 0: neither side may change for it
COPY_ROWS_CASES = [dict(name=f"v{v}_{'scatter' if sc else 'gather'}", vectors=v, slot=[2, -1, 0], slots=3, scatter=sc) for v in (3, 66000) for sc in (1, 0)]

# the composite of pc_conv's two routes: the (24, 24) and (16, 24) samples of table A, every patch asking, in pc_all's order
CONV_TABLE = TABLE_A[:2]
CONV_PATCHES = [(b, py, px) for b, (h, w, _s) in enumerate(CONV_TABLE) for py in range(h // P0) for px in range(w // P0)]
CONV_CIN, CONV_N = 64, 128
CONV_MODES = {"stride1": dict(stride=1, up=0), "stride2": dict(stride=2, up=0), "up": dict(stride=1, up=1)}


def rand_bf16(gen, shape, emin=-12, emax=12):
    """random finite bf16 bit patterns: any sign and mantissa, exponent 2^emin .. 2^emax"""
    n = int(np.prod(shape))
    sign = torch.randint(0, 2, (n,), generator=gen).numpy().astype(np.uint16) << 15
    expo = torch.randint(127 + emin, 128 + emax, (n,), generator=gen).numpy().astype(np.uint16) << 7
    man = torch.randint(0, 128, (n,), generator=gen).numpy().astype(np.uint16)
    return torch.from_numpy((sign | expo | man).view(np.int16)).view(torch.bfloat16).reshape(shape)


def seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (1 << 31)


def level0_rows(table):
    return sum(h * w for h, w, _s in table)


def image_elems(table, level, C):
    """elements of the largest image at this level: what a state row holds"""
    return max((h >> level) * (w >> level) for h, w, _s in table) * C


def build_image_tensors(name, table, slots, level, C, ld_pad=0):
    """(generator, batch [rows, C + ld_pad], state [slots, elements of the largest image]) of random bits"""
    gen = torch.Generator().manual_seed(seed_of(name))
    rows = level0_rows(table) >> (2 * level)
    return gen, rand_bf16(gen, (rows, C + ld_pad)), rand_bf16(gen, (slots, image_elems(table, level, C)))


# ---- operands (CPU tensors; the GPU test uploads them into guarded / NaN-padded buffers) ----

def build_gather(c):
    _gen, src, _ = build_image_tensors("gather_" + c["name"], TABLE_A, SLOTS_A, c["level"], c["C"], c["ld_pad"])
    return dict(src=src, p=(P0 >> c["level"]) << c["mode"][2])


def build_scatter(c):
    p = P0 >> c["level"]
    Ps, o0 = SCATTER_KINDS[c["kind"]](p)
    gen, _, state = build_image_tensors("scatter_" + c["name"], TABLE_A, SLOTS_A, c["level"], c["C"])
    return dict(state=state, src=rand_bf16(gen, (len(PATCHES_A) * Ps * Ps, c["C"])), p=p, Ps=Ps, o0=o0)


def build_patch(c, equal_patch=None):
    """batch x and state for pc_patch_store / pc_patch_sq_diff; equal_patch: that entry of PATCHES_A holds its cached value in x"""
    gen, x, state = build_image_tensors("patch_" + c["name"], TABLE_A, SLOTS_A, c["level"], c["C"])
    p = P0 >> c["level"]
    if equal_patch is not None:
        b, py, px = PATCHES_A[equal_patch]
        h, w, slot = TABLE_A[b][0] >> c["level"], TABLE_A[b][1] >> c["level"], TABLE_A[b][2]
        row0 = sum(hh * ww for hh, ww, _s in TABLE_A[:b]) >> (2 * c["level"])
        img = x[row0:row0 + h * w].view(h, w, c["C"])
        img[py * p:(py + 1) * p, px * p:(px + 1) * p] = state[slot, :h * w * c["C"]].view(h, w, c["C"])[py * p:(py + 1) * p, px * p:(px + 1) * p]
    return dict(x=x, state=state, p=p)


def build_image_copy(c):
    gen, batch, state = build_image_tensors("image_copy_" + c["name"], c["table"], c["slots"], c["level"], c["C"])
    out = dict(batch=batch, state=state, residual=None, vec=None)
    if c.get("residual"):
        out["residual"] = rand_bf16(gen, tuple(batch.shape))
    if c.get("vec"):
        # one row per batch POSITION; as many rows as there are slots, so that a kernel that indexed it by slot would read a wrong row, not fault
        ldvec = c.get("ldvec", c["C"] + 8)
        vec = torch.full((max(len(c["table"]), c["slots"]), ldvec), float("nan"))
        vec[:, :c["C"]] = torch.randn((vec.shape[0], c["C"]), generator=gen) * 1.5
        out["vec"] = vec
    if c.get("cancel"):
        # the residual nearly cancels the gated state: the fused and the unfused evaluation of state * vec + residual then differ by a visible
        # part of the result, and the two candidates of the reference part in about one cell of a hundred
        row0 = 0
        for i, (h, w, slot) in enumerate(c["table"]):
            n = (h >> c["level"]) * (w >> c["level"])
            r0 = row0 >> (2 * c["level"])
            out["residual"][r0:r0 + n] = (-(state[slot, :n * c["C"]].view(n, c["C"]).float() * out["vec"][i, :c["C"]])).to(torch.bfloat16)
            row0 += h * w
    return out


def build_rows_stats(c):
    gen, batch, state = build_image_tensors("rows_stats_" + c["name"], c["table"], c["slots"], c["level"], c["C"])
    return dict(batch=batch, state=state, residual=rand_bf16(gen, tuple(batch.shape)))


def build_ranges(set_name, equal=False):
    s = RANGE_SETS[set_name]
    gen = torch.Generator().manual_seed(seed_of("ranges_" + set_name))
    batch, state = rand_bf16(gen, (s["rows"], s["C"])), rand_bf16(gen, (s["slots"], s["srows"] * s["C"]))
    if equal:
        row0, rows, slot, srow0 = s["ranges"][s["eq"]]
        batch[row0:row0 + rows] = state[slot, srow0 * s["C"]:(srow0 + rows) * s["C"]].view(rows, s["C"])
    return dict(batch=batch, state=state, C=s["C"], ranges=s["ranges"])


def build_sq_partial(c):
    gen = torch.Generator().manual_seed(seed_of("sq_partial_" + c["name"]))
    a, b = rand_bf16(gen, (3, 8 * c["vectors"])), rand_bf16(gen, (c["slots"], 8 * c["vectors"]))
    a[c["eq"]] = b[c["slot"][c["eq"]] if c["slot"] else c["eq"]]
    return dict(a=a, b=b)


def build_copy_rows(c):
    gen = torch.Generator().manual_seed(seed_of("copy_rows_" + c["name"]))
    return dict(batch=rand_bf16(gen, (len(c["slot"]), 8 * c["vectors"])), slotted=rand_bf16(gen, (c["slots"], 8 * c["vectors"])))
