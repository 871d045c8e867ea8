"""The cases of the glue kernels' tests (tests/test_glue_cpu.py, tests/test_glue_gpu.py): the smallest shapes at which each kernel can still go
wrong, and the operands of each.  Operands are built on the CPU, once per (case, dtype); every value encodes its own position in its tensor
(coded()), so every cell has distinct bits and a misplaced cell cannot match by chance."""
import functools

import torch

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DTYPE_IDS = ["f32", "f16", "bf16"]
NAN = float("nan")
INF = float("inf")

N_BF16 = 2 * 0x7F80                       # the finite bf16 bit patterns, both signs, zeros and subnormals included


def _bf16_pattern(q):
    """q in [0, N_BF16) -> the q-th finite bf16 bit pattern (positive ones first), as int32"""
    return torch.where(q < 0x7F80, q, q - 0x7F80 + 0x8000)


def coded(shape, dtype, salt=0):
    """a tensor whose cell k holds a value made from k: distinct bits in every cell, and distinct bf16 bits after a rounding to bf16.
    bf16: the (k A + salt)-th finite pattern.  fp32: such a pattern (every second one) in the high half and k-dependent low bits, so roundings go
    both ways.  fp16: 16 k + (k mod 8) in the magnitude, alternating sign: the bf16 rounding drops three bits and keeps the cells apart."""
    n = 1
    for s in shape:
        n *= s
    k = torch.arange(n, dtype=torch.int64)
    if dtype == torch.bfloat16:
        assert n <= N_BF16
        q = (k * 40507 + 977 * salt) % N_BF16                                # 40507 is coprime to N_BF16 = 2^8 * 3 * 5 * 17
        return _bf16_pattern(q).to(torch.int16).view(torch.bfloat16).reshape(shape)
    if dtype == torch.float32:
        assert 2 * n <= N_BF16
        q = 2 * ((k * 20251 + 977 * salt) % (N_BF16 // 2))                   # 20251 is prime
        hi = _bf16_pattern(q)                                                # even patterns: the largest, 0x7F7E, rounds up to a finite value at most
        lo = (k * 25173 + 13849) % 65536
        return ((hi << 16) | lo).to(torch.int32).view(torch.float32).reshape(shape)
    assert dtype == torch.float16 and 16 * n + 8 < 2 * 0x7C00
    m = 16 * ((k * 1031 + 7 * salt) % (2 * 0x7C00 // 16)) + (k % 8)
    pat = torch.where(m < 0x7C00, m, m - 0x7C00 + 0x8000)
    return pat.to(torch.int16).view(torch.float16).reshape(shape)


def moderate_bf16(shape, salt=0):
    """bf16 values of magnitude 2^-4 .. 2^4, either sign (2048 patterns), cell (r, c) of a [rows, cols] table drawing pattern
    (389 r + 7 c + salt) mod 2048: rows differ from each other in EVERY column, and a sum of two such values loses neither operand"""
    rows, cols = shape
    q = (389 * torch.arange(rows).reshape(-1, 1) + 7 * torch.arange(cols).reshape(1, -1) + salt) % 2048
    pat = 0x3D80 + (q % 1024) + torch.where(q >= 1024, 0x8000, 0)
    return pat.to(torch.int16).view(torch.bfloat16)


# ---- prep_latent: (B, Cin, H, W, CP) ----
PREP_CASES = [(2, 4, 5, 7, 64), (3, 9, 3, 11, 16), (1, 8, 1, 1, 8)]
# fp32 values whose rounding to bf16 is the point: ties to even downwards and upwards, +-0, bf16-subnormal magnitudes (one a tie), the largest
# fp32 (rounds up to inf) and +-inf
PREP_SPECIAL_F32 = [1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 2.0 ** -7 + 2.0 ** -8), 0.0, -0.0, 2.0 ** -130, -1.3 * 2.0 ** -128,
                    3 * 2.0 ** -135, 3.4028234663852886e38, INF, -INF]


@functools.lru_cache(maxsize=None)
def build_prep(case, dtype):
    B, Cin, H, W, CP = case
    x = coded((B, Cin, H, W), dtype, salt=1)
    if dtype == torch.float32:
        sp = torch.tensor(PREP_SPECIAL_F32, dtype=torch.float32)
        flat = x.reshape(-1)
        n = min(len(sp), flat.numel())
        flat[flat.numel() - n:] = sp[:n]                                # the last cells: the last channel of the last image
    return x


# ---- nhwc_to_nchw: (B, C, HW, ld) ----
TO_NCHW_CASES = [(2, 4, 35, 64), (1, 3, 99, 128), (2, 16, 6, 16)]
# bf16 values above the fp16 range (-> inf in fp16; 65520 is not a bf16 value, 65536 is the first above it), and in the fp16-subnormal range,
# ties among them: k 2^-25 for odd k lies halfway between two fp16 subnormals
TO_NCHW_SPECIAL = [65536.0, -65536.0, 98304.0, -2.0 ** 127, 65280.0, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, -7 * 2.0 ** -25, 1.5 * 2.0 ** -17, 1.0078125 * 2.0 ** -15,
                   -1.9921875 * 2.0 ** -16, 2.0 ** -26, 0.0, -0.0]


@functools.lru_cache(maxsize=None)
def build_to_nchw(case):
    """the whole [B * HW, ld] input: coded values in the first C columns (the special ones planted in the first cells), NaN behind them"""
    B, Cc, HW, ld = case
    x = torch.full((B * HW, ld), NAN, dtype=torch.bfloat16)
    v = coded((B * HW, Cc), torch.bfloat16, salt=2)
    sp = torch.tensor(TO_NCHW_SPECIAL, dtype=torch.float32).to(torch.bfloat16)
    assert torch.equal(sp.float(), torch.tensor(TO_NCHW_SPECIAL, dtype=torch.float32))      # every one a bf16 value
    v.reshape(-1)[:len(sp)] = sp
    x[:, :Cc] = v
    return x


# ---- patchify / unpatchify: (B, C, H, W, ps) ----
PATCH_CASES = [(2, 16, 4, 6, 2), (1, 4, 2, 2, 2), (2, 3, 3, 5, 1)]


@functools.lru_cache(maxsize=None)
def build_patchify(case, dtype):
    B, Cc, H, W, ps = case
    return coded((B, Cc, H, W), dtype, salt=3)


@functools.lru_cache(maxsize=None)
def build_unpatchify(case, pad):
    """tokens [B * h * w, K + pad]: coded in the first K columns, NaN in the padding"""
    B, Cc, H, W, ps = case
    K, rows = ps * ps * Cc, B * (H // ps) * (W // ps)
    x = torch.full((rows, K + pad), NAN, dtype=torch.bfloat16)
    x[:, :K] = coded((rows, K), torch.bfloat16, salt=4)
    return x


# ---- crop_pos: (m, h, w, d) ----
CROP_CASES = [(8, 3, 5, 16), (8, 8, 8, 8), (9, 1, 1, 8), (8, 5, 2, 24)]


@functools.lru_cache(maxsize=None)
def build_crop(case):
    m, h, w, d = case
    return coded((m, m, d), torch.bfloat16, salt=5)


# ---- clip_embed ----
EMBED_B, EMBED_L, EMBED_VOCAB = 3, 5, 11
EMBED_H = [8, 64, 1032]
# -1, vocab and vocab + 5 are clamped; 0 and vocab - 1 appear on their own too, so that a clamp to the wrong end shows
EMBED_IDS = [[-1, 0, 3, EMBED_VOCAB, 7], [EMBED_VOCAB + 5, 10, 1, 2, 2], [5, 9, 4, 6, 8]]


@functools.lru_cache(maxsize=None)
def build_embed(H):
    ids = torch.tensor(EMBED_IDS, dtype=torch.int32)
    return ids, moderate_bf16((EMBED_VOCAB, H), salt=11), moderate_bf16((EMBED_L, H), salt=501)


# ---- clip_pool ----
POOL_B, POOL_L, POOL_EOS = 6, 7, 9
POOL_H = [8, 1032]
POOL_IDS_EOS = [[9, 1, 2, 3, 4, 5, 6],           # EOS at 0
                [1, 2, 3, 4, 5, 6, 9],           # EOS at L - 1
                [1, 2, 9, 4, 9, 6, 7],           # two: the first wins
                [1, 2, 3, 4, 5, 6, 7],           # none: row 0
                [11, 2, 3, 9, 5, 6, 7],          # a larger id in front of the EOS
                [1, 9, 9, 9, 9, 9, 9]]
POOL_IDS_LEGACY = [[1, 2, 3, 4, 5, 6, 40],       # largest at the end
                   [40, 2, 3, 4, 5, 6, 7],       # largest at 0
                   [1, 40, 3, 40, 5, 40, 7],     # a tie: the first wins
                   [1, 2, 3, 40, 5, 6, 7],
                   [-3, -2, -1, -5, -4, -6, -7], # all negative
                   [2, 2, 2, 2, 2, 2, 2]]        # all equal: row 0


@functools.lru_cache(maxsize=None)
def build_pool(H):
    return coded((POOL_B, POOL_L, H), torch.bfloat16, salt=6)


# ---- sinusoids ----
TIMES = [0.0, 0.5, 1.0, 500.25, 999.0, 1000.0, 1024.0, 2048.0]
SINUS_DIMS = [64, 256, 320]
# (B, d0, text_dim, da)
TIME_EMBED_CASES = [(2, 320, 1280, 256), (2, 320, 8, 2), (3, 64, 40, 32)]


@functools.lru_cache(maxsize=None)
def build_time_embed(case):
    """timesteps [B], text_embeds [B, text_dim], time_ids [B, 6]: every value of TIMES appears among the ids of every case with B >= 2"""
    B, d0, text_dim, da = case
    t = torch.tensor([TIMES[(3 + 2 * b) % len(TIMES)] for b in range(B)], dtype=torch.float32)
    ids = torch.tensor([TIMES[(5 * b + 3 * i) % len(TIMES)] for b in range(B) for i in range(6)], dtype=torch.float32).reshape(B, 6)
    return t, coded((B, text_dim), torch.bfloat16, salt=7), ids


# ---- softmax_rows ----
SOFTMAX_ROWS = 3
SOFTMAX_L = [8, 64, 2040, 2056, 4096]
SOFTMAX_CASES = [dict(name=f"L{L}_{kind}_pad{pad}", L=L, kind=kind, pad=pad) for L in SOFTMAX_L for kind in ("s3", "s12") for pad in (0, 16)]
SOFTMAX_CASES += [dict(name=f"L{L}_plus300_pad{pad}", L=L, kind="plus300", pad=pad) for L, pad in ((64, 0), (2056, 16))]
GUARD_BF16 = 0x5A5A


@functools.lru_cache(maxsize=None)
def build_softmax(name):
    """scores bf16 [3, L]: N(0, sigma^2) rounded to bf16; the row maximum planted at the last column of row 0 and the first of row 1; row 2 holds
    entries 1e4 below its maximum in a quarter of its cells (they must come out +0).  plus300: sigma 3 and +300 on every score, where the bf16
    spacing is 2 and exp overflows unless the maximum is subtracted."""
    c = next(c for c in SOFTMAX_CASES if c["name"] == name)
    L, kind = c["L"], c["kind"]
    gen = torch.Generator().manual_seed(1000 + L + {"s3": 0, "s12": 1, "plus300": 2}[kind])
    sigma = 12.0 if kind == "s12" else 3.0
    s = torch.randn((SOFTMAX_ROWS, L), generator=gen) * sigma
    top = float(s.abs().max()) + sigma
    s[0, L - 1] = top
    s[1, 0] = top
    s[2, 1::4] -= 1.0e4
    if kind == "plus300":
        s = s + 300.0
    return s.to(torch.bfloat16)


def softmax_buffer(s, pad):
    """the [rows + 3, L + pad] buffer a launch works in: the scores, the guard pattern behind every row and in the rows behind the last"""
    rows, L = s.shape
    buf = torch.full((rows + 3, L + pad), GUARD_BF16, dtype=torch.int16).view(torch.bfloat16)
    buf[:rows, :L] = s
    return buf
