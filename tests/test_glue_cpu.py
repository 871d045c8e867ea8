"""Host half of the glue kernels' tests (tests/test_glue_gpu.py): the references of tests/glue_ref.py against the oracle's own expressions, the
cases of tests/glue_cases.py against a list of deliberately wrong references (each must be told apart from the true one by at least one case;
the counts are printed), the two derived bounds against fp32 evaluations on the CPU, and every refusal of the one-launch entry points
(include/mxdenoise.h, "Glue kernels, one launch each"), which return before anything touches a device."""
import pytest
import torch
import torch.nn.functional as F

import glue_cases as K
import glue_ref as R
from sduss_amd import lib as L

BF16 = torch.bfloat16


def _differ(a, b):
    return not torch.equal(R.bits(a.contiguous()), R.bits(b.contiguous()))


def _report(kind, told, n):
    print(f"{kind}: told apart by {told} of {n} cases")
    assert told > 0, f"no case tells the '{kind}' mistake from the reference"


# ---- the references against the oracle's expressions ----

@pytest.mark.parametrize("case", K.PATCH_CASES, ids=str)
def test_patchify_ref_is_the_patch_embedding_conv(case):
    """PatchEmbed is Conv2d(C, N, kernel = stride = ps): the im2col times the weight in (dy, dx, c) column order is that conv, in fp64"""
    B, Cc, H, W, ps = case
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((B, Cc, H, W), generator=gen, dtype=torch.float64)
    w = torch.randn((5, Cc, ps, ps), generator=gen, dtype=torch.float64)
    got = R.patchify_view(x, ps) @ w.permute(0, 2, 3, 1).reshape(5, -1).T
    want = F.conv2d(x, w, stride=ps).permute(0, 2, 3, 1).reshape(-1, 5)
    assert float((got - want).abs().max()) <= 1e-13 * ps * ps * Cc * float(x.abs().max() * w.abs().max())


@pytest.mark.parametrize("case", K.PATCH_CASES, ids=str)
def test_unpatchify_ref_is_the_oracles_einsum(case):
    B, Cc, H, W, ps = case
    tok = K.build_unpatchify(case, 8)
    h, w = H // ps, W // ps
    x = tok[:, :ps * ps * Cc].reshape(B, h, w, ps, ps, Cc)
    want = torch.einsum("nhwpqc->nchpwq", x).reshape(B, Cc, h * ps, w * ps)          # oracle/sd3_mmdit_ref.py, the last line of mmdit_forward
    assert not _differ(R.unpatchify_ref(tok, B, Cc, H, W, ps, BF16), want)
    # and it undoes patchify
    img = K.build_patchify(case, BF16)
    assert not _differ(R.unpatchify_ref(R.patchify_ref(img, ps), B, Cc, H, W, ps, BF16), img)


@pytest.mark.parametrize("case", K.CROP_CASES, ids=str)
def test_crop_pos_ref_is_the_oracles_slice(case):
    m, h, w, d = case
    table = K.build_crop(case)
    top, left = (m - h) // 2, (m - w) // 2
    want = table.reshape(1, m, m, d)[:, top:top + h, left:left + w].reshape(1, h * w, d)[0]     # oracle/sd3_mmdit_ref.py::mmdit_forward
    assert not _differ(R.crop_pos_ref(table, h, w), want)


def test_coded_operands_are_distinct_cell_by_cell():
    for dtype in K.DTYPES:
        x = K.coded((2, 16, 4, 6), dtype, salt=3)
        assert torch.isfinite(x.float()).all()
        assert len(set(R.bits(x.to(BF16)).reshape(-1).tolist())) == x.numel()
    assert len(set(R.bits(K.build_pool(1032)).reshape(-1).tolist())) == K.POOL_B * K.POOL_L * 1032
    tok = K.moderate_bf16((11, 1032), 11)
    assert all(bool((tok[a] != tok[b]).all()) for a in range(11) for b in range(a))
    # the planted roundings are what their comments say
    sp = torch.tensor(K.PREP_SPECIAL_F32, dtype=torch.float32).to(BF16).float().tolist()
    assert sp[0] == 1.0 and sp[1] == 1.0 + 2.0 ** -6 and sp[4:6] == [0.0, 0.0] and sp[6] == 2.0 ** -130 and sp[8] == 2.0 ** -133 and sp[9] == K.INF
    h = torch.tensor(K.TO_NCHW_SPECIAL).to(torch.float16).float().tolist()
    assert h[0] == K.INF and h[3] == -K.INF and h[4] == 65280.0 and h[5] == 0.0 and h[6] == 2 * 2.0 ** -24 and h[7] == 2 * 2.0 ** -24 and h[8] == -4 * 2.0 ** -24


# ---- deliberately wrong references: copies ----

def test_cases_reject_padding_channels_of_minus_zero():
    told = 0
    for case in K.PREP_CASES:
        x = K.build_prep(case, torch.float32)
        good = R.prep_latent_ref(x, case[4])
        bad = good.clone()
        bad[:, case[1]:] = -0.0
        told += _differ(good, bad)
    _report("padding channels -0", told, len(K.PREP_CASES))


def test_cases_reject_a_swapped_patch_order():
    dydx = pq = 0
    for case in K.PATCH_CASES:
        B, Cc, H, W, ps = case
        x = K.build_patchify(case, BF16)
        dydx += _differ(R.patchify_ref(x, ps), R.patchify_view(x, ps, order=(0, 2, 4, 5, 3, 1)))
        tok = K.build_unpatchify(case, 0)
        pq += _differ(R.unpatchify_ref(tok, B, Cc, H, W, ps, BF16), R.unpatchify_ref(tok, B, Cc, H, W, ps, BF16, order=(0, 5, 1, 4, 2, 3)))
    _report("dy<->dx", dydx, len(K.PATCH_CASES))
    _report("p<->q", pq, len(K.PATCH_CASES))


def test_cases_reject_a_wrong_crop():
    up = swap = 0
    for case in K.CROP_CASES:
        m, h, w, d = case
        table = K.build_crop(case)
        good = R.crop_pos_ref(table, h, w)
        top, left = (m - h + 1) // 2, (m - w + 1) // 2
        up += _differ(good, table[top:top + h, left:left + w].reshape(h * w, d))
        top, left = (m - w) // 2, (m - h) // 2
        wrong = table[top:top + h, left:left + w]
        swap += wrong.shape[:2] != (h, w) or _differ(good, wrong.reshape(h * w, d))
    _report("crop rounded up", up, len(K.CROP_CASES))
    _report("top<->left", swap, len(K.CROP_CASES))


def test_cases_reject_a_wrong_embedding_row():
    by_row = wrap = 0
    for H in K.EMBED_H:
        ids, tok, pos = K.build_embed(H)
        good = R.clip_embed_ref(ids, tok, pos)
        behind = torch.cat([pos, torch.full((ids.numel() - K.EMBED_L, H), K.NAN, dtype=BF16)])      # what lies behind the table on the device
        flat = tok[ids.clamp(0, K.EMBED_VOCAB - 1).reshape(-1).long()].float()
        by_row += _differ(good, (flat + behind.float()).to(BF16))
        wrapped = torch.tensor([[i % K.EMBED_VOCAB for i in row] for row in K.EMBED_IDS])
        wrap += _differ(good, R.clip_embed_ref(wrapped, tok, pos))
        wrap_none = _differ(R.clip_embed_ref(ids, tok, None), R.clip_embed_ref(wrapped, tok, None))
        assert wrap_none
    _report("position by row", by_row, len(K.EMBED_H))
    _report("unclamped ids wrapping", wrap, len(K.EMBED_H))


def test_cases_reject_the_last_match():
    eos = tie = 0
    for H in K.POOL_H:
        x = K.build_pool(H)
        rows = torch.arange(K.POOL_B)
        ids = torch.tensor(K.POOL_IDS_EOS)
        hit = ids == K.POOL_EOS
        last = torch.where(hit.any(-1), K.POOL_L - 1 - hit.flip(-1).int().argmax(-1), 0)
        eos += _differ(R.clip_pool_ref(ids, x, K.POOL_EOS), x[rows, last])
        ids = torch.tensor(K.POOL_IDS_LEGACY)
        last = K.POOL_L - 1 - ids.flip(-1).argmax(-1)
        tie += _differ(R.clip_pool_ref(ids, x, -1), x[rows, last])
    _report("last EOS", eos, len(K.POOL_H))
    _report("last of tied maxima", tie, len(K.POOL_H))
    # what the cases say they hold
    assert (torch.tensor(K.POOL_IDS_EOS) == K.POOL_EOS).int().argmax(-1).tolist() == [0, 6, 2, 0, 3, 1]
    assert torch.tensor(K.POOL_IDS_LEGACY).argmax(-1).tolist() == [6, 0, 1, 3, 2, 0]


# ---- the sinusoid bound ----

def _sinus_sets():
    """(name, t, dim) of every sinusoid a GPU test checks"""
    t = torch.tensor(K.TIMES, dtype=torch.float32)
    sets = [(f"sinus_embed dim {dim}", t, dim) for dim in K.SINUS_DIMS]
    for case in K.TIME_EMBED_CASES:
        ts, _text, ids = K.build_time_embed(case)
        sets += [(f"time_embed {case} tsin", ts, case[1]), (f"time_embed {case} addin", ids.reshape(-1), case[3])]
    return sets


def test_fp32_evaluations_lie_inside_the_sinusoid_bound():
    n = two = 0
    for name, t, dim in _sinus_sets():
        c, e = R.sinusoid_ref(t, dim)
        assert float(e.max()) <= 3.7e-4, name
        lo, hi = R.interval(c, e)
        for what, f in (("oracle", R.sinusoid_oracle_f32), ("kernel emulation", R.sinusoid_kernel_f32)):
            assert int(R.outside(f(t, dim).to(BF16), lo, hi).sum()) == 0, (name, what)
        n += c.numel()
        two += R.two_valued(lo, hi) * c.numel()
    print(f"sinusoids: {n} cells, {100 * two / n:.2f} % admit two bf16 values")
    assert two / n <= 0.15
    assert set(K.TIMES) == set(torch.cat([K.build_time_embed(c)[2].reshape(-1) for c in K.TIME_EMBED_CASES]).tolist())


@pytest.mark.parametrize("kind", ["swap", "j+1", "half-1", 2e-6, 1e-5])
def test_sinusoid_cases_reject_a_wrong_sinusoid(kind):
    told, sets = 0, _sinus_sets()
    for name, t, dim in sets:
        lo, hi = R.interval(*R.sinusoid_ref(t, dim))
        wrong = R.bf16_of_f64(R.sinusoid_ref(t, dim, mutate=kind)[0])
        bad = int(R.outside(wrong, lo, hi).sum())
        print(f"  {kind} {name}: {bad} of {wrong.numel()} cells leave the interval")
        told += bad > 0
    _report(f"sinusoid {kind}", told, len(sets))
    if kind == "swap":                                   # over the three dims of sinus_embed: all but the cells where cos = sin to within the bound
        t = torch.tensor(K.TIMES, dtype=torch.float32)
        inside = sum(int((~R.outside(R.bf16_of_f64(R.sinusoid_ref(t, d, mutate="swap")[0]), *R.interval(*R.sinusoid_ref(t, d)))).sum()) for d in K.SINUS_DIMS)
        assert inside <= 8


# ---- the softmax bound ----

def _sequential_f32(s):
    """the kernel's operations, one thread's worth: exp2(fl(d log2 e)), a sequential fp32 sum, one reciprocal, one product"""
    d = s.float() - s.float().max(dim=1, keepdim=True).values
    ex = torch.exp2(d * R.LOG2E_F32)
    tot = torch.from_numpy(ex.numpy().cumsum(axis=1, dtype="float32"))[:, -1:]
    return ex * (1.0 / tot)


def test_fp32_evaluations_lie_inside_the_softmax_bound():
    n = two = 0
    for c in K.SOFTMAX_CASES:
        s = K.build_softmax(c["name"])
        p, r = R.softmax_ref(s)
        near = (s.double() - s.double().max(dim=1, keepdim=True).values) > -1.0e3
        # (L + 2) 2^-24 = 2.44e-4 at L = 4096, and twice tau at the |d| <= 105 these draws reach (the planted maximum lies one sigma above the rest)
        assert float(r[near].max()) <= 2.7e-4, c["name"]
        assert float(p[~near].max() if (~near).any() else 0.0) == 0.0 and int((~near).sum()) >= c["L"] // 4
        lo, hi = R.softmax_interval(p, r)
        assert float(hi[~near].float().abs().max()) == 0.0               # 1e4 below the maximum: +0
        for what, f in (("torch.softmax", torch.softmax(s.float(), dim=1)), ("sequential", _sequential_f32(s))):
            assert int(R.outside(f.to(BF16), lo, hi).sum()) == 0, (c["name"], what)
        share = R.two_valued(lo, hi)
        assert share <= 0.15, c["name"]
        n += p.numel()
        two += share * p.numel()
        # the planted maxima
        assert int(s[0].float().argmax()) == c["L"] - 1 and int(s[1].float().argmax()) == 0
    print(f"softmax: {n} cells, {100 * two / n:.2f} % admit two bf16 values")
    assert float(K.build_softmax("L64_plus300_pad0").float().min()) > 89.0 - 1.0e4 and float(K.build_softmax("L64_plus300_pad0")[0].float().max()) > 300.0


@pytest.mark.parametrize("kind", ["over ld", "no stride tail", "half the row", 1e-3])
def test_softmax_cases_reject_a_wrong_softmax(kind):
    told = 0
    for c in K.SOFTMAX_CASES:
        s = K.build_softmax(c["name"])
        Lc = c["L"]
        lo, hi = R.softmax_interval(*R.softmax_ref(s))
        d = s.double() - s.double().max(dim=1, keepdim=True).values
        ex = torch.exp(d)
        if kind == "over ld":                                             # the row's ld columns, guard pattern included, as one softmax
            whole = K.softmax_buffer(s, c["pad"])[:K.SOFTMAX_ROWS].double()
            wrong = torch.softmax(whole - whole.max(dim=1, keepdim=True).values, dim=1)[:, :Lc]
        elif kind == "no stride tail":                                    # 256 threads x one 16-byte vector: the first 2048 columns only
            wrong = ex / ex[:, :2048].sum(dim=1, keepdim=True)
        elif kind == "half the row":
            wrong = ex / ex[:, :Lc // 2].sum(dim=1, keepdim=True)
        else:
            wrong = torch.softmax(d, dim=1) * (1.0 + kind)
        bad = int(R.outside(R.bf16_of_f64(wrong), lo, hi).sum())
        print(f"  {kind} {c['name']}: {bad} of {wrong.numel()} cells leave the interval")
        told += bad > 0
    _report(f"softmax {kind}", told, len(K.SOFTMAX_CASES))


# ---- the entry points' refusals ----

A, MIS = 0x10000, 0x10008          # a 16-byte aligned and a misaligned address: never dereferenced, every call below returns before a device is touched
F32, BF = L.MX_F32, L.MX_BF16

REFUSALS = [
    # name, arguments behind the stream, the message
    ("mx_prep_latent", (None, F32, A, 2, 4, 35, 64), "prep_latent: null operand or empty shape"),
    ("mx_prep_latent", (A, F32, None, 2, 4, 35, 64), "prep_latent: null operand or empty shape"),
    ("mx_prep_latent", (A, F32, A, 0, 4, 35, 64), "prep_latent: null operand or empty shape"),
    ("mx_prep_latent", (A, F32, A, 2, 4, 0, 64), "prep_latent: null operand or empty shape"),
    ("mx_prep_latent", (A, F32, MIS, 2, 4, 35, 64), "prep_latent: out must be 16-byte aligned"),
    ("mx_prep_latent", (A, F32, A, 2, 4, 35, 60), "prep_latent: bad channel padding"),
    ("mx_prep_latent", (A, F32, A, 2, 9, 35, 8), "prep_latent: bad channel padding"),
    ("mx_prep_latent", (A, 7, A, 2, 4, 35, 64), "prep_latent: bad dtype"),
    ("mx_nhwc_to_nchw", (None, A, F32, 2, 4, 35, 64), "nhwc_to_nchw: null operand or empty shape"),
    ("mx_nhwc_to_nchw", (A, None, F32, 2, 4, 35, 64), "nhwc_to_nchw: null operand or empty shape"),
    ("mx_nhwc_to_nchw", (A, A, F32, 2, 0, 35, 64), "nhwc_to_nchw: null operand or empty shape"),
    ("mx_nhwc_to_nchw", (A, A, F32, 2, 4, 35, 3), "nhwc_to_nchw: ld must hold the C columns"),
    ("mx_nhwc_to_nchw", (A, A, 3, 2, 4, 35, 64), "nhwc_to_nchw: bad dtype"),
    ("mx_time_embed", (None, A, A, A, A, 2, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, None, A, A, A, 2, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, None, A, A, 2, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, A, None, A, 2, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, A, A, None, 2, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, A, A, A, 0, 320, 8, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, A, A, A, 2, 320, 0, 2), "time_embed: null operand or empty shape"),
    ("mx_time_embed", (A, A, A, A, A, 2, 321, 8, 2), "time_embed: d0 and da must be even"),
    ("mx_time_embed", (A, A, A, A, A, 2, 320, 8, 3), "time_embed: d0 and da must be even"),
    ("mx_sinus_embed", (None, A, 2, 256), "sinus_embed: null operand or empty shape"),
    ("mx_sinus_embed", (A, None, 2, 256), "sinus_embed: null operand or empty shape"),
    ("mx_sinus_embed", (A, A, 2, 0), "sinus_embed: null operand or empty shape"),
    ("mx_sinus_embed", (A, A, 2, 255), "sinus_embed: dim must be even"),
    ("mx_patchify", (None, BF, A, 2, 16, 4, 6, 2), "patchify: null operand or empty shape"),
    ("mx_patchify", (A, BF, None, 2, 16, 4, 6, 2), "patchify: null operand or empty shape"),
    ("mx_patchify", (A, BF, A, 2, 16, 4, 6, 0), "patchify: null operand or empty shape"),
    ("mx_patchify", (A, BF, A, 2, 16, 5, 6, 2), "patchify: H and W must be multiples of the patch size"),
    ("mx_patchify", (A, BF, A, 2, 16, 4, 7, 2), "patchify: H and W must be multiples of the patch size"),
    ("mx_patchify", (A, 5, A, 2, 16, 4, 6, 2), "patchify: bad dtype"),
    ("mx_unpatchify", (None, A, BF, 2, 16, 4, 6, 2, 64), "unpatchify: null operand or empty shape"),
    ("mx_unpatchify", (A, None, BF, 2, 16, 4, 6, 2, 64), "unpatchify: null operand or empty shape"),
    ("mx_unpatchify", (A, A, BF, 2, 16, 0, 6, 2, 64), "unpatchify: null operand or empty shape"),
    ("mx_unpatchify", (A, A, BF, 2, 16, 5, 6, 2, 64), "unpatchify: H and W must be multiples of the patch size"),
    ("mx_unpatchify", (A, A, BF, 2, 16, 4, 7, 2, 64), "unpatchify: H and W must be multiples of the patch size"),
    ("mx_unpatchify", (A, A, BF, 2, 16, 4, 6, 2, 63), "unpatchify: ld must hold the ps*ps*C columns"),
    ("mx_unpatchify", (A, A, -1, 2, 16, 4, 6, 2, 64), "unpatchify: bad dtype"),
    ("mx_crop_pos", (None, A, 8, 3, 5, 16), "crop_pos: null operand or empty shape"),
    ("mx_crop_pos", (A, None, 8, 3, 5, 16), "crop_pos: null operand or empty shape"),
    ("mx_crop_pos", (A, A, 8, 0, 5, 16), "crop_pos: null operand or empty shape"),
    ("mx_crop_pos", (MIS, A, 8, 3, 5, 16), "crop_pos: table and out must be 16-byte aligned"),
    ("mx_crop_pos", (A, MIS, 8, 3, 5, 16), "crop_pos: table and out must be 16-byte aligned"),
    ("mx_crop_pos", (A, A, 8, 3, 5, 12), "crop_pos: bad geometry"),
    ("mx_crop_pos", (A, A, 8, 9, 5, 16), "crop_pos: bad geometry"),
    ("mx_crop_pos", (A, A, 8, 3, 9, 16), "crop_pos: bad geometry"),
    ("mx_softmax_rows", (None, 3, 64, 64), "softmax_rows: null operand or empty shape"),
    ("mx_softmax_rows", (A, 0, 64, 64), "softmax_rows: null operand or empty shape"),
    ("mx_softmax_rows", (A, 3, 0, 64), "softmax_rows: null operand or empty shape"),
    ("mx_softmax_rows", (A, 3, 64, 56), "softmax_rows: null operand or empty shape"),
    ("mx_softmax_rows", (MIS, 3, 64, 64), "softmax_rows: scores must be 16-byte aligned"),
    ("mx_softmax_rows", (A, 3, 60, 64), "softmax_rows: L and ld must be multiples of 8"),
    ("mx_softmax_rows", (A, 3, 64, 68), "softmax_rows: L and ld must be multiples of 8"),
    ("mx_clip_embed", (None, A, A, A, 15, 5, 64, 11), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, None, A, A, 15, 5, 64, 11), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, A, A, None, 15, 5, 64, 11), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, A, None, None, 15, 5, 64, 11), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, A, A, A, 15, 5, 64, 0), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, A, A, A, 15, 0, 64, 11), "clip_embed: null operand or empty shape"),
    ("mx_clip_embed", (A, MIS, A, A, 15, 5, 64, 11), "clip_embed: tables and out must be 16-byte aligned"),
    ("mx_clip_embed", (A, A, MIS, A, 15, 5, 64, 11), "clip_embed: tables and out must be 16-byte aligned"),
    ("mx_clip_embed", (A, A, None, MIS, 15, 5, 64, 11), "clip_embed: tables and out must be 16-byte aligned"),
    ("mx_clip_embed", (A, A, None, A, 15, 5, 60, 11), "clip_embed: hidden size must be a multiple of 8"),
    ("mx_clip_pool", (None, A, A, 6, 7, 8, 9), "clip_pool: null operand or empty shape"),
    ("mx_clip_pool", (A, None, A, 6, 7, 8, 9), "clip_pool: null operand or empty shape"),
    ("mx_clip_pool", (A, A, None, 6, 7, 8, 9), "clip_pool: null operand or empty shape"),
    ("mx_clip_pool", (A, A, A, 6, 0, 8, 9), "clip_pool: null operand or empty shape"),
    ("mx_clip_pool", (A, MIS, A, 6, 7, 8, 9), "clip_pool: x and out must be 16-byte aligned"),
    ("mx_clip_pool", (A, A, MIS, 6, 7, 8, 9), "clip_pool: x and out must be 16-byte aligned"),
    ("mx_clip_pool", (A, A, A, 6, 7, 12, 9), "clip_pool: hidden size must be a multiple of 8"),
    ("mx_clip_pool", (A, A, A, 6, 7, 1036, -1), "clip_pool: hidden size must be a multiple of 8"),
]


@pytest.mark.parametrize("name,args,message", REFUSALS, ids=[f"{i}-{r[0]}" for i, r in enumerate(REFUSALS)])
def test_entry_points_refuse(name, args, message):
    lib = L.load()
    assert len(args) + 1 == len(L.SYMBOLS[name][1])
    assert getattr(lib, name)(None, *args) == 1
    assert lib.mx_last_error().decode() == message


def test_every_entry_point_has_refusals():
    names = {r[0] for r in REFUSALS}
    assert names == {"mx_prep_latent", "mx_nhwc_to_nchw", "mx_time_embed", "mx_sinus_embed", "mx_patchify", "mx_unpatchify", "mx_crop_pos", "mx_softmax_rows",
                     "mx_clip_embed", "mx_clip_pool"} and names <= set(L.SYMBOLS)
