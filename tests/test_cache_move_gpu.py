"""The kernels that move the block-skip cache's state, ONE LAUNCH per test body through the entry points of include/mxdenoise.h ("Block-skip cache
kernels, one launch each"): the cases of tests/cache_move_cases.py against the references of tests/cache_move_ref.py.

Every copy is compared BIT FOR BIT, whole tensors: outputs and in / out tensors live in guarded buffers (guard rows behind them, guard columns
behind every state row, which the launch is told about as the row stride), inputs carry NaN behind their last row and in their padding columns,
and a cell the operation does not own must hold what it held before.  The only bounds are the derived ones of cache_move_ref.py: the row
statistics of pc_rows_load_stats and the three squared-difference kernels; those tests print their worst err / bound, and the gate path of
pc_image_copy prints how many cells took the fused and the unfused evaluation (profiles/cache_move_digest.txt holds one run's figures).

test_conv_routes_agree holds the two routes of pc_conv (unet_sdxl.cpp) against each other and against the fp64 bound of the literal per-patch conv."""
import ctypes as C

import pytest
import torch

import cache_move_cases as K
import cache_move_ref as R
import kernel_ref as KR
from sduss_amd import lib as L

pytestmark = pytest.mark.gpu
NAN = float("nan")
EPS = 1e-5


def _ids(cases):
    return [c["name"] for c in cases]


def _in(t, dev, extra=2):
    """an operand the launch only reads: NaN rows behind it"""
    buf = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), NAN, dtype=t.dtype, device=dev)
    buf[:t.shape[0]] = t.to(dev)
    return buf


def _out(t, dev, pad=0):
    """a bf16 tensor the launch writes (wholly or in part): its present contents in a guarded buffer; returns (buffer, view, row stride)"""
    rows, cols = t.shape
    buf, view = R.guarded(rows, cols, cols + pad, torch.bfloat16, dev)
    view.copy_(t.to(dev))
    return buf, view, cols + pad


def _nan_f(n, dtype, dev, tail=64):
    return torch.full((n + tail,), NAN, dtype=dtype, device=dev)


def _same(got, want, what):
    g, w = R.bits(got.cpu().contiguous()), R.bits(want.contiguous())
    assert g.shape == w.shape, what
    bad = g != w
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {g.numel()} cells differ bit for bit, the first at {tuple(bad.nonzero()[0].tolist())}"


def _guards(buf, rows, cols, what):
    assert R.guard_violations(buf, rows, cols) == 0, f"{what}: wrote outside its rows / columns"


def _table(arr, dev):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _samples(table, dev):
    arr, row0 = (L.PcSample * len(table))(), 0
    for i, (h, w, slot) in enumerate(table):
        arr[i] = L.PcSample(row0, h, w, slot, max(w // K.P0, 1))
        row0 += h * w
    return _table(arr, dev)


def _patches(patches, dev):
    arr = (L.PcPatch * len(patches))()
    for i, (b, py, px) in enumerate(patches):
        arr[i] = L.PcPatch(b, py, px, 0x5A5A)
    return _table(arr, dev)


def _ranges(ranges, dev):
    arr = (L.PcRange * len(ranges))()
    for i, r in enumerate(ranges):
        arr[i] = L.PcRange(*r)
    return _table(arr, dev)


def _launch(status, what):
    L.check(status, what)
    torch.cuda.synchronize()


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- pc_gather ----

@pytest.mark.parametrize("c", K.GATHER_CASES, ids=_ids(K.GATHER_CASES))
def test_pc_gather(cuda_device, c):
    dev, Cc, (lo, hi, up) = cuda_device, c["C"], c["mode"]
    o = K.build_gather(c)
    geo = R.geometry(K.TABLE_A, c["level"], K.P0)
    want = R.gather_ref(o["src"], Cc, geo, K.PATCHES_A, o["p"], lo, hi, up)
    src = o["src"].clone()
    if c["ld_pad"]:
        src[:, Cc:] = NAN                                          # the padding columns of a wider tensor are not the gather's to read
    d_src = _in(src, dev)
    n, P = len(K.PATCHES_A), o["p"] + lo + hi
    buf, view = R.guarded(n * P * P, Cc, Cc, torch.bfloat16, dev)
    samp, lst = _samples(K.TABLE_A, dev), _patches(K.PATCHES_A, dev)
    _launch(L.load().mx_pc_gather(L.current_stream(), d_src.data_ptr(), Cc + c["ld_pad"], Cc, buf.data_ptr(), lst.data_ptr(), n, samp.data_ptr(), c["level"],
                                  o["p"], lo, hi, up), c["name"])
    _same(view, want.reshape(-1, Cc), f"pc_gather {c['name']}")
    _guards(buf, n * P * P, Cc, c["name"])


# ---- pc_scatter, pc_patch_store ----

@pytest.mark.parametrize("c", K.SCATTER_CASES, ids=_ids(K.SCATTER_CASES))
def test_pc_scatter(cuda_device, c):
    dev, Cc = cuda_device, c["C"]
    o = K.build_scatter(c)
    geo = R.geometry(K.TABLE_A, c["level"], K.P0)
    want = R.scatter_ref(o["state"], o["src"], o["Ps"], o["o0"], Cc, geo, K.PATCHES_A, o["p"])
    buf, view, ld = _out(o["state"], dev, pad=8)
    d_src = _in(o["src"], dev)
    samp, lst = _samples(K.TABLE_A, dev), _patches(K.PATCHES_A, dev)
    _launch(L.load().mx_pc_scatter(L.current_stream(), d_src.data_ptr(), o["Ps"], o["o0"], Cc, buf.data_ptr(), ld, lst.data_ptr(), len(K.PATCHES_A), samp.data_ptr(),
                                   c["level"], o["p"]), c["name"])
    _same(view, want, f"pc_scatter {c['name']}")
    _guards(buf, *o["state"].shape, c["name"])


@pytest.mark.parametrize("c", K.PATCH_CASES, ids=_ids(K.PATCH_CASES))
def test_pc_patch_store(cuda_device, c):
    dev, Cc = cuda_device, c["C"]
    o = K.build_patch(c)
    geo = R.geometry(K.TABLE_A, c["level"], K.P0)
    want = R.patch_store_ref(o["state"], o["x"], Cc, geo, K.PATCHES_A, o["p"])
    buf, view, ld = _out(o["state"], dev, pad=8)
    d_x = _in(o["x"], dev)
    samp, lst = _samples(K.TABLE_A, dev), _patches(K.PATCHES_A, dev)
    _launch(L.load().mx_pc_patch_store(L.current_stream(), d_x.data_ptr(), buf.data_ptr(), ld, Cc, lst.data_ptr(), len(K.PATCHES_A), samp.data_ptr(), c["level"],
                                       o["p"]), c["name"])
    _same(view, want, f"pc_patch_store {c['name']}")
    _guards(buf, *o["state"].shape, c["name"])


# ---- pc_image_copy ----

@pytest.mark.parametrize("c", K.IMAGE_COPY_CASES, ids=_ids(K.IMAGE_COPY_CASES))
def test_pc_image_copy(cuda_device, c):
    dev, Cc, table, level = cuda_device, c["C"], c["table"], c["level"]
    o = K.build_image_copy(c)
    geo = R.geometry(table, level, K.P0)
    gate = c.get("gate", 0)
    want = R.image_copy_ref(o["batch"], o["state"], Cc, geo, c["to_batch"], o["vec"], o["residual"], gate)
    samp = _samples(table, dev)
    d_vec = o["vec"].to(dev) if o["vec"] is not None else None
    d_res = _in(o["residual"], dev) if o["residual"] is not None else None
    ldvec = o["vec"].shape[1] if o["vec"] is not None else 0
    if c["to_batch"]:
        bbuf, bview, _ = _out(o["batch"], dev)
        sbuf = _in(torch.cat([o["state"], torch.full((o["state"].shape[0], 8), NAN, dtype=torch.bfloat16)], 1), dev)      # NaN behind every state row
    else:
        bbuf = _in(o["batch"], dev)
        sbuf, sview, _ = _out(o["state"], dev, pad=8)
    _launch(L.load().mx_pc_image_copy(L.current_stream(), bbuf.data_ptr(), sbuf.data_ptr(), samp.data_ptr(), len(table), level, Cc, o["state"].shape[1] + 8,
                                      c["to_batch"], _ptr(d_vec), ldvec, _ptr(d_res), K.image_elems(table, level, Cc), gate), c["name"])
    if not c["to_batch"]:
        _same(sview, want, f"pc_image_copy {c['name']}")
        _guards(sbuf, *o["state"].shape, c["name"])
        return
    unfused, fused, _n = want
    got = R.bits(bview.cpu().contiguous())
    is_u, is_f = got == R.bits(unfused), got == R.bits(fused)
    if gate:
        print(f"pc_image_copy {c['name']}: {int((is_u & ~is_f).sum())} cells took the unfused value, {int((is_f & ~is_u).sum())} the fused one, "
              f"{int((is_u & is_f).sum())} of {got.numel()} are the same either way")
    bad = ~(is_u | is_f)
    assert int(bad.sum()) == 0, f"pc_image_copy {c['name']}: {int(bad.sum())} cells differ bit for bit, the first at {tuple(bad.nonzero()[0].tolist())}"
    _guards(bbuf, *o["batch"].shape, c["name"])


# ---- pc_rows_load_stats ----

@pytest.mark.parametrize("c", K.ROWS_STATS_CASES, ids=_ids(K.ROWS_STATS_CASES))
def test_pc_rows_load_stats(cuda_device, c):
    dev, Cc, table, level = cuda_device, c["C"], c["table"], c["level"]
    o = K.build_rows_stats(c)
    geo = R.geometry(table, level, K.P0)
    want, rows, (st, d_st), (fin, d_fin) = R.rows_load_stats_ref(o["batch"], o["state"], Cc, geo, o["residual"], EPS)
    M = o["batch"].shape[0]
    bbuf, bview, _ = _out(o["batch"], dev)
    sbuf = _in(torch.cat([o["state"], torch.full((o["state"].shape[0], 8), NAN, dtype=torch.bfloat16)], 1), dev)
    d_res, samp = _in(o["residual"], dev), _samples(table, dev)
    stats = _nan_f((M + 3) * 8, torch.float32, dev) if c["stats"] else None
    fins = _nan_f((M + 3) * 2, torch.float32, dev) if c["fin"] else None
    _launch(L.load().mx_pc_rows_load_stats(L.current_stream(), bbuf.data_ptr(), sbuf.data_ptr(), samp.data_ptr(), len(table), level, Cc, o["state"].shape[1] + 8,
                                           d_res.data_ptr(), _ptr(stats), _ptr(fins), EPS, max(g.h * g.w for g in geo)), c["name"])
    _same(bview, want, f"pc_rows_load_stats {c['name']}")
    _guards(bbuf, *o["batch"].shape, c["name"])
    if stats is not None:
        s = stats.cpu()
        got = s[:M * 8].view(M, 8)
        assert bool(torch.isnan(got[:, 2:]).all()) and bool(torch.isnan(s[M * 8:]).all()), f"{c['name']}: statistics written outside (sum, sum of squares) of the samples' rows"
        n, ratio = R.violations(got[rows, :2], st, d_st)
        print(f"pc_rows_load_stats {c['name']}: stats1 worst err / bound = {ratio:.3g}")
        assert n == 0, f"{c['name']}: {n} of {st.numel()} row sums outside their bound (worst err / bound = {ratio:.3g})"
    if fins is not None:
        f = fins.cpu()
        n, ratio = R.violations(f[:M * 2].view(M, 2)[rows], fin, d_fin)
        print(f"pc_rows_load_stats {c['name']}: fin worst err / bound = {ratio:.3g}")
        assert n == 0, f"{c['name']}: {n} of {fin.numel()} (mean, rstd) outside their bound (worst err / bound = {ratio:.3g})"
        assert bool(torch.isnan(f[M * 2:]).all()), f"{c['name']}: (mean, rstd) written behind the last row"


# ---- squared differences ----

def _check_partial(part, ref, bound, what):
    """part: the NaN-filled buffer after the launch; ref / bound [units, partials]"""
    n = ref.numel()
    p = part.cpu()
    assert bool(torch.isnan(p[n:]).all()), f"{what}: wrote behind its partial sums"
    got = p[:n].view(ref.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} partial sums the launch owns were not written"
    bad, ratio = R.violations(got, ref, bound)
    live = ref > 0
    ratio = float(((got - ref).abs()[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"{what}: worst err / bound = {ratio:.3g}")
    assert bad == 0, f"{what}: {bad} of {n} partial sums outside (k + 3) 2^-24 of the fp64 sum (worst err / bound = {ratio:.3g})"
    assert bool((got[ref == 0] == 0).all()), f"{what}: a unit equal to its cached value, or an empty chunk, must give exactly 0.0"
    return got


@pytest.mark.parametrize("c", K.PATCH_CASES, ids=_ids(K.PATCH_CASES))
def test_pc_patch_sq_diff(cuda_device, c):
    dev, Cc = cuda_device, c["C"]
    o = K.build_patch(c, equal_patch=3)
    geo = R.geometry(K.TABLE_A, c["level"], K.P0)
    ref, bound = R.patch_sq_diff_ref(o["x"], o["state"], Cc, geo, K.PATCHES_A, o["p"])
    assert float(ref[3].sum()) == 0.0 and float(ref.sum()) > 0.0
    d_x = _in(o["x"], dev)
    sbuf = _in(torch.cat([o["state"], torch.full((o["state"].shape[0], 8), NAN, dtype=torch.bfloat16)], 1), dev)
    samp, lst = _samples(K.TABLE_A, dev), _patches(K.PATCHES_A, dev)
    part = _nan_f(ref.numel(), torch.float64, dev)
    _launch(L.load().mx_pc_patch_sq_diff(L.current_stream(), d_x.data_ptr(), sbuf.data_ptr(), o["state"].shape[1] + 8, Cc, lst.data_ptr(), len(K.PATCHES_A),
                                         samp.data_ptr(), c["level"], o["p"], part.data_ptr()), c["name"])
    _check_partial(part, ref, bound, f"pc_patch_sq_diff {c['name']}")


@pytest.mark.parametrize("c", K.RANGE_SQ_CASES, ids=_ids(K.RANGE_SQ_CASES))
def test_pc_range_sq_diff(cuda_device, c):
    dev = cuda_device
    o = K.build_ranges(c["set"], equal=True)
    ref, bound = R.range_sq_diff_ref(o["batch"], o["state"], o["C"], o["ranges"])
    assert float(ref[K.RANGE_SETS[c["set"]]["eq"]].sum()) == 0.0
    d_x = _in(o["batch"], dev)
    sbuf = _in(torch.cat([o["state"], torch.full((o["state"].shape[0], 8), NAN, dtype=torch.bfloat16)], 1), dev)
    rng = _ranges(o["ranges"], dev)
    part = _nan_f(ref.numel(), torch.float64, dev)
    _launch(L.load().mx_pc_range_sq_diff(L.current_stream(), d_x.data_ptr(), sbuf.data_ptr(), o["state"].shape[1] + 8, o["C"], rng.data_ptr(), len(o["ranges"]),
                                         part.data_ptr()), c["name"])
    _check_partial(part, ref, bound, f"pc_range_sq_diff {c['name']}")


@pytest.mark.parametrize("c", K.SQ_PARTIAL_CASES, ids=_ids(K.SQ_PARTIAL_CASES))
def test_sq_diff_partial(cuda_device, c):
    dev = cuda_device
    o = K.build_sq_partial(c)
    ref, bound = R.sq_diff_partial_ref(o["a"], o["b"], c["slot"])
    assert float(ref[c["eq"]].sum()) == 0.0
    d_a, d_b = _in(o["a"], dev), _in(o["b"], dev)
    slot = torch.tensor(c["slot"], dtype=torch.int32, device=dev) if c["slot"] else None
    part = _nan_f(ref.numel(), torch.float64, dev)
    _launch(L.load().mx_sq_diff_partial(L.current_stream(), d_a.data_ptr(), d_b.data_ptr(), o["a"].shape[1], o["a"].shape[0], part.data_ptr(), _ptr(slot)), c["name"])
    _check_partial(part, ref, bound, f"sq_diff_partial {c['name']}")


# ---- pc_range_copy, copy_rows ----

@pytest.mark.parametrize("c", K.RANGE_COPY_CASES, ids=_ids(K.RANGE_COPY_CASES))
def test_pc_range_copy(cuda_device, c):
    dev = cuda_device
    o = K.build_ranges(c["set"])
    Cc = o["C"]
    want_b, want_s = R.range_copy_ref(o["batch"], o["state"], Cc, o["ranges"], c["to_batch"])
    bbuf, bview, _ = _out(o["batch"], dev)
    sbuf, sview, ld = _out(o["state"], dev, pad=8)
    rng = _ranges(o["ranges"], dev)
    _launch(L.load().mx_pc_range_copy(L.current_stream(), bbuf.data_ptr(), sbuf.data_ptr(), ld, Cc, rng.data_ptr(), len(o["ranges"]), c["to_batch"],
                                      max(r[1] for r in o["ranges"]) * Cc), c["name"])
    _same(bview, want_b, f"pc_range_copy {c['name']}: batch")
    _same(sview, want_s, f"pc_range_copy {c['name']}: state")
    _guards(bbuf, *o["batch"].shape, c["name"])
    _guards(sbuf, *o["state"].shape, c["name"])


@pytest.mark.parametrize("c", K.COPY_ROWS_CASES, ids=_ids(K.COPY_ROWS_CASES))
def test_copy_rows(cuda_device, c):
    dev = cuda_device
    o = K.build_copy_rows(c)
    want_b, want_s = R.copy_rows_ref(o["batch"], o["slotted"], c["slot"], c["scatter"])
    bbuf, bview, _ = _out(o["batch"], dev)
    sbuf, sview, _ = _out(o["slotted"], dev)
    slot = torch.tensor(c["slot"], dtype=torch.int32, device=dev)
    _launch(L.load().mx_copy_rows(L.current_stream(), bbuf.data_ptr(), sbuf.data_ptr(), 16 * c["vectors"], len(c["slot"]), slot.data_ptr(), c["scatter"]), c["name"])
    _same(bview, want_b, f"copy_rows {c['name']}: batch")
    _same(sview, want_s, f"copy_rows {c['name']}: slotted")
    _guards(bbuf, *o["batch"].shape, c["name"])
    _guards(sbuf, *o["slotted"].shape, c["name"])


# ---- the two routes of pc_conv ----

def conv_route_descs(mode, ptr=lambda name: 0x1000):
    """the descriptors of the two routes of pc_conv for CONV_TABLE with every patch asking (splitk = 1 on both sides), as unet_sdxl.cpp builds them:
    (compact, whole, segs, geometry) -- compact: ONE conv over the halo'd patches; whole: the grouped whole-image launch with the corner rule"""
    stride, up = K.CONV_MODES[mode]["stride"], K.CONV_MODES[mode]["up"]
    level = 1 if up else 0                                  # the level of the conv's INPUT; the output's is lo
    lo = level + (1 if stride == 2 else 0) - up
    p_in, p_out = (K.P0 >> level) << up, K.P0 >> lo
    halo = (2, 0) if stride == 2 else (1, 1)
    P = p_in + sum(halo)
    Po = (P + 1) // 2 if stride == 2 else P
    n, Cin, N = len(K.CONV_PATCHES), K.CONV_CIN, K.CONV_N
    d = L.GemmDesc()
    d.a, d.w, d.bias, d.c = ptr("cin"), ptr("w"), ptr("bias"), ptr("cout")
    d.ldc, d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = N, n, P, P, Cin, Po, Po, stride
    d.M, d.N, d.K, d.rows_per_batch, d.ldr, d.splitk = n * Po * Po, N, 9 * Cin, Po * Po, N, 1
    gin, gout = R.geometry(K.CONV_TABLE, level, K.P0), R.geometry(K.CONV_TABLE, lo, K.P0)
    segs = (L.GemmSeg * len(K.CONV_TABLE))()
    for i, (gi, go) in enumerate(zip(gin, gout)):
        s = segs[i]
        s.a, s.c = ptr("x") + 2 * gi.row0 * Cin, ptr("whole") + 2 * go.row0 * N
        s.B, s.Hin, s.Win, s.Hout, s.Wout, s.M, s.rows_per_batch = 1, gi.h, gi.w, go.h, go.w, go.h * go.w, go.h * go.w
    w = L.GemmDesc()
    w.a, w.w, w.bias, w.c = ptr("x"), ptr("w"), ptr("bias"), ptr("whole")
    w.ldc, w.B, w.Hin, w.Win, w.Cin, w.Hout, w.Wout, w.stride, w.up = N, 1, gin[0].h, gin[0].w, Cin, gout[0].h, gout[0].w, stride, up
    w.corner_patch = K.P0 >> (level - up)                   # level_patch(level - up): the output grid's edge at stride 1, the input grid's at stride 2
    w.M, w.N, w.K, w.rows_per_batch, w.ldr, w.splitk = gout[0].h * gout[0].w, N, 9 * Cin, gout[0].h * gout[0].w, N, 1
    w.segs, w.n_segs = segs, len(K.CONV_TABLE)
    return d, w, segs, dict(level=level, lo=lo, p_in=p_in, p_out=p_out, halo=halo, up=up, stride=stride, P=P, Po=Po, gin=gin, gout=gout)


@pytest.mark.parametrize("mode", list(K.CONV_MODES))
def test_conv_routes_agree(cuda_device, mode):
    """pc_conv switches between gather -> ONE conv over the compact halo'd patches -> scatter and the whole-image conv with the corner rule ->
    patch store at a 90 % threshold; with every patch asking and splitk = 1 both must leave the same state.  Both lie inside kernel_ref's fp64
    bound of the literal per-patch conv, and they are compared bit for bit: at these shapes both launches run the same instantiation,
    gemm_v2_kernel<128, 2, true, 0, false> (asserted), which adds a pixel's products in K order whatever the image size; a zero halo cell adds
    exact zeros."""
    dev, lib = cuda_device, L.load()
    Cin, N, n = K.CONV_CIN, K.CONV_N, len(K.CONV_PATCHES)
    _d, _w, _segs, g = conv_route_descs(mode)
    gen = torch.Generator().manual_seed(K.seed_of("conv_" + mode))
    x = K.rand_bf16(gen, (K.level0_rows(K.CONV_TABLE) >> (2 * g["level"]), Cin), emin=-3, emax=2)
    wt = (torch.randn((N, 9 * Cin), generator=gen) * (9 * Cin) ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=gen)
    state0 = K.rand_bf16(gen, (K.SLOTS_A, K.image_elems(K.CONV_TABLE, g["lo"], N)))
    rows_out = K.level0_rows(K.CONV_TABLE) >> (2 * g["lo"])
    t = dict(x=_in(x, dev), w=wt.to(dev), bias=bias.to(dev), cin=R.guarded(n * g["P"] ** 2, Cin, Cin, torch.bfloat16, dev)[0],
             cout=R.guarded(n * g["Po"] ** 2, N, N, torch.bfloat16, dev)[0], whole=R.guarded(rows_out, N, N, torch.bfloat16, dev)[0])
    d, w, segs, g = conv_route_descs(mode, lambda name: t[name].data_ptr())
    kd, kw = L.gemm_kernels_of(d, conv=True), L.gemm_kernels_of(w, conv=True)
    print(f"conv routes {mode}: compact on {kd}, whole on {kw}")
    assert kd == kw and len(kd) == 1, f"{mode}: the routes run {kd} and {kw}: bit equality is a property of one instantiation on both sides"
    samp, lst = _samples(K.CONV_TABLE, dev), _patches(K.CONV_PATCHES, dev)
    st = L.current_stream()
    # route 1: gather -> conv -> scatter
    sa_buf, sa, ld = _out(state0, dev, pad=8)
    _launch(lib.mx_pc_gather(st, t["x"].data_ptr(), Cin, Cin, t["cin"].data_ptr(), lst.data_ptr(), n, samp.data_ptr(), g["level"], g["p_in"], *g["halo"], g["up"]), "gather")
    _launch(lib.mx_conv3x3(st, C.byref(d)), "compact conv")
    _launch(lib.mx_pc_scatter(st, t["cout"].data_ptr(), g["Po"], 1, N, sa_buf.data_ptr(), ld, lst.data_ptr(), n, samp.data_ptr(), g["lo"], g["p_out"]), "scatter")
    # route 2: whole-image conv -> patch store
    sb_buf, sb, _ = _out(state0, dev, pad=8)
    _launch(lib.mx_conv3x3(st, C.byref(w)), "whole-image conv")
    _launch(lib.mx_pc_patch_store(st, t["whole"].data_ptr(), sb_buf.data_ptr(), ld, N, lst.data_ptr(), n, samp.data_ptr(), g["lo"], g["p_out"]), "patch store")
    for name, rows, cols in (("cin", n * g["P"] ** 2, Cin), ("cout", n * g["Po"] ** 2, N), ("whole", rows_out, N)):
        _guards(t[name], rows, cols, f"{mode}: {name}")
    # the literal per-patch conv in fp64: pad-0 conv of the halo'd patch = the interior of the pad-1 conv of it
    halo = R.gather_ref(x, Cin, g["gin"], K.CONV_PATCHES, g["p_in"], *g["halo"], g["up"])
    acc, acc_b = KR.conv_acc(halo, wt, Cin, stride=g["stride"])
    ref, bound = KR.epilogue_ref(acc, acc_b, bias=bias)
    p = g["p_out"]
    ref, bound = (v.reshape(n, g["Po"], g["Po"], N)[:, 1:1 + p, 1:1 + p] for v in (ref, bound))
    owned = torch.zeros(state0.shape, dtype=torch.bool)
    for what, view, buf in (("gather -> conv -> scatter", sa, sa_buf), ("whole-image conv -> patch store", sb, sb_buf)):
        got = view.cpu()
        tiles = torch.stack([R.state_image(got, g["gout"][b], N)[py * p:(py + 1) * p, px * p:(px + 1) * p] for b, py, px in K.CONV_PATCHES])
        bad, ratio = R.violations(tiles, ref, bound)
        print(f"conv routes {mode}: {what}: worst err / bound = {ratio:.3g}")
        assert bad == 0, f"{mode}: {what}: {bad} of {tiles.numel()} elements outside the fp64 bound of the per-patch conv (worst err / bound = {ratio:.3g})"
        for gg in g["gout"]:
            owned[gg.slot, :gg.h * gg.w * N] = True
        assert torch.equal(R.bits(got)[~owned], R.bits(state0)[~owned]), f"{mode}: {what} changed state it does not own"
        _guards(buf, *state0.shape, f"{mode}: {what}")
    _same(sa, sb.cpu(), f"{mode}: the two routes of pc_conv")
