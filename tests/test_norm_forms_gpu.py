"""The normalisation matrix on the GPU: every case of tests/norm_form_cases.py is called through the C ABI (ctypes, not the ops wrappers, which
size their buffers tightly) on NaN-padded inputs into guarded outputs, twice -- the two results must be equal bit for bit -- and every
output element is compared with the fp64 reference within that element's own bound (tests/norm_ref.py).  Each case prints its worst
err / bound; profiles/norm_forms_ratios.txt holds the table of one full run.  The test_row_forms_* tests hold the forms of the one row-norm
skeleton against each other on the raw bits."""
import ctypes as C

import pytest
import torch

import norm_form_cases as NC
import norm_ref as R
from sduss_amd import lib as L

pytestmark = pytest.mark.gpu

GUARD_BYTE = 0x5A               # every byte of a guard: R.GUARD_BF16 / R.GUARD_F32 seen as int16 / int32


def _flat_guarded(n, dtype, dev, tail=64):
    """n elements of an output followed by `tail` guard elements (any dtype: NCHW outputs, whose planes may hold an odd count)"""
    buf = torch.empty(n + tail, dtype=dtype, device=dev)
    buf.view(torch.uint8).fill_(GUARD_BYTE)
    return buf


def _flat_guard_violations(buf, n):
    return int((buf[n:].view(torch.uint8) != GUARD_BYTE).sum())


def _nan_tail(t, tail=16):
    """a contiguous copy of t followed by NaN: what a kernel reads past the end of an operand shows up in its output"""
    buf = torch.full((t.numel() + tail,), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _nan_ws(nbytes, dev):
    return torch.full((nbytes // 4 + 64,), float("nan"), dtype=torch.float32, device=dev)


class _Run:
    """one case: buffers, the launch, and what to compare.  launch() fills self.out = {name: (guarded buffer, view of the output)}"""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.p = NC.build(c, dev)
        self.lib = L.load()
        self.keep = []
        getattr(self, "_prep_" + c["kind"])()

    def _rows_out(self, names, M, Ccols, dtype=torch.bfloat16, ld=None):
        self.out = {n: R.guarded(M, Ccols, ld or Ccols, dtype, self.dev) for n in names}
        self.rows, self.cols = M, Ccols

    # ---- row norms ----
    def _prep_ln(self):
        c, p = self.c, self.p
        self.x, _ = R.nan_padded(p["x"], c["C"], extra_rows=2)
        self.g, self.b = (_nan_tail(p["gamma"]), _nan_tail(p["beta"])) if c["affine"] else (None, None)
        self._rows_out(["y"], c["M"], c["C"])
        self.call = lambda: self.lib.mx_layernorm(L.current_stream(), self.x.data_ptr(), self.out["y"][0].data_ptr(), _ptr(self.g), _ptr(self.b), c["M"], c["C"], p["eps"])

    def _mod_ptrs(self):
        c, p = self.c, self.p
        Cc = c["C"]
        self.ldmod = 6 * Cc + 4
        self.mod, _ = R.nan_padded(p["mod"], self.ldmod, extra_rows=1)
        base = self.mod.data_ptr()
        shift, scale, shift2, scale2 = (base + 4 * j * Cc for j in (0, 1, 3, 4))
        M = p["x"].shape[0]
        self.x, _ = R.nan_padded(p["x"], Cc, extra_rows=2)
        self._rows_out(["y", "y2"] if c["dual"] else ["y"], M, Cc)
        y2 = self.out["y2"][0].data_ptr() if c["dual"] else None
        return M, (L.current_stream(), self.x.data_ptr(), self.out["y"][0].data_ptr(), y2, scale, shift, scale2 if c["dual"] else None, shift2 if c["dual"] else None, self.ldmod)

    def _prep_lnmod(self):
        c, p = self.c, self.p
        M, head = self._mod_ptrs()
        self.call = lambda: self.lib.mx_layernorm_mod(*head, M, c["C"], c["rpb"], p["eps"])

    def _prep_lnmod_grouped(self):
        c, p = self.c, self.p
        _M, head = self._mod_ptrs()
        n = len(c["batches"])
        bt, rp = (C.c_int * n)(*c["batches"]), (C.c_int * n)(*c["rpbs"])
        self.keep += [bt, rp]
        self.call = lambda: self.lib.mx_layernorm_mod_grouped(*head, c["C"], p["eps"], C.cast(bt, C.c_void_p), C.cast(rp, C.c_void_p), n)

    def _prep_rms(self):
        c, p = self.c, self.p
        self.x, _ = R.nan_padded(p["x"], c["C"], extra_rows=2)
        self.w = _nan_tail(p["w"])
        self._rows_out(["y"], c["M"], c["C"])
        self.call = lambda: self.lib.mx_rmsnorm(L.current_stream(), self.x.data_ptr(), self.out["y"][0].data_ptr(), self.w.data_ptr(), c["M"], c["C"], p["eps"])

    def _prep_rms_heads(self):
        c, p = self.c, self.p
        rows, ld = p["buf"].shape
        self.buf, view = R.guarded(rows, ld, ld, torch.bfloat16, self.dev)          # in place: the operand itself sits in front of the guard rows
        self.wq, self.wk = _nan_tail(p["wq"]), _nan_tail(p["wk"])
        self.out = {}

        def call():
            view.copy_(p["buf"])
            return self.lib.mx_rmsnorm_heads(L.current_stream(), self.buf.data_ptr(), ld, c["nbatch"], c["rpb"], c["batch_rows"], c["row_off"], c["ht"], c["hq"],
                                             self.wq.data_ptr(), self.wk.data_ptr(), p["eps"], p["q_scale"])
        self.call = call

    def _prep_row_stats(self):
        c, p = self.c, self.p
        self.x, _ = R.nan_padded(p["x"], c["C"] + 8, extra_rows=2)
        self._rows_out(["stats"], c["M"], 2, torch.float32, ld=8)
        self.call = lambda: self.lib.mx_row_stats(L.current_stream(), self.x.data_ptr(), c["C"] + 8, self.out["stats"][0].data_ptr(), c["M"], c["C"])

    # ---- NHWC GroupNorm ----
    def _nhwc_operand(self, x, c1):
        """x [B, H, W, C] -> (x pointer, x2 pointer): one source, or the two contiguous sources of a concatenation, NaN behind each"""
        Cc = x.shape[-1]
        if not c1:
            a, _ = R.nan_padded(x.reshape(-1, Cc), Cc, extra_rows=2)
            self.keep.append(a)
            return a.data_ptr(), None
        a, _ = R.nan_padded(x[..., :c1].reshape(-1, c1), c1, extra_rows=2)
        b, _ = R.nan_padded(x[..., c1:].reshape(-1, Cc - c1), Cc - c1, extra_rows=2)
        self.keep += [a, b]
        return a.data_ptr(), b.data_ptr()

    def _prep_gn(self):
        c, p = self.c, self.p
        B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
        xa, xb = self._nhwc_operand(p["x"], c["c1"])
        self.g, self.b = _nan_tail(p["gamma"]), _nan_tail(p["beta"])
        self.ws = _nan_ws(self.lib.mx_groupnorm_nhwc_workspace_bytes(B, H, W, Cc), self.dev)
        self._rows_out(["y"], B * H * W, Cc)

        def call():
            self.ws.fill_(float("nan"))
            return self.lib.mx_groupnorm_nhwc_cat(L.current_stream(), xa, c["c1"] or Cc, xb, self.out["y"][0].data_ptr(), self.g.data_ptr(), self.b.data_ptr(),
                                                  B, H, W, Cc, c["groups"], p["eps"], int(c["silu"]), c["patch"], self.ws.data_ptr())
        self.call = call

    def _prep_gn_grouped(self):
        c, p = self.c, self.p
        Cc, n = c["C"], len(c["probs"])
        self.g, self.b = _nan_tail(p["gamma"]), _nan_tail(p["beta"])
        probs = (L.GnProblem * n)()
        self.out, self.srcs = {}, []
        for i, (x, (b, h, w)) in enumerate(zip(p["xs"], c["probs"])):
            xa, xb = self._nhwc_operand(x, c["c1"])
            self.out[f"y{i}"] = R.guarded(b * h * w, Cc, Cc, torch.bfloat16, self.dev)
            probs[i].x, probs[i].x2, probs[i].y = xa, xb, self.out[f"y{i}"][0].data_ptr()
            probs[i].B, probs[i].H, probs[i].W = b, h, w
            self.srcs.append((xa, xb))
        self.keep.append(probs)
        self.ws = _nan_ws(self.lib.mx_groupnorm_nhwc_grouped_workspace_bytes(probs, n, Cc), self.dev)

        def call():
            self.ws.fill_(float("nan"))
            return self.lib.mx_groupnorm_nhwc_grouped(L.current_stream(), probs, n, c["c1"] or Cc, self.g.data_ptr(), self.b.data_ptr(), Cc, c["groups"], p["eps"],
                                                      int(c["silu"]), c["patch"], self.ws.data_ptr())
        self.call = call

    def separate_launches(self):
        """every problem of a grouped case through mx_groupnorm_nhwc_cat on its own: {name: output}"""
        c, p = self.c, self.p
        Cc = c["C"]
        res = {}
        for i, ((xa, xb), (b, h, w)) in enumerate(zip(self.srcs, c["probs"])):
            buf, view = R.guarded(b * h * w, Cc, Cc, torch.bfloat16, self.dev)
            ws = _nan_ws(self.lib.mx_groupnorm_nhwc_workspace_bytes(b, h, w, Cc), self.dev)
            L.check(self.lib.mx_groupnorm_nhwc_cat(L.current_stream(), xa, c["c1"] or Cc, xb, buf.data_ptr(), self.g.data_ptr(), self.b.data_ptr(), b, h, w, Cc,
                                                   c["groups"], p["eps"], int(c["silu"]), c["patch"], ws.data_ptr()), c["name"])
            torch.cuda.synchronize()
            assert R.guard_violations(buf, b * h * w, Cc) == 0
            res[f"y{i}"] = view.clone()
        return res

    def _prep_gn_partials(self):
        c, p = self.c, self.p
        B, H, W, Cc = c["B"], c["H"], c["W"], c["C"]
        xa, _ = self._nhwc_operand(p["x"], 0)
        self.g, self.b = _nan_tail(p["gamma"]), _nan_tail(p["beta"])
        self.part = _nan_tail(p["part"])
        self.bias = _nan_tail(p["bias"]) if c["bias"] else None
        self.ws = _nan_ws(self.lib.mx_groupnorm_nhwc_workspace_bytes(B, H, W, Cc), self.dev)
        self._rows_out(["y"], B * H * W, Cc)

        def call():
            self.ws.fill_(float("nan"))
            return self.lib.mx_groupnorm_nhwc_from_partials(L.current_stream(), xa, self.out["y"][0].data_ptr(), self.g.data_ptr(), self.b.data_ptr(), B, H, W, Cc,
                                                            c["groups"], p["eps"], int(c["silu"]), self.part.data_ptr(), c["chunk"], _ptr(self.bias),
                                                            _ptr(p["rbbuf"]), Cc + 8 if c["rowbias"] else 0, self.ws.data_ptr())
        self.call = call

    # ---- NCHW GroupNorm + halo ----
    def _prep_gn_nchw(self):
        c, p = self.c, self.p
        _n, Cc, cpg, H, W = c["shape"]
        N, pad = NC.NCHW_N, c["padding"]
        dt = p["x"].dtype
        self.x = _nan_tail(p["x"])
        self.g, self.b = _nan_tail(p["gamma"]), _nan_tail(p["beta"])
        self.oshape = (N, Cc, H + 2 * pad, W + 2 * pad)
        self.n_out = N * Cc * self.oshape[2] * self.oshape[3]
        self.ybuf = _flat_guarded(self.n_out, dt, self.dev)
        self.out = {}
        lo = torch.tensor(NC.NCHW_LAT_OFF, dtype=torch.int32, device=self.dev)
        pm = torch.tensor(NC.NCHW_PMAP, dtype=torch.int32, device=self.dev)
        self.pidx = p["pidx"].to(self.dev)
        self.ws = _nan_ws(self.lib.mx_groupnorm_halo_workspace_bytes(N, Cc, cpg), self.dev)
        self.keep += [lo, pm]

        def call():
            self.ws.fill_(float("nan"))
            return self.lib.mx_groupnorm_halo(L.current_stream(), self.x.data_ptr(), self.g.data_ptr(), self.b.data_ptr(), self.ybuf.data_ptr(), N, Cc, H, W, cpg,
                                              float(p["eps"]), pad, lo.data_ptr(), len(NC.NCHW_LAT_OFF) - 1, pm.data_ptr(), self.pidx.data_ptr(),
                                              L.torch_dtype_code(dt), self.ws.data_ptr())
        self.call = call

    # ---- run and compare ----
    def launch(self):
        L.check(self.call(), self.c["name"])
        torch.cuda.synchronize()
        k = self.c["kind"]
        if k == "rms_heads":
            return {"buf": self.buf.clone()}
        if k == "gn_nchw":
            return {"buf": self.ybuf.clone()}
        return {n: buf.clone() for n, (buf, _v) in self.out.items()}

    def check(self, snap):
        """guards, the cells that must not change, and every output inside its bound; returns the worst err / bound"""
        c, p = self.c, self.p
        name, k = c["name"], c["kind"]
        ref = R.reference(c, p)
        worst = 0.0
        if k == "rms_heads":
            buf = snap["buf"]
            rows, ld = p["buf"].shape
            D = 64 * c["ht"]
            assert R.guard_violations(buf, rows, ld) == 0, f"{name}: the launch wrote past the last row"
            touched = torch.zeros((rows, ld), dtype=torch.bool, device=self.dev)
            touched[p["rows"], :D] = True
            same = _bits(buf[:rows]) == _bits(p["buf"])
            assert bool((same | touched).all()), f"{name}: a row outside the range or a padding column changed"
            got = {"y": buf[:rows][p["rows"], :D]}
        elif k == "gn_nchw":
            buf = snap["buf"]
            assert _flat_guard_violations(buf, self.n_out) == 0, f"{name}: the launch wrote past the last plane"
            got = {"y": buf[:self.n_out].view(self.oshape)}
        else:
            got = {}
            for n, buf in snap.items():
                rows, cols = self.out[n][1].shape
                assert R.guard_violations(buf, rows, cols) == 0, f"{name} {n}: the launch wrote outside its output"
                got[n] = buf[:rows, :cols]
        for n, (r, b) in ref.items():
            g = got[n].reshape(r.shape)
            R.assert_within(g, r, b, f"{name} {n}")
            worst = max(worst, R.violations(g, r, b)[1])
        return worst


@pytest.mark.parametrize("c", NC.ALL_CASES, ids=lambda c: c["name"])
def test_norm_form(cuda_device, c):
    run = _Run(c, cuda_device)
    s1 = run.launch()
    s2 = run.launch()
    for n in s1:
        assert torch.equal(_bits(s1[n]), _bits(s2[n])), f"{c['name']} {n}: two runs differ"
    ratio = run.check(s1)
    print(f"NORM_RATIO {c['name']:<34s} worst err / bound = {ratio:.3f}")
    if c["kind"] == "gn_grouped":                                   # the grouped launch equals the separate launches bit for bit
        for n, y in run.separate_launches().items():
            rows, cols = y.shape
            assert torch.equal(_bits(s1[n][:rows, :cols]), _bits(y)), f"{c['name']} {n}: grouped != separate"


# ---- the forms of the one row-norm skeleton (row_norm_kernel<VPL, CENTRE, Store>) against each other, on the raw bits ----
FORM_WIDTHS = [8, 520, 1024, 1032, 1544, 2056, 4096]        # every rung of with_vpl, ragged and full last chunks


class _RowForms:
    """rows [M, C] and one modulation matrix [B, 6 C + 4] (shift | scale | NaN ..., as _Run._mod_ptrs lays it out), both NaN-padded; every launch
    writes fresh guarded outputs and returns their bits"""

    def __init__(self, Cc, M, B, dev, zero_mod=False):
        gen = torch.Generator().manual_seed(NC.seed_of(f"row_forms_{Cc}_{M}"))
        self.lib, self.C, self.dev, self.ldmod = L.load(), Cc, dev, 6 * Cc + 4
        self.x, _ = R.nan_padded(NC.rows_input("a", M, Cc, gen).to(dev), Cc, extra_rows=2)
        mod = torch.full((B, self.ldmod), float("nan"))
        mod[:, :Cc] = 0.0 if zero_mod else torch.randn(B, Cc, generator=gen)
        mod[:, Cc:2 * Cc] = 0.0 if zero_mod else torch.randn(B, Cc, generator=gen) * 0.3
        self.mod, _ = R.nan_padded(mod.to(dev), self.ldmod, extra_rows=1)

    def _launch(self, M, n_out, call):
        outs = [R.guarded(M, self.C, self.C, torch.bfloat16, self.dev) for _ in range(n_out)]
        L.check(call(*[buf.data_ptr() for buf, _v in outs]), "row form")
        torch.cuda.synchronize()
        for buf, _v in outs:
            assert R.guard_violations(buf, M, self.C) == 0, "the launch wrote outside its output"
        return [_bits(v).clone() for _buf, v in outs]

    def _x(self, row0):
        return self.x.data_ptr() + 2 * row0 * self.C

    def _mod_args(self, b0, dual):
        shift = self.mod.data_ptr() + 4 * b0 * self.ldmod
        scale = shift + 4 * self.C
        return (scale, shift) + ((scale, shift) if dual else (None, None)) + (self.ldmod,)

    def ln(self, M, eps, gamma=None, beta=None):
        return self._launch(M, 1, lambda y: self.lib.mx_layernorm(L.current_stream(), self._x(0), y, _ptr(gamma), _ptr(beta), M, self.C, eps))[0]

    def mod_rows(self, M, rpb, eps, dual=False, row0=0, b0=0):
        """mx_layernorm_mod on rows [row0, row0 + M), whose first sample is b0; dual: the second output takes the same scale / shift slices"""
        return self._launch(M, 2 if dual else 1, lambda y, y2=None: self.lib.mx_layernorm_mod(
            L.current_stream(), self._x(row0), y, y2, *self._mod_args(b0, dual), M, self.C, rpb, eps))

    def grouped(self, batches, rpbs, eps):
        n, M = len(batches), sum(b * r for b, r in zip(batches, rpbs))
        bt, rp = (C.c_int * n)(*batches), (C.c_int * n)(*rpbs)
        return self._launch(M, 1, lambda y: self.lib.mx_layernorm_mod_grouped(
            L.current_stream(), self._x(0), y, None, *self._mod_args(0, False), self.C, eps,
            C.cast(bt, C.c_void_p), C.cast(rp, C.c_void_p), n))[0]


@pytest.mark.parametrize("Cc", FORM_WIDTHS)
def test_row_forms_plain_normalisation(cuda_device, Cc):
    """a zero modulation and the unit affine are the plain LayerNorm: n * (1 + 0) + 0 == n * 1 + 0 == the gamma == nullptr form"""
    M = 5 + (Cc // 8) % 3
    f = _RowForms(Cc, M, M, cuda_device, zero_mod=True)
    plain = f.ln(M, NC.MOD_EPS)
    assert torch.equal(f.mod_rows(M, 1, NC.MOD_EPS)[0], plain), "zero modulation != plain LayerNorm"
    ones, zeros = _nan_tail(torch.ones(Cc, device=cuda_device)), _nan_tail(torch.zeros(Cc, device=cuda_device))
    assert torch.equal(f.ln(M, NC.MOD_EPS, ones, zeros), plain), "gamma = 1, beta = 0 != plain LayerNorm"


@pytest.mark.parametrize("Cc", FORM_WIDTHS)
def test_row_forms_second_output_and_one_group(cuda_device, Cc):
    """y2 with y's own scale / shift is y, and y does not depend on y2 being asked for; a grouped launch of one group is the ungrouped launch"""
    B, rpb = 3, 2
    f = _RowForms(Cc, B * rpb, B, cuda_device)
    y = f.mod_rows(B * rpb, rpb, NC.MOD_EPS)[0]
    y_dual, y2 = f.mod_rows(B * rpb, rpb, NC.MOD_EPS, dual=True)
    assert torch.equal(y_dual, y), "y changes when a second output is written"
    assert torch.equal(y2, y), "y2 with the same scale / shift != y"
    assert torch.equal(f.grouped([B], [rpb], NC.MOD_EPS), y), "grouped launch with n = 1 != mx_layernorm_mod"


@pytest.mark.parametrize("Cc", FORM_WIDTHS)
def test_row_forms_groups_equal_their_own_launch(cuda_device, Cc):
    """every group of a mixed batch equals mx_layernorm_mod on that group's rows alone, its modulation rows starting at b0 * ldmod"""
    batches, rpbs = [1, 2, 3], [7, 1, 4]
    f = _RowForms(Cc, sum(b * r for b, r in zip(batches, rpbs)), sum(batches), cuda_device)
    y = f.grouped(batches, rpbs, NC.MOD_EPS)
    r0 = b0 = 0
    for b, r in zip(batches, rpbs):
        alone = f.mod_rows(b * r, r, NC.MOD_EPS, row0=r0, b0=b0)[0]
        assert torch.equal(y[r0:r0 + b * r], alone), f"group at row {r0} != its own launch"
        r0, b0 = r0 + b * r, b0 + b


@pytest.mark.parametrize("dn", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", NC.NCHW_SHAPES, ids=lambda s: s[0])
def test_halo_only_is_bit_exact(cuda_device, shape, dn):
    """mx_halo_only on the asymmetric table: pure data movement, bit for bit, nothing written past the last plane"""
    dev = cuda_device
    _n, Cc, _cpg, H, W = shape
    N, dt = NC.NCHW_N, NC.DTYPES[dn]
    x = NC.nchw_input(shape, dt, torch.Generator().manual_seed(NC.seed_of("halo" + shape[0] + dn))).to(dev)
    pidx = NC.asymmetric_table(N)
    xb = _nan_tail(x)
    n_out = N * Cc * (H + 2) * (W + 2)
    ybuf = _flat_guarded(n_out, dt, dev)
    pd = pidx.to(dev)
    L.check(L.load().mx_halo_only(L.current_stream(), xb.data_ptr(), ybuf.data_ptr(), N, Cc, H, W, pd.data_ptr(), L.torch_dtype_code(dt)), "mx_halo_only")
    torch.cuda.synchronize()
    assert _flat_guard_violations(ybuf, n_out) == 0
    want = R.halo_gather(x, pidx)
    assert torch.equal(_bits(ybuf[:n_out].view(want.shape)), _bits(want))
