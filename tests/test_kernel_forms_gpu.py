"""The form matrix on the GPU: every case of tests/kernel_form_cases.py first asserts (host query, mx_gemm_kernel_name / mx_attention_kernel_name)
that its descriptor resolves to the instantiation it names, then runs it twice -- the two results must be equal bit for bit -- on NaN-padded
inputs into guarded outputs, and compares every element with an fp64 reference within that element's own bound (tests/kernel_ref.py)."""
import ctypes as C
import zlib

import pytest
import torch

import kernel_form_cases as KC
import kernel_ref as R
from sduss_amd import lib as L
from sduss_amd.ops import vt_pos

pytestmark = pytest.mark.gpu

ACTS = {L.EPI_SILU: R.SILU, L.EPI_GELU: R.GELU, L.EPI_GELU_TANH: R.GELU_TANH, L.EPI_QUICK_GELU: R.QUICK_GELU}


def _seed(name):
    return zlib.crc32(name.encode())


def _randn(shape, gen, dev, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float32) * scale).to(dev)


def _ln_apply(acc, e, mean, rstd, rel_rstd, colsum, init_rel):
    """folded LayerNorm: rstd_m (acc - mean_m colsum_n).  The accumulator starts at -mean colsum (fp32 product: init_rel |mean colsum|), the
    epilogue multiplies by rstd (fp32: 2^-24, and rel_rstd of rstd itself where the kernel computes it from the slabs)"""
    mc = mean[:, None] * colsum[None, :]
    v = acc - mc
    ev = e + init_rel * mc.abs()
    out = rstd[:, None] * v
    return out, rstd[:, None] * ev + (rel_rstd[:, None] + R.U32) * out.abs()


def _rms_apply(v, e, w, eps):
    """RMSNorm of every 64-wide head: v rsqrt(mean(v^2) + eps) w.  The factor's relative error is (sum |v| e) / (sum v^2 + 64 eps) from the
    inputs, plus the fp32 sum of 64 squares and rsqrtf (64 2^-24 + 2^-21); two fp32 multiplies"""
    M = v.shape[0]
    vh, eh = v.reshape(M, -1, 64), e.reshape(M, -1, 64)
    ss = (vh * vh).sum(-1, keepdim=True)
    r = 1.0 / torch.sqrt(ss / 64.0 + eps)
    rel = (vh.abs() * eh).sum(-1, keepdim=True) / (ss + 64.0 * eps) + 64 * R.U32 + 2.0 ** -21
    out = vh * r * w.double()
    eo = (r * w.double().abs()) * (eh + vh.abs() * rel) + 2 * R.U32 * out.abs()
    return out.reshape(M, -1), eo.reshape(M, -1)


class _Problem:
    """the operands of one problem (one segment of a grouped launch): logical inputs for the reference, padded / remapped device buffers"""

    def __init__(self, c, M, rpb, gen, dev, ptrs, sfx, keep):
        bf = torch.bfloat16
        N, K, flags = c["N"], c["K"], c["flags"]
        self.M, self.rpb = M, rpb
        conv = c["kind"] == "conv"
        nb = (M + rpb - 1) // rpb if rpb else 1
        self.nb = nb
        if conv:
            H = c["Hin"] + 2 * c["vhalo"]
            x = _randn((c["B"], H, c["Win"], c["Cin"]), gen, dev).to(bf)
            if c["cin_valid"]:
                x[..., c["cin_valid"]:8] = 0                   # the kernel reads channels [0, 8): zero past cin_valid; NaN past 8 (never read)
                x[..., 8:] = float("nan")
            self.x = x
            ptrs["a" + sfx] = x.data_ptr(); keep.append(x)
        else:
            a = _randn((M, K), gen, dev).to(bf)
            if c["ln"]:
                a = (a.float() * 1.5 + 0.7).to(bf)            # a row mean away from zero: the fold's mean * colsum term matters
            self.a = a
            if c["arem"]:
                abr, aoff = c["arem"]
                m = torch.arange(M, device=dev)
                rows = (m // rpb) * abr + aoff + m % rpb
                abuf = torch.full((nb * abr + 2, K + c["lda_pad"]), float("nan"), dtype=bf, device=dev)
                abuf[rows, :K] = a
            elif c["a2"]:
                ks = c["a2"]
                abuf, _ = R.nan_padded(a[:, :ks].contiguous(), ks + c["lda_pad"], extra_rows=2)
                a2buf, _ = R.nan_padded(a[:, ks:].contiguous(), K - ks + c["lda_pad"], extra_rows=2)
                ptrs["a2"] = a2buf.data_ptr(); keep.append(a2buf)
            else:
                abuf, _ = R.nan_padded(a, K + c["lda_pad"], extra_rows=2)   # NaN in columns [K, lda) and in two rows past M
            ptrs["a" + sfx] = abuf.data_ptr(); keep.append(abuf)
        # output rows (joint-sequence remap of C, the residual and the V^T key index)
        m = torch.arange(M, device=dev)
        if c["crem"]:
            cbr, coff = c["crem"]
            self.orow, self.crows = (m // rpb) * cbr + coff + m % rpb, nb * cbr
            self.key = coff + m % rpb
        else:
            self.orow, self.crows = m, M
            self.key = m % rpb if rpb else m
        self.res = self.rb = self.gate = None
        if c["residual"]:
            rrows = rpb if flags & L.EPI_RES_BCAST else M
            self.res = _randn((rrows, N), gen, dev).to(bf)
            rbuf = torch.full((max(self.crows, rrows) + 2, N + c["ldr_pad"]), float("nan"), dtype=bf, device=dev)
            rbuf[self.orow if rrows == M else torch.arange(rrows, device=dev), :N] = self.res
            ptrs["residual" + sfx] = rbuf.data_ptr(); keep.append(rbuf)
        if c["rowbias"]:
            rbb, self.rb = R.nan_padded(_randn((nb, N), gen, dev), N + 4, extra_rows=1)
            ptrs["rowbias" + sfx] = rbb.data_ptr(); keep.append(rbb)
        if c["gate"]:
            gb, self.gate = R.nan_padded(1.0 + _randn((nb, N), gen, dev, 0.5), N + 4, extra_rows=1)
            ptrs["gate" + sfx] = gb.data_ptr(); keep.append(gb)
        if c["ln"] == "stats":
            # slabs of (sum, sum of squares) per row: the row split into ln_slabs column ranges, summed in fp64, stored fp32; entries past the
            # last slab are NaN (never read)
            slabs = c["ln_slabs"]
            pitch = (slabs + 3) & ~3
            st = torch.full((M, pitch, 2), float("nan"), dtype=torch.float32, device=dev)
            a64 = self.a.double()
            for i, part in enumerate(torch.tensor_split(a64, slabs, dim=1)):
                st[:, i, 0], st[:, i, 1] = part.sum(1).float(), (part * part).sum(1).float()
            s1, s2 = st[:, :slabs, 0].double().sum(1), st[:, :slabs, 1].double().sum(1)
            self.mean = s1 / K
            var = (s2 / K - self.mean ** 2).clamp_min(0)
            self.rstd = 1.0 / torch.sqrt(var + 1e-5)
            # the kernel adds the slabs and forms mean / var in fp32: var loses 2^-23 (s2 / K + mean^2) by cancellation, rsqrtf 2^-22
            self.rel_rstd = 0.5 * (slabs + 3) * R.U32 * (s2 / K + self.mean ** 2) / (var + 1e-5) + 2.0 ** -21
            self.ln_init_rel = (slabs + 2) * R.U32
            ptrs["ln_stats" + sfx] = st.data_ptr(); keep.append(st)
        elif c["ln"] == "final":
            fin = torch.stack([_randn((M,), gen, dev, 0.5) + 0.7, 0.5 + torch.rand(M, generator=gen).to(dev)], dim=1).contiguous()
            self.mean, self.rstd = fin[:, 0].double(), fin[:, 1].double()
            self.rel_rstd, self.ln_init_rel = torch.zeros_like(self.mean), R.U32
            ptrs["ln_final"] = fin.data_ptr(); keep.append(fin)
        out_f32 = bool(flags & L.EPI_OUT_F32)
        self.nout = KC.nout_of(c)
        self.cbuf, _ = R.guarded(self.crows, self.nout, self.nout + c["ldc_pad"], torch.float32 if out_f32 else bf, dev)
        ptrs["c" + sfx] = self.cbuf.data_ptr()
        self.vtbuf = None
        if flags & L.EPI_QKV:
            ldvt = KC.ldvt_of(c)
            self.vtbuf, _ = R.guarded(nb * (N // c["period"]), ldvt, ldvt, bf, dev)
            ptrs["vt" + sfx] = self.vtbuf.data_ptr()

    def snapshot(self):
        return self.cbuf.clone(), (self.vtbuf.clone() if self.vtbuf is not None else None)

    def check(self, c, w, bias, colsum, rms_w, snap, what):
        dev = w.device
        flags, N = c["flags"], c["N"]
        out, vt = snap
        geglu, qkv = bool(flags & L.EPI_GEGLU), bool(flags & L.EPI_QKV)
        if c["kind"] == "conv":
            acc, e = R.conv_acc(self.x, w, c["Cin"], c["stride"], c["up"], vhalo=c["vhalo"])
        else:
            acc, e = R.gemm_acc(self.a, w)
        if c["ln"]:
            acc, e = _ln_apply(acc, e, self.mean, self.rstd, self.rel_rstd, colsum.double(), self.ln_init_rel)
        if geglu:
            ref, bound = R.geglu_ref(acc, e, bias, gated_tanh=bool(flags & L.EPI_GEGLU_TANH))
        elif qkv:
            seg, per = c["seg"], c["period"]
            n = torch.arange(N, device=dev)
            pos = (n // seg) % per
            v = acc + bias.double()
            ev = e + R.U32 * v.abs()                                     # fp32 add of the bias
            if c["rms"]:
                for p_, wv in ((0, rms_w[0]), (1, rms_w[1])):
                    cols = pos == p_
                    vv, ee = _rms_apply(v[:, cols], ev[:, cols], wv, 1e-6)
                    v[:, cols], ev[:, cols] = vv, ee
            if c["out_scale"]:
                q = pos == 0                                            # q segments only: fp32 multiply by out_scale
                v[:, q] = v[:, q] * c["out_scale"]
                ev[:, q] = ev[:, q] * abs(c["out_scale"]) + R.U32 * v[:, q].abs()
            ref, bound = v, ev + 2.0 ** -8 * (v.abs() + ev)
        else:
            act = [v_ for f, v_ in ACTS.items() if flags & f]
            ref, bound = R.epilogue_ref(acc, e, bias=bias, rowbias=self.rb, gate=self.gate, rows_per_batch=self.rpb, residual=self.res,
                                        res_bcast=bool(flags & L.EPI_RES_BCAST), out_scale=c["out_scale"], act=act[0] if act else None,
                                        out_f32=bool(flags & L.EPI_OUT_F32))
        written = torch.zeros(out.shape, dtype=torch.bool, device=dev)
        if not qkv:
            written[self.orow, :self.nout] = True
            R.assert_within(out[self.orow, :self.nout], ref, bound, what)
        else:
            seg, per = c["seg"], c["period"]
            n = torch.arange(N, device=dev)
            sidx = n // seg
            grp, pos, nin = sidx // per, sidx % per, n % seg
            isv = pos == per - 1
            ccol = grp * (per - 1) * seg + pos * seg + nin
            got_qk = out[self.orow][:, ccol[~isv]]
            R.assert_within(got_qk, ref[:, ~isv], bound[:, ~isv], what + " (q / k)")
            written[self.orow[:, None], ccol[~isv][None, :]] = True
            nv = N // per
            m = torch.arange(self.M, device=dev)
            key = vt_pos(int(self.key.max()) + 16).to(dev)[self.key]
            vrow = (m // self.rpb)[:, None] * nv + (grp * seg + nin)[isv][None, :]
            kk = key[:, None].expand_as(vrow)
            R.assert_within(vt[vrow, kk], ref[:, isv], bound[:, isv], what + " (V^T)")
            vw = torch.zeros_like(vt, dtype=torch.bool)
            vw[vrow, kk] = True
            assert int(((vt.view(torch.int16) != R.GUARD_BF16) & ~vw).sum()) == 0, f"{what}: the launch wrote into the V^T padding"
        bits = out.view(torch.int16 if out.dtype == torch.bfloat16 else torch.int32)
        pat = R.GUARD_BF16 if out.dtype == torch.bfloat16 else R.GUARD_F32
        assert int(((bits != pat) & ~written).sum()) == 0, f"{what}: the launch wrote outside its output rows / columns"


def run_gemm_case(c, dev):
    gen = torch.Generator().manual_seed(_seed(c["name"]))
    N, K = c["N"], c["K"]
    conv = c["kind"] == "conv"
    ptrs, keep = {}, []
    w = _randn((N, K), gen, dev, K ** -0.5).to(torch.bfloat16)
    if conv and c["cin_valid"]:
        w.view(N, 9, c["Cin"])[..., c["cin_valid"]:8] = 0
        w.view(N, 9, c["Cin"])[..., 8:] = float("nan")                    # (never read by the small-Cin kernel)
    ptrs["w"] = w.data_ptr()
    bias = _randn((N,), gen, dev) if c["bias"] else None
    ptrs["bias"] = bias.data_ptr() if bias is not None else None
    colsum = rms_w = None
    if c["ln"]:
        colsum = _randn((N,), gen, dev, 2.0)
        ptrs["ln_colsum"] = colsum.data_ptr()
    if c["rms"]:
        rms_w = (_randn((64,), gen, dev, 0.3) + 1.0, _randn((64,), gen, dev, 0.3) + 1.0)
        ptrs["rms_wq"], ptrs["rms_wk"] = rms_w[0].data_ptr(), rms_w[1].data_ptr()
    if c["segs"] is None:
        probs = [_Problem(c, c["M"], c["rpb"], gen, dev, ptrs, "", keep)]
    else:
        probs = [_Problem(c, m, rpb, gen, dev, ptrs, str(i), keep) for i, (m, rpb) in enumerate(c["segs"])]
    if conv and c["cin_valid"]:
        for p_ in probs:
            p_.x = p_.x.clone(); p_.x[..., 8:] = 0                         # the reference: channels past 8 are zero (the kernel never reads them)
        w_ref = w.clone(); w_ref.view(N, 9, c["Cin"])[..., 8:] = 0
    else:
        w_ref = w
    d = KC.gemm_desc(c, lambda n: ptrs.get(n))
    assert L.gemm_kernels_of(d, conv) == c["target"], f"{c['name']}: descriptor no longer resolves to {c['target']}"
    lib = L.load()
    if c["splitk"] > 1:
        assert lib.mx_gemm_splitk(C.byref(d), int(conv)) == c["splitk"], f"{c['name']}: the launch is no longer split {c['splitk']} ways"
    launch = lib.mx_conv3x3 if conv else lib.mx_gemm

    def run():
        L.check(launch(L.current_stream(), C.byref(d)), c["name"])
        torch.cuda.synchronize()
        return [p_.snapshot() for p_ in probs]

    s1 = run()
    s2 = run()
    for (c1, v1), (c2, v2) in zip(s1, s2):
        bits = torch.int16 if c1.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(c1.view(bits), c2.view(bits)), f"{c['name']}: two runs differ"
        if v1 is not None:
            assert torch.equal(v1.view(torch.int16), v2.view(torch.int16)), f"{c['name']}: two runs differ (V^T)"
    for i, (p_, snap) in enumerate(zip(probs, s1)):
        p_.check(c, w_ref, bias, colsum, rms_w, snap, c["name"] + (f" problem {i}" if len(probs) > 1 else ""))


@pytest.mark.parametrize("c", KC.GEMM_CASES + KC.CONV_CASES, ids=lambda c: c["name"])
def test_gemm_form(cuda_device, c):
    run_gemm_case(c, cuda_device)


def run_attn_case(c, dev):
    gen = torch.Generator().manual_seed(_seed(c["name"]))
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    bf = torch.bfloat16
    D = H * 64
    scale_log2 = 1.0 if c["pre"] else 0.125 * 1.4426950408889634
    qs = 0.125 * 1.4426950408889634 if c["pre"] else 1.0
    q = _randn((B * Lq, D), gen, dev, qs)
    k = _randn((B * Lk, D), gen, dev)
    v = _randn((B * Lk, D), gen, dev)
    if c["causal"]:
        # scores rise steeply with the key index: q . k = 2 j + noise (exact in bf16), so each row's largest visible score is its diagonal and one
        # leaked future key outweighs everything the row may see
        j = torch.arange(Lk, device=dev, dtype=torch.float32).repeat(B)
        for h in range(H):
            q[:, h * 64] = 32.0; q[:, h * 64 + 1] = 2.0
            k[:, h * 64] = torch.div(j, 16, rounding_mode="floor"); k[:, h * 64 + 1] = j % 16
            q[:, h * 64 + 2:h * 64 + 64] *= 0.1
    q, k, v = q.to(bf), k.to(bf), v.to(bf)
    qbuf, _ = R.nan_padded(q, D + 8 + c["ldq_pad"], extra_rows=0)                  # NaN in the columns past H * 64
    kbuf, _ = R.nan_padded(k, D + 8, extra_rows=16)                                 # ... and in the rows past the last batch's keys
    nch = c["chunks"] or 1
    kc = Lk // nch                              # keys per chunk (the whole sequence without chunks)
    ldvt = KC.vt_ld(kc) + 8
    # V^T image: positions [0, MX_VT_LD(keys)) hold the keys in MX_VT_POS order, zero where no key lands (the kernels read whole 16-key groups
    # and rely on 0 there); the columns past it up to ldvt are NaN
    vt = torch.full((nch, B, D, ldvt), float("nan"), dtype=bf, device=dev)
    vt[..., :KC.vt_ld(kc)] = 0
    vt[..., vt_pos(kc).to(dev)] = v.view(B, nch, kc, D).permute(1, 0, 3, 2)
    if nch > 1:                                 # patch-parallel layout: K rows rank-major, chunk c of batch b at c * B * kc + b * kc
        kbuf, _ = R.nan_padded(k.view(B, nch, kc, D).transpose(0, 1).reshape(B * Lk, D), D + 8, extra_rows=16)
    ldo = D + c["ldo_pad"]
    obuf, _ = R.guarded(B * Lq, D, ldo, bf, dev)
    biasbuf = None
    ldb = (Lk + 63) // 64 * 64
    if c["bias"]:
        biasbuf = torch.zeros((H, Lq, ldb), dtype=torch.float32, device=dev)
        biasbuf[:, :, :Lk] = _randn((H, Lq, Lk), gen, dev)
    assert KC.attn_target_of(c) == c["target"], f"{c['name']}: problem no longer resolves to {c['target']}"
    lib = L.load()
    args = (L.current_stream(), qbuf.data_ptr(), qbuf.shape[1], kbuf.data_ptr(), kbuf.shape[1], vt.data_ptr(), ldvt, D * ldvt, obuf.data_ptr(), ldo, B, H)

    def run():
        if c["causal"]:
            st = lib.mx_attention_prescaled_causal(*args, Lq)
        elif c["bias"]:
            st = lib.mx_attention_prescaled_bias(*args, Lq, Lk, biasbuf.data_ptr(), ldb)
        elif c["cross"]:
            st = lib.mx_attention_cross_prescaled(*args, Lq, Lk)
        elif nch > 1:
            st = lib.mx_attention_prescaled_chunked(*args, Lq, Lk, kc, kc * kbuf.shape[1], B * kc * kbuf.shape[1], B * D * ldvt)
        elif c["pre"]:
            st = lib.mx_attention_prescaled(*args, Lq, Lk)
        else:
            st = lib.mx_attention(*args, Lq, Lk, 0.125)
        L.check(st, c["name"])
        torch.cuda.synchronize()
        return obuf.clone()

    o1 = run()
    o2 = run()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)), f"{c['name']}: two runs differ"
    assert R.guard_violations(o1, B * Lq, D) == 0, f"{c['name']}: the launch wrote outside O[:B*Lq, :H*64]"
    for b in range(B):
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            ref, bound = R.attention_ref(q[b * Lq:(b + 1) * Lq, sl], k[b * Lk:(b + 1) * Lk, sl], v[b * Lk:(b + 1) * Lk, sl], scale_log2,
                                         causal=c["causal"], bias=biasbuf[h, :, :Lk] if c["bias"] else None)
            R.assert_within(o1[b * Lq:(b + 1) * Lq, sl], ref, bound, f"{c['name']} b{b} h{h}")


@pytest.mark.parametrize("c", KC.ATTN_CASES, ids=lambda c: c["name"])
def test_attention_form(cuda_device, c):
    run_attn_case(c, cuda_device)
