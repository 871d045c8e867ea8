"""Elementwise fp64 comparator for the GEMM / conv / attention kernels, with guarded output buffers and NaN-padded inputs.

The reference is computed in float64 from the bf16 values the kernel actually receives (on the tensors' own device), and every output
element gets its OWN bound, the sum of the rounding steps the kernel's arithmetic can take on the way to it:

  accumulation   fp32 sums of exact bf16 x bf16 products over K terms:        K 2^-24 (|A| |W|^T)_ij    (conv: |x| and |w| of the 3x3 taps)
  epilogue fp32  each fp32 add / multiply after the accumulator (bias, row bias, gate, residual, out_scale): 2^-24 |intermediate| per op
  activation     SiLU / GELU / GELU-tanh / QuickGELU are 1.13-Lipschitz:    1.13 x (bound of the input)
                 plus their own evaluation (__expf / v_rcp / v_exp, the erf polynomial of gelu_fast): ACT_EVAL |x| + 2^-22
  GEGLU          h gelu(g): |gelu(g)| (bound of h) + |h| (1.13 (bound of g) + ACT_EVAL |g| + 2^-22)
  output         bf16 round to nearest: 2^-8 (|ref| + bound so far);  fp32 out: 2^-22 (|ref| + bound so far)
  attention      P rounded to bf16 before P V:                              2^-7 (P |V|)_id
                 scores in fp32 (64 products, log2 domain):                  2 ln2 * 64 2^-23 max_j(|q_i| |k_j|) (P |V|)_id
                 plus the output rounding above

A bound is widened only in the term that names the rounding step that needs the room.  Guards: outputs are allocated with rows past M
and columns up to ld > N, filled with a fixed bit pattern that must come back unchanged bit for bit; inputs carry NaN in their padding,
so a kernel that reads padding produces NaN in its output.
"""
import math

import torch

U32 = 2.0 ** -24               # fp32 unit roundoff
LIP = 1.13                     # Lipschitz bound of SiLU, GELU (erf and tanh forms) and QuickGELU
ACT_EVAL = 2.0 ** -18          # relative evaluation error of the activations (exp / rcp approximations, rounded arguments)
GUARD_BF16 = 0x5A5A            # guard bit patterns (int16 / int32 views)
GUARD_F32 = 0x5A5A5A5A
GUARD_ROWS = 3

SILU, GELU, GELU_TANH, QUICK_GELU = "silu", "gelu", "gelu_tanh", "quick_gelu"


def act_ref(kind, x):
    if kind == SILU:
        return x * torch.sigmoid(x)
    if kind == QUICK_GELU:
        return x * torch.sigmoid(1.702 * x)
    if kind == GELU:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == GELU_TANH:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    raise ValueError(kind)


def act_bound(x, e):
    """bound of act(x~) - act(x) for |x~ - x| <= e, including the activation's own evaluation error"""
    return LIP * e + ACT_EVAL * x.abs() + 2.0 ** -22


# ---- guarded / padded buffers ----

def guarded(rows, cols, ld, dtype, device, guard_rows=GUARD_ROWS):
    """output buffer [rows + guard_rows, ld] filled with the guard pattern; returns (buffer, view [rows, cols])"""
    buf = torch.empty((rows + guard_rows, ld), dtype=dtype, device=device)
    if dtype == torch.bfloat16:
        buf.view(torch.int16).fill_(GUARD_BF16)
    else:
        buf.view(torch.int32).fill_(GUARD_F32)
    return buf, buf[:rows, :cols]


def guard_violations(buf, rows, cols):
    """number of guard elements (rows past `rows`, columns [cols, ld)) whose bits changed"""
    if buf.dtype == torch.bfloat16:
        bits, pat = buf.view(torch.int16), GUARD_BF16
    else:
        bits, pat = buf.view(torch.int32), GUARD_F32
    bad = int((bits[rows:] != pat).sum())
    if cols < buf.shape[1]:
        bad += int((bits[:rows, cols:] != pat).sum())
    return bad


def nan_padded(x, ld, extra_rows=0):
    """x [rows, cols] copied into a NaN-filled buffer [rows + extra_rows, ld]; returns (buffer, view)"""
    rows, cols = x.shape
    buf = torch.full((rows + extra_rows, ld), float("nan"), dtype=x.dtype, device=x.device)
    buf[:rows, :cols] = x
    return buf, buf[:rows, :cols]


# ---- references with per-element bounds ----

def epilogue_ref(acc, acc_bound, *, bias=None, rowbias=None, gate=None, rows_per_batch=0, residual=None, res_bcast=False, out_scale=0.0,
                 act=None, out_f32=False):
    """the fused epilogue of gemm_args.h in its order: (acc + bias) * out_scale -> + row bias -> * gate -> + residual -> activation -> rounding.
    acc / acc_bound: fp64 [M, N].  Returns (ref, bound)."""
    v, e = acc, acc_bound
    M = v.shape[0]
    if bias is not None:
        v = v + bias.double()
        e = e + U32 * v.abs()                                          # fp32 add of the bias
    if out_scale:
        v = v * out_scale
        e = e * abs(out_scale) + U32 * v.abs()                         # fp32 multiply by out_scale
    if rowbias is not None or gate is not None:
        bidx = torch.arange(M, device=v.device) // rows_per_batch
    if rowbias is not None:
        v = v + rowbias.double()[bidx]
        e = e + U32 * v.abs()                                          # fp32 add of the row bias
    if gate is not None:
        g = gate.double()[bidx]
        v = v * g
        e = e * g.abs() + U32 * v.abs()                                # fp32 multiply by the gate
    if residual is not None:
        r = residual.double()
        if res_bcast:
            r = r[torch.arange(M, device=v.device) % rows_per_batch]
        v = v + r
        e = e + U32 * v.abs()                                          # fp32 add of the residual
    if act is not None:
        e = act_bound(v, e)
        v = act_ref(act, v)
    return v, e + (2.0 ** -22 if out_f32 else 2.0 ** -8) * (v.abs() + e)      # output rounding


def gemm_acc(a, w):
    """fp64 A W^T and its fp32-accumulation bound K 2^-24 (|A| |W|^T) from the bf16 operands a [M, K], w [N, K]"""
    a64, w64 = a.double(), w.double()
    K = a.shape[1]
    return a64 @ w64.t(), K * U32 * (a64.abs() @ w64.abs().t())


def geglu_ref(acc, acc_bound, bias, gated_tanh=False):
    """GEGLU of the interleaved layout (weights._geglu_interleave: every 64 features of a 128-wide wave tile are 32 hidden + 32 gate ... see
    hidden_gate_split); returns (ref [M, N/2], bound)"""
    if bias is not None:
        acc = acc + bias.double()
        acc_bound = acc_bound + U32 * acc.abs()
    h, g = hidden_gate_split(acc)
    eh, eg = hidden_gate_split(acc_bound)
    kind = GELU_TANH if gated_tanh else GELU
    ag = act_ref(kind, g)
    v = h * ag
    e = ag.abs() * eh + h.abs() * act_bound(g, eg) + U32 * v.abs()     # fp32 multiply of the hidden by the activated gate
    return v, e + 2.0 ** -8 * (v.abs() + e)


def hidden_gate_split(x):
    """columns of a GEGLU launch's accumulator -> (hidden, gate), each [M, N/2] in output order: within every 64-feature wave panel the first
    32 are hidden features and the last 32 their gates (gemm_epilogue / gemm_epilogue_regs: gate blocks follow the hidden blocks)"""
    M, N = x.shape
    p = x.reshape(M, N // 64, 2, 32)
    return p[:, :, 0, :].reshape(M, N // 2), p[:, :, 1, :].reshape(M, N // 2)


def conv_acc(x, w, Cin, stride=1, up=0, vhalo=0):
    """fp64 3x3 conv (pad 1) of NHWC bf16 x [B, H, W, Cin] with packed w [N, 9 Cin] ((kh, kw, cin) order) and its accumulation bound.
    vhalo: x holds one stored halo row above and below every image ([B, H + 2, W, Cin]); the vertical taps read them instead of zeros"""
    xx = x.double().permute(0, 3, 1, 2)
    if up:
        xx = xx.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    N = w.shape[0]
    w4 = w.double().reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
    K = 9 * Cin

    def conv(xi, wi):
        B, C, H, W = xi.shape
        cols = torch.nn.functional.unfold(xi, 3, padding=(1 - vhalo, 1), stride=stride)          # [B, C*9, L]
        Ho, Wo = (H - 2 * vhalo + stride - 1) // stride, (W + stride - 1) // stride
        out = (wi.reshape(N, -1) @ cols)                                            # [B, N, L]
        return out.permute(0, 2, 1).reshape(B * Ho * Wo, N)

    return conv(xx, w4), K * U32 * conv(xx.abs(), w4.abs())


def attention_ref(q, k, v, scale_log2, causal=False, bias=None):
    """softmax2(scale_log2 q k^T [+ bias]) v in fp64 per head; q [Lq, 64], k [Lk, 64], v [Lk, 64] bf16.  Returns (ref, bound)"""
    q64, k64, v64 = q.double(), k.double(), v.double()
    s = (q64 @ k64.t()) * scale_log2
    if bias is not None:
        s = s + bias.double()
    if causal:
        Lq, Lk = s.shape
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    p = torch.exp2(s - s.max(dim=1, keepdim=True).values)
    p = p / p.sum(dim=1, keepdim=True)
    ref = p @ v64
    pv = p @ v64.abs()
    e_score = 64 * 2.0 ** -23 * abs(scale_log2) * (q64.abs() @ k64.abs().t()).max(dim=1, keepdim=True).values   # fp32 scores, log2 domain
    e = 2.0 ** -7 * pv + 2.0 * math.log(2.0) * e_score * pv                                                     # P to bf16; score rounding
    return ref, e + 2.0 ** -8 * (ref.abs() + e)


def violations(got, ref, bound):
    """(count of elements outside their bound or not finite, worst err / bound)"""
    g = got.double()
    err = (g - ref).abs()
    bad = ~(err <= bound)                       # NaN counts as outside
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max().item() if err.numel() else 0.0
    return int(bad.sum()), ratio


def assert_within(got, ref, bound, what):
    n, ratio = violations(got, ref, bound)
    assert n == 0, f"{what}: {n} of {got.numel()} elements outside their fp64 bound (worst err / bound = {ratio:.3g})"
