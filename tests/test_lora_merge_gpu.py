"""The LoRA merge kernel (mx_lora_merge through ops.lora_merge) one launch at a time, against tests/lora_ref.py: every output element inside
[rn_bf16(v - tol), rn_bf16(v + tol)] of the fp64 value, colsum within its fp32 bound and the same bits on every launch, nothing written outside
the targeted rows.  The blobs are kernel_ref.guarded buffers: the active one is pre-filled with the guard pattern, so every byte the launch did not
write is still that pattern; a "blob" here is [matrix N x K bf16][colsum N fp32][bias N fp32], the vectors in whole rows of K after the matrix."""
import pytest
import torch

import kernel_ref as R
import lora_ref

pytestmark = pytest.mark.gpu


def _blobs(N, K, dev, seed, integer=False):
    """(base buffer, active buffer, total rows, colsum_off, bias_off, W bf16 [N, K], bias fp32 [N]): the base holds W and the bias, NaN elsewhere"""
    g = torch.Generator().manual_seed(seed)
    vrows = (2 * N * 4 + K * 2 - 1) // (K * 2)
    rows = N + vrows
    w = (torch.randint(-31, 32, (N, K), generator=g).float() if integer else 0.03 * torch.randn((N, K), generator=g)).to(torch.bfloat16).to(dev)
    bias = (0.05 * torch.randn(N, generator=g)).to(dev)
    base = torch.full((rows, K), float("nan"), dtype=torch.bfloat16, device=dev)
    base[:N] = w
    cs_off, b_off = N * K * 2, N * K * 2 + N * 4
    base.view(torch.uint8).reshape(-1)[b_off:b_off + 4 * N] = bias.view(torch.uint8)
    buf, _view = R.guarded(rows, K, K, torch.bfloat16, dev)
    return base, buf, rows, cs_off, b_off, w, bias


def _factors(rows, K, r, dev, seed):
    g = torch.Generator().manual_seed(seed)
    up = (0.05 * torch.randn((rows, r), generator=g)).to(torch.bfloat16).to(dev)
    down_t = (0.05 * torch.randn((K, r), generator=g)).to(torch.bfloat16).to(dev)
    dbias = (0.02 * torch.randn(rows, generator=g)).to(dev)
    return up, down_t, dbias


def _f32_at(buf, off, n):
    return buf.view(torch.uint8).reshape(-1)[off:off + 4 * n].clone().view(torch.float32)


def _untouched(buf, spans):
    """every byte of the buffer (guard rows included) outside ``spans`` still holds the guard pattern"""
    bits = buf.view(torch.int16).reshape(-1).clone()
    for off, nb in spans:
        bits[off // 2:(off + nb) // 2] = R.GUARD_BF16
    return int((bits != R.GUARD_BF16).sum()) == 0


def _run(cuda_device, N, K, ranks, scales, row0=0, rows=None, folded=True, seed=0):
    from sduss_amd import ops
    rows = N - row0 if rows is None else rows
    base, buf, total_rows, cs_off, b_off, w, bias = _blobs(N, K, cuda_device, seed)
    terms, ref_terms, fs = [], [], []
    for i, (r, s) in enumerate(zip(ranks, scales)):
        up, down_t, dbias = _factors(rows, K, r, cuda_device, 100 * seed + i)
        t = dict(w_off=0, N=N, K=K, row0=row0, rows=rows, up=up, down_t=down_t, scale=s)
        if folded:
            t.update(colsum_off=cs_off, bias_off=b_off)
            if i % 2 == 0:                      # (a term of a folded matrix may come without a bias delta)
                t["dbias"] = dbias
        terms.append(t)
        ref_terms.append((up, down_t, s))
        fs.append((s, dbias if "dbias" in t else None))
    ops.lora_merge(base, buf[:total_rows], terms)
    torch.cuda.synchronize()
    spans = [(row0 * K * 2, rows * K * 2)] + ([(cs_off + 4 * row0, 4 * rows), (b_off + 4 * row0, 4 * rows)] if folded else [])
    assert _untouched(buf, spans), "the launch wrote outside the targeted rows (matrix, vectors or guard)"
    out = buf[row0:row0 + rows].clone()
    what = f"lora_merge {N}x{K} rows {row0}..{row0 + rows} ranks {ranks}"
    lora_ref.check_merge(out, w[row0:row0 + rows], ref_terms, what)
    cs = bvec = None
    if folded:
        cs, bvec = _f32_at(buf, cs_off + 4 * row0, rows), _f32_at(buf, b_off + 4 * row0, rows)
        lora_ref.check_colsum(cs, out, what)
        want = bias[row0:row0 + rows].double()
        mag = want.abs()
        for s, d in fs:
            if d is not None:
                want = want + lora_ref.f32_scale(s) * d.double()
                mag = mag + abs(s) * d.double().abs()
        assert bool(((bvec.double() - want).abs() <= (len(fs) + 1) * lora_ref.U32 * mag).all()), f"{what}: folded bias"
    return out, cs, bvec, w


@pytest.mark.parametrize("N,K,ranks,scales", [
    (16, 64, (32,), (1.0,)),                         # smallest: one tile, one chunk, three idle waves
    (80, 192, (32,), (0.7,)),                        # odd counts: two 32-row blocks and a 16-row tail, three k chunks for four waves
    (320, 2048, (32, 64), (0.8, -1.3)),              # SDXL's narrowest N at the context K, two adapters stacked
    (64, 320, (64,), (-0.5,)),                       # five chunks: one wave takes two
])
def test_merge_whole_matrix(cuda_device, N, K, ranks, scales):
    for folded in (False, True):
        _run(cuda_device, N, K, ranks, scales, folded=folded, seed=N + K)


def test_merge_row_range_leaves_the_other_rows(cuda_device):
    """rows 128 .. 256 of a 384-row matrix (attn1.to_k inside to_qkv): the other rows, their colsum / bias entries and the guards keep the pattern"""
    _run(cuda_device, 384, 128, (32,), (1.1,), row0=128, rows=128, seed=7)
    _run(cuda_device, 384, 128, (32, 32), (1.1, 0.3), row0=256, rows=128, folded=False, seed=8)


def test_merge_without_effect_is_bit_equal_to_base(cuda_device):
    from sduss_amd import ops
    N, K = 96, 128
    base, buf, total_rows, cs_off, b_off, w, bias = _blobs(N, K, cuda_device, 3)
    active = base.clone()
    ops.lora_merge(base, active, [])                                     # no terms: nothing is launched, the active blob stays what it was
    torch.cuda.synchronize()
    assert torch.equal(active.view(torch.int16), base.view(torch.int16))
    up, down_t, dbias = _factors(N, K, 32, cuda_device, 4)
    ops.lora_merge(base, buf[:total_rows], [dict(w_off=0, N=N, K=K, up=up, down_t=down_t, scale=0.0, colsum_off=cs_off, bias_off=b_off, dbias=dbias)])
    torch.cuda.synchronize()
    assert torch.equal(buf[:N].view(torch.int16), w.view(torch.int16)), "scale 0 must reproduce the base bits"
    assert torch.equal(_f32_at(buf, b_off, N), bias)
    lora_ref.check_colsum(_f32_at(buf, cs_off, N), buf[:N], "scale 0")
    assert R.guard_violations(buf, total_rows, K) == 0


def test_merge_is_bit_stable(cuda_device):
    a = _run(cuda_device, 320, 2048, (32, 64), (0.8, -1.3), seed=11)
    b = _run(cuda_device, 320, 2048, (32, 64), (0.8, -1.3), seed=11)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "colsum must have the same bits on every launch"
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_merge_exact_integers_asymmetric(cuda_device):
    """Integer-valued, asymmetric factors whose every partial sum is an integer below 256: fp32 and the final bf16 rounding are exact, so out must
    EQUAL v.  A transposed or permuted fragment map (rows of up against rows of down_t, the k order inside a lane's 16 bytes, the two MFMAs of a
    half chunk) moves integers to other places and cannot pass."""
    from sduss_amd import ops
    N, K, r = 48, 128, 32
    base, buf, total_rows, cs_off, b_off, w, _bias = _blobs(N, K, cuda_device, 5, integer=True)
    n, k, j = torch.arange(N)[:, None], torch.arange(K)[:, None], torch.arange(r)[None, :]
    up = (((n * 3 + j * 5) % 7) - 3).to(torch.bfloat16).to(cuda_device)               # |up| <= 3
    down_t = (((k * 2 + j * 3 + (k // 8)) % 5) - 2).to(torch.bfloat16).to(cuda_device)   # |down| <= 2: |sum| <= 192, |v| <= 223
    ops.lora_merge(base, buf[:total_rows], [dict(w_off=0, N=N, K=K, up=up, down_t=down_t, scale=1.0, colsum_off=cs_off, bias_off=b_off)])
    torch.cuda.synchronize()
    v = w.double() + up.double() @ down_t.double().t()
    assert float(v.abs().max()) < 256
    got = buf[:N].double()
    assert torch.equal(got, v), f"{int((got != v).sum())} of {v.numel()} integers differ"
    assert torch.equal(_f32_at(buf, cs_off, N).double(), v.sum(dim=1)), "integer row sums are exact in fp32"
    assert R.guard_violations(buf, total_rows, K) == 0
