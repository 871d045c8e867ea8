"""Host-only checks of the form matrix and of the fp64 comparator (no GPU: the kernel-name queries are host code, and cu_count() falls back to
the MI355X's 256 CUs without a device)."""
import math

import torch

import kernel_form_cases as KC
import kernel_ref as R
from sduss_amd import lib as L


def test_form_matrix_targets_and_coverage():
    """every case's descriptor resolves to the instantiation it names, and the cases (plus the listed gaps) name exactly the instantiations
    the launchers can start: a new instantiation without a case fails here"""
    for c in KC.GEMM_CASES + KC.CONV_CASES:
        assert KC.gemm_targets_of(c) == c["target"], c["name"]
    for c in KC.ATTN_CASES:
        assert KC.attn_target_of(c) == c["target"], c["name"]
    gemm_names, attn_names = set(L.gemm_kernel_names()), set(L.attention_kernel_names())
    assert len(gemm_names) == len(L.gemm_kernel_names()) and len(attn_names) == len(L.attention_kernel_names())
    covered = {t for c in KC.GEMM_CASES + KC.CONV_CASES for t in c["target"]}
    assert not (covered & KC.NOT_COVERED)
    assert covered | KC.NOT_COVERED == gemm_names
    acovered = {c["target"] for c in KC.ATTN_CASES}
    assert not (acovered & KC.ATTN_NOT_COVERED)
    assert acovered | KC.ATTN_NOT_COVERED == attn_names


def test_kernel_name_queries_follow_the_launch_count():
    """mx_gemm_kernel_name answers one name per launch of mx_gemm (two under the tail split) and 0 past the last"""
    lib = L.load()
    for c in KC.GEMM_CASES:
        d = KC.gemm_desc(c, KC.fake_ptrs())
        assert len(L.gemm_kernels_of(d)) == lib.mx_gemm_launches(d)


def _close(got, want, rel):
    """tests/test_ops_gpu.py's global criterion"""
    return (got - want).abs().max().item() <= rel * (want.abs().max().item() + 1e-6)


def _bf(t):
    return t.to(torch.bfloat16)


def test_comparator_flags_subtle_errors():
    """each of these, added to an exact fp64 product, is flagged by the elementwise bound; the first also passes test_ops_gpu's _close at
    2^-7 -- the gap this comparator closes"""
    g = torch.Generator().manual_seed(7)
    M, N, K = 96, 128, 256
    a = _bf(torch.randn(M, K, generator=g))
    w = _bf(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    rpb = 32
    rowbias = torch.randn(M // rpb, N, generator=g)
    res = _bf(torch.randn(M, N, generator=g))
    acc, e = R.gemm_acc(a, w)
    ref, bound = R.epilogue_ref(acc, e, bias=bias, rowbias=rowbias, rows_per_batch=rpb, residual=res)
    exact_round = ref.float().to(torch.bfloat16).double()
    assert R.violations(exact_round, ref, bound)[0] == 0          # the correctly rounded result passes

    # one 16-column block off by 0.5 % of max|C|
    bad = exact_round.clone()
    bad[:, 48:64] += 0.005 * ref.abs().max()
    assert R.violations(bad, ref, bound)[0] > 0
    assert _close(bad, ref, 2.0 ** -7)                             # the global criterion lets it through

    # one row's row bias taken from the wrong sample
    bad = exact_round.clone()
    bad[5] += rowbias[1].double() - rowbias[0].double()
    assert R.violations(bad, ref, bound)[0] > 0

    # one 64-wide K tile dropped
    a_drop = a.clone()
    a_drop[:, 128:192] = 0
    acc_d, _ = R.gemm_acc(a_drop, w)
    bad, _ = R.epilogue_ref(acc_d, e, bias=bias, rowbias=rowbias, rows_per_batch=rpb, residual=res)
    assert R.violations(bad.float().to(torch.bfloat16).double(), ref, bound)[0] > 0

    # a NaN in an output element / a changed guard
    bad = exact_round.clone()
    bad[3, 7] = math.nan
    assert R.violations(bad, ref, bound)[0] > 0
    buf, view = R.guarded(M, N, N + 8, torch.bfloat16, "cpu")
    view.copy_(exact_round)
    assert R.guard_violations(buf, M, N) == 0
    buf[M + 1, 3] = math.nan
    assert R.guard_violations(buf, M, N) == 1
    buf2, view2 = R.guarded(M, N, N + 8, torch.bfloat16, "cpu")
    buf2[2, N + 5] = 0
    assert R.guard_violations(buf2, M, N) == 1


def test_comparator_attention_bound_flags_a_leaked_key():
    """the causal reference with steep scores: letting row i see key i + 1 moves it far outside the bound"""
    L_ = 65
    g = torch.Generator().manual_seed(3)
    q = torch.randn(L_, 64, generator=g) * 0.01
    k = torch.randn(L_, 64, generator=g) * 0.01
    j = torch.arange(L_, dtype=torch.float32)
    q[:, 0], q[:, 1] = 32.0, 2.0
    k[:, 0], k[:, 1] = torch.div(j, 16, rounding_mode="floor"), j % 16
    v = torch.randn(L_, 64, generator=g)
    q, k, v = _bf(q), _bf(k), _bf(v)
    ref, bound = R.attention_ref(q, k, v, 1.0, causal=True)
    assert R.violations(ref.float().to(torch.bfloat16).double(), ref, bound)[0] == 0
    leak, _ = R.attention_ref(q, k, v, 1.0, causal=False)           # every future key visible
    assert R.violations(leak, ref, bound)[0] > 0
