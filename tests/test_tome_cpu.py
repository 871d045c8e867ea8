"""Token merging without a GPU: tests/tome_ref.py against a literal gather / scatter_reduce restatement of tomesd's
``bipartite_soft_matching_random2d`` with ``no_rand=True``, and the host-side mx_tome_sizes against the reference's sizes.  Neither tomesd nor
diffusers is installed where the tests run, so the function is restated here from its published source (tomesd/merge.py), step by step."""
import pytest
import torch

import tome_ref


def tomesd_no_rand(metric, w, h, sx, sy, r):
    """tomesd.merge.bipartite_soft_matching_random2d(metric, w, h, sx, sy, r, no_rand=True) -> (merge, unmerge); its argsort calls made stable so
    that the (otherwise unspecified) order inside the two sets is ascending"""
    B, N, _ = metric.shape
    gather = torch.gather
    hsy, wsx = h // sy, w // sx
    rand_idx = torch.zeros(hsy, wsx, 1, dtype=torch.int64)
    idx_buffer_view = torch.zeros(hsy, wsx, sy * sx, dtype=torch.int64)
    idx_buffer_view.scatter_(dim=2, index=rand_idx, src=-torch.ones_like(rand_idx, dtype=rand_idx.dtype))
    idx_buffer = idx_buffer_view.view(hsy, wsx, sy, sx).transpose(1, 2).reshape(hsy * sy, wsx * sx)
    rand_idx = idx_buffer.reshape(1, -1, 1).argsort(dim=1, stable=True)
    num_dst = hsy * wsx
    a_idx, b_idx = rand_idx[:, num_dst:, :], rand_idx[:, :num_dst, :]

    def split(x):
        C = x.shape[-1]
        return gather(x, dim=1, index=a_idx.expand(B, N - num_dst, C)), gather(x, dim=1, index=b_idx.expand(B, num_dst, C))

    metric = metric / metric.norm(dim=-1, keepdim=True)
    a, b = split(metric)
    scores = a @ b.transpose(-1, -2)
    r = min(a.shape[1], r)
    node_max, node_idx = scores.max(dim=-1)
    edge_idx = node_max.argsort(dim=-1, descending=True, stable=True)[..., None]
    unm_idx, src_idx = edge_idx[..., r:, :], edge_idx[..., :r, :]
    dst_idx = gather(node_idx[..., None], dim=-2, index=src_idx)

    def merge(x, mode="mean"):
        src, dst = split(x)
        n, t1, c = src.shape
        unm = gather(src, dim=-2, index=unm_idx.expand(n, t1 - r, c))
        src = gather(src, dim=-2, index=src_idx.expand(n, r, c))
        dst = dst.scatter_reduce(-2, dst_idx.expand(n, r, c), src, reduce=mode)
        return torch.cat([unm, dst], dim=1)

    def unmerge(x):
        unm_len = unm_idx.shape[1]
        unm, dst = x[..., :unm_len, :], x[..., unm_len:, :]
        c = unm.shape[-1]
        src = gather(dst, dim=-2, index=dst_idx.expand(B, r, c))
        out = torch.zeros(B, N, c, dtype=x.dtype)
        out.scatter_(dim=-2, index=b_idx.expand(B, num_dst, c), src=dst)
        out.scatter_(dim=-2, index=gather(a_idx.expand(B, a_idx.shape[1], 1), dim=1, index=unm_idx).expand(B, unm_len, c), src=unm)
        out.scatter_(dim=-2, index=gather(a_idx.expand(B, a_idx.shape[1], 1), dim=1, index=src_idx).expand(B, r, c), src=src)
        return out

    return merge, unmerge


@pytest.mark.parametrize("h,w,sy,sx,ratio", [(8, 8, 2, 2, 0.5), (12, 12, 2, 2, 0.25), (6, 16, 2, 4, 0.75), (9, 8, 3, 2, 0.5), (8, 6, 1, 2, 0.4)])
def test_reference_is_tomesd_without_randomness(h, w, sy, sx, ratio):
    """a per-row function sees the same rows whatever their order: unmerge(f(merge(x))) must agree although the unmerged rows are ordered differently"""
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(2, h * w, 24, generator=g, dtype=torch.float64)
    wf = torch.randn(24, 24, generator=g, dtype=torch.float64)
    f = lambda t: torch.tanh(t @ wf) + t * t                      # noqa: E731
    r = int(h * w * ratio)
    merge, unmerge = tomesd_no_rand(x, w, h, sx, sy, r)
    tables = tome_ref.select(*tome_ref.match(x, h, w, sy, sx), h, w, sy, sx, min(r, tome_ref.sets(h, w, sy, sx)[1].numel()))
    got = tome_ref.unmerge(f(tome_ref.merge(x, tables, h, w, sy, sx)), tables)
    assert (got - unmerge(f(merge(x)))).abs().max().item() <= 1e-12
    assert sorted(tables[0][0].tolist()) != list(range(h * w)), "rows were merged"


def test_sizes_against_the_reference():
    import ctypes as C
    from sduss_amd import lib as _lib
    lib = _lib.load()
    for px in (512, 768, 1024):
        for level in (1, 2):
            for ratio in (0.25, 0.5, 0.75):
                hw = px // 8 >> level
                out = (C.c_int * 4)()
                rc = lib.mx_tome_sizes(hw, hw, 2, 2, C.c_float(ratio), out)
                want = tome_ref.sizes(hw, hw, 2, 2, ratio)
                assert tuple(out) == want and (rc == 0) == (want[2] > 0), (px, level, ratio, tuple(out), want)
                assert want[3] % 64 == 0
                assert px == 768 or want[2] == min(want[1], int(hw * hw * ratio)), "a power-of-two level loses no merge to the 64-row rule"
    out = (C.c_int * 4)()
    assert lib.mx_tome_sizes(9, 8, 2, 2, C.c_float(0.5), out) != 0 and tuple(out) == (0, 0, 0, 72) and tome_ref.sizes(9, 8, 2, 2, 0.5) == (0, 0, 0, 72)
    assert lib.mx_tome_sizes(12, 12, 2, 2, C.c_float(0.5), out) == 0 and tuple(out) == tome_ref.sizes(12, 12, 2, 2, 0.5) == (36, 108, 16, 128)
