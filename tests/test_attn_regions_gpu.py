"""mx_attention_cross_regions, one launch per case, against regions_ref.blend_ref per (batch, head): sum_r w_r ref_r within sum_r |w_r| bound_r.
Sample 0 has one set (the plain short-key arithmetic, bit for bit), sample 1 all of them; padding rows and unused sets are NaN."""
import pytest
import torch

import kernel_ref as R
from regions_ref import blend_ref
from sduss_amd import lib as _lib, ops
from sduss_amd.lib import MxError

pytestmark = pytest.mark.gpu
B, H, D, QS, BF = 2, 2, 128, 0.125 * 1.4426950408889634, torch.bfloat16


def _weights(pattern, gen, n_sets, Lq):
    w = torch.zeros(n_sets, Lq)
    if pattern == "halves":         # disjoint by query index: whole 32-query blocks skip a set
        w[torch.arange(Lq) * n_sets // Lq, torch.arange(Lq)] = 1.0
    elif pattern == "soft":         # every set everywhere, some negative
        w = torch.randn(n_sets, Lq, generator=gen)
    else:                           # single: sets >= 1 weigh exactly one query of a block each
        w[0], r = 1.0, torch.arange(1, n_sets)
        w[r, 3 * r + 1] = 0.7
    return w


def _problem(dev, seed, Lq, seg, n_sets, pattern, dominant=False):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    seg_ld, counts = ops.vt_ld(seg), [1, n_sets]
    q, k, v = rnd(B * Lq, D) * QS, rnd(B, n_sets, seg, D), rnd(B, n_sets, seg, D)
    if dominant:                    # every key of set 1 scores 48 + noise, every key of set 0 0 + noise (log2 domain)
        for h in range(H):
            q[:, h * 64], k[:, 0, :, h * 64], k[:, 1, :, h * 64] = 4.0, 0.0, 12.0
    q, k, v = (t.to(BF).to(dev) for t in (q, k, v))
    kb = torch.full((B, n_sets, seg_ld, D), float("nan"), dtype=BF, device=dev)
    vb = kb.clone()
    w = torch.stack([torch.full((n_sets, Lq), float("nan")), _weights(pattern, gen, n_sets, Lq)])
    for b in range(B):
        kb[b, :counts[b], :seg], vb[b, :counts[b], :seg] = k[b, :counts[b]], v[b, :counts[b]]
    kbuf, _ = R.nan_padded(kb.view(B * n_sets * seg_ld, D), D + 8)
    return dict(q=q, k=k, v=v, kbuf=kbuf, vt=ops.pack_vt(vb.view(B, n_sets * seg_ld, D)), w=w.to(dev), counts=torch.tensor(counts, dtype=torch.int32, device=dev),
                Lq=Lq, seg=seg, n_sets=n_sets)


_launch = lambda p: ops.attention_cross_regions(p["q"], p["kbuf"], p["vt"], p["w"], p["counts"], H, p["Lq"], p["n_sets"], p["seg"])


def _check(o, p, what):
    Lq, seg, n = p["Lq"], p["seg"], p["n_sets"]
    plain = ops.attention_cross(p["q"][:Lq].contiguous(), p["k"][0, 0].contiguous(), ops.pack_vt(p["v"][0, :1].reshape(1, seg, D)), H, Lq, seg)
    assert torch.equal(o[:Lq].view(torch.int16), plain.view(torch.int16)), f"{what}: the one-set sample is not bit-equal to mx_attention_cross_prescaled"
    for h in range(H):
        sl = slice(h * 64, h * 64 + 64)
        ref, bound = blend_ref(p["q"][Lq:, sl], [p["k"][1, r, :, sl] for r in range(n)], [p["v"][1, r, :, sl] for r in range(n)], p["w"][1])
        R.assert_within(o[Lq:, sl], ref, bound, f"{what} h{h}")


@pytest.mark.parametrize("pattern", ["halves", "soft", "single"])
@pytest.mark.parametrize("n_sets", [2, 4])
@pytest.mark.parametrize("seg", [77, 50])
@pytest.mark.parametrize("Lq", [37, 70])
def test_regions_launch(cuda_device, Lq, seg, n_sets, pattern):
    p = _problem(cuda_device, 1000 * Lq + 10 * seg + n_sets, Lq, seg, n_sets, pattern)
    _check(_launch(p), p, f"Lq{Lq} seg{seg} n{n_sets} {pattern}")


@pytest.mark.parametrize("seg", [77, 50])
def test_regions_dominant_set(cuda_device, seg):      # a maximum or a sum shared across the sets would wipe set 0's term out
    p = _problem(cuda_device, 7 + seg, 37, seg, 2, "soft", dominant=True)
    for h in range(H):
        sl = slice(h * 64, h * 64 + 64)
        s = [p["q"][37:, sl].double() @ p["k"][1, r, :, sl].double().t() for r in range(2)]
        assert float(s[1].min()) - float(s[0].max()) >= 30.0
    _check(_launch(p), p, f"dominant seg{seg}")


@pytest.mark.parametrize("what", ["n_sets", "seg_len", "null", "ldvt"])
def test_regions_refusals(cuda_device, what):          # each returns before any launch
    p = _problem(cuda_device, 5, 37, 77, 2, "soft")
    o = torch.empty_like(p["q"])
    n_sets, seg, ldvt = (5 if what == "n_sets" else 2), (97 if what == "seg_len" else 77), (152 if what == "ldvt" else p["vt"].shape[2])
    with pytest.raises(MxError):
        _lib.check(_lib.load().mx_attention_cross_regions(_lib.current_stream(), None if what == "null" else p["q"].data_ptr(), D, p["kbuf"].data_ptr(), D + 8,
                                                          p["vt"].data_ptr(), ldvt, D * p["vt"].shape[2], p["w"].data_ptr(), p["counts"].data_ptr(), o.data_ptr(), D,
                                                          B, H, 37, n_sets, seg), "mx_attention_cross_regions")
