"""mx_attention_cross_ip, one launch per case, against kernel_ref.attention_ref twice per (batch, head): ref_text + s ref_img, bound_text + |s| bound_img."""
import pytest
import torch

import kernel_ref as R
from sduss_amd import ops
from sduss_amd.lib import MxError

pytestmark = pytest.mark.gpu
B, H, D, QS, BF = 2, 2, 128, 0.125 * 1.4426950408889634, torch.bfloat16


def _problem(dev, seed, Lq, Lk, n_img, scales, dominant=False):      # image token rows >= n_img and the V^T positions of those keys are NaN
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = rnd(B * Lq, D) * QS, rnd(B * Lk, D), rnd(B * Lk, D)
    ki, vi = rnd(B, ops.IP_KEYS, D), rnd(B, ops.IP_KEYS, D)
    if dominant:            # image key 0 scores 48 + noise, every text key 0 + noise (log2 domain): a shared maximum or a shared sum wipes the text term out
        for h in range(H):
            q[:, h * 64], k[:, h * 64], ki[:, :, h * 64] = 4.0, 0.0, 0.0
            ki[:, 0, h * 64] = 12.0
    q, k, v, ki, vi = (t.to(BF).to(dev) for t in (q, k, v, ki, vi))
    ki_buf, vi_buf = ki.clone(), vi.clone()
    ki_buf[:, n_img:], vi_buf[:, n_img:] = float("nan"), float("nan")
    k_ip, _ = R.nan_padded(ki_buf.reshape(B * ops.IP_KEYS, D), D + 8)
    return dict(q=q, k=k, v=v, vt=ops.pack_vt(v.view(B, Lk, D)), ki=ki, vi=vi, k_ip=k_ip, vt_ip=ops.pack_vt(vi_buf), Lq=Lq, Lk=Lk, n_img=n_img,
                scale=torch.tensor(scales, dtype=torch.float32, device=dev))


def _check(o, p, what):
    Lq, Lk, n = p["Lq"], p["Lk"], p["n_img"]
    for b in range(B):
        for s, h in ((float(p["scale"][b]), h) for h in range(H)):
            sl = slice(h * 64, h * 64 + 64)
            qh = p["q"][b * Lq:(b + 1) * Lq, sl]
            rt, bt = R.attention_ref(qh, p["k"][b * Lk:(b + 1) * Lk, sl], p["v"][b * Lk:(b + 1) * Lk, sl], 1.0)
            ri, bi = R.attention_ref(qh, p["ki"][b, :n, sl], p["vi"][b, :n, sl], 1.0)
            R.assert_within(o[b * Lq:(b + 1) * Lq, sl], rt + s * ri, bt + abs(s) * bi, f"{what} b{b} h{h}")


_launch = lambda p: ops.attention_cross_ip(p["q"], p["k"], p["vt"], p["k_ip"], p["vt_ip"], p["n_img"], p["scale"], H, p["Lq"], p["Lk"])


@pytest.mark.parametrize("n_img", [1, 4, 16])
@pytest.mark.parametrize("Lk", [77, 50, 96])
@pytest.mark.parametrize("Lq", [37, 64])
def test_ip_launch(cuda_device, Lq, Lk, n_img):
    p = _problem(cuda_device, 1000 * Lq + 10 * Lk + n_img, Lq, Lk, n_img, [0.0, 1.0])
    o = _launch(p)
    _check(o, p, f"Lq{Lq} Lk{Lk} n{n_img}")
    plain = ops.attention_cross(p["q"], p["k"], p["vt"], H, Lq, Lk)
    assert torch.equal(o[:Lq].view(torch.int16), plain[:Lq].view(torch.int16)), "the scale-0 row is not bit-equal to mx_attention_cross_prescaled"
    assert not torch.equal(o[Lq:].view(torch.int16), plain[Lq:].view(torch.int16)), "the scaled row carries no image term"


@pytest.mark.parametrize("Lk,scales,dominant", [(77, [-0.5, 2.0], False), (77, [1.0, 1.0], True), (50, [1.0, 0.5], True)])
def test_ip_scales_and_dominant_image_key(cuda_device, Lk, scales, dominant):
    p = _problem(cuda_device, 7 + Lk, 37, Lk, 4, scales, dominant)
    for h in range(H if dominant else 0):
        sl = slice(h * 64, h * 64 + 64)
        st = p["q"][:, sl].double() @ p["k"][:, sl].double().t()
        si = p["q"].view(B, 37, D)[:, :, sl].double() @ p["ki"][:, 0, sl].double().unsqueeze(2)
        assert float(si.min()) - float(st.max()) >= 30.0
    _check(_launch(p), p, f"Lk{Lk} scales {scales}")


def test_ip_grouped_launch(cuda_device):
    ps = [_problem(cuda_device, 31, 37, 77, 4, [0.0, 1.0]), _problem(cuda_device, 32, 64, 77, 4, [1.5, 0.0])]
    outs = ops.attention_cross_ip_grouped([(p["q"], p["k"], p["vt"], p["k_ip"], p["vt_ip"], p["scale"], p["Lq"], p["Lk"]) for p in ps], H, 4)
    for i, (o, p) in enumerate(zip(outs, ps)):
        _check(o, p, f"grouped problem {i}")


@pytest.mark.parametrize("Lk,n_img", [(97, 4), (77, 17)])
def test_ip_refusals(cuda_device, Lk, n_img):
    p = dict(_problem(cuda_device, 5, 37, Lk, min(n_img, 16), [0.0, 1.0]), n_img=n_img)
    with pytest.raises(MxError):
        _launch(p)
