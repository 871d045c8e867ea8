"""MxUNet.set_adapters / clear_adapters on the GPU: UNetConfig.tiny(), batch 2, 32x32 latents.

The active blob is checked tensor by tensor against the base blob with the rule of tests/lora_ref.py; the forward with an adapter set against the
fp32 oracle (oracle/sdxl_unet_ref.py) evaluated on P + s (alpha / r) B A, within the bound tests/test_unet_gpu.py::_check uses for the plain
forward (4 % of max, 2 % relative L2), and it must differ from the forward WITHOUT the adapter by more than 3x its own error, so that an adapter
that was ignored cannot pass.  Switching sets, clearing and the cross-attention context store are checked bit for bit."""
import pytest
import torch

import lora_ref

pytestmark = pytest.mark.gpu

from oracle import sdxl_unet_ref as ref  # noqa: E402  (checker only)

SCALE_X = 0.1


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd import lora
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    cfg, ocfg = UNetConfig.tiny(), ref.UNetConfig.tiny()
    P = ref.init_params(ocfg)
    net = MxUNet(cfg, P, device="cuda:0")
    targets = sorted(lora.lora_targets(cfg))
    x = lora.LoraAdapter.from_state_dict(cfg, lora_ref.random_adapter_sd(cfg, 21))                      # every target
    some = {m for m in targets if ".attn2." in m or m.endswith("ff.net.0.proj") or m.startswith("mid_block")}
    y = lora.LoraAdapter.from_state_dict(cfg, lora_ref.random_adapter_sd(cfg, 22, ranks=(24, 40), modules=some, prefix="unet."))
    assert 0 < len(y.modules) < len(x.modules)
    s, t, e, te, ti = ref.make_inputs(ocfg, 2, 32)
    inputs = (s.cuda().to(torch.bfloat16), t.cuda(), e.cuda().to(torch.bfloat16), te.cuda(), ti.cuda())
    plain = _forward(net, inputs)
    return dict(cfg=cfg, ocfg=ocfg, P=P, net=net, x=x, y=y, cpu_inputs=(s, t, e, te, ti), inputs=inputs, plain=plain)


def _forward(net, inputs, key=0):
    s, t, e, te, ti = inputs
    net.set_context_key(key)
    return net.forward({"256": s}, t, e, added_cond_kwargs={"text_embeds": te, "time_ids": ti}, return_dict=False, is_sliced=False, patch_size=256,
                       input_indices={"256": ["0", "1"]})[0]["256"].clone()


def _tensor(blob, net, name, dtype):
    off, nb = next((o, n) for nm, o, n in net.weights.names if nm == name)
    return blob[off:off + nb].view(dtype)


def _check_blob(net, adapters, what):
    """every packed tensor of the active blob against the base blob: targeted row ranges by the interval rule, their colsum / bias by their bounds,
    everything else bit-equal"""
    from sduss_amd import lora
    base, active = net.weights.blob, net._lora.active
    terms = lora.scaled_terms(net._lora.layout, adapters)
    by_name = {}
    for t in terms:
        by_name.setdefault(t["packed"], {}).setdefault((t["row0"], t["rows"]), []).append(t)
    checked = 0
    for name, off, nb in net.weights.names:
        b, a = base[off:off + nb], active[off:off + nb]
        stem, kind = name.rsplit(".", 1)
        ranges = by_name.get(stem)
        folded = ranges is not None and "colsum_off" in next(iter(ranges.values()))[0]
        if ranges is None or (kind in ("colsum", "bias") and not folded):
            assert torch.equal(a, b), f"{what}: {name} is not targeted, yet it differs from the base"
            continue
        K = next(iter(ranges.values()))[0]["K"]
        touched = torch.zeros(nb // (2 * K if kind == "weight" else 4), dtype=torch.bool, device=b.device)
        for (row0, rows), ts in ranges.items():
            touched[row0:row0 + rows] = True
            out = a.view(torch.bfloat16).reshape(-1, K)[row0:row0 + rows] if kind == "weight" else a.view(torch.float32)[row0:row0 + rows]
            if kind == "weight":
                lora_ref.check_merge(out, b.view(torch.bfloat16).reshape(-1, K)[row0:row0 + rows], [(t["up"], t["down_t"], t["scale"]) for t in ts],
                                     f"{what}: {name} rows {row0}..{row0 + rows}")
            elif kind == "colsum":
                w = _tensor(active, net, f"{stem}.weight", torch.bfloat16).reshape(-1, K)[row0:row0 + rows]
                lora_ref.check_colsum(out, w, f"{what}: {name}")
            else:
                want = b.view(torch.float32)[row0:row0 + rows].double()
                mag = want.abs()
                for t in ts:
                    want = want + lora_ref.f32_scale(t["scale"]) * t["dbias"].double()
                    mag = mag + abs(t["scale"]) * t["dbias"].double().abs()
                assert bool(((out.double() - want).abs() <= (len(ts) + 1) * lora_ref.U32 * mag).all()), f"{what}: {name}"
                assert not torch.equal(out, b.view(torch.float32)[row0:row0 + rows]), f"{what}: {name} did not move"
            checked += 1
        rest_a = a.view(torch.bfloat16).reshape(-1, K)[~touched] if kind == "weight" else a.view(torch.float32)[~touched]
        rest_b = b.view(torch.bfloat16).reshape(-1, K)[~touched] if kind == "weight" else b.view(torch.float32)[~touched]
        assert torch.equal(rest_a.view(torch.int16 if kind == "weight" else torch.int32), rest_b.view(torch.int16 if kind == "weight" else torch.int32)), \
            f"{what}: {name}: rows outside the targeted ranges differ from the base"
    groups = {(t["packed"], t["row0"]) for t in terms}
    assert checked == len(groups) + 2 * len({(t["packed"], t["row0"]) for t in terms if "colsum_off" in t})


def test_adapter_forward_matches_oracle_on_merged_parameters(tiny):
    from sduss_amd import lora
    net, x = tiny["net"], tiny["x"]
    base_before = net.weights.blob.clone()
    net.set_adapters([(x, SCALE_X)])
    _check_blob(net, [(x, SCALE_X)], "set X")
    assert torch.equal(net.weights.blob, base_before), "the base blob must stay pristine"
    got = _forward(net, tiny["inputs"]).float().cpu()
    want = ref.unet_forward(lora.merged_params(tiny["P"], [(x, SCALE_X)]), tiny["ocfg"], *tiny["cpu_inputs"])
    assert torch.isfinite(got).all()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    l2 = ((got - want).norm() / want.norm()).item()
    moved = (got - tiny["plain"].float().cpu()).abs().max().item()
    print(f"adapter forward: max err {err:.4f} ({err / scale:.4f} of max), rel L2 {l2:.4f}; moved by {moved:.4f} against the plain forward")
    assert err <= 0.04 * scale, f"max err {err} vs scale {scale}"
    assert l2 <= 0.02, f"rel L2 {l2}"
    assert moved > 3 * err, f"the adapter moved the output by {moved}, no more than 3x the error {err}: an ignored adapter would pass"
    # the same set again: merged from the base, not on top of itself
    net.set_adapters([(x, SCALE_X)])
    assert torch.equal(_forward(net, tiny["inputs"]).float().cpu(), got)
    net.clear_adapters()


def test_clear_adapters_restores_the_plain_forward(tiny):
    net = tiny["net"]
    net.set_adapters([(tiny["x"], SCALE_X)])
    assert not torch.equal(_forward(net, tiny["inputs"]), tiny["plain"])
    net.clear_adapters()
    assert torch.equal(_forward(net, tiny["inputs"]), tiny["plain"]), "after clear_adapters the forward must be that of a net that never had an adapter"


def test_set_x_then_y_equals_fresh_y(tiny):
    """X targets every module, Y some of them: what X dirtied and Y does not target is copied back from the base; stacked sets too"""
    from sduss_amd.unet import MxUNet
    net, x, y = tiny["net"], tiny["x"], tiny["y"]
    fresh = MxUNet(tiny["cfg"], tiny["P"], device="cuda:0")
    for second in ([(y, -0.7)], [(y, 0.4), (x, 0.05)], []):
        net.set_adapters([(x, SCALE_X)])
        net.set_adapters(second)
        fresh.set_adapters(second)
        want = fresh._lora.active if fresh._lora.active is not None else fresh.weights.blob
        # (tensor by tensor: the alignment gaps between the packed tensors are never initialised)
        for name, off, nb in net.weights.names:
            assert torch.equal(net._lora.active[off:off + nb], want[off:off + nb]), f"set X then {len(second)} adapters: {name} differs from a fresh net's"
        if second:
            _check_blob(net, second, f"X then {len(second)}")
            assert torch.equal(_forward(net, tiny["inputs"]), _forward(fresh, tiny["inputs"]))
        else:
            assert torch.equal(_forward(net, tiny["inputs"]), tiny["plain"])
    net.clear_adapters()


def test_refused_set_changes_nothing(tiny):
    from sduss_amd import lib, lora
    net, cfg = tiny["net"], tiny["cfg"]
    m = "mid_block.attentions.0.proj_in"
    big = lora.LoraAdapter.from_state_dict(cfg, {f"{m}.lora_A.weight": torch.randn(520, 256), f"{m}.lora_B.weight": torch.randn(256, 520)})
    net.set_adapters([(tiny["y"], 0.3)])
    before = net._lora.active.clone()
    with pytest.raises(lib.MxError, match="MX_LORA_MAX_RANK"):
        net.set_adapters([(big, 1.0)])
    assert torch.equal(net._lora.active, before), "a refused set must leave the active blob as it was"
    net.clear_adapters()


def test_context_store_is_dropped_by_a_switch(tiny):
    """forward announced with a key, then set_adapters, then a forward with the SAME key: it must not be served the K / V^T projected with the old
    weights (X targets attn2.to_k / to_v)"""
    net = tiny["net"]
    net.clear_adapters()
    key = 77001
    first = _forward(net, tiny["inputs"], key=key)
    assert torch.equal(first, tiny["plain"])
    h0, m0 = net.context_stats()
    assert torch.equal(_forward(net, tiny["inputs"], key=key), tiny["plain"]) and net.context_stats() == (h0 + 1, m0), "the key must be stored before the switch"
    net.set_adapters([(tiny["x"], SCALE_X)])
    announced = _forward(net, tiny["inputs"], key=key)
    unannounced = _forward(net, tiny["inputs"])
    assert torch.equal(announced, unannounced), "a stale K / V^T was served after the switch"
    assert not torch.equal(announced, tiny["plain"])
    assert net.context_stats() == (h0 + 1, m0 + 1), "the forward after the switch must project anew"
    net.clear_adapters()
    assert torch.equal(_forward(net, tiny["inputs"], key=key), tiny["plain"]), "nor may the adapter's K / V^T survive clear_adapters"
