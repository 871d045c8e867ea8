"""Latency of the VAE decoder step plan (mx_vae_decode) at the SDXL widths, random-init weights.
Usage on the GPU box: python tools/vae_bench.py > gpurun_out/vae_bench.log"""
# Options:
#   --rgb8            only the image leg: latents -> host-resident 8-bit images, the float path (A) against mx_vae_decode_rgb8 (B), alternating
#   --kernels RES B   only N decodes of each kind at one shape, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/vae_bench.py ...)
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd.vae import MxVAEDecoder, VAEConfig  # noqa: E402


def shapes(cfg):
    out = {}
    lc, top = cfg.latent_channels, cfg.block_out_channels[-1]
    out["post_quant_conv.weight"] = (lc, lc, 1, 1); out["post_quant_conv.bias"] = (lc,)
    out["decoder.conv_in.weight"] = (top, lc, 3, 3); out["decoder.conv_in.bias"] = (top,)

    def resnet(p, cin, cout):
        out[f"{p}.norm1.weight"] = (cin,); out[f"{p}.norm1.bias"] = (cin,)
        out[f"{p}.conv1.weight"] = (cout, cin, 3, 3); out[f"{p}.conv1.bias"] = (cout,)
        out[f"{p}.norm2.weight"] = (cout,); out[f"{p}.norm2.bias"] = (cout,)
        out[f"{p}.conv2.weight"] = (cout, cout, 3, 3); out[f"{p}.conv2.bias"] = (cout,)
        if cin != cout:
            out[f"{p}.conv_shortcut.weight"] = (cout, cin, 1, 1); out[f"{p}.conv_shortcut.bias"] = (cout,)
    resnet("decoder.mid_block.resnets.0", top, top)
    a = "decoder.mid_block.attentions.0"
    out[f"{a}.group_norm.weight"] = (top,); out[f"{a}.group_norm.bias"] = (top,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        out[f"{a}.{n}.weight"] = (top, top); out[f"{a}.{n}.bias"] = (top,)
    resnet("decoder.mid_block.resnets.1", top, top)
    c, n = top, len(cfg.block_out_channels)
    for i in range(n):
        cout = cfg.block_out_channels[n - 1 - i]
        for j in range(cfg.layers_per_block + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}", c, cout); c = cout
        if i != n - 1:
            out[f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"] = (c, c, 3, 3); out[f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"] = (c,)
    out["decoder.conv_norm_out.weight"] = (c,); out["decoder.conv_norm_out.bias"] = (c,)
    out["decoder.conv_out.weight"] = (cfg.out_channels, c, 3, 3); out["decoder.conv_out.bias"] = (cfg.out_channels,)
    return out


def _timed(fn):
    """host clock around work fenced by device synchronises on both sides, ms"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _spread(ts):
    q = statistics.quantiles(ts, n=10)
    return f"median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  p10 {q[0]:8.3f}  p90 {q[-1]:8.3f}  max {max(ts):8.3f}", q[-1] - q[0]


def _events(fn, n):
    """device events around n back-to-back calls -> us per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def rgb8_leg(vae, reps=24, warm=3):
    """latents -> host-resident uint8 [n, res, res, 3], two ways in one process, alternating:
      A  the float path: post_inference "pt" (decode fp32, / 2 + 0.5, clamp) -> permute -> .cpu() -> numpy * 255, round, astype(uint8)
      B  post_inference "uint8" (mx_vae_decode_rgb8) -> the pinned copy (MxVAEDecoder.images_to_host)"""
    from sduss_amd import ops
    from sduss_amd.vae import post_inference
    for res, batch in ((512, 1), (1024, 1), (1024, 4)):
        g = torch.Generator().manual_seed(res + batch)
        reqs = {str(res): [SimpleNamespace(latents=torch.randn(1, 4, res // 8, res // 8, generator=g).to(torch.bfloat16).cuda()) for _ in range(batch)]}

        def leg_a():
            img = post_inference(vae, reqs)[str(res)]
            return (img.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")

        def leg_b():
            return vae.images_to_host(post_inference(vae, reqs, output_type="uint8"))[str(res)]

        for _ in range(warm):
            a, b = leg_a(), leg_b()
        diff = abs(a.astype("int16") - b.astype("int16"))
        ta, tb = [], []
        for _ in range(reps):
            ta.append(_timed(leg_a)[0])
            tb.append(_timed(leg_b)[0])
        sa, wa = _spread(ta)
        sb, _wb = _spread(tb)
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"latents -> host uint8 images {res}x{res} batch {batch}, {reps} alternating repetitions after {warm} warm-ups:")
        print(f"  A float path + host quantise : {sa}")
        print(f"  B rgb8 path + pinned copy    : {sb}")
        print(f"  B - A = {mb - ma:+.3f} ms ({(mb / ma - 1) * 100:+.2f} %); p10..p90 spread of A {wa:.3f} ms -> B {'is not' if mb <= ma + wa else 'IS'} slower than A by more than "
              f"A's spread; bytes differing between A and B {float((diff > 0).mean()):.4f}, max {int(diff.max())} level(s)", flush=True)
        # the last launches alone, device events over back-to-back launches at this shape (Cin = block_out_channels[0])
        cin = vae.cfg.block_out_channels[0]
        x = torch.randn(batch, res, res, cin, device="cuda", dtype=torch.bfloat16)
        w = (torch.randn(4, 9 * cin, device="cuda") * (9 * cin) ** -0.5).to(torch.bfloat16)
        bias = torch.zeros(4, device="cuda")
        out = torch.empty((batch, res, res, 3), dtype=torch.uint8, device="cuda")
        t_rgb8 = _events(lambda: ops.conv3x3_rgb8(x, w, bias, out=out), 20)
        t_conv = _events(lambda: ops.conv3x3(x, w, bias), 20)
        print(f"  last launch alone (device events, 20 back-to-back launches): conv3x3_rgb8 {t_rgb8:.1f} us; conv_out as conv3x3_small_n (bf16 NHWC out, "
              f"its nhwc_to_nchw pass not included) {t_conv:.1f} us", flush=True)


def main():
    cfg = VAEConfig.sdxl()
    g = torch.Generator().manual_seed(1)
    P = {}
    for k, s in shapes(cfg).items():
        if len(s) > 1:
            fan = 1
            for d in s[1:]:
                fan *= d
            P[k] = torch.randn(s, generator=g) * fan ** -0.5
        else:
            P[k] = (1.0 if k.endswith("weight") else 0.0) + 0.05 * torch.randn(s, generator=g)
    if "--kernels" in sys.argv:
        i = sys.argv.index("--kernels")
        res, batch = int(sys.argv[i + 1]), int(sys.argv[i + 2])
        vae = MxVAEDecoder(cfg, P, device="cuda:0")
        lat = torch.randn(batch, 4, res // 8, res // 8, device="cuda:0", dtype=torch.bfloat16)
        for _ in range(6):
            vae.decode(lat); vae.decode_images(lat)
        torch.cuda.synchronize()
        return
    if "--rgb8" in sys.argv:
        rgb8_leg(MxVAEDecoder(cfg, P, device="cuda:0"))
        return
    vae = MxVAEDecoder(cfg, P, device="cuda:0", out_dtype=torch.bfloat16)
    for res, batch in ((512, 1), (1024, 1), (1024, 4)):
        lat = torch.randn(batch, 4, res // 8, res // 8, device="cuda:0", dtype=torch.bfloat16)
        for _ in range(2):
            out = vae.decode(lat)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            out = vae.decode(lat)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        print(f"vae decode {res}x{res} batch {batch}: {ms:.2f} ms ({ms / batch:.2f} ms/image), finite {bool(torch.isfinite(out.float()).all())}", flush=True)
    del vae
    rgb8_leg(MxVAEDecoder(cfg, P, device="cuda:0"))


if __name__ == "__main__":
    main()
