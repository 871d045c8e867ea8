"""Cost of self-attention guidance: mx_attention_colmass and mx_sag_degrade at the shapes an SDXL-base step at 4 x 1024 px gets, and the whole
SDXLDenoiser.denoising_step of that batch with 0, 1 and 4 SAG requests.
Usage, on a machine with the GPU: python tools/sag_bench.py [--out profiles/sag.txt] [--reps 30] [--tiny]
Every comparison alternates its sides window by window in ONE process (same clocks, same thermal state), device events around each window, after a
warm-up of all of them; reported: median [p10 .. p90] per call.  A launch window is 20 back-to-back launches between one pair of events.
  launch: mx_attention_colmass (both launches) at B 4, 20 heads, L 1024 beside the plain self-attention launch of those rows; mx_sag_degrade at
          4 x 4 x 128 x 128 bf16 latents with a 32 x 32 mask; mx_sag_fold on the same rows.
  step:   one denoising_step of four 1024 px requests (their step index put back each time), 0 / 1 / 4 of them with set_sag(0.75).
The weights are random, so nothing here says what SAG does to an image: only times are reported.
The file's last section ("headline step ...") is not measured here: it is the ms_per_step of `python bench.py --gpus 1 --steps 20 --warmup 3` in
this tree and in a checkout of the parent commit, alternating.  A run with --out keeps it as it is."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import ops  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.pipeline import SDXLDenoiser, synthetic_request  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402
from hypertile_bench import alternate, fmt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny() and small launches: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sag_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev, bf = "cuda:0", torch.bfloat16
    say(f"# Self-attention guidance on {torch.cuda.get_device_name(0)}{' (tiny rehearsal)' if args.tiny else ''}")
    B, H, hm, lat = (2, 4, 10, 40) if args.tiny else (4, 20, 32, 128)
    L, D = hm * hm, H * 64
    qk = torch.randn(B * L, 2 * D, device=dev).to(bf)
    q, k = qk[:, :D], qk[:, D:]
    qc, kc = q.contiguous(), k.contiguous()         # (ops.attention takes whole buffers; the step plan hands the kernel the same views as colmass gets)
    vt = ops.pack_vt(torch.randn(B, L, D, device=dev).to(bf))
    x, eps = torch.randn(B, 4, lat, lat, device=dev).to(bf), torch.randn(2 * B, 4, lat, lat, device=dev).to(bf)
    sig = torch.full((B,), 3.0, device=dev)
    mask = ops.attention_colmass(q, k, H, B, prescaled=True)[1].view(B, hm, hm)
    eps_d = torch.randn(B, 4, lat, lat, device=dev).to(bf)
    names = [f"colmass B {B} H {H} L {L}", "plain attention of those rows", f"degrade {B} x 4 x {lat} x {lat}", "fold"]
    fns = [lambda: ops.attention_colmass(q, k, H, B, prescaled=True), lambda: ops.attention(qc, kc, vt, H, L, L, prescaled=True),
           lambda: ops.sag_degrade(x, eps, sig, mask, 1.0), lambda: ops.sag_fold_(eps, eps_d, [0.15] * B)]
    say(f"launch: median [p10 .. p90] over {args.reps} windows of 20 calls, alternating (each call includes its output allocation)")
    for n, t in zip(names, alternate(fns, args.reps, 20)):
        say(f"  {n:36s} {fmt(t, 1e3, 'us')}")
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    net = MxUNet(cfg, ref.fast_params(ocfg), device=dev)
    res, nreq = (lat * 8, 4)
    den = SDXLDenoiser(net, guidance_scale=5.0)
    reqs = [synthetic_request(i, res, 20, cfg, den, dev) for i in range(nreq)]
    start = [r.latents.clone() for r in reqs]

    def step(n_sag):
        def run():
            for i, r in enumerate(reqs):
                den.set_sag(r, 0.75 if i < n_sag else 0.0)
                r.step_index, r.latents = 0, start[i]
            den.denoising_step({str(res): reqs})
        return run
    modes = [0, 1, nreq]
    reps = max(args.reps // 3, 5)
    say(f"step: denoising_step of {nreq} requests at {res} px (batch {2 * nreq} forward); median [p10 .. p90] over {reps} alternating steps")
    times = alternate([step(m) for m in modes], reps, 1)
    base = statistics.median(times[0])
    for m, tt in zip(modes, times):
        say(f"  {m} SAG requests {fmt(tt, 1.0, 'ms')}   {statistics.median(tt) - base:+.2f} ms, ratio {statistics.median(tt) / base:.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if os.path.exists(args.out):       # the section that is not this tool's (docstring) stays
            old = open(args.out).read().splitlines()
            at = next((i for i, ln in enumerate(old) if ln.startswith("headline step")), len(old))
            lines += old[at:]
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
