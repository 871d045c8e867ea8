"""Cost of changing the LoRA adapter set of a full-width SDXL UNet slot: MxUNet.set_adapters (one mx_lora_merge launch over the packed blob) beside
the only route there was before it, ``pack()`` of the merged parameters on the host plus the upload of a new blob.
Usage, on a machine with the GPU: python tools/lora_swap_bench.py [--out profiles/lora_swap.txt] [--reps 10]
Synthetic adapters of rank 16 and 64 over ALL targets (every linear of the transformer blocks, proj_in, proj_out), two per rank.
Legs:
  (a)  set_adapters alternating between the two sets of a rank (every targeted row range is rewritten from the base each time; nothing is copied
       back, both sets target the same ranges), device events on the stream around each call, after a warm-up of both sets (the first use of an
       adapter places and uploads its factors).  The events span the table copy, the one wait for the stream inside mx_lora_merge and the launch;
  (a') ops.lora_merge alone on the same table and blobs: the launch plus the table copy;
  (b)  lora.merged_params + weights.pack + PackedWeights (the upload), ONCE per rank 64 only: a host clock around work that ends in a device
       synchronise.  It takes tens of seconds; repeating it would measure the same host loop again.
Beside each time of (a) / (a'): the bytes the merge has to move (every targeted row read once and written once; the factors are a few MB and are
left out) over the time, and the HBM floor of those bytes at DESIGN.md section 4's stream rate.  Before timing, the active blob of leg (a) is
compared with the blob of leg (b) matrix by matrix (two roundings apart: the fold's and the merge's)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd import lora, ops, weights  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402

HBM_STREAM = 6.3e12          # the rate its floors are quoted at


def synthetic_adapter(cfg, rank, seed):
    """factors ~ N(0, 1) K^-1/2 and 0.02 N(0, 1): |B A| about a tenth of |W| at rank 64"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for m, t in lora.lora_targets(cfg).items():
        sd[f"{m}.lora_A.weight"] = torch.randn((rank, t.K), generator=g) * t.K ** -0.5
        sd[f"{m}.lora_B.weight"] = 0.02 * torch.randn((t.rows, rank), generator=g)
    return lora.LoraAdapter.from_state_dict(cfg, sd)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tiny", action="store_true", help="UNetConfig.tiny(): a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lora_swap_bench needs the GPU: a time taken elsewhere says nothing"
    from oracle import sdxl_unet_ref as ref
    cfg, ocfg = (UNetConfig.tiny(), ref.UNetConfig.tiny()) if args.tiny else (UNetConfig.sdxl_base(), ref.UNetConfig.sdxl_base())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    P = ref.fast_params(ocfg)
    t0 = time.perf_counter()
    net = MxUNet(cfg, P, device="cuda:0")
    torch.cuda.synchronize()
    say(f"# LoRA swap on {torch.cuda.get_device_name(0)}: {'tiny (rehearsal)' if args.tiny else 'SDXL-base full width'}, blob {net.weights.nbytes / 1e9:.3f} GB, "
        f"{len(lora.lora_targets(cfg))} target linears; building the slot (pack + upload) took {time.perf_counter() - t0:.1f} s")
    parent = None
    for rank in (16, 64):
        sets = [synthetic_adapter(cfg, rank, 100 + rank), synthetic_adapter(cfg, rank, 200 + rank)]
        for ad in sets:                                   # warm-up: placing + upload of the factors, the kernel's code object, the active blob
            net.set_adapters([(ad, 0.8)])
        torch.cuda.synchronize()
        terms = lora.scaled_terms(net._lora.layout, [(sets[0], 0.8)])
        moved = 2 * sum(t["rows"] * t["K"] * 2 for t in terms)
        factor_bytes = sum(t["up"].numel() * 2 + t["down_t"].numel() * 2 for t in terms)
        floor_ms = moved / HBM_STREAM * 1e3
        a_ms, k_ms = [], []
        for i in range(args.reps):
            for ad in sets:
                a_ms.append(event_ms(lambda: net.set_adapters([(ad, 0.8)])))
                k_ms.append(event_ms(lambda: ops.lora_merge(net.weights.blob, net._lora.active, terms, table=net._lora.table)))
        net.set_adapters([(sets[0], 0.8)])
        torch.cuda.synchronize()
        say(f"rank {rank} (padded to {terms[0]['up'].shape[1]}): {len(terms)} terms, {moved / 1e9:.3f} GB read + written, factors {factor_bytes / 1e6:.1f} MB; "
            f"HBM floor at 6.3 TB/s {floor_ms:.3f} ms")
        for name, v in (("(a)  set_adapters", a_ms), ("(a') lora_merge alone", k_ms)):
            med = statistics.median(v)
            say(f"  {name:24s} median {med:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({len(v)} calls)  -> {moved / med / 1e6:7.1f} GB/s, "
                f"{100 * floor_ms / med:5.1f} % of the floor rate")
        if rank == 64:
            t0 = time.perf_counter()
            merged = lora.merged_params(P, [(sets[0], 0.8)])
            t1 = time.perf_counter()
            entries = weights.pack(cfg, merged)
            t2 = time.perf_counter()
            parent = weights.PackedWeights(entries, net.device)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            say(f"  (b)  the repack route        {t3 - t0:8.2f} s   = merged_params {t1 - t0:.2f} s + pack {t2 - t1:.2f} s + upload {t3 - t2:.2f} s   (once)")
            say(f"       set_adapters is {1e3 * (t3 - t0) / statistics.median(a_ms):.0f}x faster than the repack route")
            worst, worst_name = 0.0, ""
            for (name, off, nb), (pname, poff, pnb) in zip(net.weights.names, parent.names):
                assert (name, nb) == (pname, pnb)
                if name.endswith(".weight") and any(t["w_off"] == off for t in terms):
                    a = net._lora.active[off:off + nb].view(torch.bfloat16).float()
                    b = parent.blob[poff:poff + pnb].view(torch.bfloat16).float()
                    rel = float((a - b).norm() / b.norm())
                    if rel > worst:
                        worst, worst_name = rel, name
            say(f"       merged blob against the repacked blob: worst relative L2 over the targeted matrices {worst:.2e} ({worst_name}); bf16 rounds at 2^-9 = 1.95e-03 rms-wise")
    net.clear_adapters()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
