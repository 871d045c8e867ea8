"""What the block-skip cache costs and saves at SDXL width (mx_unet_forward_cached, random-init weights, synthetic inputs).
Per batch size: the exact step (mx_unet_forward, graph replay), the cached entry with every block run (the price of the seven
comparisons, the host round trips and the un-captured launch sequence), with the up blocks reused, and with every block reused.
Usage on the GPU box: python tools/block_cache_bench.py > gpurun_out/block_cache_bench.log"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sduss_amd.block_cache import BlockSkipCache  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402
from sduss_amd.weights import synthetic_params  # noqa: E402


class Blocks:
    """run exactly the blocks of `mask`"""
    def __init__(self, mask):
        self.mask = mask

    def predict(self, f):
        f = np.asarray(f)
        return np.full(len(f), (self.mask >> int(f[0, 0])) & 1)


def timed(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    dev = torch.device("cuda:0")
    cfg = UNetConfig.sdxl_base()
    net = MxUNet(cfg, synthetic_params(cfg, device=dev), device=dev)
    print(f"{'batch':>5s} {'px':>5s} {'exact ms':>9s} {'all run':>9s} {'down+mid':>9s} {'down only':>9s} {'none':>9s}")
    for batch, px in ((2, 1024), (8, 1024), (2, 512), (16, 512)):
        hw = px // 8
        g = torch.Generator(device=dev).manual_seed(batch)
        s = torch.randn(batch, 4, hw, hw, device=dev, generator=g).to(torch.bfloat16)
        t = torch.full((batch,), 801.0, device=dev)
        e = torch.randn(batch, 77, cfg.cross_attention_dim, device=dev, generator=g).to(torch.bfloat16)
        te = torch.randn(batch, cfg.text_embed_dim, device=dev, generator=g).to(torch.bfloat16)
        ti = torch.tensor([[px, px, 0, 0, px, px]], device=dev, dtype=torch.float32).repeat(batch, 1)
        row = [timed(lambda: net.forward_one(s, t, e, te, ti))]
        for mask in (0x7f, 0x0f, 0x07, 0x00):
            pred = Blocks(0x7f)
            bc = BlockSkipCache(pred, forced_after=1 << 30)      # the timing wants the same decision every step
            net.forward_one_cached(bc, s, t, e, te, ti, batch_key=1)
            pred.mask = mask
            row.append(timed(lambda: net.forward_one_cached(bc, s, t, e, te, ti, batch_key=1)))
            assert bc.history[-1] == mask
        print(f"{batch:5d} {px:5d} " + " ".join(f"{v:9.2f}" for v in row), flush=True)
        state_mb = bc.state.numel() / 2 ** 20
        print(f"      cache state {state_mb:.0f} MiB", flush=True)


def main_sd3():
    from sduss_amd.block_cache import FORCED_RUN_AFTER_SD3  # noqa: F401
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    from sduss_amd.weights import synthetic_mmdit_params
    dev = torch.device("cuda:0")
    cfg = MMDiTConfig.sd35_medium()
    net = MxSD3Transformer(cfg, synthetic_mmdit_params(cfg, device=dev), device=dev)
    n = cfg.num_layers
    full = (1 << n) - 1
    print(f"SD3.5-medium, {n} blocks")
    print(f"{'batch':>5s} {'px':>5s} {'exact ms':>9s} {'all run':>9s} {'even only':>9s} {'none':>9s}")
    for batch, px in ((2, 1024), (8, 1024), (2, 512)):
        hw = px // 8
        g = torch.Generator(device=dev).manual_seed(batch)
        lat = torch.randn(batch, cfg.in_channels, hw, hw, device=dev, generator=g).to(torch.bfloat16)
        t = torch.full((batch,), 801.0, device=dev)
        e = torch.randn(batch, 333, cfg.joint_attention_dim, device=dev, generator=g).to(torch.bfloat16)
        p = torch.randn(batch, cfg.pooled_projection_dim, device=dev, generator=g).to(torch.bfloat16)
        row = [timed(lambda: net.forward_one(lat, t, e, p))]
        for mask in (full, full & 0x555555555555, 0):
            pred = Blocks(full)
            bc = BlockSkipCache(pred, forced_after=1 << 30)
            net.forward_one(lat, t, e, p, cache=bc, batch_key=1)
            pred.mask = mask
            row.append(timed(lambda: net.forward_one(lat, t, e, p, cache=bc, batch_key=1)))
            assert bc.history[-1] == mask
        print(f"{batch:5d} {px:5d} " + " ".join(f"{v:9.2f}" for v in row), flush=True)
        print(f"      cache state {bc.state.numel() / 2 ** 20:.0f} MiB", flush=True)
        del bc
        torch.cuda.empty_cache()


class Fraction:
    """ask a fixed fraction of the patches of every block, the same ones every step: the first round(f * n) rows of the call (so whole samples
    drop out first, the way a predictor with per-request thresholds behaves), or, spread=True, every k-th patch (every sample keeps some asking
    patches: what costs the per-sample attention problems their batching)"""
    def __init__(self, f, spread=False):
        self.f, self.spread = f, spread

    def predict(self, feats):
        feats = np.asarray(feats)
        n = len(feats)
        out = np.zeros(n, dtype=np.int64)
        k = int(round(self.f * n))
        if self.spread and k > 0:
            out[np.unique(np.linspace(0, n - 1, k).round().astype(int))] = 1
        else:
            out[:k] = 1
        out[feats[:, 2] > 1e18] = 1
        return out


def main_patch_unit():
    """The cache at the reference's unit (mx_unet_forward_cached_mixed, is_sliced=True / patch 256): step time against the fraction of patches that
    ask, SDXL-base.  `exact` = mx_unet_forward_mixed of the same batch (sliced, no cache, graph replay).  Every block runs with the given asking
    fraction: the convolutions, attn1's core + to_out and the whole attn2 scale with it; GroupNorm, LayerNorms, q|k|v, the feed-forward and the
    state copies do not (as in the reference)."""
    from sduss_amd.block_cache import PatchSkipCache
    dev = torch.device("cuda:0")
    cfg = UNetConfig.sdxl_base()
    net = MxUNet(cfg, synthetic_params(cfg, device=dev), device=dev)
    print("patch-unit cache (is_sliced=True, patch 256 px): ms per forward against the asking fraction")
    print(f"{'batch':>14s} {'exact':>8s} " + " ".join(f"{'f=' + str(f):>8s}" for f in (1.0, 0.75, 0.5, 0.25, 0.125, 0.0)) + "   (f = 0.5 spread over all samples)   state MiB")
    for comp in (((2, 1024),), ((8, 1024),), ((2, 512), (2, 768), (2, 1024))):
        g = torch.Generator(device=dev).manual_seed(3)
        xs = [torch.randn(b, 4, px // 8, px // 8, device=dev, generator=g).to(torch.bfloat16) for b, px in comp]
        btot = sum(b for b, _ in comp)
        t = torch.full((btot,), 801.0, device=dev)
        e = torch.randn(btot, 77, cfg.cross_attention_dim, device=dev, generator=g).to(torch.bfloat16)
        te = torch.randn(btot, cfg.text_embed_dim, device=dev, generator=g).to(torch.bfloat16)
        ti = torch.cat([torch.tensor([[px, px, 0, 0, px, px]], device=dev, dtype=torch.float32).repeat(b, 1) for b, px in comp])
        ids = [f"r{i}" for i in range(btot)]
        row = [timed(lambda: net.forward_mixed(xs, t, e, te, ti, gn_patch=32))]
        for f, spread in ((1.0, False), (0.75, False), (0.5, False), (0.25, False), (0.125, False), (0.0, False), (0.5, True)):
            pred = Fraction(1.0)
            pc = PatchSkipCache(pred, forced_after=1 << 30)
            net.forward_mixed_cached(pc, xs, ids, t, e, te, ti, gn_patch=32)
            pred.f, pred.spread = f, spread
            row.append(timed(lambda: net.forward_mixed_cached(pc, xs, ids, t, e, te, ti, gn_patch=32), n=6))
            state = pc.state.numel() / 2 ** 20
            del pc
            torch.cuda.empty_cache()
        name = "+".join(f"{b}x{px}" for b, px in comp)
        print(f"{name:>14s} " + " ".join(f"{v:8.2f}" for v in row[:7]) + f"   {row[7]:8.2f}   {state:8.0f}", flush=True)


def block_threshold_forest(thresholds, n_features):
    """ONE forest for the blocks of `thresholds` (block -> threshold): splits on feature 0, the block index, lead to one threshold chain per
    block (CompiledForest.from_threshold's: run when any input difference exceeds the block's threshold)"""
    from sduss_amd.block_cache import CompiledForest
    left, right, feat, thr, p1 = [], [], [], [], []

    def node(l, r, f, t, p):
        left.append(l); right.append(r); feat.append(f); thr.append(t); p1.append(p)
        return len(left) - 1
    leaf0, leaf1 = node(-1, -1, -2, -2.0, 0.0), node(-1, -1, -2, -2.0, 1.0)
    nxt = leaf1                                              # a block nobody calibrated: run
    for blk in sorted(thresholds, reverse=True):
        on = leaf0
        for k in range(n_features - 1, 1, -1):              # the chain, last feature first: x <= thr goes on, anything larger runs
            on = node(on, leaf1, k, float(thresholds[blk]), 0.0)
        nxt = node(on, nxt, 0, blk + 0.5, 0.0)               # block index <= blk + 0.5: this block's chain (larger indices were split off above)
    return CompiledForest.from_tables(left, right, feat, thr, p1, [nxt], n_features)


def main_decide(where, steps=20):
    """--decide device|host: the patch / chunk-unit cached forward with the decision taken on the device (mx_block_cache.dev_down) or on the host.
    The asking fraction is fixed by calibration: a host pass with QuantilePredictor(q) records the feature rows, each block's threshold is the q
    quantile of its rows' largest input difference, and ONE forest per row width built from those thresholds then serves BOTH paths, so they
    execute the same patches.  Latents drift from step to step by a different amount per patch, cycling through a fixed set."""
    from sduss_amd.block_cache import PatchSkipCache, QuantilePredictor
    dev = torch.device("cuda:0")
    wheres = where.split(",")                                # "host,device,host,device": alternating legs over ONE model and ONE calibration
    assert all(w in ("host", "device") for w in wheres), "--decide device|host"

    def drifting(shape, patch, n_sets, g):
        base = torch.randn(shape, device=dev, generator=g)
        sets = []
        for _ in range(n_sets):
            amp = torch.rand(shape[0], 1, shape[2] // patch, shape[3] // patch, device=dev, generator=g)
            amp = amp.repeat_interleave(patch, 2).repeat_interleave(patch, 3)
            sets.append((base + 0.3 * amp * torch.randn(shape, device=dev, generator=g)).to(torch.bfloat16))
        return sets

    def measure(name, exact, cached, widths, q, n_blocks, mmdit_ctx_len=None):
        if q is None:                                        # asking fraction 1.0: a threshold below every difference
            thr = {b: -1.0 for b in range(n_blocks)}
        else:
            cal = PatchSkipCache(QuantilePredictor(q), forced_after=1 << 30, mmdit_ctx_len=mmdit_ctx_len)
            cal.record_features = True
            for s in range(6):
                cached(cal, s)
            thr = {}
            for f in cal.features[n_blocks:]:                # the first forward is uncached
                m = f[:, 2:].max(axis=1)
                thr.setdefault(int(f[0, 0]), []).append(m)
            thr = {b: float(np.quantile(np.concatenate(v), q)) for b, v in thr.items()}
            del cal
            torch.cuda.empty_cache()
        down = block_threshold_forest(thr, widths[0])
        up = block_threshold_forest(thr, widths[1]) if widths[1] != widths[0] else down
        for leg in wheres:
            pc = PatchSkipCache(down, up, forced_after=1 << 30, mmdit_ctx_len=mmdit_ctx_len, on_device=leg == "device")
            for s in range(3):
                cached(pc, s)
            torch.cuda.synchronize()
            a0, t0n = pc.patches_asked, pc.patches_total
            t0 = time.perf_counter()
            for s in range(steps):
                cached(pc, 3 + s)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            frac = (pc.patches_asked - a0) / max(1, pc.patches_total - t0n)
            ex = timed(exact, n=steps)
            print(f"{name:>30s} decide={leg:6s} target f={1.0 if q is None else 1 - q:4.2f} reached f={frac:5.3f} cached {ms:8.2f} ms   exact {ex:8.2f} ms   "
                  f"cached/exact {ms / ex:5.3f}   ({steps} timed steps)", flush=True)
            del pc
            torch.cuda.empty_cache()

    # ---- SDXL, 8 x 1024^2, patch 256 px ----
    cfg = UNetConfig.sdxl_base()
    net = MxUNet(cfg, synthetic_params(cfg, device=dev), device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    b, px = 8, 1024
    sets = drifting((b, 4, px // 8, px // 8), 32, 5, g)
    t = torch.full((b,), 801.0, device=dev)
    e = torch.randn(b, 77, cfg.cross_attention_dim, device=dev, generator=g).to(torch.bfloat16)
    te = torch.randn(b, cfg.text_embed_dim, device=dev, generator=g).to(torch.bfloat16)
    ti = torch.tensor([[px, px, 0, 0, px, px]], device=dev, dtype=torch.float32).repeat(b, 1)
    ids = [f"r{i}" for i in range(b)]
    exact = lambda: net.forward_mixed([sets[0]], t, e, te, ti, gn_patch=32)
    cached = lambda pc, s: net.forward_mixed_cached(pc, [sets[s % len(sets)]], ids, t, e, te, ti, gn_patch=32)
    n_blocks = 2 * len(cfg.block_out_channels) + 1
    for q in (None, 0.5):
        measure("SDXL 8x1024 patch unit", exact, cached, (3, 2 + cfg.layers_per_block + 2), q, n_blocks)
    del net
    torch.cuda.empty_cache()

    # ---- SD3.5-medium, 1024^2, chunk unit ----
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    from sduss_amd.weights import synthetic_mmdit_params
    mcfg = MMDiTConfig.sd35_medium()
    mnet = MxSD3Transformer(mcfg, synthetic_mmdit_params(mcfg, device=dev), device=dev)
    b, lt = 8, 333
    msets = drifting((b, mcfg.in_channels, px // 8, px // 8), 32, 5, g)
    t = torch.full((b,), 801.0, device=dev)
    e = torch.randn(b, lt, mcfg.joint_attention_dim, device=dev, generator=g).to(torch.bfloat16)
    p = torch.randn(b, mcfg.pooled_projection_dim, device=dev, generator=g).to(torch.bfloat16)
    exact = lambda: mnet.forward_mixed([msets[0]], t, e, p)
    cached = lambda pc, s: mnet.forward_mixed_cached(pc, [msets[s % len(msets)]], ids, t, e, p, 32)
    measure("SD3.5-medium 8x1024 chunk unit", exact, cached, (3, 3), 0.5, mcfg.num_layers, mmdit_ctx_len=lt)


if __name__ == "__main__":
    if "--decide" in sys.argv:
        main_decide(sys.argv[sys.argv.index("--decide") + 1])
    elif len(sys.argv) > 1 and sys.argv[1] == "patch":
        main_patch_unit()
    else:
        main()
        main_sd3()
        main_patch_unit()
