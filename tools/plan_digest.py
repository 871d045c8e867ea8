"""sha256 of what the UNet's and the MMDiT's entry points write, for seeded inputs: the counterpart of `bench.py --dump-outputs` for the entry
points the benchmark does not run (mixed, trace, per-sample and per-patch / per-chunk block cache, patch-parallel).  Two builds of the library (MXDENOISE_LIB selects
one) that issue the same launches print the same lines; a host-side change of the step plan that moves one launch changes a line.
Usage, on a machine with the GPU: python tools/plan_digest.py > digest.txt     (prints `case -> digest`, one line per output tensor)"""
import hashlib
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import sd3_mmdit_ref as mref, sdxl_unet_ref as ref  # noqa: E402  (inputs and parameters only)
from sduss_amd.block_cache import BlockSkipCache, PatchSkipCache, ThresholdPredictor  # noqa: E402
from sduss_amd.config import MMDiTConfig, UNetConfig  # noqa: E402
from sduss_amd.transformer_sd3 import MxSD3Transformer  # noqa: E402
from sduss_amd.unet import MxUNet  # noqa: E402


def say(case, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        raw = t.contiguous().view(torch.uint8).cpu().numpy().tobytes()
        print(f"{case}{'' if len(tensors) == 1 else f'[{i}]'} -> {hashlib.sha256(raw).hexdigest()}", flush=True)


def inputs(ocfg, batch, hw, seed=0):
    s, t, e, te, ti = ref.make_inputs(ocfg, batch, hw, seed=seed)
    return [s.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), te.cuda(), ti.cuda()]


def mixed_inputs(ocfg, spec, seed):
    ins = [inputs(ocfg, b, hw, seed + i) for i, (b, hw) in enumerate(spec)]
    return [x[0] for x in ins], [torch.cat([x[k] for x in ins]) for k in range(1, 5)]


class Script:
    """a predictor whose answers are set from outside: `mask(n)` gives the rows that ask"""
    mask = staticmethod(lambda n: np.ones(n))

    def predict(self, f):
        return np.asarray(self.mask(len(f)))


def tiny_cases():
    ocfg = ref.UNetConfig.tiny()
    net = MxUNet(UNetConfig.tiny(), ref.init_params(ocfg), device="cuda:0")
    x = inputs(ocfg, 2, 32)
    for gp in (0, 16, 8):
        say(f"forward_one b2 32x32 gn_patch {gp}", net.forward_one(*x, gn_patch=gp))
    spec = [(1, 16), (2, 24), (1, 32)]
    xs, cond = mixed_inputs(ocfg, spec, 10)
    for gp in (0, 8):
        say(f"forward_mixed 16/24/32 gn_patch {gp}", *net.forward_mixed(xs, *cond, gn_patch=gp))
    for stage, shape in (("up_blocks.0.resnets.1", (2 * 8 * 8, 256)), ("down_blocks.1.attentions.0", (2 * 16 * 16, 128)), ("conv_out", (2 * 32 * 32, 4))):
        say(f"trace {stage}", net.forward_one(*x, stage=stage, stage_shape=shape))

    # per-sample block cache under the scripted masks of tests/test_block_cache_gpu.py::test_partial_reuse_recomputes_only_what_was_asked
    pred, up = Script(), Script()
    bc = BlockSkipCache(pred, up)
    x1 = inputs(ocfg, 2, 32, 1)
    say("forward_one_cached all run", net.forward_one_cached(bc, *x, batch_key=9))
    up.mask = lambda n: np.zeros(n)
    say("forward_one_cached up blocks reused", net.forward_one_cached(bc, x1[0], *x[1:], batch_key=9))
    pred.mask = up.mask
    say("forward_one_cached none run", net.forward_one_cached(bc, x1[0], *x[1:], batch_key=9))
    pred.mask = lambda n: np.ones(n)
    up.mask = lambda n: np.eye(n)[-1]
    say("forward_one_cached last sample asks for the up blocks", net.forward_one_cached(bc, x1[0], *x[1:], batch_key=9))

    # per-patch cache over the mixed batch: 4 + 2 * 9 + 16 = 38 patches of 8 x 8 latent pixels
    pred = Script()
    pc = PatchSkipCache(pred, forced_after=1 << 30, max_latent=32)
    ids = ["a", "b", "c", "d"]
    step = lambda seed: net.forward_mixed_cached(pc, mixed_inputs(ocfg, spec, seed)[0], ids, *cond, gn_patch=8)
    say("forward_mixed_cached first step (nothing cached: all ask)", *step(10))
    say("forward_mixed_cached all ask", *step(11))
    pred.mask = lambda n: np.zeros(n)
    say("forward_mixed_cached none asks", *step(12))
    pred.mask = lambda n: (np.arange(n) % 13 == 5).astype(np.int64)
    say("forward_mixed_cached 3 of 38 ask (compact conv)", *step(13))
    pred.mask = lambda n: (np.arange(n) % 13 != 5).astype(np.int64)
    say("forward_mixed_cached 35 of 38 ask (whole-image fallback)", *step(14))
    print(f"forward_mixed_cached blocks run {[hex(h) for h in pc.history]}, {pc.patches_asked} of {pc.patches_total} patch-blocks asked", flush=True)

    # one group whose patch covers it (two 16 x 16 latents, gn_patch 16): the cache's unit stays 16 where a plain forward would run gn_patch 0
    pred = Script()
    pc = PatchSkipCache(pred, forced_after=1 << 30, max_latent=16)
    cond1 = mixed_inputs(ocfg, [(2, 16)], 20)[1]
    step = lambda seed: net.forward_mixed_cached(pc, mixed_inputs(ocfg, [(2, 16)], seed)[0], ["e", "f"], *cond1, gn_patch=16)
    say("forward_mixed_cached one covered group, first step (nothing cached: all ask)", *step(20))
    say("forward_mixed_cached one covered group, all ask", *step(21))
    pred.mask = lambda n: np.zeros(n)
    say("forward_mixed_cached one covered group, none asks", *step(22))
    print(f"forward_mixed_cached one covered group blocks run {[hex(h) for h in pc.history]}, {pc.patches_asked} of {pc.patches_total} patch-blocks asked", flush=True)


def pp_unet_outs():
    """tests/test_pp_gpu.py::test_two_ranks_equal_one_rank's shape"""
    from sduss_amd.patch_parallel import PatchParallelUNet
    ocfg = ref.UNetConfig.tiny()
    net = MxUNet(UNetConfig.tiny(), ref.init_params(ocfg), device="cuda:0")
    x0 = inputs(ocfg, 2, 64)
    x1 = inputs(ocfg, 2, 64, 1)[0]
    outs = [("synchronous", PatchParallelUNet(net).forward(*x0))]
    for mode in ("stale_gn", "corrected_async_gn"):
        pp = PatchParallelUNet(net, mode=mode, warmup_steps=0)
        outs += [(f"{mode} warm-up", pp.forward(*x0)), (f"{mode} stale step", pp.forward(x1, *x0[1:]))]
        pp.reset()
    return outs


def pp_mmdit_outs():
    """tests/test_pp_gpu.py::test_sd3_two_ranks_equal_one_rank_and_stale_steps' shape"""
    from sduss_amd.patch_parallel import PatchParallelSD3
    ocfg = mref.MMDiTConfig.tiny()
    net = MxSD3Transformer(MMDiTConfig.tiny(), mref.init_params(ocfg), device="cuda:0")
    x0 = sd3_inputs(ocfg, 2, 32, lt=77)
    x1 = sd3_inputs(ocfg, 2, 32, 1, lt=77)[0]
    pp = PatchParallelSD3(net, mode="stale_gn", warmup_steps=0)
    outs = [("mmdit synchronous", PatchParallelSD3(net).forward(*x0)), ("mmdit stale_gn warm-up", pp.forward(*x0)), ("mmdit stale_gn stale step", pp.forward(x1, *x0[1:]))]
    pp.reset()
    return outs


def pp_rank(rank, world, port, model):
    """both ranks on cuda:0, exchanging through gloo"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.set_num_threads(8)
    torch.cuda.set_device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        outs = pp_unet_outs() if model == "unet" else pp_mmdit_outs()
        for r in range(world):                   # rank by rank, so that the lines come out in one order
            if r == rank:
                for what, t in outs:
                    say(f"pp rank {rank} of {world} {what}", t)
            dist.barrier()
    finally:
        dist.destroy_process_group()


def pp_cases(model="unet"):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [mp.get_context("spawn").Process(target=pp_rank, args=(r, 2, port, model)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        if p.exitcode != 0:
            raise SystemExit(f"patch-parallel rank ended with {p.exitcode}")


def base_width_case():
    """tests/test_headline_shapes_gpu.py::test_sdxl_base_mixed_forward_512_768_1024_one_sequence's shapes"""
    ocfg = ref.UNetConfig.sdxl_base()
    net = MxUNet(UNetConfig.sdxl_base(), ref.fast_params(ocfg), device="cuda:0")
    xs, cond = mixed_inputs(ocfg, [(1, 64), (1, 96), (1, 128)], 30)
    say("SDXL-base forward_mixed 512/768/1024 gn_patch 32", *net.forward_mixed(xs, *cond, gn_patch=32))


def sd3_inputs(ocfg, batch, hw, seed=0, lt=20):
    x, t, e, p = mref.make_inputs(ocfg, batch, hw, seed=seed, ctx_len=lt)
    return [x.cuda().to(torch.bfloat16), t.cuda(), e.cuda(), p.cuda()]


def sd3_mixed_inputs(ocfg, spec, seed):
    ins = [sd3_inputs(ocfg, b, hw, seed + i) for i, (b, hw) in enumerate(spec)]
    return [x[0] for x in ins], [torch.cat([x[k] for x in ins]) for k in range(1, 4)]


def mmdit_cases():
    """the tiny MMDiT (4 joint blocks, 0 and 1 dual, 2 heads), 20 text tokens"""
    ocfg = mref.MMDiTConfig.tiny()
    net = MxSD3Transformer(MMDiTConfig.tiny(), mref.init_params(ocfg), device="cuda:0")
    d = 64 * ocfg.num_attention_heads
    for hw in (16, 24):
        say(f"mmdit forward_one b2 {hw}x{hw}", net.forward_one(*sd3_inputs(ocfg, 2, hw)))
    x = sd3_inputs(ocfg, 2, 16)
    for stage, shape in (("embed", (2 * 64, d)), ("transformer_blocks.1", (2 * 64, d)), ("transformer_blocks.2.context", (2 * 20, d))):
        say(f"mmdit trace {stage}", net.forward_one(*x, stage=stage, stage_shape=shape))
    spec = [(1, 16), (2, 24), (1, 32)]
    xs, cond = sd3_mixed_inputs(ocfg, spec, 10)
    say("mmdit forward_mixed 16/24/32", *net.forward_mixed(xs, *cond))

    # per-sample block cache (one state row per request) under scripted answers
    pred = Script()
    net.enable_block_cache(pred, forced_after=1 << 30)
    step = lambda seed: net.forward({"128": sd3_inputs(ocfg, 2, 16, seed)[0]}, encoder_hidden_states=x[2], pooled_projections=x[3], timestep=x[1],
                                    return_dict=False, is_sliced=False, input_indices={"128": ["a", "b"]})[0]["128"]
    for k, (what, mask) in enumerate((("all run", np.ones), ("none run", np.zeros), ("the last sample alone asks", lambda n: np.eye(n)[-1]), ("all run again", np.ones))):
        pred.mask = mask
        say(f"mmdit forward_cached {what}", step(k))
    print(f"mmdit forward_cached blocks run {[hex(h) for h in net._block_caches['128'].history]}", flush=True)
    net.disable_block_cache()

    # chunk-unit cache over the mixed batch, the host decision under scripted masks: 4 + 2 * 9 + 16 = 38 chunks of 8 x 8 latent pixels
    def some(*idx):
        def mask(n):
            m = np.zeros(n)
            m[list(idx)] = 1
            return m
        return mask
    pred = Script()
    pc = PatchSkipCache(pred, forced_after=1 << 30, max_latent=32, mmdit_ctx_len=20)
    ids = ["a", "b", "c", "d"]
    step = lambda seed: net.forward_mixed_cached(pc, sd3_mixed_inputs(ocfg, spec, seed)[0], ids, *cond, 8)
    for k, (what, mask) in enumerate((("first step (nothing cached: all ask)", np.ones), ("all ask", np.ones), ("none asks (both streams reused)", np.zeros),
                                      ("the 16 x 16 group silent", lambda n: (np.arange(n) >= 4).astype(np.int64)),
                                      ("1 of the 32 x 32 request's 16 chunks asks (sparse attn2 renewal)", some(-1)),
                                      ("3 of 16 ask (whole attn2 renewal)", some(-1, -2, -3)))):
        pred.mask = mask
        say(f"mmdit forward_mixed_cached {what}", *step(10 + k))
    print(f"mmdit forward_mixed_cached blocks run {[hex(h) for h in pc.history]}, {pc.patches_asked} of {pc.patches_total} chunk-blocks asked", flush=True)

    # the same entry point with the decision on the device: a threshold on the input difference, and latents redrawn where a chunk shall ask
    # (block 0's input is local to the token, so its mask is exactly the redrawn chunks; the later blocks follow from what block 0 renewed)
    pcd = PatchSkipCache(ThresholdPredictor(1e-4), forced_after=1 << 30, max_latent=32, mmdit_ctx_len=20, on_device=True)
    lat = [t.clone() for t in xs]
    g = torch.Generator().manual_seed(77)

    def redraw(i, rows=None):
        lat[i] = lat[i].clone()
        r = lat[i].shape[2] if rows is None else rows
        lat[i][:, :, :r, :] = torch.randn(lat[i][:, :, :r, :].shape, generator=g).to(lat[i])
    for what, change in (("first step", ()), ("all redrawn: all ask", ((0, None), (1, None), (2, None))), ("nothing moved: none asks", ()),
                         ("the 16 x 16 group unmoved", ((1, None), (2, None))), ("two latent rows of the 32 x 32 request redrawn: 1 of 16 asks", ((2, 2),)),
                         ("four latent rows redrawn: 2 of 16 ask", ((2, 4),))):
        for i, rows in change:
            redraw(i, rows)
        say(f"mmdit forward_mixed_cached on the device, {what}", *net.forward_mixed_cached(pcd, lat, ids, *cond, 8))
        print(f"  asking chunks per block {[(int(b), int(np.asarray(m).sum())) for b, m in pcd.decisions]}", flush=True)
    print(f"mmdit forward_mixed_cached on the device blocks run {[hex(h) for h in pcd.history]}, {pcd.patches_asked} of {pcd.patches_total} chunk-blocks asked", flush=True)


def denoiser_cases(model):
    """SDXLDenoiser / SD3Denoiser over the tiny model, through the public API only: the sha256 of every request's latents after every step.
    Latents of 16 / 24 / 32 pixels, patch_size 64 (every resolution a multiple of the patch and larger: the cached-unit route), requests of 4 and 6
    steps and of their own embeddings, so that the per-request scalars and the row order show."""
    from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
    from sduss_amd.pipeline_sd3 import SD3Denoiser, synthetic_sd3_request
    if model == "unet":
        cfg = UNetConfig.tiny()
        net = MxUNet(cfg, ref.init_params(ref.UNetConfig.tiny()), device="cuda:0")
        new_denoiser = lambda: SDXLDenoiser(net)
        request = lambda den, rid, res: synthetic_request(rid, res, 4 + 2 * (rid % 2), cfg, den, "cuda:0", seed=500 + rid)
    else:
        cfg = MMDiTConfig.tiny()
        net = MxSD3Transformer(cfg, mref.init_params(mref.MMDiTConfig.tiny()), device="cuda:0")
        new_denoiser = lambda: SD3Denoiser(net)
        request = lambda den, rid, res: synthetic_sd3_request(rid, res, 4 + 2 * (rid % 2), cfg, den, "cuda:0", seed=500 + rid, ctx_len=20)
    one, three = [(256, 2)], [(128, 1), (192, 2), (256, 1)]

    def run(what, spec, steps, drop=None, masks=None, concurrent=True, **step_kwargs):
        den = new_denoiser()
        den.concurrent_resolutions = concurrent
        rids = iter(range(sum(n for _res, n in spec)))
        batch = {str(res): [request(den, next(rids), res) for _ in range(n)] for res, n in spec}
        for k in range(steps):
            if masks is not None:
                pred.mask = masks[k]
            den.denoising_step(batch, patch_size=64, **step_kwargs)
            for reqs in batch.values():
                for r in reqs:
                    say(f"{model} denoiser {what} step {k + 1} request {r.request_id}", r.latents)
            if drop is not None and k + 1 == drop[1]:
                del batch[drop[0]]

    run("one resolution, CFG", one, 3, is_sliced=False)
    run("one resolution, no CFG", one, 2, is_sliced=False, do_classifier_free_guidance=False)
    run("three resolutions, one sequence, 192 px leaves after step 2", three, 3, drop=("192", 2), is_sliced=True)
    net.mixed_one_sequence = False
    for concurrent in (True, False):
        run(f"three resolutions, one sequence per resolution, {'side streams' if concurrent else 'serial'}", three, 2, concurrent=concurrent, is_sliced=True)
    net.mixed_one_sequence = True

    pred = Script()
    asks = (np.ones, np.zeros, np.ones)
    net.enable_block_cache(pred, forced_after=1 << 30)
    run("block cache, patch / chunk unit, all / none / all ask", three, 3, masks=asks, is_sliced=True)
    pc = net._patch_cache
    print(f"{model} denoiser patch / chunk unit blocks run {[hex(h) for h in pc.history]}, {pc.patches_asked} of {pc.patches_total} asked", flush=True)
    net.enable_block_cache(pred, forced_after=1 << 30)
    run("block cache, per-sample unit, all / none / all ask", one, 3, masks=asks, is_sliced=False)
    print(f"{model} denoiser per-sample unit blocks run {[hex(h) for h in net._block_caches['256'].history]}", flush=True)
    net.disable_block_cache()


if __name__ == "__main__":
    tiny_cases()
    pp_cases()
    base_width_case()
    mmdit_cases()
    pp_cases("mmdit")
    denoiser_cases("unet")
    denoiser_cases("mmdit")
