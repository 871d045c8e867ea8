"""sha256 of what the UNet's entry points write, for seeded inputs: the counterpart of `bench.py --dump-outputs` for the entry points the
benchmark does not run (mixed, trace, per-sample and per-patch block cache, patch-parallel).  Two builds of the library (MXDENOISE_LIB selects
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
from oracle import sdxl_unet_ref as ref  # noqa: E402  (inputs and parameters only)
from sduss_amd.block_cache import BlockSkipCache, PatchSkipCache  # noqa: E402
from sduss_amd.config import UNetConfig  # noqa: E402
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


def pp_rank(rank, world, port):
    """tests/test_pp_gpu.py::test_two_ranks_equal_one_rank's shape: both ranks on cuda:0, exchanging through gloo"""
    import torch.distributed as dist
    from sduss_amd.patch_parallel import PatchParallelUNet
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.set_num_threads(8)
    torch.cuda.set_device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ocfg = ref.UNetConfig.tiny()
        net = MxUNet(UNetConfig.tiny(), ref.init_params(ocfg), device="cuda:0")
        x0 = inputs(ocfg, 2, 64)
        x1 = inputs(ocfg, 2, 64, 1)[0]
        outs = [("synchronous", PatchParallelUNet(net).forward(*x0))]
        for mode in ("stale_gn", "corrected_async_gn"):
            pp = PatchParallelUNet(net, mode=mode, warmup_steps=0)
            outs += [(f"{mode} warm-up", pp.forward(*x0)), (f"{mode} stale step", pp.forward(x1, *x0[1:]))]
            pp.reset()
        for r in range(world):                   # rank by rank, so that the lines come out in one order
            if r == rank:
                for what, t in outs:
                    say(f"pp rank {rank} of {world} {what}", t)
            dist.barrier()
    finally:
        dist.destroy_process_group()


def pp_cases():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [mp.get_context("spawn").Process(target=pp_rank, args=(r, 2, port)) for r in range(2)]
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


if __name__ == "__main__":
    tiny_cases()
    pp_cases()
    base_width_case()
