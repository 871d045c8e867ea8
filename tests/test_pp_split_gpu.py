"""The split-batch decomposition of patch parallelism (CfgSplitLayout: the CFG branches on two rank groups, distrifuser's default) on the GPU.

Step kernels: mx_cfg_euler_step_rows / mx_cfg_flow_step_rows read the world gather where it lies; per element they run the operations of
mx_cfg_euler_step / mx_cfg_flow_step in the same order, so the result must equal theirs on the re-assembled tensor BIT FOR BIT (no tolerance).

Forward: the ranks share cuda:0 of the one-GPU test box and exchange through gloo, as tests/test_pp_gpu.py does.  One rank per branch (world 2) runs
the single-rank kernel sequence on one batch row: bit-equal to MxUNet.forward_one on that row.  Two ranks per branch (world 4) are bounded as the
existing patch-parallel tests are: 3 % of the output range from the single-rank forward, 4 % from the fp32 oracle (other GEMM tile shapes and
per-rank GroupNorm sums: the bf16 noise floor, tests/test_pp_gpu.py).  The step after the gather runs the same kernel on the same gathered bytes on
every rank: the latents are bit-equal across ranks, and bit-equal to the one-GPU step kernel on the re-assembled forward output."""
import os
import queue
import socket
import time
from datetime import timedelta

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SHAPES = [            # (n, C, H, W, n_slabs)
    (1, 4, 8, 8, 1),           # one slab: today's layout
    (1, 4, 8, 8, 2),           # two slabs
    (2, 4, 16, 8, 4),          # two latents, four slabs
    (1, 16, 6, 10, 2),         # slot of 480 elements with a 10-element row: a run of 30 elements is no whole number of 16-byte vectors
    (1, 4, 128, 128, 4),       # headline-sized latent
]
_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _cut(noise, n, n_slabs):
    """[2n, C, H, W] -> the slot layout [2 * n_slabs, n, C, H / n_slabs, W]: slot k the uncond rows of slab k, slot n_slabs + k the cond rows"""
    hs = noise.shape[2] // n_slabs
    return torch.stack([noise[b * n:(b + 1) * n, :, k * hs:(k + 1) * hs] for b in range(2) for k in range(n_slabs)]).contiguous()


def _step_inputs(shape, dtype):
    n, c, h, w, _s = shape
    g = torch.Generator().manual_seed(1234 + n * 1000 + h)
    noise = torch.randn(2 * n, c, h, w, generator=g).to(dtype).cuda()
    lat = (3.0 * torch.randn(n, c, h, w, generator=g)).to(dtype).cuda()
    sig = torch.tensor([9.1375, 2.4062][:n])
    sig_next = torch.tensor([7.9216, 1.9103][:n])
    return noise, lat, sig, sig_next


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_rows_equal_the_step_on_the_reassembled_prediction(cuda_device, shape, dtype):
    from sduss_amd import ops
    n, _c, _h, _w, n_slabs = shape
    noise, lat, sig, sig_next = _step_inputs(shape, dtype)
    gathered = _cut(noise, n, n_slabs)
    for rows_fn, whole_fn in ((ops.cfg_euler_step_rows_, ops.cfg_euler_step_), (ops.cfg_flow_step_rows_, ops.cfg_flow_step_)):
        for g in (5.0, 0.0):                           # guidance off: the plain prediction = the first n rows / the first n_slabs slots
            want = whole_fn(noise, lat.clone(), sig, sig_next, g)
            got = rows_fn(gathered, lat.clone(), sig, sig_next, g, n_slabs)
            assert not torch.equal(got.view(_INT[dtype]), lat.view(_INT[dtype]))
            assert torch.equal(got.view(_INT[dtype]), want.view(_INT[dtype])), f"{rows_fn.__name__} g={g}: bits differ from {whole_fn.__name__}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_step_rows_on_buffers_off_the_16_byte_grid(cuda_device, dtype):
    """runs that ARE whole vectors, in buffers that do not start on a 16-byte boundary: the vector path must not be taken"""
    from sduss_amd import ops
    shape = (1, 4, 8, 8, 2)
    noise, lat, sig, sig_next = _step_inputs(shape, dtype)
    cut = _cut(noise, 1, 2)
    for off_g, off_l in ((1, 0), (0, 1), (1, 1)):
        gbuf = torch.zeros(cut.numel() + 8, dtype=dtype, device="cuda")
        lbuf = torch.zeros(lat.numel() + 8, dtype=dtype, device="cuda")
        gathered = gbuf[off_g:off_g + cut.numel()].view(cut.shape).copy_(cut)
        mine = lbuf[off_l:off_l + lat.numel()].view(lat.shape).copy_(lat)
        assert (gathered.data_ptr() % 16 != 0) == bool(off_g) and (mine.data_ptr() % 16 != 0) == bool(off_l)
        want = ops.cfg_euler_step_(noise, lat.clone(), sig, sig_next, 5.0)
        got = ops.cfg_euler_step_rows_(gathered, mine, sig, sig_next, 5.0, 2)
        assert torch.equal(got.view(_INT[dtype]), want.view(_INT[dtype]))
        assert float(lbuf[:off_l].abs().sum()) == 0 and float(lbuf[off_l + lat.numel():].abs().sum()) == 0, "wrote outside the latents"


def test_step_rows_reject_bad_geometry(cuda_device):
    from sduss_amd import lib
    l = lib.load()
    noise, lat, sig, sig_next = _step_inputs((1, 4, 8, 8, 2), torch.bfloat16)
    before = lat.clone()
    sg, sn = sig.cuda(), sig_next.cuda()
    for fn in (l.mx_cfg_euler_step_rows, l.mx_cfg_flow_step_rows):
        for n_slabs in (3, 0, -2):                     # 8 % 3 != 0; no slab
            rc = fn(lib.current_stream(), noise.data_ptr(), lat.data_ptr(), sg.data_ptr(), sn.data_ptr(), 5.0, 1, 4, 8, 8, n_slabs, lib.MX_BF16)
            assert rc != 0 and b"n_slabs" in l.mx_last_error()
        rc = fn(lib.current_stream(), noise.data_ptr(), lat.data_ptr(), sg.data_ptr(), sn.data_ptr(), 5.0, 1, 4, 8, 0, 2, lib.MX_BF16)
        assert rc != 0 and b"bad arguments" in l.mx_last_error()
        rc = fn(lib.current_stream(), noise.data_ptr(), lat.data_ptr(), sg.data_ptr(), sn.data_ptr(), 5.0, 1, 4, 8, 8, 2, 7)
        assert rc != 0 and b"dtype" in l.mx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(lat, before), "an error must not launch"


# ------------------------------------------------------------------------------------------------------------------------------------
# the forward and the step over several ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _join(rank, world, port, backend):
    """gloo: every rank on cuda:0 of the one-GPU test box, exchanging through host memory; nccl (= RCCL): one device per rank"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.set_num_threads(8)                 # several ranks share the host
    dev = f"cuda:{rank}" if backend == "nccl" else "cuda:0"
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev), timeout=timedelta(seconds=120))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    return dev


def _spawn(world, target, backend="gloo"):
    """one process per rank; every wait is bounded, a rank that dies ends the test at once, and no child outlives it"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, backend)) for r in range(world)]
    res = {}
    try:
        for p in procs:
            p.start()
        deadline = time.monotonic() + 240
        while len(res) < world:
            try:
                rank, r = q.get(timeout=2)
                res[rank] = r
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a rank ended with exit code {dead}"
                assert time.monotonic() < deadline, "the ranks did not report in time"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    return res


def _need_gpus(n):
    if torch.cuda.device_count() < n:
        pytest.skip(f"needs {n} GPUs (one rank per device over RCCL); this box has {torch.cuda.device_count()}")


def _same_on_all_ranks(t, world):
    """bit-equality of a tensor across the ranks (through host memory, whatever the backend moves)"""
    mine = t.contiguous().view(torch.uint8).cpu()          # raw bytes: a type every backend moves
    if dist.get_backend() == "gloo":
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
    else:
        dparts = [torch.empty_like(mine, device=t.device) for _ in range(world)]
        dist.all_gather(dparts, mine.to(t.device))
        parts = [p.cpu() for p in dparts]
    return all(torch.equal(p, parts[0]) for p in parts)


def _world2_worker(rank, world, port, q, backend):
    dev = _join(rank, world, port, backend)
    try:
        from oracle import sdxl_unet_ref as ref
        from sduss_amd.config import UNetConfig
        from sduss_amd.patch_parallel import CfgSplitLayout, CommLog, PatchParallelUNet
        from sduss_amd.unet import MxUNet
        ocfg = ref.UNetConfig.tiny()
        net = MxUNet(UNetConfig.tiny(), ref.init_params(ocfg), device=dev)
        s, t, e, te, ti = ref.make_inputs(ocfg, 2, 64)
        x = s.cuda().to(torch.bfloat16)
        args = (t.cuda(), e.cuda(), te.cuda(), ti.cuda())
        log = CommLog()
        pp = PatchParallelUNet(net, log=log, layout=CfgSplitLayout(world))
        got = pp.forward(x, *args)
        buf = pp.forward_gathered(x, *args)
        rows_eq = [bool(torch.equal(got[b:b + 1], net.forward_one(x[b:b + 1], *(a[b:b + 1] for a in args)))) for b in range(2)]
        torch.cuda.synchronize()
        q.put((rank, dict(rows_eq=rows_eq, shape=tuple(got.shape), buf_shape=tuple(buf.shape), buf_eq=bool(torch.equal(buf[:, 0], got)),
                          calls=len(log.calls), world_calls=log.world_calls, branch=(pp.batch_idx, pp.rank, pp.world))))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_one_rank_per_branch_is_the_single_rank_forward(cuda_device):
    """CfgSplitLayout(2): rank 0 computes the unconditional row, rank 1 the conditional one, each with the ordinary single-rank forward on the
    whole latent (no exchange); row block b of `forward` is MxUNet.forward_one on batch row b alone, bit for bit, on both ranks"""
    res = _spawn(2, _world2_worker)
    for rank in range(2):
        r = res[rank]
        assert r["branch"] == (rank, 0, 1)
        assert r["shape"] == (2, 4, 64, 64) and r["buf_shape"] == (2, 1, 4, 64, 64) and r["buf_eq"]
        assert r["rows_eq"] == [True, True], f"rank {rank}: row blocks differ from the single-rank forward: {r['rows_eq']}"
        assert r["calls"] == 0 and r["world_calls"] == [(4 * 64 * 64 * 2, 2)] * 2        # nothing inside a branch; the world gather, twice


def _world4_sdxl_worker(rank, world, port, q, backend):
    dev = _join(rank, world, port, backend)
    try:
        from oracle import sdxl_unet_ref as ref
        from sduss_amd import lib, ops
        from sduss_amd.config import UNetConfig
        from sduss_amd.patch_parallel import CfgSplitLayout, CommLog, PatchParallelDenoiser, PatchParallelUNet, walk_comm_plan
        from sduss_amd.pipeline import SDXLDenoiser, synthetic_request
        from sduss_amd.unet import MxUNet
        ocfg = ref.UNetConfig.tiny()
        P = ref.init_params(ocfg)
        pcfg = UNetConfig.tiny()
        net = MxUNet(pcfg, P, device=dev)
        s, t, e, te, ti = ref.make_inputs(ocfg, 2, 64)
        x = s.cuda().to(torch.bfloat16)
        args = (t.cuda(), e.cuda(), te.cuda(), ti.cuda())
        layout = CfgSplitLayout(world)
        log = CommLog()
        pp = PatchParallelUNet(net, log=log, layout=layout)
        got = pp.forward(x, *args)
        torch.cuda.synchronize()
        res = dict(branch=(pp.batch_idx, pp.rank, pp.world))
        # exchanges of 2 slots: the regions fit a 2-rank workspace, and the bytes per exchange are those of the host plan of (batch 1, 32 rows, 2 ranks)
        log.check(pp._ws.numel(), 2)
        plan = walk_comm_plan(net._lib.mx_unet_pp_comm_plan, net._handle, 1, 32, 64, 77, 2, rank=pp.rank)
        res["log_is_plan"] = [nb for _s, _r, nb in log.calls] == [nb for _s, _r, nb in plan] and len(plan) > 40
        res["world_calls"] = list(log.world_calls)
        if rank == 0:
            want = net.forward_one(x, *args).float()
            oracle = ref.unet_forward(P, ocfg, s, t, e, te, ti)
            res["sync"] = (float((got.float() - want).abs().max()), float(want.abs().max()), float((got.float().cpu() - oracle).abs().max()),
                           float(oracle.abs().max()))
        res["fwd_same"] = _same_on_all_ranks(got, world)
        # distrifuser's default mode: the warm-up step and a stale step on unchanged inputs reproduce the synchronous output
        stale = PatchParallelUNet(net, mode="corrected_async_gn", warmup_steps=0, layout=layout)
        a = stale.forward(x, *args)
        m0 = stale.last_step_mode
        b = stale.forward(x, *args)
        m1 = stale.last_step_mode
        stale.reset()
        res["stale"] = (m0 == lib.PP_WARMUP, m1 == lib.PP_STALE, bool(torch.equal(a, got)), bool(torch.equal(b, got)))
        # one step of one request: scale -> forward_gathered -> the step on the gather buffer
        req = synthetic_request(0, 512, 4, pcfg, SDXLDenoiser(net), dev)
        lat0 = req.latents.clone()
        sig, sig_next = torch.tensor([req.sigmas[0]]), torch.tensor([req.sigmas[1]])
        ts = torch.tensor([req.timesteps[0]] * 2)
        cond = (torch.cat([req.negative_prompt_embeds, req.prompt_embeds]), torch.cat([req.negative_pooled_prompt_embeds, req.pooled_prompt_embeds]),
                torch.cat([req.negative_add_time_ids, req.add_time_ids]))
        noise = pp.forward(ops.euler_scale_input(lat0, sig, 2), ts.cuda(), *cond)
        want_lat = ops.cfg_euler_step_(noise, lat0.clone(), sig, sig_next, 5.0)
        PatchParallelDenoiser(pp, guidance_scale=5.0).step(req)
        torch.cuda.synchronize()
        res["step"] = (req.step_index == 1, tuple(req.latents.shape) == tuple(lat0.shape), not bool(torch.equal(req.latents, lat0)),
                       bool(torch.equal(req.latents.view(torch.int16), want_lat.view(torch.int16))), _same_on_all_ranks(req.latents, world))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world4_sdxl_split_forward_modes_and_step(cuda_device, backend="gloo"):
    """CfgSplitLayout(4) on a 64 x 64 latent: two ranks per branch, 32 rows each"""
    world = 4
    res = _spawn(world, _world4_sdxl_worker, backend)
    dmax, scale, oerr, oscale = res[0]["sync"]
    print(f"split batch x4 vs single rank: max diff {dmax:.5f} ({dmax / scale:.5f} of range); vs oracle {oerr / oscale:.4f} of range")
    assert dmax <= 0.03 * scale, f"4 ranks in 2 branches differ from 1 rank by {dmax} (range {scale})"
    assert oerr <= 0.04 * oscale
    for rank in range(world):
        r = res[rank]
        assert r["branch"] == (rank // 2, rank % 2, 2)
        assert r["log_is_plan"], f"rank {rank}: the logged exchanges are not those of a 2-rank plan at batch 1"
        assert r["world_calls"] == [(4 * 32 * 64 * 2, 4)]
        assert r["fwd_same"]
        assert r["stale"] == (True, True, True, True), f"rank {rank}: (warm-up mode, stale mode, warm-up == sync, stale == sync) = {r['stale']}"
        assert r["step"] == (True, True, True, True, True), \
            f"rank {rank}: (index, shape, moved, == cfg_euler_step_ on the re-assembled forward, same on all ranks) = {r['step']}"


def _world4_sd3_worker(rank, world, port, q, backend):
    dev = _join(rank, world, port, backend)
    try:
        from oracle import sd3_mmdit_ref as ref
        from sduss_amd import ops
        from sduss_amd.config import MMDiTConfig
        from sduss_amd.patch_parallel import CfgSplitLayout, CommLog, PatchParallelSD3, PatchParallelSD3Denoiser
        from sduss_amd.pipeline_sd3 import SD3Denoiser, synthetic_sd3_request
        from sduss_amd.transformer_sd3 import MxSD3Transformer
        ocfg = ref.MMDiTConfig.tiny()
        pcfg = MMDiTConfig.tiny()
        net = MxSD3Transformer(pcfg, ref.init_params(ocfg), device=dev)
        lat, t, e, p = ref.make_inputs(ocfg, 2, 32, ctx_len=77)
        x = lat.cuda().to(torch.bfloat16)
        args = (t.cuda(), e.cuda(), p.cuda())
        log = CommLog()
        pp = PatchParallelSD3(net, log=log, layout=CfgSplitLayout(world))
        got = pp.forward(x, *args)
        torch.cuda.synchronize()
        log.check(pp._ws.numel(), 2)
        want = net.forward_one(x, *args)
        res = dict(branch=(pp.batch_idx, pp.rank, pp.world), ncalls=len(log.calls), world_calls=list(log.world_calls), shape=tuple(got.shape),
                   sync_vs_single=float((got.float() - want.float()).abs().max()) / float(want.float().abs().max()),
                   fwd_same=_same_on_all_ranks(got, world))
        req = synthetic_sd3_request(0, 256, 4, pcfg, SD3Denoiser(net), dev, ctx_len=77)
        lat0 = req.latents.clone()
        sig, sig_next = torch.tensor([req.sigmas[0]]), torch.tensor([req.sigmas[1]])
        ts = torch.tensor([req.timesteps[0]] * 2)
        cond = (torch.cat([req.negative_prompt_embeds, req.prompt_embeds]), torch.cat([req.negative_pooled_prompt_embeds, req.pooled_prompt_embeds]))
        noise = pp.forward(torch.cat([lat0, lat0]), ts.cuda(), *cond)
        want_lat = ops.cfg_flow_step_(noise, lat0.clone(), sig, sig_next, 7.0)
        PatchParallelSD3Denoiser(pp, guidance_scale=7.0).step(req)
        torch.cuda.synchronize()
        res["step"] = (req.step_index == 1, tuple(req.latents.shape) == tuple(lat0.shape), not bool(torch.equal(req.latents, lat0)),
                       bool(torch.equal(req.latents.view(torch.int16), want_lat.view(torch.int16))), _same_on_all_ranks(req.latents, world))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world4_sd3_split_forward_and_flow_step(cuda_device, backend="gloo"):
    """CfgSplitLayout(4) over the SD3 transformer on a 32 x 32 latent: two ranks per branch, 16 rows (128 image tokens) each"""
    world = 4
    res = _spawn(world, _world4_sd3_worker, backend)
    tiny_layers, tiny_dual = 4, 2
    for rank in range(world):
        r = res[rank]
        print(f"rank {rank} sd3 split batch: {r}")
        assert r["branch"] == (rank // 2, rank % 2, 2) and r["shape"] == (2, 16, 32, 32)
        assert r["sync_vs_single"] <= 0.03                      # the bound of tests/test_pp_gpu.py::test_sd3_two_ranks_equal_one_rank_and_stale_steps
        assert r["ncalls"] == 2 * tiny_layers + 2 * tiny_dual and r["world_calls"] == [(16 * 16 * 32 * 2, 4)]
        assert r["fwd_same"]
        assert r["step"] == (True, True, True, True, True), \
            f"rank {rank}: (index, shape, moved, == cfg_flow_step_ on the re-assembled forward, same on all ranks) = {r['step']}"


@pytest.mark.timeout(300)
def test_world4_sdxl_split_forward_modes_and_step_rccl(cuda_device):
    """the same over RCCL with one device per rank: inert on a one-GPU box, live on a node with four"""
    _need_gpus(4)
    test_world4_sdxl_split_forward_modes_and_step(cuda_device, backend="nccl")


@pytest.mark.timeout(300)
def test_world4_sd3_split_forward_and_flow_step_rccl(cuda_device):
    _need_gpus(4)
    test_world4_sd3_split_forward_and_flow_step(cuda_device, backend="nccl")
