"""Patch parallelism for ONE request across the GPUs of a node (BASELINE.json configs[3]): the distrifuser baseline the
reference bundles (distrifuser/distrifuser/distrifuser/models/distri_sdxl_unet_pp.py:15-216, utils.py:119-214), synchronous
and stale-asynchronous modes, behind the C ABI (``mx_unet_forward_pp`` / ``mx_unet_forward_pp_stale``, include/mxdenoise.h).

One process per GPU.  Every rank holds the whole UNet (weights are not sharded, as in distrifuser) and the latent ROWS
[rank * H / world, (rank + 1) * H / world).  The step plan itself decides what is exchanged (conv boundary rows, GroupNorm
sums, self-attention K / V^T); this module only supplies the collective: ``torch.distributed.all_gather_into_tensor`` on
views of the plan's workspace -- backend "nccl" is RCCL over xGMI on MI355X -- or, for the CPU-side tests, gloo through
host memory.  The final all-gather of the output rows mirrors distri_sdxl_unet_pp.py:193-195.

Buffer bookkeeping (what ``PatchParallelismCommManager`` does with its flat registered buffer, utils.py:119-214): the plan
allocates every send / receive region from the ONE workspace tensor, so a region is a byte range [offset, offset + n) of that
tensor and the collective needs no registration step; ``CommLog`` records the ranges so the tests can check them.

Two decompositions of the CFG batch of one request (utils.py:72-116).  ``layout=None``: batch 2 on every rank, rows over all ranks.
``layout=CfgSplitLayout(world)`` -- distrifuser's default, ``do_classifier_free_guidance=True, split_batch=True``: ranks [0, world/2) compute the
unconditional row and ranks [world/2, world) the conditional one, each half splitting the latent rows over its world/2 ranks and exchanging over
that half only; one all-gather over the whole world re-assembles [2, C, H, W] (distri_sdxl_unet_pp.py:135-171), and ``PatchParallelDenoiser`` /
``PatchParallelSD3Denoiser`` run the scheduler step straight on that gather buffer (mx_cfg_euler_step_rows / mx_cfg_flow_step_rows).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import lib as _lib
from . import ops
from .model_slot import _grow_only
from .pipeline import SDXLDenoiser
from .pipeline_sd3 import SD3Denoiser
from .step_state import StepCache


def split_rows(latents: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """this rank's rows of [B, C, H, W] (modules/pp/conv2d.py:20-40 slices the same way)"""
    h = latents.shape[2]
    assert h % world == 0, "latent height must divide evenly over the ranks"
    hl = h // world
    return latents[:, :, rank * hl:(rank + 1) * hl].contiguous()


def walk_comm_plan(plan_fn, handle, batch: int, h_local: int, w: int, ctx_len: int, world: int, rank: int = 0) -> List[Tuple[int, int, int]]:
    """Host only (no process group, no GPU): the exchanges of one forward of ``plan_fn`` (mx_unet_pp_comm_plan / mx_mmdit_pp_comm_plan of
    ``handle``) at this shape, in order, as CommLog entries (send_off, recv_off, bytes_per_rank)."""
    calls: List[Tuple[int, int, int]] = []

    def record(_ctx, _stream, send, recv, nbytes):
        calls.append((send - 0x1000, recv - 0x1000, nbytes))
        return 0
    cb = _lib.ALLGATHER_FN(record)
    comm = _lib.PPComm(rank, world, cb, None)
    if plan_fn(handle, batch, h_local, w, ctx_len, C.byref(comm)) != 0:
        raise _lib.MxError(_lib.load().mx_last_error().decode())
    return calls


class CfgSplitLayout:
    """Who computes what of the CFG batch [uncond ; cond] of one request: the rank arithmetic of distrifuser's DistriConfig (utils.py:72-116).
    Splitting (CFG and ``split_batch``): ``n_device_per_batch = world // 2`` (1 when that is 0), rank r computes batch row ``batch_idx(r)`` and the
    latent row slab ``split_idx(r)`` of it; ``batch_ranks(b)`` are the ranks of one branch (distrifuser's batch_group), ``pair_ranks(s)`` the two ranks
    holding slab s of the two branches (its split_group).  Otherwise ``n_device_per_batch = world``: every rank runs the whole batch and no group exists."""

    def __init__(self, world: int, do_classifier_free_guidance: bool = True, split_batch: bool = True):
        assert world > 0 and world & (world - 1) == 0, "the world size must be a power of two (utils.py:52)"
        self.world = world
        self.do_classifier_free_guidance, self.split_batch = do_classifier_free_guidance, split_batch
        if do_classifier_free_guidance and split_batch:          # utils.py:72-77
            self.n_device_per_batch = world // 2 or 1
        else:
            self.n_device_per_batch = world
        self.batch_groups: Optional[list] = None                 # filled by make_groups
        self.pair_groups: Optional[list] = None

    @property
    def splits(self) -> bool:
        """the CFG rows live on two rank groups (utils.py:90: groups exist from world 2 on)"""
        return self.do_classifier_free_guidance and self.split_batch and self.world >= 2

    def batch_idx(self, rank: int) -> int:                       # utils.py:102-109
        if self.do_classifier_free_guidance and self.split_batch:
            return 1 - int(rank < self.world // 2)
        return 0

    def split_idx(self, rank: int) -> int:                       # utils.py:111-116
        return rank % self.n_device_per_batch

    def batch_ranks(self, b: int) -> List[int]:                  # utils.py:93
        return list(range(b * (self.world // 2), (b + 1) * (self.world // 2)))

    def pair_ranks(self, s: int) -> List[int]:                   # utils.py:97
        return [s, s + self.world // 2]

    def make_groups(self, dist=None, **new_group_kwargs) -> None:
        """Create the torch.distributed groups in distrifuser's order (utils.py:90-98): both batch groups, then the world / 2 pair groups.  A
        collective over the default group: EVERY rank calls ``new_group`` for EVERY group, its own or not, as torch requires.  Does nothing when
        the layout does not split or the groups exist."""
        if not self.splits or self.batch_groups is not None:
            return
        if dist is None:
            import torch.distributed as dist
        assert dist.get_world_size() == self.world, "the layout is over the default process group"
        self.batch_groups = [dist.new_group(self.batch_ranks(b), **new_group_kwargs) for b in range(2)]
        self.pair_groups = [dist.new_group(self.pair_ranks(s), **new_group_kwargs) for s in range(self.world // 2)]


class CommLog:
    """byte ranges of the workspace that went through the collective, per call: (send_off, recv_off, bytes_per_rank); ``world_calls``: the gathers
    of the output rows over the whole world under a CfgSplitLayout, per call (bytes_per_rank, ranks) -- they do not touch the workspace"""

    def __init__(self):
        self.calls: List[Tuple[int, int, int]] = []
        self.world_calls: List[Tuple[int, int]] = []

    def check(self, ws_bytes: int, world: int) -> None:
        for so, ro, nb in self.calls:
            assert 0 <= so and so + nb <= ws_bytes, "send region outside the workspace"
            assert 0 <= ro and ro + nb * world <= ws_bytes, "receive region outside the workspace"
            assert so + nb <= ro or ro + nb * world <= so, "send and receive regions overlap"
            assert so % 16 == 0 and ro % 16 == 0 and nb % 16 == 0, "regions must be 16-byte aligned"


class PatchParallelUNet:
    """``forward_local(latents_local, ...)`` -> this rank's output rows; ``forward(latents, ...)`` -> the whole output on every
    rank (rows all-gathered).  ``group`` is the torch.distributed group of the ranks sharing the request (distrifuser's
    batch_group, utils.py:93-97).
    ``layout``: a CfgSplitLayout over the default process group (``group`` stays None).  When it splits, ``forward`` takes the CFG batch
    [2n, C, H, W] = [uncond... ; cond...] with 2n rows of every conditioning tensor, runs this rank's branch (n rows) on its row slab over its
    batch group, and gathers over the world; ``forward_gathered`` returns that gather as it lies.  A layout that does not split (no CFG,
    ``split_batch=False``, one rank) changes nothing."""
    STALE_SYMBOL = "forward_pp_stale"      # the UNet's stale step is a symbol of its own, and it knows corrected_async_gn

    def __init__(self, unet, group=None, log: Optional[CommLog] = None, mode: str = "sync", warmup_steps: int = 4,
                 layout: Optional[CfgSplitLayout] = None):
        """mode: "sync" (every step exchanges fresh tensors; distrifuser "full_sync"), "stale_gn" or "corrected_async_gn" (distrifuser's
        default, utils.py:30-32): `warmup_steps` synchronous steps, then stale-asynchronous ones (mx_unet_forward_pp_stale).  Call
        ``reset()`` when a new request starts (distrifuser resets its counters per generation, models/base_model.py)."""
        import torch.distributed as dist
        assert mode in ("sync", "stale_gn", "corrected_async_gn")
        self.mode, self.warmup_steps = mode, warmup_steps
        self.counter = 0
        self._state: Optional[torch.Tensor] = None
        self._pending = []                                   # collectives of the last stale step still in flight
        self._comm_stream: Optional[torch.cuda.Stream] = None
        self._cb_async = _lib.ALLGATHER_INPLACE_FN(self._all_gather_async)
        self.unet = unet
        self.dist = dist
        self.layout = layout if layout is not None and layout.splits else None
        if self.layout is not None:
            # the exchanges of the branch forward run over this rank's half of the world: rank / world below are those of the batch group
            assert group is None, "a CfgSplitLayout is over the default process group"
            layout.make_groups(dist)
            self.world_rank = dist.get_rank()
            self.batch_idx, split = layout.batch_idx(self.world_rank), layout.split_idx(self.world_rank)
            group = layout.batch_groups[self.batch_idx]
            assert dist.get_rank(group) == split and dist.get_world_size(group) == layout.n_device_per_batch
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.backend = dist.get_backend(group)
        self.log = log
        self._ws: Optional[torch.Tensor] = None
        self._cb = _lib.ALLGATHER_FN(self._all_gather)     # keep the callback object alive
        self._err: Optional[BaseException] = None

    def _gather_list(self, t: torch.Tensor, group, n: int) -> List[torch.Tensor]:
        """``t`` of each of the ``n`` ranks of ``group`` (torch.distributed.all_gather), on t's device; through host memory when the backend is
        gloo (the tests: gloo moves CPU tensors)"""
        mine = t.cpu() if self.backend == "gloo" else t
        parts = [torch.empty_like(mine) for _ in range(n)]
        self.dist.all_gather(parts, mine, group=group)
        return [p.to(t.device) for p in parts]

    # called from inside mx_unet_forward_pp (C -> Python through ctypes); returns 0 on success
    def _all_gather(self, _ctx, _stream, send, recv, nbytes) -> int:
        try:
            ws = self._ws
            so, ro = send - ws.data_ptr(), recv - ws.data_ptr()
            if self.log is not None:
                self.log.calls.append((so, ro, nbytes))
            s = ws[so:so + nbytes]
            r = ws[ro:ro + nbytes * self.world]
            if self.backend == "gloo":
                r.copy_(torch.cat(self._gather_list(s, self.group, self.world)))
            else:                                    # RCCL: device to device, ordered with the current stream by torch
                self.dist.all_gather_into_tensor(r, s, group=self.group)
            return 0
        except BaseException as e:  # noqa: BLE001  (must not propagate through the C frame)
            self._err = e
            return 1

    # stale steps: in-place all-gather over the slots of one state region; must start after what is queued on the compute stream and
    # finish before the next forward (wait_pending)
    def _all_gather_async(self, _ctx, _stream, region, nbytes) -> int:
        try:
            st = self._state
            off = region - st.data_ptr()
            assert 0 <= off and off + nbytes * self.world <= st.numel() and off % 256 == 0
            if self.log is not None:
                self.log.calls.append((-1, off, nbytes))
            r = st[off:off + nbytes * self.world]
            own = r[self.rank * nbytes:(self.rank + 1) * nbytes]
            if self.backend == "gloo":               # completes at once (a legal schedule of the async contract)
                r.copy_(torch.cat(self._gather_list(own, self.group, self.world)))
            else:                                    # RCCL on a side stream: the compute stream runs on while the slots travel
                cur = torch.cuda.current_stream()
                if self._comm_stream is None:
                    self._comm_stream = torch.cuda.Stream(device=st.device)
                ev = torch.cuda.Event()
                ev.record(cur)
                self._comm_stream.wait_event(ev)
                with torch.cuda.stream(self._comm_stream):
                    self._pending.append(self.dist.all_gather_into_tensor(r, own, group=self.group, async_op=True))
            return 0
        except BaseException as e:  # noqa: BLE001
            self._err = e
            return 1

    def wait_pending(self) -> None:
        """the compute stream waits for the collectives the last stale step left in flight"""
        for w in self._pending:
            w.wait()
        self._pending = []
        if self._comm_stream is not None:
            torch.cuda.current_stream().wait_stream(self._comm_stream)

    def reset(self) -> None:
        self.wait_pending()
        self.counter = 0

    def _stale_desc(self, sneed: int, shape_key: tuple, dev, corrected: int):
        """The state buffer and the mode of this step.  The state's layout (region offsets, bytes per rank) belongs to ONE problem shape: any
        change of (batch, local rows, width, context length, world) -- even to an equal or smaller footprint -- makes the next step a warm-up
        on a fresh layout.  In-flight collectives of the previous step are waited for BEFORE the old buffer is dropped.
        Warm-up length as distrifuser: exchanges stay synchronous while ``counter <= warmup_steps`` (modules/pp/conv2d.py:97, attn.py:136,
        groupnorm.py:46, distri_sdxl_unet_pp.py:109), i.e. warmup_steps + 1 = 5 synchronous steps at the default of 4."""
        self.wait_pending()
        if self._state is None or self._state.numel() < sneed or getattr(self, "_state_key", None) != shape_key:
            if self._state is None or self._state.numel() < sneed:
                self._state = None
                self._state = torch.empty(sneed, dtype=torch.uint8, device=dev)
            self._state_key = shape_key
            self.counter = 0                         # nothing to be stale about yet
        mode = _lib.PP_WARMUP if self.counter <= self.warmup_steps else _lib.PP_STALE
        self.last_step_mode = mode
        return _lib.PPStale(self._state.data_ptr(), self._state.numel(), mode, corrected, self._cb_async)

    def forward_local(self, latents_local: torch.Tensor, timestep: torch.Tensor, *cond: torch.Tensor) -> torch.Tensor:
        """this rank's rows in, this rank's output rows out; ``cond``: the model's conditioning tensors (its COND) for the batch"""
        u = self.unet
        x = latents_local.contiguous()
        b, _c, hl, w = x.shape
        ctx_len = cond[0].shape[1]
        ts, *cond = u._conditioning(b, timestep, *cond)
        shape = (b, hl, w, ctx_len, self.world)
        ws = _grow_only(vars(self), "_ws", u._fn("workspace_bytes_pp")(u._handle, *shape), f"mx_{u.ABI}_workspace_bytes_pp", u.device)
        out = torch.empty((b, u.cfg.out_channels, hl, w), dtype=x.dtype, device=u.device)
        comm = _lib.PPComm(self.rank, self.world, self._cb, None)
        self._err = None
        stale = None
        if self.mode != "sync":
            sneed = u._fn("pp_state_bytes")(u._handle, *shape)
            if sneed == 0:
                raise _lib.MxError(f"mx_{u.ABI}_pp_state_bytes: " + u._lib.mx_last_error().decode())
            stale = self._stale_desc(sneed, (u.ABI, *shape), u.device, int(self.STALE_SYMBOL is not None and self.mode == "corrected_async_gn"))
            self.counter += 1
        head = (u._handle, _lib.current_stream(), x.data_ptr(), _lib.torch_dtype_code(x.dtype), ts.data_ptr(), *(c.data_ptr() for c in cond),
                out.data_ptr(), b, hl, w, ctx_len, C.byref(comm))
        stale_ref = None if stale is None else C.byref(stale)
        if self.STALE_SYMBOL is None:        # one symbol: the stale descriptor, or NULL for a synchronous step
            rc = u._fn("forward_pp")(*head, stale_ref, ws.data_ptr(), ws.numel())
        elif stale is None:
            rc = u._fn("forward_pp")(*head, ws.data_ptr(), ws.numel())
        else:
            rc = u._fn(self.STALE_SYMBOL)(*head, stale_ref, ws.data_ptr(), ws.numel())
        if self._err is not None:
            raise self._err
        _lib.check(rc, f"mx_{u.ABI}_forward_pp")
        return out

    def _single_rank(self, latents, timestep, *cond) -> torch.Tensor:
        """one rank per branch (world 2): nothing to exchange, the ordinary forward (mx_unet_forward / mx_mmdit_forward)"""
        return self.unet.forward_one(latents.contiguous(), timestep, *cond)

    def forward_gathered(self, latents: torch.Tensor, timestep, *cond) -> torch.Tensor:
        """Under a splitting layout: the CFG batch [2n, C, H, W] and its conditioning in (the arguments of ``forward``), the world gather out as it
        lies: [world, n, C, H / n_device_per_batch, W], slot r = the output rows of world rank r (distri_sdxl_unet_pp.py:135-168) -- the
        ``gathered`` of ops.cfg_step_rows_ with n_slabs = n_device_per_batch."""
        lay = self.layout
        assert lay is not None, "forward_gathered needs a CfgSplitLayout that splits the CFG batch"
        assert latents.shape[0] % 2 == 0, "the CFG batch is [uncond... ; cond...]"
        n = latents.shape[0] // 2
        rows = slice(self.batch_idx * n, (self.batch_idx + 1) * n)                     # :137-147
        if torch.is_tensor(timestep) and timestep.ndim > 0 and timestep.numel() > 1:
            assert timestep.numel() == 2 * n
            timestep = timestep.reshape(-1)[rows]
        cond = tuple(c[rows] for c in cond)
        if self.world == 1:
            local = self._single_rank(latents[rows], timestep, *cond)
        else:
            local = self.forward_local(split_rows(latents[rows], self.rank, self.world), timestep, *cond)
        local = local.contiguous()
        if self.log is not None:
            self.log.world_calls.append((local.numel() * local.element_size(), lay.world))
        if self.backend == "gloo":
            return torch.stack(self._gather_list(local, None, lay.world))
        buf = torch.empty((lay.world, *local.shape), dtype=local.dtype, device=local.device)
        self.dist.all_gather_into_tensor(buf, local)
        return buf

    def _forward_split(self, latents: torch.Tensor, timestep, *cond) -> torch.Tensor:
        """[2n, C, H, W]: slots [0, npb) concatenated along the rows into row block 0, slots [npb, world) into row block 1 (:169-170)"""
        buf = self.forward_gathered(latents, timestep, *cond)
        _world, n, c, hs, w = buf.shape
        npb = self.world
        return buf.view(2, npb, n, c, hs, w).permute(0, 2, 3, 1, 4, 5).reshape(2 * n, c, npb * hs, w)

    def forward(self, latents: torch.Tensor, timestep, *cond: torch.Tensor) -> torch.Tensor:
        """whole latent in, whole noise prediction out on every rank (distri_sdxl_unet_pp.py:167-195)."""
        if self.layout is not None:
            return self._forward_split(latents, timestep, *cond)
        local = self.forward_local(split_rows(latents, self.rank, self.world), timestep, *cond)
        return torch.cat(self._gather_list(local, self.group, self.world), dim=2)


class PatchParallelSD3(PatchParallelUNet):
    """The same for the SD3 / SD3.5 transformer (``mx_mmdit_forward_pp``; distrifuser models/distri_sd3_transformer_pp.py:87-97,
    modules/pp/attn.py:202-277): rank r owns the image tokens of its latent rows, every rank computes the text stream, each joint block
    all-gathers the image K / V^T.  ``forward(latents, timestep, encoder_hidden_states, pooled)``."""

    STALE_SYMBOL = None                    # mx_mmdit_forward_pp takes the stale descriptor itself; no corrected GroupNorm (there is none)


class PatchParallelDenoiser:
    """One step of ONE request of pipeline.py (``Request``) under a splitting CfgSplitLayout, as SDXLDenoiser._step_resolution runs it on one
    GPU: mx_euler_scale_input (CFG duplication fused) -> ``PatchParallelUNet.forward_gathered`` -> mx_cfg_euler_step_rows on the gather buffer.
    Every rank holds the whole latents, as in distrifuser, and applies the same kernel to the same gathered bytes: after a step the latents are
    bit-identical on all ranks."""

    hooks = SDXLDenoiser          # the model's side of a step, shared with the one-GPU denoiser: _cond, _scale_input, flow

    def __init__(self, pp: PatchParallelUNet, guidance_scale: float = 5.0):
        assert pp.layout is not None, "the step on the gather buffer needs a CfgSplitLayout that splits the CFG batch"
        self.pp = pp
        self.guidance_scale = guidance_scale
        self._cache = StepCache(pp.unet.device)

    @torch.inference_mode()
    def step(self, req) -> None:
        if getattr(req, "inpaint", None) is not None:        # the step on the gather buffer has no masked form
            raise _lib.MxError("inpainting is not available under patch parallelism")
        if getattr(req, "sampler", "euler") != "euler":      # nor a multistep form: the history would have to follow the row slabs
            raise _lib.MxError("multistep samplers are not available under patch parallelism")
        e = self._cache.entry((req.resolution, req.request_id, id(req)), [req], lambda: self.hooks._cond([req], True))
        lat = self._cache.latents(e, [req])
        sig, sig_next, ts = self._cache.step_scalars(e, [req])
        buf = self.pp.forward_gathered(self.hooks._scale_input(lat, sig, True), torch.cat([ts, ts], dim=0), *e.cond)
        ops.cfg_step_rows_(buf, lat, sig, sig_next, self.guidance_scale, self.pp.world, self.hooks.flow)
        req.step_index += 1
        req.latents = lat[0:1]


class PatchParallelSD3Denoiser(PatchParallelDenoiser):
    """The same for one ``SD3Request`` of pipeline_sd3.py over a PatchParallelSD3: no input scaling, the flow-match step (mx_cfg_flow_step_rows)."""

    hooks = SD3Denoiser

    def __init__(self, pp: PatchParallelSD3, guidance_scale: float = 7.0):
        super().__init__(pp, guidance_scale)
