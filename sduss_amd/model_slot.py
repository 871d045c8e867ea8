"""What the two model-slot adapters (unet.py ``MxUNet``, transformer_sd3.py ``MxSD3Transformer``) share above the C ABI: the preparation of the
conditioning, the per-stream scratch arena, the group array of a mixed batch, the error protocol of a cached forward, and the routing of the
reference's ``forward(dict of resolutions, ...)``.  A subclass names its ABI prefix (``mx_<ABI>_*``), its conditioning tensors, its reference
``forward`` signature and how it builds its block-skip caches.  PyTorch is used for device memory and the current stream only; every FLOP runs
in the HIP library."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import lib as _lib
from .weights import PackedWeights


class _Config(dict):
    """``.config`` as the pipeline reads it (attribute and item access)."""
    __getattr__ = dict.__getitem__


def _row_ids(ids, n_rows):
    """one id per row of a resolution's batch: the request ids repeat once per classifier-free-guidance half ([uncond..., cond...])"""
    return [f"{ids[i % len(ids)]}#{i // len(ids)}" for i in range(n_rows)]


def _grow_only(slots: dict, key, need: int, size_fn: str, device) -> torch.Tensor:
    """The grow-only scratch buffer ``slots[key]``, at least ``need`` bytes (``vars(obj)`` as ``slots`` keeps it in an attribute).  ``need == 0``
    is the size function ``size_fn`` refusing the shape.  The old buffer is dropped BEFORE the new one is allocated: the two never exist
    together, which is what keeps the peak of device memory down."""
    if need == 0:
        raise _lib.MxError(f"{size_fn}: " + _lib.load().mx_last_error().decode())
    buf = slots.get(key)
    if buf is None or buf.numel() < need:
        slots[key] = None
        buf = slots[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


class ModelSlot:
    ABI = ""               # the symbols are mx_<ABI>_*
    COND = ()              # the conditioning tensors after the timestep: (dtype, shape after the row dimension; a str names a cfg field, None is free)
    GN_PATCH = False       # the patch edge is an argument of EVERY forward (the UNet: GroupNorm statistics per patch), not of the cached mixed one alone
    CACHE_CTX_LEN = False  # the block-skip state holds text rows too (the MMDiT's joint blocks): sized by, and valid for, one text length

    def __init__(self, cfg, config_c, packed: dict, device):
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        self._lib = _lib.load()
        self._handle = self._fn("create")(C.byref(config_c))
        if not self._handle:
            raise _lib.MxError(f"mx_{self.ABI}_create: " + self._lib.mx_last_error().decode())
        self.weights = PackedWeights(packed, self.device)
        _lib.check(self._fn("set_weights")(self._handle, self.weights.blob.data_ptr(), self.weights.blob.numel(), self.weights.table,
                                           len(self.weights.names)), f"mx_{self.ABI}_set_weights")
        self.mixed_one_sequence = True     # False: one launch sequence per resolution (the round-2 form; A/B and tests)
        self.max_mixed_groups = _lib.MAX_SEGS
        self._cond_spec = [(dt, tuple(getattr(cfg, d) if isinstance(d, str) else d for d in tail)) for dt, tail in self.COND]
        self._ws_by_stream: Dict[int, Optional[torch.Tensor]] = {}
        self._ws_need = {}
        self._block_caches = None          # enable_block_cache: {resolution key: BlockSkipCache}
        self._patch_cache = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            self._fn("destroy")(h)
            self._handle = None

    def to(self, *args, **kwargs):
        return self

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def _fn(self, name: str):
        return getattr(self._lib, f"mx_{self.ABI}_{name}")

    # ---- the pieces of one call ---------------------------------------------------------------------
    def _conditioning(self, rows: int, timestep, *cond) -> list:
        """[timesteps fp32 [rows], *conditioning] as the library reads them: on the device, contiguous, in COND's dtypes; one timestep (a tensor
        of one element or a Python number) serves every row."""
        if not torch.is_tensor(timestep):
            timestep = torch.tensor([float(timestep)], device=self.device)
        ts = timestep.to(device=self.device, dtype=torch.float32).reshape(-1)
        if ts.numel() == 1:
            ts = ts.expand(rows)
        assert ts.shape[0] == rows, f"{ts.shape[0]} timesteps for {rows} rows"
        assert len(cond) == len(self._cond_spec)
        out = [ts.contiguous()]
        for t, (dtype, tail) in zip(cond, self._cond_spec):
            t = t.to(device=self.device, dtype=dtype).contiguous()
            assert t.ndim == 1 + len(tail) and t.shape[0] == rows and all(w is None or s == w for s, w in zip(t.shape[1:], tail)), \
                f"conditioning of shape {tuple(t.shape)}, expected {(rows, *tail)}"
            out.append(t)
        return out

    def _arena(self, stream, key: tuple, size_fn: str, *size_args) -> torch.Tensor:
        """grow-only arena, one per stream: launch sequences issued on different streams (the denoisers run the resolutions of a mixed batch
        concurrently) must not share scratch.  ``mx_<ABI>_<size_fn>`` is a dry run of the whole plan: once per shape ``key``."""
        need = self._ws_need.get(key)
        if need is None:
            need = self._ws_need[key] = self._fn(size_fn)(self._handle, *size_args)
        return _grow_only(self._ws_by_stream, int(stream or 0), need, f"mx_{self.ABI}_{size_fn}", self.device)

    def _workspace(self, batch: int, h: int, w: int, ctx_len: int, stream) -> torch.Tensor:
        """the arena of a one-resolution forward, cached or not"""
        return self._arena(stream, (batch, h, w, ctx_len), "workspace_bytes", batch, h, w, ctx_len)

    def _groups(self, samples: List[torch.Tensor]):
        """(mx_unet_group array, output tensors, shapes (batch, H, W), the contiguous samples the array points into) of a mixed batch"""
        assert 1 <= len(samples) <= _lib.MAX_SEGS, f"a mixed batch holds up to {_lib.MAX_SEGS} resolutions"
        samples = [x.contiguous() for x in samples]
        dt = samples[0].dtype
        assert all(x.is_cuda and x.ndim == 4 and x.dtype == dt for x in samples)
        outs = [torch.empty((x.shape[0], self.cfg.out_channels, x.shape[2], x.shape[3]), dtype=dt, device=self.device) for x in samples]
        groups = (_lib.UNetGroup * len(samples))()
        for g, (x, o) in enumerate(zip(samples, outs)):
            groups[g].latents, groups[g].out = x.data_ptr(), o.data_ptr()
            groups[g].batch, groups[g].H, groups[g].W = x.shape[0], x.shape[2], x.shape[3]
        return groups, outs, tuple((x.shape[0], x.shape[2], x.shape[3]) for x in samples), samples

    def _call_cached(self, cache, name: str, *args) -> None:
        """``mx_<ABI>_<name>(*args)`` under a block-skip cache already bound.  A forward that stopped part-way stored some blocks' rows and not
        others: nothing cached survives it; the predictor's own exception wins over the library's "predictor failed"."""
        rc = self._fn(name)(*args)
        if rc:
            err = cache.error
            cache.invalidate()
            if err is not None:
                raise err
        _lib.check(rc, f"mx_{self.ABI}_{name}")
        cache.after_forward()

    def _before_forward(self) -> None:
        """right before the launch sequence of an uncached forward (the UNet hands over its context key here)"""

    def _one(self, sample: torch.Tensor, timestep, cond, patch: int = 0, cache=None, batch_key: int = 0, row_ids=None,
             stage: Optional[str] = None, stage_shape=None) -> torch.Tensor:
        """One launch sequence over a batch of same-resolution latents [B, C, H, W] (any of fp32/fp16/bf16): plain, through ``cache`` (a
        block_cache.BlockSkipCache), or stopped at ``stage``, whose activation [stage_shape] bf16 is then returned."""
        assert sample.is_cuda and sample.ndim == 4
        sample = sample.contiguous()
        b, _c, h, w = sample.shape
        ctx_len = cond[0].shape[1]
        ts, *cond = self._conditioning(b, timestep, *cond)
        out = torch.empty((b, self.cfg.out_channels, h, w), dtype=sample.dtype, device=self.device)
        stream = _lib.current_stream()
        ws = self._workspace(b, h, w, ctx_len, stream)
        args = (self._handle, stream, sample.data_ptr(), _lib.torch_dtype_code(sample.dtype), ts.data_ptr(), *(c.data_ptr() for c in cond),
                out.data_ptr(), b, h, w, ctx_len, *((patch,) if self.GN_PATCH else ()), ws.data_ptr(), ws.numel())
        if cache is not None:
            assert stage is None
            desc = cache.bind(self, b, h, w, batch_key, ctx_len=ctx_len if self.CACHE_CTX_LEN else None, row_ids=row_ids)
            self._call_cached(cache, "forward_cached", *args, desc)
            return out
        if stage is None:
            self._before_forward()
            _lib.check(self._fn("forward")(*args), f"mx_{self.ABI}_forward")
            return out
        st = torch.empty(stage_shape, dtype=torch.bfloat16, device=self.device)
        _lib.check(self._fn("forward_trace")(*args, stage.encode(), st.data_ptr(), st.numel() * 2), f"mx_{self.ABI}_forward_trace")
        return st

    def _mixed(self, samples: List[torch.Tensor], timestep, cond, patch: int = 0, cache=None, row_ids=None, stage: Optional[str] = None):
        """ONE launch sequence over the latents of several resolutions: ``samples[g]`` is [B_g, C, H_g, W_g]; the conditioning rows are those of
        all groups concatenated in list order.  Through ``cache`` (a block_cache.PatchSkipCache; ``row_ids``: one id per sample in row order,
        request id + CFG half) the unit of reuse is the patch of ``patch`` latent pixels.  With ``stage``: [that stage's activation of all
        groups] (tests)."""
        groups, outs, shapes, samples = self._groups(samples)
        n = len(samples)
        ctx_len = cond[0].shape[1]
        ts, *cond = self._conditioning(sum(s[0] for s in shapes), timestep, *cond)
        stream = _lib.current_stream()
        head = (self._handle, stream, groups, n, _lib.torch_dtype_code(samples[0].dtype), ts.data_ptr(), *(c.data_ptr() for c in cond), ctx_len)
        if cache is not None:
            assert patch > 0 and stage is None and cache.mmdit_ctx_len == (ctx_len if self.CACHE_CTX_LEN else None)
            ws = self._arena(stream, ("mixed_cached", shapes, ctx_len, patch), "workspace_bytes_cached_mixed", groups, n, ctx_len, patch)
            desc = cache.bind(self, shapes, row_ids, patch)
            self._call_cached(cache, "forward_cached_mixed", *head, patch, ws.data_ptr(), ws.numel(), desc)
            return outs
        ws = self._arena(stream, ("mixed", shapes, ctx_len), "workspace_bytes_mixed", groups, n, ctx_len)
        args = (*head, *((patch,) if self.GN_PATCH else ()), ws.data_ptr(), ws.numel())
        if stage is None:
            self._before_forward()
            _lib.check(self._fn("forward_mixed")(*args), f"mx_{self.ABI}_forward_mixed")
            return outs
        st = torch.empty(64 << 20, dtype=torch.bfloat16, device=self.device)        # large enough for any stage of the test shapes
        _lib.check(self._fn("forward_mixed_trace")(*args, stage.encode(), st.data_ptr(), st.numel() * 2), f"mx_{self.ABI}_forward_mixed_trace")
        return [st]

    # ---- the reference's forward(dict of resolutions, ...) -------------------------------------------
    def _take_announcement(self):
        """what the caller announced for THIS forward() (the UNet's one-shot context key); it reaches the library only through _announce"""
        return None

    def _announce(self, announced) -> None:
        """the forward() is ONE uncached launch sequence: what was announced for it holds for that sequence"""

    def _route(self, sample: Dict[str, torch.Tensor], timestep, cond, is_sliced: bool, patch_size: Optional[int], input_indices: Optional[dict]):
        """Row order contract (same as the reference): resolutions in the dict's (ascending) order, the conditioning rows of all resolutions
        concatenated in that order."""
        # What the caller announced for this call (the UNet's one-shot context key) is taken here, so that no sequence below sees it by accident;
        # _announce() gives it back on the two routes where the call is ONE uncached launch sequence, whose _before_forward() then consumes it.
        # Every other route (a cached one, a loop over several resolutions) runs unannounced.
        announced = self._take_announcement()
        keys = [k for k in sample if sample[k] is not None and sample[k].shape[0] > 0]
        if not is_sliced:
            keys = keys[:1]  # the reference's unsliced branch runs the first resolution only (unet.py:268-272, SD3Transformer.py:105-109)
        caches, ids = self._block_caches, input_indices or {}
        if caches is not None:                         # ESYMRED_USE_CACHE=TRUE (enable_block_cache)
            assert all(k in ids and len(ids[k]) > 0 and sample[k].shape[0] % len(ids[k]) == 0 for k in keys), \
                "the block-skip cache keys its state by input_indices[resolution] (cache_manager.py:105, 166)"
        one_sequence = is_sliced and len(keys) <= _lib.MAX_SEGS
        if one_sequence and caches is not None and patch_size is not None and all(int(k) % patch_size == 0 and int(k) > patch_size for k in keys):
            # the cache at its reference unit, the patch / token chunk; every resolution in ONE launch sequence
            ctx_len = cond[0].shape[1] if self.CACHE_CTX_LEN else None
            if self._patch_cache is None or self._patch_cache.mmdit_ctx_len != ctx_len:
                self._patch_cache = self._new_patch_cache(ctx_len)
            row_ids = [r for k in keys for r in _row_ids(ids[k], sample[k].shape[0])]
            res = self._mixed([sample[k] for k in keys], timestep, cond, patch_size // 8, cache=self._patch_cache, row_ids=row_ids)
            return (dict(zip(keys, res)),)
        if one_sequence and caches is None and len(keys) > 1 and self.mixed_one_sequence:
            # the resolutions of a mixed batch as ONE launch sequence (the reference: one patch batch, unet.py:242-260, SD3Transformer.py:86)
            patch = 0
            if self.GN_PATCH:
                assert patch_size is not None and all(int(k) % patch_size == 0 for k in keys)
                patch = patch_size // 8
            self._announce(announced)
            return (dict(zip(keys, self._mixed([sample[k] for k in keys], timestep, cond, patch))),)
        out: Dict[str, torch.Tensor] = {}
        row = 0
        for key in keys:
            x = sample[key]
            n = x.shape[0]
            patch = 0
            if is_sliced and self.GN_PATCH:
                assert patch_size is not None and int(key) % patch_size == 0
                patch = patch_size // 8
            sl = slice(row, row + n)
            ts = timestep if (not torch.is_tensor(timestep) or timestep.ndim == 0) else timestep[sl]
            part = [c[sl] for c in cond]
            if caches is not None:
                bc = caches.get(key)
                if bc is None:
                    bc = caches[key] = self._new_block_cache()
                out[key] = self._one(x, ts, part, patch, cache=bc, row_ids=_row_ids(ids[key], n))
            else:
                if len(keys) == 1:
                    self._announce(announced)
                out[key] = self._one(x, ts, part, patch)
            row += n
        return (out,)

    def _install_block_cache(self, new_block_cache, new_patch_cache) -> None:
        """forward() goes through the block-skip cache from now on: ``new_block_cache()`` per resolution key (the per-sample unit, is_sliced=False),
        ``new_patch_cache(ctx_len)`` once (the patch / chunk unit, is_sliced=True: all resolutions in one sequence)"""
        self._new_block_cache, self._new_patch_cache = new_block_cache, new_patch_cache
        self._block_caches = {}
        self._patch_cache = None

    def disable_block_cache(self) -> None:
        self._block_caches = None
        self._patch_cache = None
