"""Per-batch-composition device state of the step mirrors (pipeline.py, pipeline_sd3.py).

The reference rebuilds everything from Python lists every step: per-request sigma / timestep lists -> fresh device tensors
(scheduling_euler_discrete.py:171-175, 213-217) and ``torch.cat`` of the per-request embeddings
(pipeline_stable_diffusion_xl_esymred.py:287-339).  Under continuous batching the same set of requests steps together for
tens of steps, so here the concatenated conditioning, a [3, n, S] table (sigma, sigma_next, timestep per request and step)
and a device-resident step index are built ONCE per composition; a step then costs one gather and one increment on the
device and no host-to-device copy.  The host list of step indices is compared every step, so a caller that rewinds or
skips a request (bench.py keeps its batch full by resetting step_index) is followed with one small asynchronous upload.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def _upload(host: torch.Tensor, device) -> torch.Tensor:
    """asynchronous H2D from pinned memory (torch.tensor(list, device=...) is a synchronous pageable copy)"""
    if torch.device(device).type == "cpu":
        return host
    return host.pin_memory().to(device, non_blocking=True)


class _Entry:
    __slots__ = ("cond", "table", "idx", "rows", "host_idx", "lat", "limit", "uid", "inpaint")

_next_uid = [0]


def new_uid() -> int:
    """a process-wide, never reused, non-zero name for a batch composition (MxUNet.set_context_key)"""
    _next_uid[0] += 1
    return _next_uid[0]


class StepCache:
    def __init__(self, device, max_entries: int = 16):
        self.device = device
        self.max_entries = max_entries
        self._entries: "OrderedDict[tuple, _Entry]" = OrderedDict()

    def entry(self, key: tuple, reqs: Sequence, build_cond: Callable[[], tuple], build_inpaint: Optional[Callable[[], tuple]] = None) -> _Entry:
        """the entry of a batch composition, built on first use.  ``build_inpaint``: the packed rows of its inpainting requests (Denoiser._inpaint_rows;
        None for a composition without one), fixed for the composition like ``cond``."""
        e = self._entries.get(key)
        if e is not None:
            self._entries.move_to_end(key)
            return e
        e = _Entry()
        e.uid = new_uid()
        e.cond = build_cond()
        e.inpaint = build_inpaint() if build_inpaint is not None else None
        n = len(reqs)
        s_max = max(len(r.timesteps) for r in reqs)
        tab = np.zeros((3, n, s_max), dtype=np.float32)
        for i, r in enumerate(reqs):
            k = len(r.timesteps)
            tab[0, i, :k] = r.sigmas[:k]
            tab[1, i, :k] = r.sigmas[1:k + 1]
            tab[2, i, :k] = r.timesteps
        e.table = _upload(torch.from_numpy(tab), self.device)
        e.rows = torch.arange(n, device=self.device)
        e.host_idx = None
        e.idx = torch.zeros(n, dtype=torch.int64, device=self.device)
        e.limit = [len(r.timesteps) for r in reqs]
        e.lat = None
        self._entries[key] = e
        while len(self._entries) > self.max_entries:
            self._entries.popitem(last=False)
        return e

    def step_scalars(self, e: _Entry, reqs: Sequence) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(sigma, sigma_next, timestep) fp32 [n] of the requests' CURRENT step; advances the device-side index."""
        host = [r.step_index for r in reqs]
        for h, lim in zip(host, e.limit):
            if not 0 <= h < lim:
                raise IndexError(f"step_index {h} outside the request's {lim} steps")
        if host != e.host_idx:
            e.idx.copy_(_upload(torch.tensor(host, dtype=torch.int64), self.device), non_blocking=True)
        vals = e.table[:, e.rows, e.idx]          # [3, n]
        e.idx += 1
        e.host_idx = [h + 1 for h in host]
        return vals[0], vals[1], vals[2]

    def latents(self, e: _Entry, reqs: Sequence) -> torch.Tensor:
        """the batch's latents as one [n, ...] tensor.  After a step every request holds a view of row i of the same
        buffer, so the concatenation of the next step is that buffer itself -- no copy."""
        lat = e.lat
        if lat is not None and lat.shape[0] == len(reqs) and all(
                r.latents.data_ptr() == lat[i].data_ptr() and r.latents.dtype == lat.dtype and r.latents.shape[1:] == lat.shape[1:]
                for i, r in enumerate(reqs)):
            return lat
        e.lat = torch.cat([r.latents for r in reqs], dim=0).contiguous()
        return e.lat
