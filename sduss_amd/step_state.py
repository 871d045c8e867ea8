"""Per-batch-composition device state of the step mirrors (pipeline.py, pipeline_sd3.py).

The reference rebuilds everything from Python lists every step: per-request sigma / timestep lists -> fresh device tensors
(scheduling_euler_discrete.py:171-175, 213-217) and ``torch.cat`` of the per-request embeddings
(pipeline_stable_diffusion_xl_esymred.py:287-339).  Under continuous batching the same set of requests steps together for
tens of steps, so here the concatenated conditioning, a [3, n, S] table (sigma, sigma_next, timestep per request and step)
and a device-resident step index are built ONCE per composition; a step then costs one gather and one increment on the
device and no host-to-device copy.  The host list of step indices is compared every step, so a caller that rewinds or
skips a request (bench.py keeps its batch full by resetting step_index) is followed with one small asynchronous upload.

A composition with a multistep sampler (DPM-Solver++ 2M, AB2: csrc/scheduler_step.hip) also holds its rows' kinds, their coefficient table of
every step in both orders and the fp32 history buffer; the step's [n, 3] coefficients are one more gather by the same device index, and the
order of every row (second only right after a step that left its history) is followed on the host like the step index.  With a stochastic
sampler (Euler ancestral, DPM-Solver++ 2M SDE) it holds the rows' seeds and noise coefficients of every step as well; the step's [n] noise
coefficients are a further gather, and the device-side step index itself is the counter word of the rows' generators.
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
    __slots__ = ("cond", "table", "idx", "rows", "host_idx", "lat", "limit", "uid", "inpaint", "multistep")


class _Multistep:
    """the multistep rows of a composition: ``kind`` int32 [n] on the device (``host_kind`` the same list on the host), ``table`` fp32 [n, S, 2, 3] =
    (cx, c0, c1) of every step in first and in second order, ``order`` int64 [n] on the device (1 = second order; ``host_order`` what the host
    last uploaded), ``coef`` fp32 [n, 3] of the current step, ``hist`` the fp32 history buffer [n, C, h, w].  A composition with a stochastic row
    (mx_cfg_stochastic_step) also: ``cn_table`` fp32 [n, S], ``seed`` int64 [n] (the uint64 bits), and ``cn`` fp32 [n] / ``nstep`` int32 [n] of the
    current step; ``seed`` is None otherwise"""
    __slots__ = ("kind", "host_kind", "table", "order", "host_order", "coef", "hist", "cn_table", "seed", "cn", "nstep")


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

    def entry(self, key: tuple, reqs: Sequence, build_cond: Callable[[], tuple], build_inpaint: Optional[Callable[[], tuple]] = None,
              build_multistep: Optional[Callable[[], tuple]] = None) -> _Entry:
        """the entry of a batch composition, built on first use.  ``build_inpaint``: the packed rows of its inpainting requests (Denoiser._inpaint_rows;
        None for a composition without one), fixed for the composition like ``cond``.  ``build_multistep``: the kinds and the [n, S, 4] coefficient
        table of its rows (Denoiser._multistep_rows; None for a composition of Euler requests)."""
        e = self._entries.get(key)
        if e is not None:
            self._entries.move_to_end(key)
            return e
        e = _Entry()
        e.uid = new_uid()
        e.cond = build_cond()
        e.inpaint = build_inpaint() if build_inpaint is not None else None
        e.multistep = self._multistep(build_multistep() if build_multistep is not None else None)
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

    def _multistep(self, built: Optional[tuple]) -> Optional[_Multistep]:
        if built is None:
            return None
        kinds, tab4 = built[:2]                           # tab4 [n, S, 4] = (cx, c0 first order, c0 second order, c1 second order): mx_sampler_coeffs
        m = _Multistep()
        m.host_kind = [k if k in (1, 2) else 0 for k in kinds]
        m.kind = _upload(torch.tensor(m.host_kind, dtype=torch.int32), self.device)
        both = np.zeros(tab4.shape[:2] + (2, 3), dtype=np.float32)
        both[:, :, 0, :2] = tab4[:, :, :2]                # first order: c1 = 0, the history is not read
        both[:, :, 1, 0] = tab4[:, :, 0]
        both[:, :, 1, 1:] = tab4[:, :, 2:]
        m.table = _upload(torch.from_numpy(both), self.device)
        m.order = torch.zeros(len(kinds), dtype=torch.int64, device=self.device)
        m.host_order = [0] * len(kinds)
        m.coef = m.hist = m.cn_table = m.seed = m.cn = m.nstep = None
        if len(built) > 2:                                # (cn [n, S], seeds): the noise rows of the stochastic requests
            cn, seeds = built[2]
            m.cn_table = _upload(torch.from_numpy(np.ascontiguousarray(cn, dtype=np.float32)), self.device)
            m.seed = _upload(torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64), self.device)
        return m

    @staticmethod
    def _orders(m: _Multistep, reqs: Sequence) -> List[int]:
        """1 for the rows that step second order now: a multistep row whose request carries the history of the step right before this one (not the
        first step of a request wherever it starts, not a rewound one)"""
        return [int(bool(k) and r.history is not None and r.history_step == r.step_index - 1) for k, r in zip(m.host_kind, reqs)]

    def step_scalars(self, e: _Entry, reqs: Sequence) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(sigma, sigma_next, timestep) fp32 [n] of the requests' CURRENT step; advances the device-side index."""
        host = [r.step_index for r in reqs]
        for h, lim in zip(host, e.limit):
            if not 0 <= h < lim:
                raise IndexError(f"step_index {h} outside the request's {lim} steps")
        if host != e.host_idx:
            e.idx.copy_(_upload(torch.tensor(host, dtype=torch.int64), self.device), non_blocking=True)
        vals = e.table[:, e.rows, e.idx]          # [3, n]
        m = e.multistep
        if m is not None:                         # (cx, c0, c1) of this step in each row's order, by the same index
            order = self._orders(m, reqs)
            if order != m.host_order:             # a request's first step, its second, a rewind: in between the orders stand
                m.order.copy_(_upload(torch.tensor(order, dtype=torch.int64), self.device), non_blocking=True)
                m.host_order = order
            m.coef = m.table[e.rows, e.idx, m.order]          # [n, 3]
            if m.seed is not None:                            # the noise coefficient of this step, and the step index as the generators' counter
                m.cn, m.nstep = m.cn_table[e.rows, e.idx], e.idx.to(torch.int32)
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

    def history(self, e: _Entry, reqs: Sequence, lat: torch.Tensor) -> torch.Tensor:
        """the composition's fp32 history buffer [n, C, h, w], shaped as the latents ``lat``.  After a step every multistep request holds a view of row
        i of it, so it is that buffer itself; otherwise (a request arrived from another composition or denoiser) it is rebuilt by concatenation.
        Only second-order rows are read by the step: the other rows of a rebuilt buffer are uninitialised."""
        m = e.multistep
        order = self._orders(m, reqs)
        h = m.hist
        if h is not None and h.shape == lat.shape and all(not o or (r.history.data_ptr() == h[i].data_ptr() and r.history.shape[1:] == h.shape[1:])
                                                          for i, (o, r) in enumerate(zip(order, reqs))):
            return h
        blank = torch.empty((1,) + tuple(lat.shape[1:]), dtype=torch.float32, device=lat.device)
        m.hist = torch.cat([r.history.to(device=lat.device, dtype=torch.float32) if o else blank for o, r in zip(order, reqs)], dim=0).contiguous()
        return m.hist
