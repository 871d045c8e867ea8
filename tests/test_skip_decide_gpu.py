"""The block-skip decision taken on the device (mx_block_cache.dev_down; patch_cache.hip pc_decide_kernel) against the host decision.

Everything is integer- or bit-exact: the kernel and its host twin (mx_skip_decide_host) are compiled from one statement of the rule
(sduss_amd/csrc/skip_decide.h), and a cached forward with ``PatchSkipCache(on_device=True)`` must give, step after step, the outputs, the
decisions, the blocks run, the patch counts and the reuse counters of the same forward with ``on_device=False``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sdxl_unet_ref as ref  # noqa: E402  (inputs and parameters only)
from sduss_amd import lib  # noqa: E402
from sduss_amd.block_cache import CompiledForest, MSE_UNCACHED, PatchSkipCache, ThresholdPredictor  # noqa: E402

SAMPLE = np.dtype([("row0", "<i8"), ("h", "<i4"), ("w", "<i4"), ("slot", "<i4"), ("npx", "<i4")])
PATCH = np.dtype([("b", "<i4"), ("py", "<i4"), ("px", "<i4"), ("pad", "<i4")])
RANGE = np.dtype([("row0", "<i8"), ("rows", "<i4"), ("slot", "<i4"), ("srow0", "<i4"), ("pad", "<i4")])


@functools.lru_cache(maxsize=None)
def _forest(n_estimators, n_feat, seed):
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(seed)
    n = 1200
    X = np.column_stack([rng.integers(0, 7, n).astype(np.float64), rng.integers(0, 1000, n).astype(np.float64)] +
                        [rng.uniform(0, 1, n) * np.where(rng.uniform(size=n) < 0.5, 1.0, 0.05) for _ in range(n_feat - 2)])
    y = ((X[:, 2:].max(axis=1) > 0.2 + 0.05 * X[:, 0]) ^ (rng.uniform(size=n) < 0.1)).astype(np.int64)
    return CompiledForest(RandomForestClassifier(n_estimators=n_estimators, max_depth=6, random_state=seed).fit(X, y))


def _host_struct(cf):
    f = lib.DeviceForestC()
    for k in ("left", "right", "feature", "threshold", "p1", "roots"):
        setattr(f, k, getattr(cf, k).ctypes.data)
    f.n_trees, f.n_nodes, f.n_feat = len(cf.roots), len(cf.left), cf.n_features
    return f


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _back(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("kind,B,n_feat,trees", [(0, 1, 3, 1), (0, 3, 6, 16), (1, 1, 3, 16), (1, 3, 3, 1)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_kernel_equals_its_host_twin(cuda_device, n, B, n_feat, trees, kind):
    """n lands on and around the wave (64), workgroup / chunk (256) and multi-chunk (1024) boundaries of the ordered compaction; kind 0 = patches
    (the UNet's unit, one or four inputs), kind 1 = token ranges (the MMDiT's: always one input, group counts)"""
    l = lib.load()
    B = min(B, n)
    rng = np.random.default_rng(1000 * n + 10 * n_feat + trees + kind)
    cf = _forest(trees, n_feat, seed=trees + n_feat)
    dfo = cf.to_device("cuda:0")
    n_in, forced_after, block = n_feat - 2, 2 + 2 * kind, 3
    # samples with unequal unit counts, scattered over the state rows; one of three holds no state
    cuts = np.sort(rng.choice(np.arange(1, n), B - 1, replace=False)) if B > 1 else np.array([], dtype=np.int64)
    counts = np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int64)
    unit_sample = np.repeat(np.arange(B), counts).astype(np.int32)
    n_slots = B + 2
    slots = rng.permutation(n_slots)[:B].astype(np.int32)
    grid_w = 7
    ups = int(-(-counts.max() // grid_w) * grid_w)
    valid = np.ones(B, dtype=np.uint8)
    if B == 3:
        valid[1] = 0
    group = (np.arange(B) * 2 // max(B, 1)).astype(np.int32)          # two resolution groups when B == 3
    ts = rng.integers(0, 1000, B).astype(np.float32)
    within = np.concatenate([np.arange(c) for c in counts]).astype(np.int32)      # unit index inside its sample
    samples = np.zeros(B, dtype=SAMPLE); samples["slot"] = slots; samples["h"] = samples["w"] = 8; samples["npx"] = grid_w
    if kind == 0:
        units = np.zeros(n, dtype=PATCH); units["b"] = unit_sample; units["py"] = within // grid_w; units["px"] = within % grid_w
        units["pad"] = rng.integers(0, 1 << 20, n)                     # carried into the asking list untouched
        part_len = [int(v) for v in (16, 8, 4, 4)[:n_in]]
        elems = [float(pl * pl * c) for pl, c in zip(part_len, (64, 128, 256, 256))]
    else:
        rows, d = 16, 128
        units = np.zeros(n, dtype=RANGE); units["rows"] = rows; units["slot"] = slots[unit_sample]; units["srow0"] = within * rows
        part_len, elems = [64], [float(d)]
    offs, parts, mse = [], [], np.zeros((n, n_in), dtype=np.float32)
    off = 0
    for i in range(n_in):
        scale = np.where(rng.uniform(size=(n, 1)) < 0.5, 1.0, 0.03)    # about half the units hardly moved
        denom = elems[i] * (rows if kind == 1 else 1)                  # the elements the partial sums of a unit cover
        p = rng.uniform(0, 1, (n, part_len[i])) * denom / part_len[i] * scale
        total = np.cumsum(p, axis=1)[:, -1]                            # the fp64 sum in order
        mse[:, i] = (total / denom).astype(np.float32)
        offs.append(off); parts.append(p.reshape(-1)); off += p.size
    counters = rng.integers(0, forced_after + 1, (n_slots, ups)).astype(np.int32)
    cidx = slots[unit_sample].astype(np.int64) * ups + within

    # ---- host twin ----
    hf = _host_struct(cf)
    cnt_h = np.ascontiguousarray(counters.reshape(-1)[cidx])
    run_h = np.zeros(n, dtype=np.uint8); ask_h = np.full(n, -1, dtype=np.int32); first_h = np.zeros(B + 1, dtype=np.int32); nask_h = np.zeros(1, dtype=np.int32)
    assert l.mx_skip_decide_host(C.byref(hf), block, forced_after, n, B, unit_sample.ctypes.data, valid.ctypes.data, ts.ctypes.data, mse.ctypes.data,
                                 cnt_h.ctypes.data, run_h.ctypes.data, ask_h.ctypes.data, first_h.ctypes.data, nask_h.ctypes.data) == 0, l.mx_last_error()
    n_ask = int(nask_h[0])

    # ---- the kernel ----
    d_units, d_samples, d_us, d_group, d_valid = _dev(units), _dev(samples), _dev(unit_sample), _dev(group), _dev(valid)
    d_ts, d_part, d_cnt = _dev(ts), _dev(np.concatenate(parts)), _dev(counters)
    d_run = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d_ask_units = torch.zeros(n * PATCH.itemsize, dtype=torch.uint8, device="cuda")
    d_ask_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_rec = torch.full((lib.SKIP_REC_FIRST + B + 1,), -5, dtype=torch.int32, device="cuda")
    a = lib.SkipDecideArgs()
    a.forest = C.pointer(dfo.struct)
    a.block, a.forced_after, a.n, a.n_samples, a.n_in, a.kind = block, forced_after, n, B, n_in, kind
    a.units, a.samples, a.unit_sample, a.sample_group = d_units.data_ptr(), d_samples.data_ptr(), d_us.data_ptr(), d_group.data_ptr()
    a.sample_valid, a.timesteps, a.partial = d_valid.data_ptr(), d_ts.data_ptr(), d_part.data_ptr()
    for i in range(n_in):
        a.part_off[i], a.part_len[i], a.part_elems[i] = offs[i], part_len[i], elems[i]
    a.counters, a.units_per_slot, a.grid_w, a.n_counters = d_cnt.data_ptr(), ups, grid_w, n_slots * ups
    a.run, a.ask_index, a.record = d_run.data_ptr(), d_ask_idx.data_ptr(), d_rec.data_ptr()
    a.ask_units = d_ask_units.data_ptr() if kind == 0 else None
    lib.check(l.mx_skip_decide_device(lib.current_stream(), C.byref(a)), "mx_skip_decide_device")
    torch.cuda.synchronize()

    rec = d_rec.cpu().numpy()
    run_d = d_run.cpu().numpy()
    assert rec[lib.SKIP_REC_STATUS] == 0 and rec[lib.SKIP_REC_NASK] == n_ask
    assert np.array_equal(run_d, run_h)
    assert n < 8 or 0 < n_ask < n, "the case must mix asking and reusing units"
    assert np.array_equal(d_ask_idx.cpu().numpy()[:n_ask], ask_h[:n_ask])              # the same list in the same order
    assert np.array_equal(rec[lib.SKIP_REC_FIRST:lib.SKIP_REC_FIRST + B + 1], first_h)
    want_cnt = counters.reshape(-1).copy(); want_cnt[cidx] = cnt_h                      # the units' counters updated, every other one untouched
    assert np.array_equal(_back(d_cnt, np.int32), want_cnt)
    if kind == 0:
        assert np.array_equal(_back(d_ask_units, PATCH)[:n_ask], units[ask_h[:n_ask]])
    gask = [int(run_h[group[unit_sample] == g].sum()) for g in range(lib.MAX_SEGS)]
    gtot = [int((group[unit_sample] == g).sum()) for g in range(lib.MAX_SEGS)]
    assert rec[lib.SKIP_REC_GASK:lib.SKIP_REC_GASK + lib.MAX_SEGS].tolist() == gask
    assert rec[lib.SKIP_REC_GTOT:lib.SKIP_REC_GTOT + lib.MAX_SEGS].tolist() == gtot
    if B == 3:                                                          # the sample without state: every unit runs, counters cleared
        assert run_d[unit_sample == 1].all() and (_back(d_cnt, np.int32)[cidx[unit_sample == 1]] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the UNet at the patch unit: host decision against device decision
# ---------------------------------------------------------------------------------------------------------------------------------------
GN_PATCH = 16
THRESHOLD = 0.01          # block 0 sees 1.9 for a patch whose latents were redrawn, 0.04 for its edge neighbours, 5e-4 for the diagonal one, 0 beyond


@pytest.fixture(scope="module")
def tiny(cuda_device):
    from sduss_amd.config import UNetConfig
    from sduss_amd.unet import MxUNet
    ocfg = ref.UNetConfig.tiny()
    return ocfg, MxUNet(UNetConfig.tiny(), ref.init_params(ocfg), device="cuda:0")


def _unet_steps(ocfg, comps, repeat_step):
    """per step: (row ids per group, latents per group, the concatenated conditions).  Two resolution groups (latents 32 and 48).  From one step to
    the next only the top-left patch of every request is redrawn -- so per step some patches move a lot, their neighbours a little (the 3x3
    conv_in) and the far ones not at all; request "c" is redrawn whole every step; step `repeat_step` repeats the previous one entirely."""
    g = torch.Generator().manual_seed(5)
    hw = {"a": 32, "b": 48, "c": 48, "d": 48}
    base = {k: ref.make_inputs(ocfg, 1, hw[k], seed=40 + i) for i, k in enumerate(hw)}
    lat = {k: base[k][0].clone() for k in hw}
    steps = []
    for s, ids in enumerate(comps):
        if s > 0 and s != repeat_step:
            for k in hw:
                if k == "c":
                    lat[k] = torch.randn(lat[k].shape, generator=g)
                else:
                    lat[k] = lat[k].clone(); lat[k][:, :, :GN_PATCH, :GN_PATCH] = torch.randn(1, 4, GN_PATCH, GN_PATCH, generator=g)
        t = 801.0 - 40.0 * (s - 1 if s == repeat_step else s)
        order = [k for grp in ids for k in grp]
        cond = [torch.cat([base[k][j] for k in order]).cuda() for j in (2, 3, 4)]
        xs = [torch.cat([lat[k] for k in grp]).cuda().to(torch.bfloat16) for grp in ids]
        steps.append(([f"{k}#0" for k in order], xs, torch.full((len(order),), t).cuda(), cond))
    return steps


def _run_unet(net, steps, on_device, record=False, predictor=None):
    cache = PatchSkipCache(predictor or ThresholdPredictor(THRESHOLD), forced_after=4, max_latent=48, on_device=on_device)
    if record:
        cache.record_features = True
    outs, decisions = [], []
    for row_ids, xs, ts, (ehs, te, ti) in steps:
        got = net.forward_mixed_cached(cache, xs, row_ids, ts, ehs, te, ti, GN_PATCH)
        outs.append([o.clone() for o in got])
        decisions.append([(int(b), np.asarray(m).copy()) for b, m in cache.decisions])
    torch.cuda.synchronize()
    return cache, outs, decisions


def _assert_same_run(host, dev):
    (ch, oh, dh), (cd, od, dd) = host, dev
    for s, (a, b) in enumerate(zip(oh, od)):
        for g, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), f"step {s}, group {g}: outputs differ"
    for s, (a, b) in enumerate(zip(dh, dd)):
        assert [blk for blk, _ in a] == [blk for blk, _ in b], f"step {s}: blocks decided"
        for (blk, ma), (_b, mb) in zip(a, b):
            assert np.array_equal(ma, mb), f"step {s}, block {blk}: decisions differ"
    assert ch.history == cd.history
    assert (ch.patches_asked, ch.patches_total) == (cd.patches_asked, cd.patches_total)
    assert ch.previous == cd.previous


def _host_record_shows(cache, decisions, predictor):
    """on the HOST path's own record: a partially asking block, a wholly skipped block, a forced run (ran although the predictor said reuse and
    the unit was cached)"""
    flat = [m for step in decisions for _b, m in step]
    assert len(flat) == len(cache.features)
    partial = any(0 < m.sum() < len(m) for m in flat)
    skipped = any(m.sum() == 0 for m in flat)
    forced = any(bool((m & (np.asarray(predictor.predict(f)) == 0) & (f[:, 2] < MSE_UNCACHED * 0.5)).any()) for m, f in zip(flat, cache.features))
    return partial, skipped, forced


def test_unet_patch_unit_device_decision_equals_the_host_decision(tiny):
    ocfg, net = tiny
    steps = _unet_steps(ocfg, [(["a"], ["b", "c"])] * 8, repeat_step=2)
    host = _run_unet(net, steps, on_device=False, record=True)
    assert _host_record_shows(host[0], host[2], ThresholdPredictor(THRESHOLD)) == (True, True, True)
    assert len(host[2][0]) == 7 and all(m.all() for _b, m in host[2][0])                 # the first forward: nothing cached, every patch runs
    dev = _run_unet(net, steps, on_device=True)
    assert len(dev[0].previous) == 7
    _assert_same_run(host, dev)


def test_unet_composition_change_keeps_the_staying_requests_counters(tiny):
    """between steps 3 and 4 request "c" leaves and "d" joins: the checks above still hold, every patch of "d" runs in its first step and "b"
    (static but for its top-left patch) keeps counting: its far patch is forced at step 5 as if nothing had happened"""
    ocfg, net = tiny
    comps = [(["a"], ["b", "c"])] * 4 + [(["a"], ["b", "d"])] * 4
    steps = _unet_steps(ocfg, comps, repeat_step=2)
    host = _run_unet(net, steps, on_device=False, record=True)
    assert _host_record_shows(host[0], host[2], ThresholdPredictor(THRESHOLD)) == (True, True, True)
    dev = _run_unet(net, steps, on_device=True)
    _assert_same_run(host, dev)
    n_a, n_48 = (32 // GN_PATCH) ** 2, (48 // GN_PATCH) ** 2
    d_units, b_far = slice(n_a + n_48, n_a + 2 * n_48), n_a + n_48 - 1
    assert all(m[d_units].all() for _b, m in dev[2][4])                                    # the new request: all of its patches run
    blk0 = [step[0][1][b_far] for step in dev[2]]                                          # block 0, the bottom-right patch of "b"
    assert blk0 == [True, False, False, False, False, True, False, False]                  # four reuses, the forced run at step 5: the counter survived
    assert dev[0].previous[0]["b#0-2-2"] == 2


def test_predict_is_never_called_in_device_mode(tiny):
    ocfg, net = tiny
    steps = _unet_steps(ocfg, [(["a"], ["b", "c"])] * 3, repeat_step=2)
    calls = []

    def spy(*args):
        calls.append(args[1])
        return 1
    cache = PatchSkipCache(ThresholdPredictor(THRESHOLD), forced_after=4, max_latent=48, on_device=True)
    cb = lib.SKIP_PREDICT_FN(spy)
    cache.desc.predict = cb
    for row_ids, xs, ts, (ehs, te, ti) in steps:
        net.forward_mixed_cached(cache, xs, row_ids, ts, ehs, te, ti, GN_PATCH)
    torch.cuda.synchronize()
    assert calls == [] and len(cache.history) == 3 and cache.history[0] == 0x7f


def test_no_valid_slot_every_unit_runs_and_equals_the_mixed_forward(tiny):
    """the first forward of a fresh cache: nothing is read back, every unit runs, and the output is the host path's first forward bit for bit --
    which tests/test_block_cache_gpu.py holds against forward_mixed"""
    ocfg, net = tiny
    steps = _unet_steps(ocfg, [(["a"], ["b", "c"])], repeat_step=-1)
    row_ids, xs, ts, (ehs, te, ti) = steps[0]
    want = net.forward_mixed(xs, ts, ehs, te, ti, gn_patch=GN_PATCH)
    host = _run_unet(net, steps, on_device=False)
    dev = _run_unet(net, steps, on_device=True)
    _assert_same_run(host, dev)
    n_units = (32 // GN_PATCH) ** 2 + 2 * (48 // GN_PATCH) ** 2
    assert dev[0].history == [0x7f] and dev[0].patches_asked == dev[0].patches_total == 7 * n_units
    assert all(m.all() and len(m) == n_units for _b, m in dev[2][0])
    assert all(v == 0 for blk in dev[0].previous.values() for v in blk.values())
    for o, w in zip(dev[1][0], want):
        l2 = float((o.float() - w.float()).norm() / w.float().norm())
        assert l2 <= 0.025, f"rel L2 {l2}"         # the bound of test_patch_unit_cached_forward_all_asking_equals_the_mixed_forward: the cached entry
        #                                            rounds to bf16 before the time-embedding / residual adds, so it is not forward_mixed bit for bit


def test_unet_fitted_forest_on_device_equals_the_host(tiny):
    """the same comparison with fitted forests (16 trees; 3 features for the down / mid blocks, 6 for the up blocks) instead of the threshold chain"""
    ocfg, net = tiny
    steps = _unet_steps(ocfg, [(["a"], ["b", "c"])] * 4, repeat_step=2)
    down, up = _forest(16, 3, seed=3), _forest(16, 6, seed=4)

    def run(on_device):
        cache = PatchSkipCache(down, up, forced_after=4, max_latent=48, on_device=on_device)
        outs, decisions = [], []
        for row_ids, xs, ts, (ehs, te, ti) in steps:
            outs.append([o.clone() for o in net.forward_mixed_cached(cache, xs, row_ids, ts, ehs, te, ti, GN_PATCH)])
            decisions.append([(int(b), np.asarray(m).copy()) for b, m in cache.decisions])
        return cache, outs, decisions
    _assert_same_run(run(False), run(True))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the MMDiT at the chunk unit
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mmdit_chunk_unit_device_decision_equals_the_host_decision(cuda_device):
    """tiny SD3 config, two groups (latents 16 and 32, chunks of 8 latent pixels: 4 and 16 token ranges), forced_after = 2, six steps.  A chunk is a
    range of token rows and block 0's input (patch embedding + positions) is local to the token, so redrawing the top two latent rows of the
    32-latent alone makes exactly ONE of its 16 chunks ask in block 0 (the <= 1/16 "renew the asking chunks only" rule of the dual blocks)
    while the other group has no asking chunk at all."""
    from oracle import sd3_mmdit_ref as m
    from sduss_amd.config import MMDiTConfig
    from sduss_amd.transformer_sd3 import MxSD3Transformer
    ocfg = m.MMDiTConfig.tiny()
    net = MxSD3Transformer(MMDiTConfig.tiny(), m.init_params(ocfg), device="cuda:0")
    lt, patch, thr = 20, 8, 1e-4
    base = {k: m.make_inputs(ocfg, 1, hw, seed=60 + i, ctx_len=lt) for i, (k, hw) in enumerate([("a", 16), ("b", 32)])}
    g = torch.Generator().manual_seed(9)
    lat = {k: base[k][0].clone() for k in base}
    steps = []
    for s in range(6):                                                  # step 2 repeats step 1 entirely: every block is skipped as a whole
        if s in (1, 3, 5):
            lat["b"] = lat["b"].clone(); lat["b"][:, :, :2, :] = torch.randn(1, ocfg.in_channels, 2, 32, generator=g)
        if s == 4:
            lat["a"] = torch.randn(lat["a"].shape, generator=g)
        xs = [lat[k].cuda().to(torch.bfloat16) for k in ("a", "b")]
        cond = [torch.cat([base[k][j] for k in ("a", "b")]).cuda() for j in (2, 3)]
        steps.append((["a#0", "b#0"], xs, torch.full((2,), 901.0 - 60.0 * (1 if s == 2 else s)).cuda(), cond))

    def run(on_device):
        cache = PatchSkipCache(ThresholdPredictor(thr), forced_after=2, max_latent=32, mmdit_ctx_len=lt, on_device=on_device)
        if not on_device:
            cache.record_features = True
        outs, decisions = [], []
        for row_ids, xs, ts, (ehs, pooled) in steps:
            outs.append([o.clone() for o in net.forward_mixed_cached(cache, xs, row_ids, ts, ehs, pooled, patch)])
            decisions.append([(int(b), np.asarray(mk).copy()) for b, mk in cache.decisions])
        torch.cuda.synchronize()
        return cache, outs, decisions
    host = run(False)
    assert _host_record_shows(host[0], host[2], ThresholdPredictor(thr)) == (True, True, True)
    masks = [mk for step in host[2] for _b, mk in step]
    assert all(len(mk) == 20 for mk in masks)
    assert any(mk[:4].sum() == 0 and mk[4:].sum() > 0 for mk in masks)                     # a block where one group has no asking chunk
    assert any(mk[4:].sum() == 1 for b, mk in host[2][1] if b in ocfg.dual_attention_layers)   # a dual block with a group at 1 of 16 asking
    dev = run(True)
    assert len(dev[0].previous) == ocfg.num_layers
    _assert_same_run(host, dev)
