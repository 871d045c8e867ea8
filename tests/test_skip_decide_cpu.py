"""The device-side block-skip decision, host half (no GPU): mx_skip_decide_host -- the host twin of patch_cache.hip's pc_decide_kernel, built from
the same statement of the rule (sduss_amd/csrc/skip_decide.h) -- against the Python chain the host path runs today
(CompiledForest.predict -> decide() -> "uncached runs"), CompiledForest.from_threshold against ThresholdPredictor, and the argument checks of
the cached entry points, which are made before anything is launched.  Everything is integer- or bit-exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from sduss_amd import config, lib
from sduss_amd.block_cache import CompiledForest, MSE_UNCACHED, PatchSkipCache, QuantilePredictor, ThresholdPredictor, decide


def host_forest(cf):
    """mx_device_forest over the HOST tables of a CompiledForest (what mx_skip_decide_host takes)"""
    f = lib.DeviceForestC()
    for k in ("left", "right", "feature", "threshold", "p1", "roots"):
        setattr(f, k, getattr(cf, k).ctypes.data)
    f.n_trees, f.n_nodes, f.n_feat = len(cf.roots), len(cf.left), cf.n_features
    return f


def fit_forest(n_estimators, n_feat, seed):
    """a forest on rows [block, timestep, differences]: the differences lie on a binary grid, so every split threshold (a midpoint) is an fp32 number
    and a feature can be set EXACTLY to it"""
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(seed)
    n = 1500
    X = np.column_stack([rng.integers(0, 7, n).astype(np.float64), rng.integers(0, 1000, n).astype(np.float64)] +
                        [rng.integers(0, 256, n) / 64.0 for _ in range(n_feat - 2)])
    X[rng.uniform(size=n) < 0.5, 2:] /= 16.0                            # rows whose every difference is small (still on a binary grid)
    y = ((X[:, 2:].max(axis=1) > 1.0 + 0.25 * X[:, 0]) ^ (rng.uniform(size=n) < 0.1)).astype(np.int64)
    return RandomForestClassifier(n_estimators=n_estimators, max_depth=6, random_state=seed).fit(X, y)


def python_chain(cf, block, forced_after, unit_sample, valid, ts, mse, counters):
    """what PatchSkipCache._predict computes, with the library's marking of samples that hold no state"""
    n = len(unit_sample)
    m = np.where(valid[unit_sample][:, None] != 0, mse, np.float32(MSE_UNCACHED)).astype(np.float32)
    feats = np.empty((n, 2 + mse.shape[1]), dtype=np.float64)
    feats[:, 0] = float(block); feats[:, 1] = ts[unit_sample]; feats[:, 2:] = m
    uncached = feats[:, 2] >= MSE_UNCACHED * 0.5
    prev = np.where(uncached, 0, counters)
    run, new_prev = decide(cf.predict(feats), prev, forced_after)
    run = run | uncached
    ask = np.flatnonzero(run)
    first = np.zeros(len(valid) + 1, dtype=np.int64)
    np.add.at(first, unit_sample[ask] + 1, 1)
    return run, np.where(uncached, 0, new_prev), ask, np.cumsum(first)


def call_host(l, cf, block, forced_after, unit_sample, valid, ts, mse, counters):
    n, B = len(unit_sample), len(valid)
    f = host_forest(cf)
    us = np.ascontiguousarray(unit_sample, dtype=np.int32); va = np.ascontiguousarray(valid, dtype=np.uint8)
    t = np.ascontiguousarray(ts, dtype=np.float32); m = np.ascontiguousarray(mse, dtype=np.float32)
    cnt = np.ascontiguousarray(counters, dtype=np.int32).copy()
    run = np.full(n, 9, dtype=np.uint8); ask = np.full(n, -1, dtype=np.int32); first = np.full(B + 1, -1, dtype=np.int32); n_ask = np.zeros(1, dtype=np.int32)
    rc = l.mx_skip_decide_host(C.byref(f), block, forced_after, n, B, us.ctypes.data, va.ctypes.data, t.ctypes.data, m.ctypes.data, cnt.ctypes.data,
                               run.ctypes.data, ask.ctypes.data, first.ctypes.data, n_ask.ctypes.data)
    assert rc == 0, l.mx_last_error()
    return run.astype(bool), cnt, ask[:int(n_ask[0])], first, int(n_ask[0])


@pytest.mark.parametrize("n_feat", [3, 6])
@pytest.mark.parametrize("n_estimators", [1, 16])
def test_host_twin_equals_the_python_chain(n_estimators, n_feat):
    l = lib.load()
    cf = CompiledForest(fit_forest(n_estimators, n_feat, seed=10 * n_estimators + n_feat))
    rng = np.random.default_rng(n_feat)
    B = 4
    unit_sample = np.repeat(np.arange(B), [5, 1, 37, 90])           # unequal unit counts
    n = len(unit_sample)
    valid = np.array([1, 1, 0, 1], dtype=np.uint8)                   # sample 2 holds no state: its units are uncached
    ts = rng.integers(0, 1000, B).astype(np.float32)
    inner = np.flatnonzero((cf.left >= 0) & (cf.feature >= 2))
    assert len(inner) > 0
    for forced_after in (2, 4):
        counters = rng.integers(0, forced_after + 1, n).astype(np.int32)      # some equal forced_after: forced runs
        assert (counters == forced_after).any()
        mse = (rng.integers(0, 256, (n, n_feat - 2)) / 64.0).astype(np.float32)
        mse[rng.uniform(size=n) < 0.5] /= np.float32(16.0)            # rows whose every difference is small: the forest answers "reuse"
        # rows sitting exactly on a node's threshold (the walk goes LEFT on equality)
        ties = 0
        for k, node in enumerate(inner[:12]):
            thr = cf.threshold[node]
            if np.float64(np.float32(thr)) == thr:
                mse[100 + k, cf.feature[node] - 2] = np.float32(thr); ties += 1
        assert ties > 0
        for block in (0, 5):
            want = python_chain(cf, block, forced_after, unit_sample, valid, ts, mse, counters)
            got = call_host(l, cf, block, forced_after, unit_sample, valid, ts, mse, counters)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == len(want[2])
            assert 0 < got[4] < n                                     # a mixed answer
            assert got[0][unit_sample == 2].all() and (got[1][unit_sample == 2] == 0).all()


def test_the_tie_goes_left_and_the_counter_rule_holds():
    """a hand-made forest: one split on feature 2 at 0.5, left leaf p1 = 0, right leaf p1 = 1"""
    l = lib.load()
    cf = CompiledForest.from_threshold(0.5, 3)
    us = np.zeros(6, dtype=np.int32); valid = np.ones(1, dtype=np.uint8); ts = np.array([7.0], dtype=np.float32)
    mse = np.array([[0.5], [np.nextafter(np.float32(0.5), np.float32(1))], [0.25], [0.25], [0.25], [MSE_UNCACHED]], dtype=np.float32)
    counters = np.array([0, 3, 2, 1, 4, 3], dtype=np.int32)
    run, cnt, ask, first, n_ask = call_host(l, cf, 1, 2, us, valid, ts, mse, counters)
    #                 tie: reuse  above: run  forced(2)  reuse  past the mark: reuse  uncached: run
    assert run.tolist() == [False, True, True, False, False, True]
    assert cnt.tolist() == [1, 0, 0, 2, 5, 0]
    assert ask.tolist() == [1, 2, 5] and first.tolist() == [0, 3] and n_ask == 3


@pytest.mark.parametrize("thr", [0.0123, 0.0625])                     # the second is an fp32 number: a feature can equal it exactly
@pytest.mark.parametrize("n_in", [1, 4])
def test_from_threshold_equals_the_threshold_predictor(n_in, thr):
    cf = CompiledForest.from_threshold(thr, 2 + n_in)
    tp = ThresholdPredictor(thr)
    t32 = np.float32(thr)
    below, above = np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1))
    vals = np.array([0.0, below, t32, above, 1.0, MSE_UNCACHED], dtype=np.float32)
    rows = []
    for col in range(n_in):
        for v in vals:
            for rest in (0.0, below, t32):
                r = np.full(n_in, rest, dtype=np.float32); r[col] = v
                rows.append(np.concatenate([[3.0, 500.0], r]))
    X = np.asarray(rows, dtype=np.float32).astype(np.float64)        # the rows the library hands over: fp32 values
    want = tp.predict(X)
    assert 0 < want.sum() < len(want)
    assert np.array_equal(cf.predict(X), want)
    # and through the host twin (fresh counters, far from the forced run)
    l = lib.load()
    n = len(X)
    run, _cnt, _ask, _first, _n = call_host(l, cf, 3, 99, np.zeros(n, dtype=np.int32), np.ones(1, dtype=np.uint8), np.array([500.0], dtype=np.float32),
                                            X[:, 2:].astype(np.float32), np.zeros(n, dtype=np.int32))
    uncached = X[:, 2] >= MSE_UNCACHED * 0.5
    assert np.array_equal(run, (want > 0) | uncached)


def test_on_device_needs_a_predictor_the_device_can_evaluate():
    class Anything:
        def predict(self, f):
            return np.ones(len(f))
    for bad in (QuantilePredictor(0.5), Anything()):
        with pytest.raises(TypeError, match="QuantilePredictor"):
            PatchSkipCache(bad, on_device=True)
    pc = PatchSkipCache(ThresholdPredictor(0.1), on_device=True)
    assert not pc.desc.predict                                         # no callback in device mode
    with pytest.raises(ValueError):
        pc.record_features = True
    assert PatchSkipCache(ThresholdPredictor(0.1)).desc.predict        # the default is unchanged


def _unet_handle(l):
    pcfg = config.UNetConfig.tiny()
    cc = lib.UNetConfigC()
    cc.in_channels, cc.out_channels, cc.n_levels, cc.layers_per_block = 4, 4, 3, 2
    for i, v in enumerate(pcfg.block_out_channels):
        cc.block_out_channels[i] = v; cc.down_has_attn[i] = int(pcfg.down_has_attn[i])
        cc.transformer_layers[i] = pcfg.transformer_layers_per_block[i]; cc.num_heads[i] = pcfg.num_heads[i]
    cc.cross_attention_dim, cc.addition_time_embed_dim = pcfg.cross_attention_dim, pcfg.addition_time_embed_dim
    cc.projection_class_embeddings_input_dim, cc.norm_num_groups = pcfg.projection_class_embeddings_input_dim, 32
    return l.mx_unet_create(C.byref(cc))


def test_bad_arguments_are_refused_before_anything_is_launched():
    """status + mx_last_error, no device needed: the checks come before the first HIP call (the pointers below are never dereferenced)"""
    from sduss_amd.transformer_sd3 import mmdit_config_c
    l = lib.load()
    h = _unet_handle(l)
    assert h
    fake = 0x10000                                                      # 256-byte aligned, never touched
    down, up = host_forest(CompiledForest.from_threshold(0.1, 3)), host_forest(CompiledForest.from_threshold(0.1, 6))
    slots = (C.c_int32 * 2)(0, 1); valid = (C.c_ubyte * 2)(0, 0)
    groups = (lib.UNetGroup * 1)()
    groups[0].latents, groups[0].out, groups[0].batch, groups[0].H, groups[0].W = fake, fake, 2, 32, 32
    n_blocks, units = 7, (32 // 16) ** 2
    need = l.mx_skip_counters_bytes(n_blocks, 2, units)
    assert need >= 4 * n_blocks * 2 * units and l.mx_skip_counters_bytes(0, 2, units) == 0

    def cache(**kw):
        d = lib.BlockCacheC()
        d.state, d.state_bytes, d.n_slots, d.max_h, d.max_w = fake, 1 << 30, 2, 32, 32
        d.slots, d.slot_valid = C.cast(slots, C.POINTER(C.c_int32)), C.cast(valid, C.POINTER(C.c_ubyte))
        d.dev_down, d.dev_up, d.dev_counters, d.dev_counters_bytes, d.forced_after = C.pointer(down), C.pointer(up), fake, need, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def mixed(d):
        rc = l.mx_unet_forward_cached_mixed(h, None, groups, 1, lib.MX_BF16, fake, fake, fake, fake, 77, 16, fake, 1 << 20, C.byref(d))
        return rc, l.mx_last_error()
    # a forest whose rows are not as wide as the blocks' feature rows: down / mid blocks have one input, the up blocks layers_per_block + 2
    rc, msg = mixed(cache(dev_down=C.pointer(up)))
    assert rc != 0 and b"dev_down has n_feat 6" in msg
    rc, msg = mixed(cache(dev_up=C.pointer(down)))
    assert rc != 0 and b"dev_up has n_feat 3" in msg
    rc, msg = mixed(cache(dev_up=None))                                # no dev_up: dev_down decides the up blocks too -- and is too narrow
    assert rc != 0 and b"dev_up has n_feat 3" in msg
    # observe is a host callback
    obs = lib.SKIP_OBSERVE_FN(lambda *a: None)
    rc, msg = mixed(cache(observe=obs))
    assert rc != 0 and b"observe" in msg
    # counters that are too small, or missing
    rc, msg = mixed(cache(dev_counters_bytes=need - 256))
    assert rc != 0 and b"dev_counters too small" in msg
    rc, msg = mixed(cache(dev_counters=None))
    assert rc != 0 and b"dev_counters too small" in msg
    # well-formed device arguments get past these checks: the next refusal is about the weights, which this handle never received
    rc, msg = mixed(cache())
    assert rc != 0 and b"weights not set" in msg
    # the sample-unit entries keep the host decision
    cb = lib.SKIP_PREDICT_FN(lambda *a: 1)
    rc = l.mx_unet_forward_cached(h, None, fake, lib.MX_BF16, fake, fake, fake, fake, fake, 2, 32, 32, 77, 16, fake, 1 << 20, C.byref(cache(predict=cb)))
    assert rc != 0 and b"dev_down" in l.mx_last_error() and b"patch unit only" in l.mx_last_error()
    l.mx_unet_destroy(h)

    m = l.mx_mmdit_create(C.byref(mmdit_config_c(config.MMDiTConfig.tiny())))
    assert m
    groups[0].H = groups[0].W = 16
    d = cache(max_h=16, max_w=16, dev_down=C.pointer(up), dev_up=None)
    rc = l.mx_mmdit_forward_cached_mixed(m, None, groups, 1, lib.MX_BF16, fake, fake, fake, 37, 8, fake, 1 << 20, C.byref(d))
    assert rc != 0 and b"dev_down has n_feat 6" in l.mx_last_error()
    rc = l.mx_mmdit_forward_cached(m, None, fake, lib.MX_BF16, fake, fake, fake, fake, 2, 16, 16, 37, fake, 1 << 20, C.byref(cache(predict=cb)))
    assert rc != 0 and b"chunk unit only" in l.mx_last_error()
    l.mx_mmdit_destroy(m)
