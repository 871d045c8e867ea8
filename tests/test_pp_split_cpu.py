"""The split-batch decomposition of patch parallelism (CfgSplitLayout: distrifuser's default, CFG branches on two rank groups) on the host:
the rank arithmetic against the formulas of distrifuser/distrifuser/distrifuser/utils.py:72-116, restated here, and what one step exchanges,
walked with mx_unet_pp_comm_plan / mx_mmdit_pp_comm_plan and a recording callback (no process group, no GPU)."""
import ctypes as C

import pytest


def test_layout_is_distri_config_rank_arithmetic():
    from sduss_amd.patch_parallel import CfgSplitLayout
    for world in (1, 2, 4, 8):
        lay = CfgSplitLayout(world)                                    # DistriConfig defaults: do_classifier_free_guidance=True, split_batch=True
        npb = world // 2                                               # utils.py:73
        if npb == 0:                                                   # utils.py:74-75
            npb = 1
        assert lay.n_device_per_batch == npb
        for rank in range(world):
            assert lay.batch_idx(rank) == 1 - int(rank < (world // 2))          # utils.py:107
            assert lay.split_idx(rank) == rank % npb                            # utils.py:116
        for i in range(2):
            assert lay.batch_ranks(i) == list(range(i * (world // 2), (i + 1) * (world // 2)))    # utils.py:93
        for i in range(world // 2):
            assert lay.pair_ranks(i) == [i, i + world // 2]                     # utils.py:97
        assert lay.splits == (world >= 2)                                       # utils.py:90: groups from two ranks on
        if world >= 2:
            # every rank is in exactly one batch group, at position split_idx, and in exactly one pair group, at position batch_idx
            for rank in range(world):
                assert lay.batch_ranks(lay.batch_idx(rank))[lay.split_idx(rank)] == rank
                assert lay.pair_ranks(lay.split_idx(rank))[lay.batch_idx(rank)] == rank
        for kw in (dict(do_classifier_free_guidance=False), dict(split_batch=False)):
            flat = CfgSplitLayout(world, **kw)
            assert flat.n_device_per_batch == world and not flat.splits          # utils.py:76-77
            assert all(flat.batch_idx(r) == 0 and flat.split_idx(r) == r for r in range(world))     # utils.py:109, 116
            flat.make_groups()                                                    # no group is made (and no process group is needed)
            assert flat.batch_groups is None and flat.pair_groups is None
    for bad in (0, 3, 6, 12):
        with pytest.raises(AssertionError):                                       # utils.py:52
            CfgSplitLayout(bad)


def _base_handle():
    """SDXL-base geometry without weights: the comm-plan walk only needs the config"""
    from sduss_amd import config, lib
    l = lib.load()
    pcfg = config.UNetConfig.sdxl_base()
    cc = lib.UNetConfigC()
    cc.in_channels, cc.out_channels, cc.n_levels, cc.layers_per_block = pcfg.in_channels, pcfg.out_channels, len(pcfg.block_out_channels), pcfg.layers_per_block
    for i, v in enumerate(pcfg.block_out_channels):
        cc.block_out_channels[i] = v; cc.down_has_attn[i] = int(pcfg.down_has_attn[i])
        cc.transformer_layers[i] = pcfg.transformer_layers_per_block[i]; cc.num_heads[i] = pcfg.num_heads[i]
    cc.cross_attention_dim, cc.addition_time_embed_dim = pcfg.cross_attention_dim, pcfg.addition_time_embed_dim
    cc.projection_class_embeddings_input_dim, cc.norm_num_groups = pcfg.projection_class_embeddings_input_dim, pcfg.norm_num_groups
    h = l.mx_unet_create(C.byref(cc))
    assert h
    return l, h


def test_sdxl_base_1024_world8_split_batch_walk():
    """BASELINE configs[3] on 8 ranks, both decompositions: (full) batch 2, 16 rows per rank, 8-rank gathers; (split) CfgSplitLayout(8): batch 1,
    32 rows per rank, 4-rank gathers inside the branch.  The split issues the same exchanges, sends no more per rank, and receives 3 slots per
    exchange against 7: received_split = 3 x sent_split < 0.5 x received_full = 0.5 x 7 x sent_full (a bound from the slot counts: 3 / 7 < 0.5
    and sent_split <= sent_full; nothing is measured)."""
    from sduss_amd.patch_parallel import CfgSplitLayout, CommLog, walk_comm_plan
    l, h = _base_handle()
    lat, ctx, world = 128, 77, 8
    lay = CfgSplitLayout(world)
    npb = lay.n_device_per_batch
    assert npb == 4
    res = {}
    for name, batch, ranks in (("full", 2, world), ("split", 1, npb)):
        rows = lat // ranks
        need = l.mx_unet_workspace_bytes_pp(h, batch, rows, lat, ctx, ranks)
        assert need > 0, l.mx_last_error()
        per_rank = [walk_comm_plan(l.mx_unet_pp_comm_plan, h, batch, rows, lat, ctx, ranks, rank=r) for r in (0, ranks - 1)]
        assert per_rank[0] == per_rank[1], "the ranks of a branch must issue the same sequence of exchanges"
        log = CommLog(); log.calls = per_rank[0]
        log.check(need, ranks)
        sent = sum(nb for _s, _r, nb in log.calls)
        res[name] = dict(n=len(log.calls), sent=sent, recv=sent * (ranks - 1), state=l.mx_unet_pp_state_bytes(h, batch, rows, lat, ctx, ranks))
    l.mx_unet_destroy(h)
    full, split = res["full"], res["split"]
    print(f"full: {full}\nsplit: {split}")
    assert split["n"] == full["n"] > 0
    assert split["sent"] <= full["sent"]
    assert split["recv"] == 3 * split["sent"] and full["recv"] == 7 * full["sent"]
    assert split["recv"] < 0.5 * full["recv"]
    assert 0 < split["state"] < full["state"]


def test_sd3_split_batch_walk():
    """mx_mmdit_pp_comm_plan at tiny width, world 2 inside a branch: batch 1 (one CFG row) issues the exchanges of the existing SD3 walk
    (tests/test_pp_gloo.py: two per joint block, two more per dual block), each of half the bytes of batch 2"""
    from sduss_amd import config, lib
    from sduss_amd.patch_parallel import CommLog, walk_comm_plan
    from sduss_amd.transformer_sd3 import mmdit_config_c
    l = lib.load()
    pcfg = config.MMDiTConfig.tiny()
    h = l.mx_mmdit_create(C.byref(mmdit_config_c(pcfg)))
    assert h
    world, Hl, W, Lt = 2, 16, 32, 77
    both = walk_comm_plan(l.mx_mmdit_pp_comm_plan, h, 2, Hl, W, Lt, world, rank=1)
    one = walk_comm_plan(l.mx_mmdit_pp_comm_plan, h, 1, Hl, W, Lt, world, rank=1)
    assert len(one) == len(both) == 2 * pcfg.num_layers + 2 * len(pcfg.dual_attention_layers)
    assert [2 * nb for _s, _r, nb in one] == [nb for _s, _r, nb in both]
    need = l.mx_mmdit_workspace_bytes_pp(h, 1, Hl, W, Lt, world)
    log = CommLog(); log.calls = one
    log.check(need, world)
    assert 0 < l.mx_mmdit_pp_state_bytes(h, 1, Hl, W, Lt, world) < l.mx_mmdit_pp_state_bytes(h, 2, Hl, W, Lt, world)
    l.mx_mmdit_destroy(h)
