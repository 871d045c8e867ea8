"""The six sizing entry points of the block-skip cache (mx_{unet,mmdit}_block_cache_bytes, _patch_cache_bytes, _workspace_bytes_cached_mixed)
return the byte counts recorded in tests/golden/cached_sizing.json: the tiny configurations, the full ones at the shapes tests/asan_walk.cpp
walks, its two three-resolution group lists, and its refused arguments (which return 0).  Host only: a sizing walk launches nothing.
The file was recorded with `python tests/test_cached_sizing_cpu.py` and is compared for equality."""
import ctypes as C
import json
import os

import pytest

from sduss_amd import config, lib
from sduss_amd.transformer_sd3 import mmdit_config_c

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cached_sizing.json")
TINY3_UNET, TINY3_MMDIT = [[1, 16, 16], [2, 24, 24], [3, 32, 32]], [[1, 16, 16], [2, 24, 24], [1, 32, 32]]
TWO = [[1, 16, 16], [2, 32, 32]]
# (configuration, entry point, its arguments after the handle; a list of [batch, H, W] stands for (groups, n_groups))
CASES = [
    ("unet_tiny", "mx_unet_block_cache_bytes", [8, 32, 32]), ("unet_tiny", "mx_unet_block_cache_bytes", [2, 16, 24]),
    ("unet_tiny", "mx_unet_block_cache_bytes", [8, 30, 32]), ("unet_tiny", "mx_unet_block_cache_bytes", [0, 32, 32]),
    ("unet_tiny", "mx_unet_patch_cache_bytes", [8, 32, 32, 8]), ("unet_tiny", "mx_unet_patch_cache_bytes", [16, 32, 32, 8]),
    ("unet_tiny", "mx_unet_patch_cache_bytes", [8, 32, 32, 16]), ("unet_tiny", "mx_unet_patch_cache_bytes", [8, 32, 32, 5]),
    ("unet_tiny", "mx_unet_patch_cache_bytes", [8, 32, 32, 4]), ("unet_tiny", "mx_unet_patch_cache_bytes", [0, 32, 32, 8]),
    ("unet_tiny", "mx_unet_patch_cache_bytes", [8, 32, 32, 0]),
    ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TWO, 77, 8]), ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TWO, 77, 16]),
    ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TWO, 77, 0]), ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TWO, 77, 32]),
    ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [[], 77, 8]), ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TWO, 0, 8]),
    ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [TINY3_UNET, 77, 8]), ("unet_tiny", "mx_unet_workspace_bytes_cached_mixed", [[[2, 16, 16]], 77, 16]),
    ("sdxl_base", "mx_unet_block_cache_bytes", [8, 128, 128]), ("sdxl_base", "mx_unet_block_cache_bytes", [8, 30, 32]),
    ("sdxl_base", "mx_unet_patch_cache_bytes", [8, 128, 128, 32]),
    ("sdxl_base", "mx_unet_workspace_bytes_cached_mixed", [[[2, 64, 64], [2, 96, 96], [2, 128, 128]], 77, 32]),
    ("mmdit_tiny", "mx_mmdit_block_cache_bytes", [8, 32, 32, 37]), ("mmdit_tiny", "mx_mmdit_block_cache_bytes", [2, 16, 24, 20]),
    ("mmdit_tiny", "mx_mmdit_block_cache_bytes", [8, 31, 32, 37]), ("mmdit_tiny", "mx_mmdit_block_cache_bytes", [8, 32, 32, 0]),
    ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [8, 32, 32, 8, 37]), ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [16, 32, 32, 8, 37]),
    ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [4, 32, 32, 8, 37]), ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [8, 32, 32, 5, 37]),
    ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [8, 64, 64, 8, 37]), ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [8, 32, 32, 8, 0]),
    ("mmdit_tiny", "mx_mmdit_patch_cache_bytes", [8, 32, 32, 0, 37]),
    ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [TWO, 37, 8]), ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [TWO, 37, 0]),
    ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [TWO, 37, 32]), ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [[], 37, 8]),
    ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [TWO, 0, 8]), ("mmdit_tiny", "mx_mmdit_workspace_bytes_cached_mixed", [TINY3_MMDIT, 37, 8]),
    ("sd35_medium", "mx_mmdit_block_cache_bytes", [8, 128, 128, 333]), ("sd35_medium", "mx_mmdit_block_cache_bytes", [8, 127, 128, 333]),
    ("sd35_medium", "mx_mmdit_patch_cache_bytes", [8, 128, 128, 32, 333]),
    ("sd35_medium", "mx_mmdit_workspace_bytes_cached_mixed", [[[2, 64, 64], [4, 96, 96], [6, 128, 128]], 333, 32]),
]


def unet_handle(l, cfg):
    cc = lib.UNetConfigC()
    cc.in_channels, cc.out_channels, cc.n_levels, cc.layers_per_block = cfg.in_channels, cfg.out_channels, len(cfg.block_out_channels), cfg.layers_per_block
    for i, v in enumerate(cfg.block_out_channels):
        cc.block_out_channels[i] = v; cc.down_has_attn[i] = int(cfg.down_has_attn[i])
        cc.transformer_layers[i] = cfg.transformer_layers_per_block[i]; cc.num_heads[i] = cfg.num_heads[i]
    cc.cross_attention_dim, cc.addition_time_embed_dim = cfg.cross_attention_dim, cfg.addition_time_embed_dim
    cc.projection_class_embeddings_input_dim, cc.norm_num_groups = cfg.projection_class_embeddings_input_dim, cfg.norm_num_groups
    return l.mx_unet_create(C.byref(cc))


def measure(l):
    """every case's returned value, in the order of CASES"""
    made = {"unet_tiny": unet_handle(l, config.UNetConfig.tiny()), "sdxl_base": unet_handle(l, config.UNetConfig.sdxl_base()),
            "mmdit_tiny": l.mx_mmdit_create(C.byref(mmdit_config_c(config.MMDiTConfig.tiny()))),
            "sd35_medium": l.mx_mmdit_create(C.byref(mmdit_config_c(config.MMDiTConfig.sd35_medium())))}
    assert all(made.values())
    got = []
    for cfg, fn, args in CASES:
        call = []
        for a in args:
            if isinstance(a, list):
                groups = (lib.UNetGroup * max(len(a), 1))()
                for g, (b, h, w) in enumerate(a):
                    groups[g].batch, groups[g].H, groups[g].W = b, h, w
                call += [groups if a else None, len(a)]
            else:
                call.append(a)
        got.append(int(getattr(l, fn)(made[cfg], *call)))
    for cfg, h in made.items():
        (l.mx_unet_destroy if "mmdit" not in cfg and cfg != "sd35_medium" else l.mx_mmdit_destroy)(h)
    return got


def test_cached_sizing_entry_points_return_the_recorded_bytes():
    want = json.load(open(GOLDEN))
    assert [[c, f, a] for c, f, a in CASES] == [[r["config"], r["entry"], r["args"]] for r in want]
    got = measure(lib.load())
    for r, v in zip(want, got):
        assert v == r["bytes"], (r, v)
    assert any(r["bytes"] == 0 for r in want) and any(r["bytes"] > 0 for r in want)


if __name__ == "__main__":
    rows = [{"config": c, "entry": f, "args": a, "bytes": v} for (c, f, a), v in zip(CASES, measure(lib.load()))]
    with open(GOLDEN, "w") as out:
        out.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
