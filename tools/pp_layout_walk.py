"""The two decompositions of BASELINE configs[3] (one 1024 px SDXL-base request under CFG on 8 GPUs), walked on the host: what one step
exchanges.  No process group and no GPU: mx_unet_pp_comm_plan calls a recording callback once per exchange of a forward.

  (a) layout=None: batch 2 on every rank, 16 latent rows per rank, every exchange an 8-rank all-gather, the output rows gathered over the 8 ranks;
  (b) CfgSplitLayout(8), distrifuser's default (do_classifier_free_guidance and split_batch): batch 1, 32 latent rows per rank, every exchange a
      4-rank all-gather inside the branch, then ONE all-gather of the output rows over the world.

Bytes are what a synchronous step moves per rank: sent = the rank's own slot of every all-gather, received = the other ranks' slots.  A host
walk counts bytes; it measures no time.  Neither decomposition has been run on more than one GPU.

    python tools/pp_layout_walk.py > profiles/pp_split_batch_walk.txt
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sduss_amd import config, lib                                        # noqa: E402
from sduss_amd.patch_parallel import CfgSplitLayout, CommLog, walk_comm_plan  # noqa: E402


def base_handle(l):
    """SDXL-base geometry without weights: the walk only needs the config"""
    pcfg = config.UNetConfig.sdxl_base()
    cc = lib.UNetConfigC()
    cc.in_channels, cc.out_channels, cc.n_levels, cc.layers_per_block = pcfg.in_channels, pcfg.out_channels, len(pcfg.block_out_channels), pcfg.layers_per_block
    for i, v in enumerate(pcfg.block_out_channels):
        cc.block_out_channels[i] = v; cc.down_has_attn[i] = int(pcfg.down_has_attn[i])
        cc.transformer_layers[i] = pcfg.transformer_layers_per_block[i]; cc.num_heads[i] = pcfg.num_heads[i]
    cc.cross_attention_dim, cc.addition_time_embed_dim = pcfg.cross_attention_dim, pcfg.addition_time_embed_dim
    cc.projection_class_embeddings_input_dim, cc.norm_num_groups = pcfg.projection_class_embeddings_input_dim, pcfg.norm_num_groups
    h = l.mx_unet_create(C.byref(cc))
    assert h, l.mx_last_error()
    return pcfg, h


def walk(l, h, pcfg, batch, rows, ranks, out_ranks, lat=128, ctx=77, io_bytes=2):
    """(exchanges, sent, received, workspace, stale state) of one step: the plan's exchanges over `ranks` + the output gather over `out_ranks`"""
    calls = walk_comm_plan(l.mx_unet_pp_comm_plan, h, batch, rows, lat, ctx, ranks)
    need = l.mx_unet_workspace_bytes_pp(h, batch, rows, lat, ctx, ranks)
    assert need > 0, l.mx_last_error()
    log = CommLog(); log.calls = calls
    log.check(need, ranks)
    sent = sum(nb for _s, _r, nb in calls)
    out = batch * pcfg.out_channels * rows * lat * io_bytes               # this rank's output rows
    return dict(exchanges=len(calls), sent=sent, recv=sent * (ranks - 1), out_sent=out, out_recv=out * (out_ranks - 1), workspace=need,
                state=l.mx_unet_pp_state_bytes(h, batch, rows, lat, ctx, ranks))


def show(title, r, ranks, out_ranks):
    mb = lambda b: f"{b / 1e6:9.3f} MB"
    print(title)
    print(f"  exchanges per forward            {r['exchanges']:6d}   ({ranks}-rank all-gathers)  + 1 gather of the output rows over {out_ranks} ranks")
    print(f"  sent per rank per step       {mb(r['sent'])}  + {mb(r['out_sent'])} output rows = {mb(r['sent'] + r['out_sent'])}")
    print(f"  received per rank per step   {mb(r['recv'])}  + {mb(r['out_recv'])} output rows = {mb(r['recv'] + r['out_recv'])}")
    print(f"  workspace {mb(r['workspace'])}, stale-step state {mb(r['state'])}")


def main():
    l = lib.load()
    pcfg, h = base_handle(l)
    world = 8
    lay = CfgSplitLayout(world)
    npb = lay.n_device_per_batch
    a = walk(l, h, pcfg, 2, 128 // world, world, world)
    b = walk(l, h, pcfg, 1, 128 // npb, npb, world)
    l.mx_unet_destroy(h)
    print("SDXL-base, one 1024 x 1024 request under CFG (latent 128 x 128, bf16), world 8: bytes of one synchronous step, walked on the host")
    print("(mx_unet_pp_comm_plan with a recording callback; no process group, no GPU, no time measured)")
    print()
    show(f"(a) layout=None: batch 2 on every rank, {128 // world} latent rows per rank", a, world, world)
    print()
    show(f"(b) CfgSplitLayout({world}): batch 1 per branch, {128 // npb} latent rows per rank, exchanges inside the branch of {npb} ranks", b, npb, world)
    print()
    ta, tb = a["recv"] + a["out_recv"], b["recv"] + b["out_recv"]
    print(f"(b) / (a): exchanges {b['exchanges']} / {a['exchanges']}, sent {(b['sent'] + b['out_sent']) / (a['sent'] + a['out_sent']):.3f}, "
          f"received {tb / ta:.3f} (slots received per exchange: {npb - 1} against {world - 1})")


if __name__ == "__main__":
    main()
