"""What the four cached forwards (mx_unet_forward_cached, mx_unet_forward_cached_mixed, mx_mmdit_forward_cached, mx_mmdit_forward_cached_mixed)
refuse, and with which words: a table of bad calls, each wrong in ONE way unless it says otherwise, paired with the substring of mx_last_error
it produces.  No device: the pointers are fake 256-byte-aligned addresses that are never dereferenced, and every row is refused before the
first HIP call.  The handles marked `weights` carry a dummy one-entry blob, which is what it takes to get past "weights not set" (the io
dtype, the state's alignment in the sample-unit forms, the slot table, the size of the state).
Two checks have no row because no argument reaches them: "more inputs than MX_SKIP_MAX_IN" (the blocks' input counts are fixed by the
configuration) and the MMDiT's "equal chunks" (a group that is whole patches of whole tokens always splits evenly)."""
import ctypes as C

import pytest

from sduss_amd import config, lib
from sduss_amd.block_cache import CompiledForest
from sduss_amd.transformer_sd3 import mmdit_config_c
from test_skip_decide_cpu import _unet_handle, host_forest

FAKE = 0x10000
PREDICT = lib.SKIP_PREDICT_FN(lambda *a: 1)
OBSERVE = lib.SKIP_OBSERVE_FN(lambda *a: None)
DOWN, UP = host_forest(CompiledForest.from_threshold(0.1, 3)), host_forest(CompiledForest.from_threshold(0.1, 6))
BLOB = (C.c_ubyte * 64)()
ENTRY = (lib.WeightEntry * 1)()
ENTRY[0].name, ENTRY[0].offset, ENTRY[0].bytes = b"dummy", 0, 64


def int_array(ctype, values):
    """the row's values, then padding: a refused call may read the table up to its sample count"""
    return None if values is None else (ctype * 8)(*(list(values) + [100] * (8 - len(values))))


def make_cache(model, form, kw):
    """a descriptor the entry point accepts (host decision), then the row's changes; returns it with the arrays it points to"""
    if kw.get("cache", 0) is None:
        return None, ()
    d = lib.BlockCacheC()
    d.predict, d.state, d.state_bytes = PREDICT, FAKE, 1 << 30
    slots, valid = None, None
    if form == "mixed":
        side = 32 if model == "unet" else 16
        d.n_slots, d.max_h, d.max_w = 2, side, side
        slots, valid = [0, 1], [0, 0]
    slots, valid = kw.get("slots", slots), kw.get("slot_valid", valid)
    keep = (int_array(C.c_int32, slots), int_array(C.c_ubyte, valid))
    if keep[0] is not None:
        d.slots = C.cast(keep[0], C.POINTER(C.c_int32))
    if keep[1] is not None:
        d.slot_valid = C.cast(keep[1], C.POINTER(C.c_ubyte))
    if kw.get("device"):
        n_blocks, units = (7, 4) if model == "unet" else (4, 4)
        d.predict = lib.SKIP_PREDICT_FN()
        d.dev_down, d.dev_up = C.pointer(DOWN), (C.pointer(UP) if model == "unet" else None)
        d.dev_counters, d.dev_counters_bytes, d.forced_after = FAKE, lib.load().mx_skip_counters_bytes(n_blocks, 2, units), 4
    for k, v in kw.get("desc", {}).items():
        setattr(d, k, v)
    return d, keep


def call(l, handles, model, form, kw):
    """the row's call: a good call of the entry point with the row's arguments changed"""
    h = None if kw.get("handle", 0) is None else handles[(model, bool(kw.get("weights")))]
    d, keep = make_cache(model, form, kw)
    a = dict(io=lib.MX_BF16, latents=FAKE, timesteps=FAKE, ehs=FAKE, text_embeds=FAKE, time_ids=FAKE, pooled=FAKE, out=FAKE, batch=2,
             H=32 if model == "unet" else 16, ctx_len=77 if model == "unet" else 37, unit=16 if model == "unet" else 8, workspace=FAKE, n_groups=1)
    a["W"] = a["H"]
    a.update(kw.get("args", {}))
    cache = C.byref(d) if d is not None else None
    if form == "sample":
        if model == "unet":
            rc = l.mx_unet_forward_cached(h, None, a["latents"], a["io"], a["timesteps"], a["ehs"], a["text_embeds"], a["time_ids"], a["out"], a["batch"],
                                          a["H"], a["W"], a["ctx_len"], a.get("gn_patch", 0), a["workspace"], 1 << 20, cache)
        else:
            rc = l.mx_mmdit_forward_cached(h, None, a["latents"], a["io"], a["timesteps"], a["ehs"], a["pooled"], a["out"], a["batch"], a["H"], a["W"],
                                           a["ctx_len"], a["workspace"], 1 << 20, cache)
        return rc, l.mx_last_error()
    groups = None
    if kw.get("groups", 0) is not None:
        spec = kw.get("groups", [dict()])
        groups = (lib.UNetGroup * lib.MAX_SEGS)()
        for g in range(lib.MAX_SEGS):
            q = dict(latents=FAKE, out=FAKE, batch=2 if g == 0 else 1, H=a["H"], W=a["W"])
            q.update(spec[g] if g < len(spec) else {})
            groups[g].latents, groups[g].out, groups[g].batch, groups[g].H, groups[g].W = q["latents"], q["out"], q["batch"], q["H"], q["W"]
    if model == "unet":
        rc = l.mx_unet_forward_cached_mixed(h, None, groups, a["n_groups"], a["io"], a["timesteps"], a["ehs"], a["text_embeds"], a["time_ids"], a["ctx_len"],
                                            a["unit"], a["workspace"], 1 << 20, cache)
    else:
        rc = l.mx_mmdit_forward_cached_mixed(h, None, groups, a["n_groups"], a["io"], a["timesteps"], a["ehs"], a["pooled"], a["ctx_len"], a["unit"],
                                             a["workspace"], 1 << 20, cache)
    return rc, l.mx_last_error()


def rows():
    """(model, form, what is wrong, the message)"""
    out = []
    for model in ("unet", "mmdit"):
        m = model.encode()
        own = (m + b"_forward_cached: ", m + b"_forward_cached_mixed: ")
        unit_only = b"patch unit only (mx_unet_forward_cached_mixed)" if model == "unet" else b"chunk unit only (mx_mmdit_forward_cached_mixed)"
        operands = ["latents", "timesteps", "ehs", "out", "workspace"] + (["text_embeds", "time_ids"] if model == "unet" else ["pooled"])
        # ---- the sample unit ----
        s = []
        s.append((dict(handle=None), m + b": null handle"))
        s.append((dict(cache=None), own[0] + b"cache, cache->predict and cache->state are required"))
        s.append((dict(desc=dict(predict=lib.SKIP_PREDICT_FN())), own[0] + b"cache, cache->predict and cache->state are required"))
        s.append((dict(desc=dict(state=None)), own[0] + b"cache, cache->predict and cache->state are required"))
        s.append((dict(weights=True, desc=dict(state=FAKE + 16)), own[0] + b"cache->state must be 256-byte aligned"))
        s.append((dict(desc=dict(dev_down=C.pointer(DOWN))), own[0] + b"the device decision (dev_down) serves the " + unit_only))
        for k, v in (("batch", 0), ("H", 0), ("W", -16), ("ctx_len", 0)):
            s.append((dict(args={k: v}), m + b": bad shape"))
        for k in operands:
            s.append((dict(args={k: None}), m + b": null operand"))
        s.append((dict(), m + b": weights not set"))
        s.append((dict(weights=True, args=dict(io=99)), m + b": bad io dtype"))
        s.append((dict(weights=True, slots=[0, 1], slot_valid=[0, 0], desc=dict(n_slots=1)), own[0] + b"slots need slot_valid and n_slots >= batch"))
        s.append((dict(weights=True, slots=[0, 1], desc=dict(n_slots=2)), own[0] + b"slots need slot_valid and n_slots >= batch"))
        s.append((dict(weights=True, slots=[1, 1], slot_valid=[0, 0], desc=dict(n_slots=2)), own[0] + b"slots must be distinct and inside [0, n_slots)"))
        s.append((dict(weights=True, slots=[0, 2], slot_valid=[0, 0], desc=dict(n_slots=2)), own[0] + b"slots must be distinct and inside [0, n_slots)"))
        s.append((dict(weights=True, slots=[0, 1], slot_valid=[0, 0], desc=dict(n_slots=2, state_bytes=0)), own[0] + b"state buffer too small"))
        if model == "unet":
            s.append((dict(args=dict(H=30)), b"unet: H, W must be divisible by 2^(levels-1)"))
            s.append((dict(args=dict(gn_patch=-1)), b"unet: gn_patch must be >= 0"))
            s.append((dict(args=dict(gn_patch=12)), b"unet: H, W must be multiples of gn_patch"))
            s.append((dict(args=dict(gn_patch=4)), b"unet: gn_patch too small for the deepest level"))
        else:
            s.append((dict(args=dict(H=15)), b"mmdit: H, W must be multiples of patch_size"))
            s.append((dict(args=dict(W=50)), b"mmdit: latent larger than the positional table"))
        # wrong in two ways, the first message pinned: the unit comes before everything (tests/test_skip_decide_cpu.py relies on it)
        s.append((dict(desc=dict(dev_down=C.pointer(DOWN), predict=lib.SKIP_PREDICT_FN()), args=dict(batch=0)), unit_only))
        out += [(model, "sample", kw, msg) for kw, msg in s]
        # ---- the patch / chunk unit ----
        x = []
        required = own[1] + b"cache with predict (or dev_down), state, slots and slot_valid is required"
        x.append((dict(handle=None), m + b": null handle"))
        x.append((dict(cache=None), required))
        x.append((dict(desc=dict(predict=lib.SKIP_PREDICT_FN())), required))
        x.append((dict(desc=dict(state=None)), required))
        x.append((dict(slots=None), required))
        x.append((dict(slot_valid=None), required))
        x.append((dict(desc=dict(state=FAKE + 16)), own[1] + b"cache->state must be 256-byte aligned"))
        x.append((dict(groups=None), own[1] + b"1..MX_MAX_SEGS resolution groups"))
        x.append((dict(args=dict(n_groups=0)), own[1] + b"1..MX_MAX_SEGS resolution groups"))
        x.append((dict(args=dict(n_groups=lib.MAX_SEGS + 1)), own[1] + b"1..MX_MAX_SEGS resolution groups"))
        if model == "unet":
            unit_msg, slots_msg = own[1] + b"the patch unit needs is_sliced (gn_patch > 0, >= 2 pixels at the deepest level)", b"max_w (multiples of gn_patch) are required"
            multiple, bad_units = own[1] + b"every group's H, W must be multiples of gn_patch", (0, -8, 4)
        else:
            unit_msg, slots_msg = own[1] + b"the chunk unit (latent pixels per patch edge) must be a multiple of patch_size", b"max_w (multiples of the patch) are required"
            multiple, bad_units = own[1] + b"every group's H, W must be multiples of the patch", (0, -8, 3)
        side = 32 if model == "unet" else 16
        for v in bad_units:
            x.append((dict(args=dict(unit=v)), unit_msg))
        for k, v in (("n_slots", 0), ("max_h", 0), ("max_w", -side), ("max_h", side + side // 4)):
            x.append((dict(desc={k: v}), own[1] + b"cache->n_slots, max_h, " + slots_msg))
        x.append((dict(args=dict(ctx_len=0)), m + b": bad shape"))
        for k, v in (("batch", 0), ("H", 0), ("W", -side), ("H", side - side // 4)):
            x.append((dict(groups=[{k: v}]), multiple))
            x.append((dict(args=dict(n_groups=2), groups=[{}, {k: v}], desc=dict(n_slots=4)), multiple))
        x.append((dict(groups=[dict(H=2 * side)]), own[1] + b"a group is larger than the state rows (max_h, max_w)"))
        x.append((dict(args=dict(n_groups=2), groups=[{}, dict(W=2 * side)], desc=dict(n_slots=4)), own[1] + b"a group is larger than the state rows (max_h, max_w)"))
        x.append((dict(groups=[dict(latents=None)]), m + b": null group operand"))
        x.append((dict(args=dict(n_groups=2), groups=[{}, dict(out=None)], desc=dict(n_slots=4)), m + b": null group operand"))
        x.append((dict(groups=[dict(batch=3)]), own[1] + b"more samples than state rows (n_slots)"))
        x.append((dict(args=dict(n_groups=2), groups=[{}, {}]), own[1] + b"more samples than state rows (n_slots)"))
        x.append((dict(device=True, desc=dict(observe=OBSERVE)), own[1] + b"observe is a host callback and must be NULL with a device forest (dev_down)"))
        x.append((dict(device=True, desc=dict(dev_down=C.pointer(UP))), own[1] + b"dev_down has n_feat 6, its blocks need 3"))
        if model == "unet":
            x.append((dict(device=True, desc=dict(dev_up=C.pointer(DOWN))), own[1] + b"dev_up has n_feat 3, its blocks need 6"))
            x.append((dict(device=True, desc=dict(dev_up=None)), own[1] + b"dev_up has n_feat 3, its blocks need 6"))
        x.append((dict(device=True, desc=dict(forced_after=-1)), own[1] + b"forced_after must not be negative"))
        x.append((dict(device=True, desc=dict(dev_counters=None)), own[1] + b"dev_counters too small (mx_skip_counters_bytes)"))
        x.append((dict(device=True, desc=dict(dev_counters=FAKE + 4)), own[1] + b"dev_counters too small (mx_skip_counters_bytes)"))
        x.append((dict(device=True, desc=dict(dev_counters_bytes=64)), own[1] + b"dev_counters too small (mx_skip_counters_bytes)"))
        for k in operands:
            if k not in ("latents", "out"):
                x.append((dict(args={k: None}), m + b": null operand"))
        x.append((dict(), m + b": weights not set"))
        x.append((dict(device=True), m + b": weights not set"))
        x.append((dict(weights=True, args=dict(io=99)), m + b": bad io dtype"))
        x.append((dict(weights=True, slots=[1, 1]), own[1] + b"slots must be distinct and inside [0, n_slots)"))
        x.append((dict(weights=True, slots=[0, -1]), own[1] + b"slots must be distinct and inside [0, n_slots)"))
        x.append((dict(weights=True, desc=dict(state_bytes=256)), own[1] + b"state buffer too small"))
        if model == "mmdit":
            x.append((dict(groups=[dict(H=64, W=64)], desc=dict(max_h=64, max_w=64)), b"mmdit: latent larger than the positional table"))
        # wrong in two ways, the first message pinned: the forest comes before the weights (tests/test_skip_decide_cpu.py relies on it)
        x.append((dict(device=True, desc=dict(dev_down=C.pointer(UP)), args=dict(io=99)), own[1] + b"dev_down has n_feat 6, its blocks need 3"))
        out += [(model, "mixed", kw, msg) for kw, msg in x]
    return out


ROWS = rows()


@pytest.fixture(scope="module")
def handles():
    l = lib.load()
    made = {}
    for weights in (False, True):
        made[("unet", weights)] = _unet_handle(l)
        made[("mmdit", weights)] = l.mx_mmdit_create(C.byref(mmdit_config_c(config.MMDiTConfig.tiny())))
        assert made[("unet", weights)] and made[("mmdit", weights)]
    assert l.mx_unet_set_weights(made[("unet", True)], BLOB, 64, ENTRY, 1) == 0 and l.mx_mmdit_set_weights(made[("mmdit", True)], BLOB, 64, ENTRY, 1) == 0
    yield l, made
    for (model, _w), h in made.items():
        (l.mx_unet_destroy if model == "unet" else l.mx_mmdit_destroy)(h)


def test_every_check_has_a_row():
    said = b"\n".join(msg for _m, _f, _kw, msg in ROWS)
    for words in (b"null handle", b"are required", b"is required", b"256-byte aligned", b"unit only", b"bad shape", b"resolution groups", b"is_sliced", b"multiple of patch_size",
                  b"multiples of gn_patch) are required", b"multiples of the patch) are required", b"must be multiples of gn_patch", b"must be multiples of the patch",
                  b"larger than the state rows", b"null group operand", b"more samples than state rows", b"observe", b"dev_down has n_feat", b"dev_up has n_feat", b"forced_after",
                  b"dev_counters too small", b"null operand", b"weights not set", b"bad io dtype", b"slots need slot_valid", b"slots must be distinct", b"state buffer too small",
                  b"divisible by 2^(levels-1)", b"gn_patch must be >= 0", b"gn_patch too small", b"multiples of patch_size", b"positional table"):
        assert words in said, words
    assert len(ROWS) > 150


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[f"{m}-{f}-{k}" for k, (m, f, _kw, _msg) in enumerate(ROWS)])
def test_the_bad_call_is_refused_with_its_message(handles, k):
    l, made = handles
    model, form, kw, msg = ROWS[k]
    rc, said = call(l, made, model, form, kw)
    assert rc != 0 and msg in said, (kw, said)
