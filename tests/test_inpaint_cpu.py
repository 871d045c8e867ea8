"""Host-side checks of inpainting: the five entries of csrc/scheduler_step.hip and csrc/inpaint.hip are declared, exported and bound; each refuses bad arguments before any
launch; the mask reference is diffusers' mask processor; the start mix of both models; the packed rows of a mixed batch; the request types still
construct as before.  No GPU: the library loads without a device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inpaint_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mx_cfg_euler_step_masked", "mx_cfg_flow_step_masked", "mx_inpaint_renoise", "mx_mask_to_latent", "mx_rgb8_paste")
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal


def test_entries_are_declared_exported_and_bound():
    from sduss_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in lib.SYMBOLS and hasattr(l, name)
        assert getattr(l, name).argtypes == lib.SYMBOLS[name][1]
    assert "} mx_inpaint_rows;" in hdr
    assert [f[0] for f in lib.InpaintRows._fields_] == ["k", "slot", "init", "noise", "mask"]
    assert l.mx_version() == 1


def _rows(k=0, slot=None, init=None, noise=None, mask=None):
    from sduss_amd import lib
    r = lib.InpaintRows()
    r.k, r.slot, r.init, r.noise, r.mask = k, slot, init, noise, mask
    return r


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_masked_step_refuses_without_a_launch(entry):
    from sduss_amd import lib
    fn = getattr(lib.load(), entry)
    good = _rows()
    full = dict(slot=OK, init=OK, noise=OK, mask=OK)
    cases = [((None, OK, OK, OK, 5.0, 2, 4, 16, 2, good), b"null"), ((OK, None, OK, OK, 5.0, 2, 4, 16, 2, good), b"null"),
             ((OK, OK, None, OK, 5.0, 2, 4, 16, 2, good), b"null"), ((OK, OK, OK, None, 5.0, 2, 4, 16, 2, good), b"null"),
             ((OK, OK, OK, OK, 5.0, 2, 4, 16, 2, None), b"null"),
             ((OK, OK, OK, OK, 5.0, 0, 4, 16, 2, good), b"positive"), ((OK, OK, OK, OK, 5.0, 2, 0, 16, 2, good), b"positive"),
             ((OK, OK, OK, OK, 5.0, 2, 4, -3, 2, good), b"positive"),
             ((OK, OK, OK, OK, 5.0, 2, 4, 16, 3, good), b"bad dtype"), ((OK, OK, OK, OK, 5.0, 2, 4, 16, -1, good), b"bad dtype"),
             ((OK, OK, OK, OK, 5.0, 2, 4, 16, 2, _rows(k=-1, **full)), b"negative")]
    for missing in full:
        cases.append(((OK, OK, OK, OK, 5.0, 2, 4, 16, 2, _rows(k=1, **{**full, missing: None})), b"need slot, init, noise and mask"))
    for args, msg in cases:
        rows = args[-1]
        status = fn(None, *args[:-1], C.byref(rows) if rows is not None else None)
        assert status != 0 and msg in lib.load().mx_last_error(), (args, lib.load().mx_last_error())


def test_small_entries_refuse_without_a_launch():
    from sduss_amd import lib
    l = lib.load()
    for args, msg in (((None, OK, OK + 64, OK, OK, 2, 64, 2), b"null"), ((OK, None, OK + 64, OK, OK, 2, 64, 2), b"null"),
                      ((OK, OK + 64, None, OK, OK, 2, 64, 2), b"null"), ((OK, OK + 64, OK + 128, None, OK, 2, 64, 2), b"null"),
                      ((OK, OK + 64, OK + 128, OK, None, 2, 64, 2), b"null"),
                      ((OK, OK + 64, OK + 128, OK, OK, 0, 64, 2), b"positive"), ((OK, OK + 64, OK + 128, OK, OK, 2, 0, 2), b"positive"),
                      ((OK, OK + 64, OK + 128, OK, OK, 2, 64, 5), b"bad dtype"),
                      ((OK, OK + 64, OK, OK, OK, 2, 64, 2), b"alias"), ((OK, OK + 64, OK + 64, OK, OK, 2, 64, 2), b"alias")):
        assert l.mx_inpaint_renoise(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((None, OK, 1, 16, 16, 8), b"null"), ((OK, None, 1, 16, 16, 8), b"null"), ((OK, OK, 0, 16, 16, 8), b"positive"),
                      ((OK, OK, 1, 16, 16, 0), b"positive"), ((OK, OK, 1, 20, 16, 8), b"multiples of the factor"),
                      ((OK, OK, 1, 16, 12, 8), b"multiples of the factor")):
        assert l.mx_mask_to_latent(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
    for args, msg in (((None, OK, OK, 1, 4, 4), b"null"), ((OK, None, OK, 1, 4, 4), b"null"), ((OK, OK + 64, None, 1, 4, 4), b"null"),
                      ((OK, OK + 64, OK, 1, 0, 4), b"positive"), ((OK, OK + 64, OK, 1, 4, -1), b"positive"), ((OK, OK, OK + 64, 1, 4, 4), b"alias")):
        assert l.mx_rgb8_paste(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())


def test_wrappers_check_shapes_and_dtypes():
    """the ops wrappers refuse with MxError before the library is called (CPU tensors: nothing could be launched anyway)"""
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    lat = torch.zeros(2, 4, 4, 4, dtype=torch.bfloat16)
    pred = torch.zeros(4, 4, 4, 4, dtype=torch.bfloat16)
    sg = torch.ones(2)
    slot = torch.tensor([0, -1], dtype=torch.int32)
    init = torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16)
    mask = torch.zeros(1, 4, 4, dtype=torch.uint8)
    for fn in (ops.cfg_euler_step_masked_, ops.cfg_flow_step_masked_):
        with pytest.raises(MxError, match="prediction"):
            fn(pred[:3], lat, sg, sg, 5.0)
        with pytest.raises(MxError, match="need slot"):
            fn(pred, lat, sg, sg, 5.0, init=init)
        with pytest.raises(MxError, match="slot must"):
            fn(pred, lat, sg, sg, 5.0, slot.long(), init, init, mask)
        with pytest.raises(MxError, match="noise must"):
            fn(pred, lat, sg, sg, 5.0, slot, init, init.float(), mask)
        with pytest.raises(MxError, match="mask must"):
            fn(pred, lat, sg, sg, 5.0, slot, init, init, mask[:, :3])
        with pytest.raises(MxError, match="one value per latent row"):
            fn(pred, lat, sg[:1], sg, 5.0)
    with pytest.raises(MxError):
        ops.inpaint_renoise(init, init, 1.0, 1.0)                       # not on the device
    with pytest.raises(MxError):
        ops.mask_to_latent(mask, 2)
    with pytest.raises(MxError):
        ops.rgb8_paste_(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), mask)


def test_latent_mask_is_the_mask_processor():
    """binarise at 0.5 of 255, then the nearest interpolation to the latent grid: non-square, with the two bytes either side of the threshold"""
    g = torch.Generator().manual_seed(4)
    for (b, H, W, f) in ((2, 24, 40, 8), (1, 8, 8, 8), (1, 12, 20, 4)):
        m = torch.randint(0, 256, (b, H, W), generator=g, dtype=torch.uint8)
        m[:, ::f, ::f] = torch.where(torch.rand(b, H // f, W // f, generator=g) < 0.5, 127, 128).to(torch.uint8)
        m[0, 0, 0], m[0, H - f, W - f] = 127, 128                       # (the two may be one pixel: 128 then stands)
        want = F.interpolate((m.float() / 255 >= 0.5).float()[:, None], size=(H // f, W // f))[:, 0]
        got = I.latent_mask(m, f)
        assert got.dtype == torch.uint8 and got.shape == (b, H // f, W // f)
        assert torch.equal(got.float(), want) and int(got[0, -1, -1]) == 1 and (H == f or int(got[0, 0, 0]) == 0)
        assert H == f or (bool((m[:, ::f, ::f] == 127).any()) and bool((m[:, ::f, ::f] == 128).any()))


def _denoisers():
    from sduss_amd.pipeline import SDXLDenoiser
    from sduss_amd.pipeline_sd3 import SD3Denoiser
    model = SimpleNamespace(device="cpu")
    return SDXLDenoiser(model), SD3Denoiser(model)


def test_start_mix_of_both_models():
    from sduss_amd.pipeline import start_step
    sdxl, sd3 = _denoisers()
    s = np.float32(0.7)
    keep, sigma = sdxl._start_mix(s)
    assert keep.dtype == np.float32 and keep == np.float32(1.0) and sigma == s
    keep, sigma = sd3._start_mix(s)
    assert keep.dtype == np.float32 and keep == np.float32(1.0) - s and sigma == s
    # the same arithmetic as the kernels' keep: fp32 1 - sigma
    assert float(keep) == float(I.step_keep(True, torch.tensor([0.7]))[0]) and float(I.step_keep(False, torch.tensor([0.7]))[0]) == 1.0
    # where a request starts, and from what: inside the schedule from the noised image, at strength 1 from pure noise
    for den, steps in ((sdxl, 10), (sd3, 8)):
        req = SimpleNamespace(num_inference_steps=steps)
        den.set_timesteps(req)
        t = start_step(steps, 0.5)
        assert den._inpaint_start_mix(req, t, 0.5) == den._start_mix(np.float32(req.sigmas[t]))
    req = SimpleNamespace(num_inference_steps=10)
    sdxl.set_timesteps(req)
    assert sdxl._inpaint_start_mix(req, 0, 1.0) == (np.float32(0.0), np.float32(sdxl.init_noise_sigma(10)))
    req = SimpleNamespace(num_inference_steps=8)
    sd3.set_timesteps(req)
    assert sd3._inpaint_start_mix(req, 0, 1.0) == (np.float32(0.0), np.float32(1.0))        # scale_noise at sigma 1: the noise itself


def test_requests_construct_as_before_and_rows_pack_in_batch_order():
    from sduss_amd.pipeline import Denoiser, InpaintState, Request
    from sduss_amd.pipeline_sd3 import SD3Request
    t = torch.zeros(1)
    a = Request(0, 128, 10, t, t, t, t, t, t, t)
    b = SD3Request(1, 128, 8, t, t, t, t, t)
    assert a.inpaint is None and b.inpaint is None and a.step_index == 0 and not a.done()
    assert Denoiser._inpaint_rows([a, a]) is None

    def state(v):
        return InpaintState(torch.full((1, 4, 2, 2), float(v)), torch.full((1, 4, 2, 2), -float(v)), torch.full((1, 2, 2), v, dtype=torch.uint8), None,
                            torch.zeros(1, 8, 8, dtype=torch.uint8), False)
    reqs = [Request(i, 128, 10, t, t, t, t, t, t, t) for i in range(4)]
    reqs[1].inpaint, reqs[3].inpaint = state(1), state(2)
    slot, init, noise, mask = Denoiser._inpaint_rows(reqs)
    assert slot.dtype == torch.int32 and slot.tolist() == [-1, 0, -1, 1]
    assert init.shape == (2, 4, 2, 2) and init[:, 0, 0, 0].tolist() == [1.0, 2.0] and noise[:, 0, 0, 0].tolist() == [-1.0, -2.0]
    assert mask.dtype == torch.uint8 and mask.shape == (2, 2, 2) and mask[:, 0, 0].tolist() == [1, 2]


def test_patch_parallel_refuses_inpainting():
    from sduss_amd.lib import MxError
    from sduss_amd.patch_parallel import PatchParallelDenoiser
    den = PatchParallelDenoiser.__new__(PatchParallelDenoiser)          # the refusal comes before anything of the model is touched
    with pytest.raises(MxError, match="inpainting is not available under patch parallelism"):
        den.step(SimpleNamespace(inpaint=object()))
