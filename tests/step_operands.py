"""What the GPU tests of the scheduler step forms share (tests/test_inpaint_gpu.py, test_sampler_gpu.py, test_scheduler_step_forms_gpu.py): the
dtypes, the three shapes at which each access path can go wrong, the inpainting slots, and operands placed between guard elements."""
import pytest
import torch

import inpaint_ref as I

DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.float16, id="f16"), pytest.param(torch.bfloat16, id="bf16")]
# (n_lat, C, h, w), element offset of every tensor's base -> the path it takes
STEP_SHAPES = [pytest.param((3, 4, 5, 3), 0, id="3x4x5x3-elements"),          # hw = 15: no whole vector
               pytest.param((3, 16, 16, 16), 0, id="3x16x16x16-vectors"),     # 12288 elements: more than one block
               pytest.param((2, 4, 8, 8), 1, id="2x4x8x8-offset-base")]       # hw a whole number of vectors, every base off by one element
SLOTS = {3: [-1, 1, 0], 2: [1, -1]}                                           # k = 2, permuted: row != slot
K = 2
GUARD = 64


def placed(t, offset):
    """t on the device as a contiguous view ``offset`` elements into a buffer of its dtype with guard elements either side -> (buffer, view)"""
    fill = 77 if t.dtype in (torch.uint8, torch.int32) else 77.0
    buf = torch.full((GUARD + offset + t.numel() + GUARD,), fill, dtype=t.dtype, device="cuda")
    view = buf[GUARD + offset:GUARD + offset + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    ref = torch.full_like(buf, 77 if buf.dtype in (torch.uint8, torch.int32) else 77.0)
    return torch.equal(I.bits(buf[:lo]), I.bits(ref[:lo])) and torch.equal(I.bits(buf[lo + view.numel():]), I.bits(ref[lo + view.numel():]))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(I.bits(a), I.bits(b))
