"""The seeded noise on the GPU (csrc/noise.h, noise.hip): mx_noise_fill against the numpy restatement (tests/noise_ref.py) -- the generator's words
bit for bit, the fp32 normals within a derived bound of fp64 on the same words, 16-bit outputs as the fp32 ones rounded once -- on the element path,
the vector path over more than one block, from offset bases and on rows whose last group is partial; and a request's noise not seeing its batch."""
import numpy as np
import pytest
import torch

import noise_ref as N
from step_operands import DTYPES, STEP_SHAPES, guards_intact, placed, same_bits

pytestmark = pytest.mark.gpu

# 27 elements per row: the last Philox group is partial, and row 1 does not start on a group of the batch -> the element path
SHAPES = STEP_SHAPES + [pytest.param((2, 3, 3, 3), 0, id="2x3x3x3-partial-group")]
SEEDS = [0xDEADBEEF12345678, 3, 2 ** 64 - 1]              # both halves of the key, and the sign bit of the int64 that carries it
STEPS = [0, 19, 2 ** 32 - 1]


def fill(shape, offset, dtype, seeds, steps, domain, scale=None, raw=False):
    """one mx_noise_fill into a guarded buffer at an element offset -> the rows it left, on the CPU (int32 bits when raw); guards checked"""
    from sduss_amd import lib, ops
    n = shape[0]
    buf, view = placed(torch.zeros(shape, dtype=torch.int32 if raw else dtype), offset)
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    sd, st = ops._seeds_and_steps("test", n, list(seeds[:n]), list(steps[:n]), "cuda")
    sc = None if scale is None else torch.tensor(scale[:n], dtype=torch.float32).cuda()
    l = lib.load()
    lib.check(l.mx_noise_fill(lib.current_stream(), view.data_ptr(), 0 if raw else lib.torch_dtype_code(dtype), n, view[0].numel(), sd.data_ptr(), st.data_ptr(),
                              domain, None if sc is None else sc.data_ptr(), int(raw)), "mx_noise_fill")
    torch.cuda.synchronize()
    assert guards_intact(buf, view)
    return view.cpu()


@pytest.mark.parametrize("shape,offset", SHAPES)
def test_raw_words(cuda_device, shape, offset):
    n, elems = shape[0], int(np.prod(shape[1:]))
    for domain in (N.INIT, N.STEP):
        got = fill(shape, offset, None, SEEDS, STEPS, domain, raw=True).reshape(n, elems).numpy().view(np.uint32)
        for r in range(n):
            want = N.words(SEEDS[r], STEPS[r], domain, elems)
            assert np.array_equal(got[r], want), (domain, r, np.nonzero(got[r] != want)[0][:8])


@pytest.mark.parametrize("shape,offset", SHAPES)
def test_normals(cuda_device, shape, offset):
    """fp32 normals within 4e-6 absolute of the fp64 Box-Muller on the same words.  u and t2 are exact in fp32, so only the chain rounds:
    r <= sqrt(-2 ln 2^-24) = 5.77; logf (1 ulp), the product by -2 (exact), sqrtf (halves the relative error, adds half an ulp) leave about 1.5 ulp
    relative on r, 1e-6 absolute at most; sincospif at <= 2 ulp of a value <= 1, times r, 1.4e-6; the final product half an ulp of |z| <= 5.77,
    3.4e-7 -- 2.8e-6 in all, under the 4e-6 held here.  With a scale the bound scales: one more product, half an ulp more."""
    n, elems = shape[0], int(np.prod(shape[1:]))
    scale = [14.6146, 0.25, 1.0]
    got = fill(shape, offset, torch.float32, SEEDS, STEPS, N.STEP).reshape(n, elems).double().numpy()
    scaled = fill(shape, offset, torch.float32, SEEDS, STEPS, N.STEP, scale=scale).reshape(n, elems).double().numpy()
    worst = 0.0
    for r in range(n):
        want = N.normals(SEEDS[r], STEPS[r], N.STEP, elems)
        worst = max(worst, float(np.abs(got[r] - want).max()))
        assert np.abs(got[r] - want).max() <= 4e-6, (r, np.abs(got[r] - want).max())
        s = float(np.float32(scale[r]))
        assert np.abs(scaled[r] - s * want).max() <= s * (4e-6 + 2.0 ** -24 * 5.77), r
        assert np.array_equal(scaled[r].astype(np.float32), (np.float32(scale[r]) * got[r].astype(np.float32)).astype(np.float32))      # one fp32 multiply
    print(f"largest distance from the fp64 normals: {worst:.3g}")


@pytest.mark.parametrize("shape,offset", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_16_bit_outputs_are_the_fp32_ones_rounded_once(cuda_device, dtype, shape, offset):
    for scale in (None, [14.6146, 0.25, 1.0]):
        wide = fill(shape, offset, torch.float32, SEEDS, STEPS, N.START, scale=scale)
        got = fill(shape, offset, dtype, SEEDS, STEPS, N.START, scale=scale)
        assert got.dtype == dtype and same_bits(got, wide.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_requests_noise_does_not_see_the_batch(cuda_device, dtype):
    """the same (seed, step) alone, as row 0 of 3 and as row 2 of 3: bit-equal rows, on the vector path, from an offset base and on 27-element rows
    (where row 2 of the batch starts at element 54, inside a group of the batch's own indexing)"""
    seed, step = SEEDS[0], 7
    for row_shape, offset in (((16, 16, 16), 0), ((4, 8, 8), 1), ((3, 3, 3), 0)):
        alone = fill((1,) + row_shape, offset, dtype, [seed], [step], N.STEP)
        first = fill((3,) + row_shape, offset, dtype, [seed, 11, 12], [step, 0, 1], N.STEP)
        last = fill((3,) + row_shape, offset, dtype, [11, 12, seed], [0, 1, step], N.STEP)
        assert same_bits(first[0:1], alone) and same_bits(last[2:3], alone), (row_shape, offset)
        assert not same_bits(first[1:2], alone) and not same_bits(last[0:1], last[1:2])
        other_step = fill((1,) + row_shape, offset, dtype, [seed], [step + 1], N.STEP)
        other_domain = fill((1,) + row_shape, offset, dtype, [seed], [step], N.INIT)
        assert not same_bits(other_step, alone) and not same_bits(other_domain, alone)


def test_seeded_noise_wrapper(cuda_device):
    from sduss_amd import ops
    from sduss_amd.lib import MxError
    z = ops.seeded_noise((2, 4, 8, 8), [5, 2 ** 64 - 1], 3, N.INIT, dtype=torch.bfloat16, scale=2.0)
    assert z.shape == (2, 4, 8, 8) and z.dtype == torch.bfloat16 and z.is_cuda
    want = fill((2, 4, 8, 8), 0, torch.bfloat16, [5, 2 ** 64 - 1], [3, 3], N.INIT, scale=[2.0, 2.0])
    assert same_bits(z.cpu(), want)
    raw = ops.seeded_noise((1, 27), 5, 3, N.INIT, raw=True)
    assert raw.dtype == torch.int32 and np.array_equal(raw.cpu().numpy().view(np.uint32)[0], N.words(5, 3, N.INIT, 27))
    with pytest.raises(MxError, match="one .* value per row"):
        ops.seeded_noise((2, 4), [1, 2, 3], 0, 0)
    with pytest.raises(MxError, match="shape"):
        ops.seeded_noise((4,), 1, 0, 0)
