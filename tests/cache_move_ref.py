"""CPU references for the kernels that move the block-skip cache's state (csrc/patch_cache.hip: pc_image_copy, pc_rows_load_stats, pc_gather,
pc_scatter, pc_patch_store, pc_patch_sq_diff, pc_range_copy, pc_range_sq_diff; csrc/elementwise.hip: sq_diff_partial, copy_rows), in the style
of kernel_ref.py / norm_ref.py and with their guards, NaN padding and comparator.

Almost everything these kernels do is a copy, so almost every reference here returns the BITS the kernel must leave (torch tensors on the CPU,
compared as int16): whole tensors, so that every cell the operation does not own is compared with what it held before.  Each reference is written
from the statement of its operation on images, patches and rows -- slicing [h, w, C] views -- not from the kernel's index arithmetic.

Geometry: samples are given at level 0 as (h, w, slot) with a common patch edge p0.  At level l the image is (h >> l, w >> l), its first row of a
batch tensor is row0 >> 2l (row0 = the level-0 pixels of the samples in front of it) and the patch edge is p0 >> l.  A batch tensor is
[rows, ld] with the images one after the other; a state tensor is [slots, row elements] with sample b's image at the start of row slot[b].

Arithmetic (the only places with any):
  image_copy, to_batch    fp32 in the kernel's order, then ONE round-to-nearest-even to bf16.  state + vec + residual is adds only: bit-exact.
                          gate: state * vec + residual may or may not be contracted into one fused multiply-add (patch_cache.hip is built with
                          contraction allowed): BOTH IEEE results are returned and a cell must equal one of them.
  rows_load_stats         bf16(state + residual) bit-exact; (sum, sum of squares) of the STORED values within norm_ref.row_stats_ref's bounds
                          (C 2^-24 sum|x|, C 2^-24 sum x^2); fin = (mean, rstd): d_mean = d_sum / C + 2^-24 |mean|,
                          d_var = d_q / C + 2 |mean| d_mean + d_mean^2 + 2 2^-24 (q / C), rstd by norm_ref.rstd_interval with rsqrtf's 2^-21.
  sq_diff (all three)     fp64 sum over the partition the kernel writes (a patch's pixel row; a chunk of ceil(vectors / 64) 16-byte vectors).
                          Every term is non-negative, so the bound is relative: (k + 3) 2^-24 ref, k = the squared terms ONE thread adds in
                          fp32 = 8 x the 16-byte vectors it visits = 8 ceil(vectors of the partition / 256) (256 threads stride the
                          partition; the 3: the difference's rounding, twice in its square, and the square's own).  The sum across threads is
                          fp64.  A unit equal to its cached value gives exactly 0.0, and so does an empty chunk.
"""
import math
from types import SimpleNamespace

import torch

import norm_ref
from kernel_ref import U32, assert_within, guard_violations, guarded, nan_padded, violations  # noqa: F401

THREADS = 256        # threads that stride one partition of a sq_diff launch
CHUNKS = 64          # chunks per range / per sample of pc_range_sq_diff and sq_diff_partial


def bits(t):
    return t.view(torch.int16)


# ---- geometry ----

def geometry(samples, level, p0):
    """samples [(h, w, slot)] at level 0 -> per sample (h, w, row0, slot, p) at `level`"""
    out, row0 = [], 0
    for h, w, slot in samples:
        assert row0 % (1 << 2 * level) == 0
        out.append(SimpleNamespace(h=h >> level, w=w >> level, row0=row0 >> (2 * level), slot=slot, p=p0 >> level))
        row0 += h * w
    return out


def total_rows(samples, level):
    return sum(h * w for h, w, _s in samples) >> (2 * level)


def batch_image(t, g, C):
    """the [h, w, C] view of sample g's image in a batch tensor [rows, ld]"""
    return t[g.row0:g.row0 + g.h * g.w, :C].reshape(g.h, g.w, C)


def state_image(state, g, C):
    """the [h, w, C] view (writable) of sample g's image in its row of a state tensor [slots, row elements]"""
    return state[g.slot, :g.h * g.w * C].view(g.h, g.w, C)


# ---- pc_gather ----

def halo_patch(img, py, px, p):
    """the plain rule: patch (py, px) of img [H, W, C] with a 1-pixel halo -> [p + 2, p + 2, C].  Halo rows from the vertical neighbours; halo
    columns and all four corners from the horizontal neighbour's pixel of the patch's OWN first / last row; zeros at the image border."""
    H, W, C = img.shape
    y0, x0 = py * p, px * p
    out = img.new_zeros((p + 2, p + 2, C))
    out[1:p + 1, 1:p + 1] = img[y0:y0 + p, x0:x0 + p]
    if y0 > 0:
        out[0, 1:p + 1] = img[y0 - 1, x0:x0 + p]
    if y0 + p < H:
        out[p + 1, 1:p + 1] = img[y0 + p, x0:x0 + p]
    for there, xs, xo in ((x0 > 0, x0 - 1, 0), (x0 + p < W, x0 + p, p + 1)):
        if there:
            col = img[y0:y0 + p, xs]
            out[1:p + 1, xo] = col
            out[0, xo], out[p + 1, xo] = col[0], col[-1]
    return out


def nearest_2x(img):
    return img.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)


def ring_in_front(h11):
    """(halo_lo, halo_hi) = (2, 0) from the (1, 1) result: one row and one column of zeros in front, the last halo row and column dropped"""
    out = torch.zeros_like(h11)
    out[1:, 1:] = h11[:-1, :-1]
    return out


def gather_ref(src, C, geo, patches, p, halo_lo, halo_hi, up):
    """src [rows, ld_src >= C] at the level of `geo`; patches [(b, py, px)]; p: the patch edge the launch takes (AFTER the upsample when up).
    Returns [n, P, P, C], P = p + halo_lo + halo_hi."""
    assert (halo_lo, halo_hi) in ((0, 0), (1, 1), (2, 0))
    out = []
    for b, py, px in patches:
        g = geo[b]
        assert p == g.p << up
        img = batch_image(src, g, C)
        if up:                                   # == the plain rule applied to the nearest-2x image with p doubled
            img = nearest_2x(img)
        h11 = halo_patch(img, py, px, p)
        out.append(h11[1:-1, 1:-1] if halo_lo == 0 else h11 if halo_lo == 1 else ring_in_front(h11))
    return torch.stack(out)


# ---- pure index moves ----

def scatter_ref(state, src, Ps, o0, C, geo, patches, p):
    """compact src [n, Ps, Ps, C]: the p x p pixels from (o0, o0) -> the patch's place in its request's state row.  Returns the new state."""
    out = state.clone()
    s = src.reshape(len(patches), Ps, Ps, C)
    for i, (b, py, px) in enumerate(patches):
        state_image(out, geo[b], C)[py * p:(py + 1) * p, px * p:(px + 1) * p] = s[i, o0:o0 + p, o0:o0 + p]
    return out


def patch_store_ref(state, batch, C, geo, patches, p):
    out = state.clone()
    for b, py, px in patches:
        state_image(out, geo[b], C)[py * p:(py + 1) * p, px * p:(px + 1) * p] = batch_image(batch, geo[b], C)[py * p:(py + 1) * p, px * p:(px + 1) * p]
    return out


def range_copy_ref(batch, state, C, ranges, to_batch):
    """ranges [(row0, rows, slot, srow0)]; returns (new batch, new state)"""
    nb, ns = batch.clone(), state.clone()
    for row0, rows, slot, srow0 in ranges:
        seg = ns[slot, srow0 * C:(srow0 + rows) * C].view(rows, C)
        if to_batch:
            nb[row0:row0 + rows, :C] = seg
        else:
            seg.copy_(batch[row0:row0 + rows, :C])
    return nb, ns


def copy_rows_ref(batch, slotted, slot, scatter):
    """rows between batch [B, n] and slotted [slots, n]; slot[i] < 0: neither side changes for sample i.  Returns (new batch, new slotted)"""
    nb, ns = batch.clone(), slotted.clone()
    for i, s in enumerate(slot):
        if s < 0:
            continue
        if scatter:
            ns[s] = batch[i]
        else:
            nb[i] = slotted[s]
    return nb, ns


def _fma_f32(a, b, c):
    """round_to_f32(a * b + c) with ONE rounding, for a bf16, b fp32, c bf16 given as fp64 tensors.  a * b is exact in fp64 (8 x 24 bits); the sum
    is rounded to 53 bits first, which can only mislead the second rounding when it lands exactly on an fp32 tie: there the exact remainder
    (two-sum) says on which side the true value lies"""
    t = a * b
    x = t + c
    bb = x - t
    err = (t - (x - bb)) + (c - bb)
    tie = (x.view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
    nudged = torch.where(err > 0, torch.nextafter(x, torch.full_like(x, math.inf)), torch.where(err < 0, torch.nextafter(x, torch.full_like(x, -math.inf)), x))
    return torch.where(tie, nudged, x).float()


def image_copy_ref(batch, state, C, geo, to_batch, vec=None, residual=None, gate=0):
    """to_batch = 0: returns the new state (a pure move).  to_batch = 1: returns (a, b, fused cells): two candidate batch tensors -- equal except
    under the gate, where a holds the unfused and b the fused evaluation of state * vec + residual -- and the number of cells where they differ.
    vec fp32 [positions, >= C] is indexed by the sample's POSITION in the table; residual is a batch tensor."""
    if not to_batch:
        out = state.clone()
        for g in geo:
            state_image(out, g, C).copy_(batch_image(batch, g, C))
        return out
    a, b = batch.clone(), batch.clone()
    for i, g in enumerate(geo):
        s = state_image(state, g, C)
        if vec is None and residual is None:
            ya = yb = s
        else:
            x = s.float()
            r = batch_image(residual, g, C).float() if residual is not None else None
            if vec is not None and gate:
                v = vec[i, :C]
                ya = x * v                                                         # one fp32 rounding ...
                if r is not None:
                    yb = _fma_f32(s.double(), v.double(), r.double())              # ... or none before the add
                    ya = ya + r
                else:
                    yb = ya
            else:
                ya = x + vec[i, :C] if vec is not None else x
                if r is not None:
                    ya = ya + r
                yb = ya
            ya, yb = ya.to(torch.bfloat16), yb.to(torch.bfloat16)                  # round to nearest even
        a[g.row0:g.row0 + g.h * g.w, :C] = ya.reshape(-1, C)
        b[g.row0:g.row0 + g.h * g.w, :C] = yb.reshape(-1, C)
    return a, b, int((bits(a) != bits(b)).sum())


# ---- pc_rows_load_stats ----

def rows_load_stats_ref(batch, state, C, geo, residual, eps):
    """Returns (new batch, rows, (stats ref, bound) [n, 2], (fin ref, bound) [n, 2]) with rows = the batch rows the launch owns, in order"""
    out = batch.clone()
    rows = []
    for g in geo:
        y = (state_image(state, g, C).float() + batch_image(residual, g, C).float()).to(torch.bfloat16)
        out[g.row0:g.row0 + g.h * g.w, :C] = y.reshape(-1, C)
        rows += range(g.row0, g.row0 + g.h * g.w)
    rows = torch.tensor(rows)
    x = out[rows, :C]
    st, d_st = norm_ref.row_stats_ref(x)
    mean = st[:, 0] / C
    d_mean = d_st[:, 0] / C + U32 * mean.abs()
    q = st[:, 1] / C
    var = (q - mean * mean).clamp_min(0.0)
    d_var = d_st[:, 1] / C + 2.0 * mean.abs() * d_mean + d_mean ** 2 + 2.0 * U32 * q
    rstd, d_rstd = norm_ref.rstd_interval(var, d_var, eps, rel=norm_ref.RSQRT)
    return out, rows, (st, d_st), (torch.stack([mean, rstd], 1), torch.stack([d_mean, d_rstd], 1))


# ---- squared differences ----

def sq_terms(vectors):
    """k: the squared terms one of the 256 threads adds in fp32 over a partition of `vectors` 16-byte vectors"""
    return 8 * ((vectors + THREADS - 1) // THREADS)


def _sq(a, b):
    d = a.double() - b.double()
    return float((d * d).sum())


def patch_sq_diff_ref(x, state, C, geo, patches, p):
    """partial[patch][pixel row]: (ref, bound) [n, p]; k = 8 ceil(p (C / 8) / 256)"""
    ref = torch.zeros((len(patches), p), dtype=torch.float64)
    for i, (b, py, px) in enumerate(patches):
        xa = batch_image(x, geo[b], C)[py * p:(py + 1) * p, px * p:(px + 1) * p]
        xs = state_image(state, geo[b], C)[py * p:(py + 1) * p, px * p:(px + 1) * p]
        for y in range(p):
            ref[i, y] = _sq(xa[y], xs[y])
    return ref, (sq_terms(p * (C // 8)) + 3) * U32 * ref


def _chunked(a, b):
    """a, b flat bf16 of 8 n elements -> (ref [64], bound): chunk c = vectors [c per, min((c + 1) per, n)), per = ceil(n / 64); k = 8 ceil(per / 256)"""
    n = a.numel() // 8
    per = (n + CHUNKS - 1) // CHUNKS
    ref = torch.zeros(CHUNKS, dtype=torch.float64)
    for c in range(CHUNKS):
        v0, v1 = min(c * per, n), min((c + 1) * per, n)
        ref[c] = _sq(a[8 * v0:8 * v1], b[8 * v0:8 * v1])
    return ref, (sq_terms(per) + 3) * U32 * ref


def range_sq_diff_ref(x, state, C, ranges):
    out = [_chunked(x[row0:row0 + rows, :C].reshape(-1), state[slot, srow0 * C:(srow0 + rows) * C]) for row0, rows, slot, srow0 in ranges]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def sq_diff_partial_ref(a, b, slot=None):
    """a [B, n], b [slots, n]; sample i against row slot[i] (or i)"""
    out = [_chunked(a[i], b[slot[i] if slot is not None else i]) for i in range(a.shape[0])]
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
