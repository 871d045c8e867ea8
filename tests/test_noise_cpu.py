"""Host-side checks of the seeded noise (csrc/noise.h, noise.hip): the numpy restatement (tests/noise_ref.py) against Random123's known answers and
as a distribution, and the entry's declaration, binding and refusals.  No GPU: the library loads without a device."""
import math
import os
import re

import numpy as np

import noise_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 4096                    # any aligned non-null address: nothing is dereferenced before a refusal


def test_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter and key all zero, counter and key all ones"""
    zero = N.philox(np.zeros(4, dtype=np.uint32), (0, 0))
    ones = N.philox(np.full(4, 0xFFFFFFFF, dtype=np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))
    assert [int(w) for w in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised over groups: the same function of each counter, and the counter's high word of q, its step and its domain all matter
    many = N.philox(np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.uint32), (0, 0))
    assert np.array_equal(many[0], zero) and len({tuple(r) for r in many.tolist()}) == 6


def test_layout_of_a_row():
    """element idx takes word idx & 3 of group idx >> 2; a row of 27 elements leaves its last group partly used; seed halves are the key"""
    w = N.words(0x0123456789ABCDEF, 7, N.STEP, 27)
    g = N.group_words(0x0123456789ABCDEF, 7, N.STEP, 7)
    assert w.shape == (27,) and np.array_equal(w, g.reshape(-1)[:27])
    for q in (0, 3, 6):
        assert np.array_equal(g[q], N.philox(np.array([q, 0, 7, N.STEP], dtype=np.uint32), (0x89ABCDEF, 0x01234567)))
    assert np.array_equal(N.normals(5, 1, N.INIT, 27), N.normals(5, 1, N.INIT, 64)[:27])          # a prefix does not depend on the length
    assert not np.array_equal(N.words(5, 1, N.INIT, 8), N.words(5, 1, N.START, 8))
    assert not np.array_equal(N.words(5, 1, N.INIT, 8), N.words(5 + 2 ** 32, 1, N.INIT, 8))       # the seed's high half


def test_distribution():
    """2^20 reference normals at seed 1 (domain 2, step 0).  With b = 5 / sqrt(2^20): |mean| < b, |var - 1| < sqrt(2) b and |corr| < b between
    neighbouring elements, between steps k and k + 1 of one element and between seeds s and s + 1 -- five-sigma bounds of the sample statistics of
    independent N(0, 1) values.  They are conditions on the reference: seed 1 was checked to meet them (it does by a factor of more than 2; so did
    seeds 2 .. 5), and the device is held to the reference value by value (tests/test_noise_gpu.py)."""
    n, seed = 2 ** 20, 1
    b = 5.0 / math.sqrt(n)
    z = N.normals(seed, 0, N.STEP, n)
    assert z.dtype == np.float64 and np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(-2.0 * math.log(2.0 ** -24)) + 1e-12

    def corr(a, c):
        return float(np.corrcoef(a, c)[0, 1])
    figures = {"mean": abs(float(z.mean())) / b, "var": abs(float(z.var()) - 1.0) / (math.sqrt(2.0) * b), "neighbours": abs(corr(z[:-1], z[1:])) / b,
               "steps": abs(corr(z, N.normals(seed, 1, N.STEP, n))) / b, "seeds": abs(corr(z, N.normals(seed + 1, 0, N.STEP, n))) / b}
    print({k: f"{v:.3f} of the bound" for k, v in figures.items()})
    assert all(v < 1.0 for v in figures.values()), figures
    # and inside a group: the cos / sin pair of one radius, and the two pairs
    g = z.reshape(-1, 4)
    for i, j in ((0, 1), (0, 2), (1, 3), (2, 3)):
        assert abs(corr(g[:, i], g[:, j])) < 2.0 * b, (i, j)                  # 2^18 pairs: the same five sigma


def test_entry_is_declared_exported_and_bound():
    from sduss_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "mxdenoise.h")).read()
    declared = set(re.findall(r"\b(mx_[a-z0-9_]+)\s*\(", hdr))
    assert "mx_noise_fill" in declared and "mx_noise_fill" in lib.SYMBOLS and hasattr(l, "mx_noise_fill")
    assert l.mx_noise_fill.argtypes == lib.SYMBOLS["mx_noise_fill"][1]
    assert "enum { MX_NOISE_INIT = 0, MX_NOISE_START = 1, MX_NOISE_STEP = 2, MX_NOISE_POSTERIOR = 3 };" in hdr
    assert (lib.MX_NOISE_INIT, lib.MX_NOISE_START, lib.MX_NOISE_STEP, lib.MX_NOISE_POSTERIOR) == (N.INIT, N.START, N.STEP, N.POSTERIOR) == (0, 1, 2, 3)


def test_noise_fill_refuses_without_a_launch():
    from sduss_amd import lib
    l = lib.load()
    fn = l.mx_noise_fill
    cases = [((None, 0, 2, 16, OK, OK, 2, None, 0), b"null"), ((OK, 0, 2, 16, None, OK, 2, None, 0), b"null"), ((OK, 0, 2, 16, OK, None, 2, None, 0), b"null"),
             ((OK, 0, 0, 16, OK, OK, 2, None, 0), b"positive"), ((OK, 0, 2, 0, OK, OK, 2, None, 0), b"positive"), ((OK, 0, -1, 16, OK, OK, 2, None, 1), b"positive"),
             ((OK, 3, 2, 16, OK, OK, 2, None, 0), b"bad dtype"), ((OK, -1, 2, 16, OK, OK, 2, OK, 0), b"bad dtype"),
             ((OK, 0, 2, 16, OK, OK, -1, None, 0), b"domain"), ((OK, 0, 2, 16, OK, OK, 2, None, 2), b"raw")]
    for args, msg in cases:
        assert fn(None, *args) != 0 and msg in l.mx_last_error(), (args, l.mx_last_error())
