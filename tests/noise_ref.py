"""Numpy restatement of the noise function of a seeded request (csrc/noise.h) for tests/test_noise_cpu.py, test_noise_gpu.py and
test_stochastic_step_gpu.py: Philox4x32-10 with the Random123 constants, key = (seed low, seed high), counter = (q low, q high, step, domain) with
q = idx >> 2 and idx the element's index in the request's own tensor; element idx takes word / normal idx & 3 of its group.  The integer half is
exact (the device must return the same words); the normals are Box-Muller in fp64 on the same words, which the device's fp32 chain is held to."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
INIT, START, STEP, POSTERIOR = 0, 1, 2, 3
MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key) -> np.ndarray:
    """Philox4x32-10: counter uint32 [..., 4], key (k0, k1) -> the output words uint32 [..., 4]"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def group_words(seed: int, step: int, domain: int, n_groups: int) -> np.ndarray:
    """the words uint32 [n_groups, 4] of groups 0 .. n_groups - 1 of (seed, step, domain)"""
    q = np.arange(n_groups, dtype=np.uint64)
    ctr = np.stack([q & MASK, q >> np.uint64(32), np.full_like(q, step & 0xFFFFFFFF), np.full_like(q, domain & 0xFFFFFFFF)], axis=-1)
    seed = int(seed) & (2 ** 64 - 1)
    return philox(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def words(seed: int, step: int, domain: int, elems: int) -> np.ndarray:
    """uint32 [elems]: what mx_noise_fill(raw = 1) leaves in a row (a last group is partly used when elems is no multiple of 4)"""
    return group_words(seed, step, domain, (elems + 3) // 4).reshape(-1)[:elems]


def normals_of(w: np.ndarray) -> np.ndarray:
    """fp64 normals of whole groups of words uint32 [..., 4]: (w0, w1) -> (z0, z1), (w2, w3) -> (z2, z3)"""
    w = w.astype(np.uint64)
    out = np.empty(w.shape, dtype=np.float64)
    for a in (0, 2):
        u = (2.0 * (w[..., a] >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
        t2 = (2.0 * (w[..., a + 1] >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -23
        r = np.sqrt(-2.0 * np.log(u))
        out[..., a], out[..., a + 1] = r * np.cos(np.pi * t2), r * np.sin(np.pi * t2)
    return out


def normals(seed: int, step: int, domain: int, elems: int) -> np.ndarray:
    """fp64 [elems]: the N(0, 1) values of a request's tensor of ``elems`` elements"""
    return normals_of(group_words(seed, step, domain, (elems + 3) // 4)).reshape(-1)[:elems]
