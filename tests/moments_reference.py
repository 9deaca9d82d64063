"""The reference of the moments tests (tests/test_hip_moments.py on the GPU, tests/test_moments_host.py without one): the exact
float64 moments of a float32 grid, and the bound any float64 summation of their terms keeps.

For a channel's n = D^3 voxels g (float32) and targets t (float32) the terms (double)g, (double)g * (double)g and
(double)g * (double)t are exact float64 numbers (24 + 24 bits fit 53), so the only rounding of a float64 summation is in its adds.
moments_of() returns the correctly rounded EXACT sums: math.fsum over the terms. Tens of millions of terms do not go through
math.fsum one by one: every row is first split, without error, into a few float64 components whose exact sum is the row's (each
component is the plain sum of the terms' bits inside one window of binary places, narrow enough that no add of that sum rounds),
and math.fsum adds the components. bound() is (n - 1) 2^-53 sum|term|, the worst case of any summation order of n exact terms.
"""
from __future__ import annotations

import math

import numpy as np

ROWS_AT_ONCE = 1 << 22  # terms per block of rows


def terms_of(grid32, target32=None):
    """The exact float64 terms of the moments of a float32 grid (..., C, D, D, D): an array (..., C, K, n), K = 2 | 3 (with a
    (C, D, D, D) float32 target), n = D^3."""
    g = np.asarray(grid32)
    assert g.dtype == np.float32 and g.ndim >= 4
    lead, n = g.shape[:-3], int(np.prod(g.shape[-3:]))
    g = g.reshape(lead + (n,)).astype(np.float64)
    out = [g, g * g]
    if target32 is not None:
        t = np.asarray(target32)
        assert t.dtype == np.float32 and t.shape == np.asarray(grid32).shape[-4:]
        out.append(g * t.reshape(t.shape[0], n).astype(np.float64))
    return np.stack(out, axis=-2)


def exact_sums(terms):
    """The correctly rounded exact sums over the last axis of a float64 array, as math.fsum gives them."""
    x = np.array(terms, dtype=np.float64)  # (a copy: peeled in place)
    lead, n = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, n)
    assert np.isfinite(x).all()
    R = x.shape[0]
    out = np.zeros(R)
    if n == 0 or R == 0:
        return out.reshape(lead)
    grow = max(1, math.ceil(math.log2(n)))  # n terms of at most 2^e sum to at most 2^(e + grow)
    for r0 in range(0, R, max(1, ROWS_AT_ONCE // n)):
        blk = x[r0:r0 + max(1, ROWS_AT_ONCE // n)]
        big = np.abs(blk).max(axis=1)
        # k: n max|term| <= 2^k. The terms' bits at or above 2^(k - 52) are hi = (term + 1.5 2^k) - 1.5 2^k: multiples of 2^(k - 52)
        # whose sum stays below 2^(k + 1), so every add of hi.sum() is exact; term - hi is exact and at most 2^(k - 53): the next
        # window starts 53 - grow places lower.
        k = np.where(big > 0, np.frexp(big)[1] + grow, 0).astype(np.int64)
        comps = []
        while blk.any():
            A = np.ldexp(1.5, np.maximum(k, -1000).astype(np.int32))[:, None]
            hi = (blk + A) - A
            comps.append(hi.sum(axis=1))
            blk -= hi
            k = k - 53 + grow
            assert len(comps) < 64
        for i in range(blk.shape[0]):
            out[r0 + i] = math.fsum(c[i] for c in comps)
    return out.reshape(lead)


def bound(terms):
    """(n - 1) 2^-53 sum|term| over the last axis: the worst case of any float64 summation order of n exact terms."""
    t = np.asarray(terms, dtype=np.float64)
    return (t.shape[-1] - 1) * 2.0 ** -53 * np.abs(t).sum(axis=-1)


def moments_and_bound(grid32, target32=None):
    """(moments, bound), both (..., C, K), of a float32 grid (..., C, D, D, D) - molecule by molecule, so that the float64 terms
    of a large batch never exist all at once."""
    g = np.asarray(grid32)
    if g.ndim == 4:
        t = terms_of(g, target32)
        return exact_sums(t), bound(t)
    n = int(np.prod(g.shape[-3:]))
    step = max(1, ROWS_AT_ONCE // (n * g.shape[1]))
    m, b = [], []
    for b0 in range(0, g.shape[0], step):
        t = terms_of(g[b0:b0 + step], target32)
        m.append(exact_sums(t))
        b.append(bound(t))
    K = 2 if target32 is None else 3
    if not m:
        return np.zeros((0, g.shape[1], K)), np.zeros((0, g.shape[1], K))
    return np.concatenate(m), np.concatenate(b)


def moments_of(grid32, target32=None):
    """The float64 moments (..., C, K) of a float32 grid (..., C, D, D, D): [sum g, sum g * g(, sum g * target)] per channel,
    computed exactly (math.fsum over the exact float64 terms)."""
    return moments_and_bound(grid32, target32)[0]
