"""The reference of the moments-gradient tests (tests/test_hip_moments_grad.py on the GPU, tests/test_moments_grad_host.py without
one): the upstream the moments walk forms, as the float64 array tests/grad_reference.reference takes for G.

For dL/dm[c, 0..2] = G0, G1, G2 the walk uses the float32 coefficients a0 = (float)G0, a1 = (float)(2.0 * G1), a2 = (float)G2 and
u = fmaf(a1, g, fmaf(a2, t, a0)) per voxel in float32. The reference is the same expression in float64, G = a0 + a1 g + a2 t, from
the float32 grid g and the float32 target t; its companion |a0| + |a1| |g| + |a2| |t| takes G's place for the bound, so that
cancellation inside u cannot hide behind a small |G|. What separates the two: the float32 roundings of the two fmaf, each at most
2^-24 of a value below that companion - inside GRAD_REL = 2e-5 of the bound by a factor of about 170.
"""
from __future__ import annotations

import numpy as np


def coefficients(gm):
    """(a0, a1, a2), each (..., C) float64 holding float32 values, from dL/dm (..., C, K), K = 2 | 3 (K = 2: a2 = 0)."""
    gm = np.asarray(gm, np.float64)
    a0 = gm[..., 0].astype(np.float32).astype(np.float64)
    a1 = (2.0 * gm[..., 1]).astype(np.float32).astype(np.float64)
    a2 = gm[..., 2].astype(np.float32).astype(np.float64) if gm.shape[-1] == 3 else np.zeros_like(a0)
    return a0, a1, a2


def upstream(grid32, gm, target32=None):
    """(G, Gabs), both (C, D, D, D) float64, for one molecule: its float32 grid (C, D, D, D), dL/dm (C, K) and the float32 target
    (C, D, D, D) or None (then K = 2)."""
    g = np.asarray(grid32)
    assert g.dtype == np.float32 and g.ndim == 4
    assert np.asarray(gm).shape == (g.shape[0], 2 if target32 is None else 3)
    a0, a1, a2 = (a[:, None, None, None] for a in coefficients(gm))
    g = g.astype(np.float64)
    t = np.zeros_like(g) if target32 is None else np.asarray(target32).astype(np.float64)
    if target32 is not None:
        assert np.asarray(target32).dtype == np.float32 and t.shape == g.shape
    return a0 + a1 * g + a2 * t, np.abs(a0) + np.abs(a1) * np.abs(g) + np.abs(a2) * np.abs(t)
