"""float64 reference of the scores against a field grid (mvx_score_batch), built on tests/grad_reference.py.

The score S = <F, grid> of one molecule is linear in the grid and the grid splits exactly into atoms (every cull is decided per
atom), so S = sum_n s_n with
  s_n = sum_c w[n,c] sum_v F[c,v] rho_nc(v)
and sum_v F[c,v] rho_nc(v) is what grad_reference.reference returns as the feature gradient for G = F, with the sum of the
absolute values of its terms. Contracted with w it gives s_n and its bound sum_c |w[n,c]| sum_v |F[c,v]| rho_nc(v); the molecule
score is the sum of the s_n and its bound the sum of their bounds. Types and single mode are features mode with one-hot rows
(a type beyond the channels: a zero row); channel-wise radii in types mode are the radius of each atom's type, culled as a
radius per atom (as grad_reference does).
"""
import numpy as np

from tests import grad_reference as gr


def weights(N, C_, mode, w=None, types=None):
    """(N, C) float64 channel weights: the feature rows, onehot(type) (zero for a type >= C), or ones on channel 0."""
    if mode == "features":
        return np.asarray(w, np.float64).reshape(N, C_)
    W = np.zeros((N, C_))
    for n in range(N):
        t = 0 if mode == "single" else int(types[n])
        if t < C_:
            W[n, t] = 1.0
    return W


def score_reference(xyz, F, radii, radii_type="scalar", *, w=None, mode="features", types=None, precision=32, **kw):
    """Scores of one molecule against F (C, D, D, D) float64 (the field as the kernel reads it: bfloat16 widened).

    xyz: (N, 3) positions as the kernel sees them; radii: python float | (N,) | (C,) in the call's values; kw: res, sigma,
    blockdim, density as for grad_reference.reference. Returns (s (N,), its bound (N,), S, its bound)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    N, C_ = xyz.shape[0], F.shape[0]
    W = weights(N, C_, mode, w, types)
    if mode != "features" and radii_type == "channel-wise":
        fp = np.float32 if precision == 32 else np.float64
        rad = np.asarray(radii).astype(fp)
        radii = np.array([rad[t] if t < rad.shape[0] else fp(1.0) for t in types], fp)
        radii_type = "atom-wise"
    if N == 0:
        return np.zeros(0), np.zeros(0), 0.0, 0.0
    gw, bw = gr.reference(xyz, F, radii, radii_type, w=W, mode="features", precision=precision, **kw)["features"]
    s = (W * gw).sum(1)
    b = (np.abs(W) * bw).sum(1)
    return s, b, float(s.sum()), float(b.sum())


def batch_reference(xyz, off, F, radii, radii_type="scalar", *, w=None, mode="features", types=None, **kw):
    """score_reference molecule by molecule. F: (C, D, D, D) shared or (B, C, D, D, D). Returns (s (N,), bound (N,), S (B,),
    bound (B,))."""
    B, N = len(off) - 1, int(off[-1])
    s, b, S, Sb = np.zeros(N), np.zeros(N), np.zeros(B), np.zeros(B)
    for m in range(B):
        lo, hi = int(off[m]), int(off[m + 1])
        r = radii[lo:hi] if radii_type == "atom-wise" else radii
        s[lo:hi], b[lo:hi], S[m], Sb[m] = score_reference(
            xyz[lo:hi], F if F.ndim == 4 else F[m], r, radii_type, w=None if w is None else w[lo:hi], mode=mode,
            types=None if types is None else types[lo:hi], **kw)
    return s, b, S, Sb
