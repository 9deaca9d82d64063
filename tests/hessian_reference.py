"""float64 reference of mvx_score_hessian_batch: per atom the score s_n, the gradient g_n = dS/dp_n and the Hessian H_n of the
score against a constant field, in the grid frame, and the twist gradient and Hessian of a molecule about a pivot.

Built on tests/grad_reference.py's Geometry, atom_density and kfac: the same membership and the same radii and coefficient
rounding per precision. With d = p_n - voxel centre, rho the density, u(v) = sum_c F[c,v] w[n,c] and e = u rho kfac over the
admitted voxels of atom n (the admitted set is held fixed: the truncation at the radius is not differentiated):
  s_n = sum_v u rho        g_n = sum_v e d        H_n = sum_v e (I + kfac d d^T), stored as (xx, xy, xz, yy, yz, zz)
Every value comes with a bound, the same sum over the absolute values of its terms: sum_v |e| (delta_ij + |kfac| |d_i d_j|) for
H. Binary density: g = 0 and H = 0, but it scores. Channel-wise radii with features are not part of the entry.
"""
import numpy as np

from tests.grad_reference import Geometry, atom_density, kfac

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the order of a stored H row


def reference(xyz, F, radii, radii_type="scalar", *, w=None, mode="features", types=None, res=0.5, sigma=0.5, blockdim=None,
              density="gaussian", precision=32, atoms=None):
    """xyz: (N, 3) float64 positions in the grid frame (after centring and transform). F: (C, D, D, D) float64, the field as the
    kernel reads it. radii: python float | (N,) atom-wise | (C,) by type (types mode, channel-wise). mode "features" with w
    (N, C); "types" with types (N,); "single". atoms: indices to evaluate (default all).
    Returns {"s": (value (n,), bound), "g": ((n, 3), bound), "H": ((n, 6), bound)}, rows in the order of `atoms`."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    N, C_, D = xyz.shape[0], F.shape[0], F.shape[-1]
    geo = Geometry(D, res, blockdim, sigma, density, precision)
    fp = geo.fp
    assert not (radii_type == "channel-wise" and mode == "features"), "channel-wise radii with features: not part of the entry"
    if mode == "features":
        W = np.asarray(w, np.float64).reshape(N, C_)
    else:
        W = np.zeros((N, C_))
        for n in range(N):
            t = 0 if mode == "single" else int(types[n])
            if t < C_:
                W[n, t] = 1.0
    if radii_type == "scalar":
        r_atom, form = np.full(N, fp(radii)), "scalar"
    elif radii_type == "atom-wise":
        r_atom, form = np.asarray(radii).astype(fp), "atom"
    else:  # the radius of the atom's type (types beyond the radii: padding ones), as tests/grad_reference.py reads them
        rad = np.asarray(radii).astype(fp)
        padded = np.concatenate([rad, np.ones(max(0, C_ - rad.shape[0]), fp)])
        r_atom = np.array([padded[t] if t < padded.shape[0] else fp(1.0) for t in types], fp)
        form = "atom"
    sel = np.arange(N) if atoms is None else np.asarray(atoms, np.int64)
    n_out = sel.shape[0]
    s, bs = np.zeros(n_out), np.zeros(n_out)
    g, bg = np.zeros((n_out, 3)), np.zeros((n_out, 3))
    H, bH = np.zeros((n_out, 6)), np.zeros((n_out, 6))
    for j, n in enumerate(sel):
        if mode == "types" and int(types[n]) >= C_:
            continue  # beyond the channels of the call: no box
        rc = float(radii) if radii_type == "scalar" else float(r_atom[n])  # (a scalar radius culls unrounded)
        ev = atom_density(geo, xyz[n], r_atom[n:n + 1], rc, form)
        if ev is None:
            continue
        sl, d, d2, rho = ev
        u = (F[(slice(None),) + sl] * W[n][:, None, None, None]).sum(0) * rho[0]  # u rho per voxel of the window
        s[j], bs[j] = u.sum(), np.abs(u).sum()
        if density != "gaussian":
            continue
        kf = kfac(r_atom[n], sigma, precision)
        e = u * kf
        for a in range(3):
            g[j, a], bg[j, a] = (e * d[a]).sum(), np.abs(e * d[a]).sum()
        for k, (a, b) in enumerate(PAIRS):
            t = e * ((1.0 if a == b else 0.0) + kf * d[a] * d[b])
            ta = np.abs(e) * ((1.0 if a == b else 0.0) + abs(kf) * np.abs(d[a] * d[b]))
            H[j, k], bH[j, k] = t.sum(), ta.sum()
    return {"s": (s, bs), "g": (g, bg), "H": (H, bH)}


def full(Hrow):
    """(..., 6) stored rows -> (..., 3, 3) symmetric matrices."""
    Hrow = np.asarray(Hrow)
    out = np.zeros(Hrow.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(PAIRS):
        out[..., a, b] = out[..., b, a] = Hrow[..., k]
    return out


def cross_matrix(r):
    """[r]x: cross_matrix(r) @ v = r x v."""
    return np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])


def twist(p, g, H, pivot, bg=None, bH=None):
    """Gradient (6,) and Hessian (6, 6) of S = sum_n s_n(p_n) at xi = 0 under p' = exp([omega]x) (p - pivot) + pivot + tau,
    xi = (tau, omega), from the atoms' positions p (N, 3), gradients g (N, 3) and Hessians H (N, 6 | N, 3, 3):
      G = sum_n J_n^T g_n,  Hxi = sum_n J_n^T H_n J_n + [omega-omega] sum_n 0.5 (g_n r_n^T + r_n g_n^T) - (g_n . r_n) I,
    J_n = [I | -[r_n]x], r_n = p_n - pivot. Atoms whose g and H rows are all zero are skipped (their p may be NaN).
    Returns (G, bound of G, Hxi, bound of Hxi); the bounds use the same formulas on |g|, |r| and the bound of H (bg, bH: default
    |g| and |H|)."""
    p, g = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(g, np.float64).reshape(-1, 3)
    H = np.asarray(H, np.float64)
    H = full(H) if H.shape[-1] == 6 else H
    bg = np.abs(g) if bg is None else np.asarray(bg, np.float64).reshape(-1, 3)
    bH = np.abs(H) if bH is None else (full(bH) if np.asarray(bH).shape[-1] == 6 else np.asarray(bH, np.float64))
    G, bG, X, bX = np.zeros(6), np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    for n in range(p.shape[0]):
        if not g[n].any() and not H[n].any():
            continue
        r = p[n] - np.asarray(pivot, np.float64)
        J = np.concatenate([np.eye(3), -cross_matrix(r)], axis=1)
        Ja = np.abs(J)
        G += J.T @ g[n]
        bG += Ja.T @ bg[n]
        X += J.T @ H[n] @ J
        bX += Ja.T @ bH[n] @ Ja
        X[3:, 3:] += 0.5 * (np.outer(g[n], r) + np.outer(r, g[n])) - np.dot(g[n], r) * np.eye(3)
        ra = np.abs(r)
        bX[3:, 3:] += 0.5 * (np.outer(bg[n], ra) + np.outer(ra, bg[n])) + np.dot(bg[n], ra) * np.eye(3)
    return G, bG, X, bX


def exp_so3(w):
    """exp([w]x) by Rodrigues' formula."""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = cross_matrix(w)
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * K @ K
