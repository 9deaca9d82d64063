"""float64 reference of the backward pass (mvx_backward_batch / mvx_backward_radii_batch), for any resolution, sigma,
blockdim, density, radii type, mode (features / types / single) and precision.

The gradient of a voxelized grid splits exactly into atoms: every cull (box and per reference block) is decided per atom,
so grid = sum_n w_n rho_n and every output is a sum over one atom's own voxels. Each atom is evaluated only in the window
of the grid its largest radius can reach. Its density rho_n is the oracles' per-(atom, voxel) rule, restated here on that
window (tests/test_grad_reference.py pins it against both oracles on the full grid):
  precision 32 (oracle/mvx_oracle.c): box cull and per-block cull in fp64 with the radius widened from float32, except the
      box cull of channel-wise features, which is evaluated in float32 around max(radii); dist = float32(sqrt(d2)),
      dr = dist / r32 in float32, member iff dr <= 1; Gaussian value exp(-0.5 (dr / sigma)^2) in float32
  precision 64 (oracle/numpy_port.py, precision=64): the same culls and rule in float64 throughout
d2 = (dx^2 + dy^2) + dz^2 with d = p - axis (cdist's order). The derivative coefficient kfac (d rho / d d2 = kfac / 2 rho)
is the kernel's: precision 32 2 ln2 k32 with k32 = float32(-0.5 log2(e) / ((double)r32 (double)sigma32)^2) (gauss_coeff),
precision 64 2 c with c = -0.5 / (r sigma)^2 (gauss_coeff64). Then
  dL/dw[n,c]   = sum_v G[c,v] rho_nc(v)
  dL/dp[n,a]   = sum_v sum_c G[c,v] w[n,c] kfac_c rho_nc(v) d_a(v)          (then M^T for a rotated call)
  dL/dr        = -sum_v sum_c G[c,v] w[n,c] (kfac_c / r_c) d2(v) rho_nc(v)  (per atom, per channel or per type)
  dL/dcenter   = -sum_n dL/dcoords[n]
Every value comes with a bound on the sum of the absolute values of its terms, which scales the tolerance.
"""
import numpy as np

LN2 = float(np.log(2.0))
LOG2E = 1.4426950408889634


def axis(D, res=0.5):
    return np.arange(D) * res - res * (D - 1) / 2.0


def k32(r, sigma=0.5):
    """gauss_coeff: float32(-0.5 log2(e) / (r32 sigma32)^2), the product taken in double."""
    rs = float(np.float32(r)) * float(np.float32(sigma))
    return float(np.float32(-0.5 * LOG2E / (rs * rs)))


def kfac(r, sigma=0.5, precision=32):
    """d rho / d d2 = kfac / 2 * rho, with the coefficient the kernels use."""
    if precision == 32:
        return 2.0 * LN2 * k32(r, sigma)
    rs = float(r) * float(sigma)
    return 2.0 * (-0.5 / (rs * rs))


class Geometry:
    def __init__(self, D, res=0.5, blockdim=None, sigma=0.5, density="gaussian", precision=32):
        self.D, self.res, self.sigma, self.density, self.precision = D, float(res), float(sigma), density, precision
        self.bd = 8 if blockdim is None else blockdim
        self.nb = -(-D // self.bd)
        self.axis = np.arange(D, dtype=np.float64) * self.res - (self.res * (D - 1)) / 2.0
        self.ub = (self.res * (D - 1)) / 2.0
        self.lb = -1 * self.ub
        self.bounds = [self.axis[b * self.bd] + (self.res / 2.0) for b in range(1, self.nb)]
        self.fp = np.float32 if precision == 32 else np.float64

    def box_keep(self, p, rc, form):
        """form "scalar": p > lb - r and p < ub + r; "atom": p + r > lb and p - r < ub; "chan32": the float32 quirk of
        channel-wise features at precision 32 (python float - np.float32 scalar evaluates in float32)."""
        if form == "scalar":
            return all(p[a] > self.lb - rc and p[a] < self.ub + rc for a in range(3))
        if form == "atom":
            return all(p[a] + rc > self.lb and p[a] - rc < self.ub for a in range(3))
        r32 = np.float32(rc)
        lo, hi = float(np.float32(self.lb) - r32), float(np.float32(self.ub) + r32)
        return all(p[a] > lo and p[a] < hi for a in range(3))

    def block_ok(self, pa, rc):
        """(nb,) bool: the atom is listed for reference block b along one axis (strict compares, fp64)."""
        ok = np.ones(self.nb, bool)
        if self.nb > 1:
            for b in range(self.nb):
                if b >= 1:
                    ok[b] &= pa > self.bounds[b - 1] - rc
                if b <= self.nb - 2:
                    ok[b] &= pa < self.bounds[b] + rc
        return ok


def atom_density(geo, p, radii, rc, form):
    """One atom at p (3,) with K radii (one per atom, or one per channel sharing the cull radius rc).
    Returns None when nothing is admitted, else (window slices, (dx, dy, dz) broadcastable, d2, rho (K, wx, wy, wz))."""
    if not geo.box_keep(p, rc, form):
        return None
    radii = np.asarray(radii, geo.fp).reshape(-1)
    reach = float(radii.max())
    sl, ds, oks = [], [], []
    for a in range(3):
        lo = max(0, int(np.floor((p[a] - reach - geo.axis[0]) / geo.res)) - 1)
        hi = min(geo.D - 1, int(np.ceil((p[a] + reach - geo.axis[0]) / geo.res)) + 1)
        if lo > hi:
            return None
        sl.append(slice(lo, hi + 1))
        ds.append(p[a] - geo.axis[lo:hi + 1])
        oks.append(geo.block_ok(p[a], rc)[np.arange(lo, hi + 1) // geo.bd])
    dx, dy, dz = ds[0][:, None, None], ds[1][None, :, None], ds[2][None, None, :]
    d2 = (dx * dx + dy * dy) + dz * dz
    adm = oks[0][:, None, None] & oks[1][None, :, None] & oks[2][None, None, :]
    dist = np.sqrt(d2).astype(geo.fp)
    rho = np.zeros((radii.shape[0],) + d2.shape)
    for k, r in enumerate(radii):
        dr = dist / r
        m = adm & (dr <= 1.0)
        if geo.density == "binary":
            rho[k][m] = 1.0
        else:
            val = np.exp(-0.5 * ((dr[m] / geo.fp(geo.sigma)) ** 2))
            rho[k][m] = val.astype(np.float64)
    return tuple(sl), (dx, dy, dz), d2, rho


def reference(xyz, G, radii, radii_type="scalar", *, w=None, mode="features", types=None, res=0.5, sigma=0.5, blockdim=None,
              density="gaussian", precision=32, atoms=None, rot=None, radii_by_type=False):
    """Gradients of L = <G, grid> for one molecule.

    xyz: (N, 3) float64 positions as the kernel sees them (after centring and transform). G: (C, D, D, D) float64 (the
    upstream as the kernel reads it: a bfloat16 upstream widened). radii: python float | (N,) | (C,) (channel-wise) in
    the call's values. mode "features" with w (N, C); "types" with types (N,); "single". rot: the call's rotation M
    (dL/dcoords = M^T dL/dp) or None. atoms: indices to evaluate (default all); the sums over atoms (channel-wise radii,
    radii by type, centre) need all of them. radii_by_type: types mode with channel-wise radii: dL/dr per type.

    Returns a dict of (value, bound) pairs: "features" (n, C) (features mode), "coords" (n, 3), "radii" ((n,) one radius
    per atom; (C,) channel-wise features; (len(radii),) radii by type), "center" (3,), rows in the order of `atoms`.
    """
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    N, C_, D = xyz.shape[0], G.shape[0], G.shape[-1]
    geo = Geometry(D, res, blockdim, sigma, density, precision)
    fp = geo.fp
    chanwise_feat = radii_type == "channel-wise" and mode == "features"
    if mode == "features":
        W = np.asarray(w, np.float64).reshape(N, C_)
    else:
        W = np.zeros((N, C_))
        for n in range(N):
            t = 0 if mode == "single" else int(types[n])
            if t < C_:
                W[n, t] = 1.0
    # per-atom radii (fp values) and the cull radius
    if radii_type == "scalar":
        r_atom, form = np.full(N, fp(radii)), "scalar"
    elif radii_type == "atom-wise":
        r_atom, form = np.asarray(radii).astype(fp), "atom"
    elif chanwise_feat:
        r_chan = np.asarray(radii).astype(fp)
        form = "chan32" if precision == 32 else "scalar"
        rc_chan = float(r_chan.max())
    else:  # channel-wise radii in types mode: the radius of the atom's type (types beyond the radii: padding ones)
        rad = np.asarray(radii).astype(fp)
        padded = np.concatenate([rad, np.ones(max(0, C_ - rad.shape[0]), fp)])
        r_atom = np.array([padded[t] if t < padded.shape[0] else fp(1.0) for t in types], fp)
        form = "atom"
    gauss = density == "gaussian"
    sel = np.arange(N) if atoms is None else np.asarray(atoms, np.int64)
    n_out = sel.shape[0]
    gw, bw = np.zeros((n_out, C_)), np.zeros((n_out, C_))
    gp, bp = np.zeros((n_out, 3)), np.zeros((n_out, 3))
    gr, br = np.zeros(n_out), np.zeros(n_out)  # one radius per atom
    gcr, bcr = (np.zeros(C_), np.zeros(C_))
    for j, n in enumerate(sel):
        if chanwise_feat:
            ev = atom_density(geo, xyz[n], r_chan, rc_chan, form)
            kf = np.array([kfac(r, sigma, precision) for r in r_chan])
        else:
            if mode == "types" and int(types[n]) >= C_:
                continue  # beyond the channels of the call: no box, no gradient
            rc = float(radii) if radii_type == "scalar" else float(r_atom[n])  # (a scalar radius culls unrounded)
            ev = atom_density(geo, xyz[n], r_atom[n:n + 1], rc, form)
            kf = np.full(C_, kfac(r_atom[n], sigma, precision))
        if ev is None:
            continue
        sl, d, d2, rho = ev
        Gw = G[(slice(None),) + sl]
        rc = rho if rho.shape[0] == C_ else np.broadcast_to(rho, (C_,) + rho.shape[1:])
        t = Gw * rc
        gw[j] = t.reshape(C_, -1).sum(1)
        bw[j] = np.abs(t).reshape(C_, -1).sum(1)
        if not gauss:
            continue
        s = (t * (W[n] * kf)[:, None, None, None]).sum(0)  # sum_c G w kfac rho
        for a in range(3):
            gp[j, a] = (s * d[a]).sum()
            bp[j, a] = np.abs(s * d[a]).sum()
        if chanwise_feat:
            u = (t * W[n][:, None, None, None] * d2).reshape(C_, -1)
            gcr += u.sum(1)
            bcr += np.abs(u).sum(1)
        elif radii_type != "scalar":
            e = s * d2 / float(r_atom[n])
            gr[j], br[j] = -e.sum(), np.abs(e).sum()
    out = {"coords": (gp, bp)}
    if rot is not None:  # M^T g for every row; |M^T g - M^T h| <= |M|^T |g - h|
        M = np.asarray(rot, np.float64)
        out["coords"] = (gp @ M, bp @ np.abs(M))
    if mode == "features":
        out["features"] = (gw, bw)
    if radii_type == "atom-wise" or (radii_type == "channel-wise" and not chanwise_feat and not radii_by_type):
        out["radii"] = (gr, br)
    elif chanwise_feat:
        sc = np.array([kfac(r, sigma, precision) / float(r) for r in r_chan])
        out["radii"] = (-sc * gcr, np.abs(sc) * bcr)
    elif radii_by_type:
        nr = np.asarray(radii).shape[0]
        gt, bt = np.zeros(nr), np.zeros(nr)
        for j, n in enumerate(sel):
            t = int(types[n])
            if t < nr:
                gt[t] += gr[j]
                bt[t] += br[j]
        out["radii"] = (gt, bt)
    gc, bc = out["coords"]
    out["center"] = (-gc.sum(0), bc.sum(0))
    return out


def ref_grads(xyz, feats, radii, radii_type, G, D, density, blockdim, wmode="features", types=None, **kw):
    """(dL/dw (N, C), its bound, dL/dp (N, 3), its bound) at resolution / sigma / precision `kw` (default 0.5, 0.5, 32).
    dL/dw is zero outside features mode."""
    assert G.shape[-1] == D
    o = reference(xyz, G, radii, radii_type, w=feats, mode=wmode, types=types, blockdim=blockdim, density=density, **kw)
    gw, bw = o.get("features", (np.zeros((xyz.shape[0], G.shape[0])),) * 2)
    return gw, bw, o["coords"][0], o["coords"][1]


def ref_radii(xyz, w, radii, radii_type, G, D, density, blockdim, types=None, **kw):
    """dL/dradii and its bound for channel weights w (N, C) (features, or one-hot types). radii_type "atom-wise": (N,);
    "channel-wise": (C,) for features, or with `types` the radius of each atom's type (dL/dr summed per type)."""
    assert G.shape[-1] == D
    if radii_type == "channel-wise" and types is not None:
        o = reference(xyz, G, radii, "channel-wise", mode="types", types=types, blockdim=blockdim, density=density,
                      radii_by_type=True, **kw)
    else:
        o = reference(xyz, G, radii, radii_type, w=w, blockdim=blockdim, density=density, **kw)
    g, b = o["radii"]
    return (g if density == "gaussian" else np.zeros_like(g)), b


def atom_grid(xyz, n, radii, radii_type, C_, D, density="gaussian", blockdim=None, res=0.5, sigma=0.5, precision=32):
    """(C', D, D, D) float64 densities of atom n alone on the full grid (C' = C for channel-wise radii, else 1)."""
    geo = Geometry(D, res, blockdim, sigma, density, precision)
    fp = geo.fp
    if radii_type == "channel-wise":
        rr = np.asarray(radii).astype(fp)
        ev = atom_density(geo, xyz[n], rr, float(rr.max()), "chan32" if precision == 32 else "scalar")
        K = C_
    else:
        r = fp(radii) if radii_type == "scalar" else np.asarray(radii).astype(fp)[n]
        rc = float(radii) if radii_type == "scalar" else float(r)
        ev = atom_density(geo, xyz[n], [r], rc, "scalar" if radii_type == "scalar" else "atom")
        K = 1
    out = np.zeros((K, D, D, D))
    if ev is not None:
        out[(slice(None),) + ev[0]] = ev[3]
    return out


def close(got, ref, bound, what, rel=2e-5, abs_=1e-7):
    """|got - ref| <= rel * bound + abs_ elementwise; returns the worst error / bar ratio."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    tol = rel * bound + abs_
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} off, worst {err[bad].max()} at {np.argwhere(bad)[:3].tolist()}"
    return float((err / tol).max()) if err.size else 0.0
