"""numpy restatement of the view selection (mvx_select_views), for the tests of forward_views.

A view keeps the atoms whose position after the view's transform passes the forward's box cull with the call's cull radius:
the scalar radius, radii[n] (atom-wise), radii[types[n]] (radii by type) or max(radii) (channel-wise features). Positions are
float64. The first functions below (cull_radius ... face_cloud) restate identity views, p = coords - center, with the C
oracle port's own box test (oracle/numpy_port.py: _box_keep on a GridSpec) and the float64 bound. The second part of the
module is the complete restatement: views under a seeded random transform (view_positions), the bound of every radii source
exactly as mvx_box_cull.inc evaluates it (compares / keep_mask / margin), the (index, offsets) pair mvx_select_views must
return (select_exact), and the comparison the GPU tests make (selection_mismatch)."""
import numpy as np

from molvoxel_amd.voxelizer.hip.transform import do_transform, draw_forward_transform
from oracle import numpy_port


def cull_radius(radii, radii_type, types=None, features_mode=False):
    """The radius (python float or float64 (N,)) the box cull of a call uses. For channel-wise features this is the radius
    only: at precision 32 the library evaluates that source's bound in float32 ((float)lb - rmax, NEP 50), so
    `select(..., cull_radius(...))`, which widens the box in float64, is NOT that mode's selection - keep_mask is."""
    if radii_type == "scalar":
        return float(radii)
    r = np.asarray(radii, np.float32)
    if radii_type == "atom-wise":
        return r.astype(np.float64)
    if features_mode:
        return float(r.max())
    return r[np.asarray(types)].astype(np.float64)


def positions(coords, center):
    return np.asarray(coords, np.float64) - np.asarray(center, np.float64).reshape(1, 3)


def select(coords, centers, size, resolution, dimension):
    """[ascending atom indices kept by view b for b in range(B)]; size: cull_radius()."""
    spec = numpy_port.GridSpec(resolution, dimension)
    return [numpy_port._box_keep(spec, positions(coords, c), size) for c in np.asarray(centers, np.float64).reshape(-1, 3)]


def count_within(coords, centers, size, resolution, dimension, slack):
    """Per view: atoms with max|p - c| < half + r + slack (the loose bound a real cull must stay under)."""
    half = resolution * (dimension - 1) / 2.0
    out = []
    for c in np.asarray(centers, np.float64).reshape(-1, 3):
        d = np.abs(positions(coords, c)).max(axis=1)
        out.append(int((d < half + size + slack).sum()))
    return out


def face_cloud(resolution, dimension, radius, axis=0):
    """Atoms exactly on the cull face of a view centred at the origin, |p| == half + r on one axis, and one ulp either side,
    on both faces; half and r are chosen representable by the caller (e.g. res 0.5, D 16, r 1.5: half + r = 5.25).
    Returns (coords (6, 3), expected keep mask): strict compares keep only the atoms one ulp inside."""
    face = resolution * (dimension - 1) / 2.0 + radius
    vals = [np.nextafter(face, 0.0), face, np.nextafter(face, np.inf)]
    xyz = np.zeros((6, 3))
    xyz[:3, axis] = vals
    xyz[3:, axis] = [-v for v in vals]
    return xyz, np.array([True, False, False, True, False, False])


# ---- the complete restatement -----------------------------------------------------------------------------------------------
def view_positions(coords, centers, seed=None, random_translation=0.0, random_rotation=False):
    """(B, N, 3) float64: the cloud as each view sees it. Identity views (seed None): coords - center. Otherwise the
    transforms are drawn per view, in view order, by draw_forward_transform after np.random.seed(seed) - forward_views'
    own protocol - and applied by the numpy branch of do_transform to coords - center."""
    xyz = np.asarray(coords, np.float64)
    cen = np.asarray(centers, np.float64).reshape(-1, 3)
    p = xyz[None, :, :] - cen[:, None, :]
    if seed is None:
        return p
    np.random.seed(seed)
    for b in range(cen.shape[0]):
        translation, quaternion = draw_forward_transform(random_translation, random_rotation)
        p[b] = do_transform(p[b], None, translation, quaternion)
    return p


def _radius_values(radii, precision):
    """radii as the library reads them: float32 widened (precision 32) or float64 (precision 64)."""
    return np.asarray(radii, np.float32).astype(np.float64) if precision == 32 else np.asarray(radii, np.float64)


def compares(p, resolution, dimension, source, radii, precision=32, types=None, num_channels=None):
    """mvx_box_cull.inc line for line. p: (..., N, 3) positions; source: "scalar" | "atom-wise" | "by-type" |
    "channel-features"; radii: python float | (N,) | (C,) | (C,); types: (N,) as the library sees them (after the int16 cast)
    or None. Returns (valid (N,) bool, low (..., N, 3), lo_bound, high (..., N, 3), hi_bound): an atom passes when it is
    valid and low > lo_bound and high < hi_bound on the three axes; the bounds broadcast against low / high."""
    p = np.asarray(p, np.float64)
    N = p.shape[-2]
    ub = resolution * (dimension - 1) / 2.0
    lb = -1 * ub
    valid = np.ones(N, bool)
    if types is not None:
        t = np.asarray(types, np.int64)
        valid = (t >= 0) & (t < num_channels)  # a type outside [0, C) never passes
    if source == "scalar":
        rc = float(radii)
        return valid, p, lb - rc, p, ub + rc  # p > lb - r and p < ub + r
    if source == "channel-features":
        if precision == 64:
            r64 = float(np.asarray(radii, np.float64).max())
            return valid, p, lb - r64, p, ub + r64
        rmax = np.asarray(radii, np.float32).max()  # np.float32 scalar: the bound is a float32 difference / sum
        return valid, p, float(np.float32(lb) - rmax), p, float(np.float32(ub) + rmax)
    r = _radius_values(radii, precision)
    if source == "by-type":
        r = np.where(valid, r[np.where(valid, t, 0)], 0.0)
    else:
        assert source == "atom-wise", source
    r = r.reshape((1,) * (p.ndim - 2) + (N, 1))
    return valid, p + r, lb, p - r, ub  # p + r > lb and p - r < ub


def keep_mask(p, resolution, dimension, source, radii, precision=32, types=None, num_channels=None):
    """(..., N) bool: the atoms that pass the box cull."""
    valid, low, lo, high, hi = compares(p, resolution, dimension, source, radii, precision, types, num_channels)
    return valid & (low > lo).all(axis=-1) & (high < hi).all(axis=-1)


def margin(p, resolution, dimension, source, radii, precision=32, types=None, num_channels=None):
    """(..., N) float64: the smallest distance between a compared quantity and its bound over the six compares (inf for an
    atom whose type is out of range: no rounding of its position changes the decision)."""
    valid, low, lo, high, hi = compares(p, resolution, dimension, source, radii, precision, types, num_channels)
    m = np.minimum(np.abs(low - lo).min(axis=-1), np.abs(high - hi).min(axis=-1))
    return np.where(valid, m, np.inf)


def select_exact(p, resolution, dimension, source, radii, precision=32, types=None, num_channels=None):
    """(index int64 (total,), offsets int64 (B + 1,)) for positions p (B, N, 3): per view the passing atoms in ascending order."""
    keep = keep_mask(p, resolution, dimension, source, radii, precision, types, num_channels)
    offsets = np.zeros(keep.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=offsets[1:])
    return np.nonzero(keep)[1].astype(np.int64), offsets  # (row-major: view by view, ascending inside a view)


def tile_counts(index, offsets, N, tile=1024):
    """(B, ceil(N / tile)) kept atoms per (view, tile): the counts the scan kernel sees."""
    B, nt = offsets.shape[0] - 1, (N + tile - 1) // tile
    view = np.repeat(np.arange(B), np.diff(offsets))
    return np.bincount(view * nt + index // tile, minlength=B * nt).reshape(B, nt)


def selection_mismatch(index, offsets, ref_index, ref_offsets):
    """None when (index, offsets) is exactly the reference, else one line naming the first difference."""
    index, offsets = np.asarray(index), np.asarray(offsets)
    if offsets.dtype != np.int64 or index.dtype != np.int64:
        return f"dtypes {index.dtype} / {offsets.dtype}, expected int64"
    if offsets.shape != ref_offsets.shape:
        return f"offsets shape {offsets.shape} vs {ref_offsets.shape}"
    bad = np.flatnonzero(offsets != ref_offsets)
    if bad.size:
        b = int(bad[0])
        return f"offsets[{b}] = {int(offsets[b])}, expected {int(ref_offsets[b])} ({bad.size} of {offsets.size} differ)"
    if index.shape != ref_index.shape:
        return f"index shape {index.shape} vs {ref_index.shape}"
    bad = np.flatnonzero(index != ref_index)
    if bad.size:
        i = int(bad[0])
        b = int(np.searchsorted(ref_offsets, i, side="right") - 1)
        return (f"index[{i}] = {int(index[i])}, expected {int(ref_index[i])}: view {b}, entry {i - int(ref_offsets[b])} "
                f"({bad.size} of {index.size} differ)")
    return None


def edge_cloud(resolution, dimension, source, radius, precision=32, axis=0, reach=4):
    """Atoms around the two cull faces of an identity view at the origin: `reach` consecutive float64 values either side of
    the place where keep_mask flips, on `axis` (other coordinates 0). radius: python float (scalar), the one radius every
    atom has (atom-wise) or the (C,) channel radii (channel-features). Returns (coords (4 * reach, 3), keep mask (4 * reach,))."""

    def radii_for(n):
        return np.full(n, radius) if source == "atom-wise" else radius

    def kept(x):
        q = np.zeros((1, 3))
        q[0, axis] = x
        return bool(keep_mask(q, resolution, dimension, source, radii_for(1), precision)[0])

    _, _, lo, _, hi = compares(np.zeros((1, 3)), resolution, dimension, source, radii_for(1), precision)
    if source == "atom-wise":  # p + r > lb, p - r < ub: the flip lies within a few float64 ulps of lb - r / ub + r
        r = float(_radius_values(radius, precision))
        lo, hi = lo - r, hi + r
    vals = []
    for face, out in ((hi, np.inf), (lo, -np.inf)):
        x = float(face)
        towards = 0.0 if not kept(x) else out
        for _ in range(64):
            nxt = np.nextafter(x, towards)
            if kept(nxt) != kept(x):
                break
            x = nxt
        else:
            raise AssertionError("no flip near the face")
        inner, outer = (nxt, x) if kept(nxt) else (x, nxt)
        for _ in range(reach):
            vals.append(inner)
            inner = np.nextafter(inner, 0.0)
        for _ in range(reach):
            vals.append(outer)
            outer = np.nextafter(outer, out)
    xyz = np.zeros((len(vals), 3))
    xyz[:, axis] = vals
    return xyz, keep_mask(xyz, resolution, dimension, source, radii_for(len(vals)), precision)
