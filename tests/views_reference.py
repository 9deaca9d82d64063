"""numpy restatement of the view selection (mvx_select_views), for the tests of forward_views.

A view keeps the atoms whose position after the view's transform passes the forward's box cull with the call's cull radius:
the scalar radius, radii[n] (atom-wise), radii[types[n]] (radii by type) or max(radii) (channel-wise features). Positions are
float64, p = coords - center (the identity view; the tests that use this module draw no random transform), and the box test
is the C oracle port's own (oracle/numpy_port.py: _box_keep on a GridSpec)."""
import numpy as np

from oracle import numpy_port


def cull_radius(radii, radii_type, types=None, features_mode=False):
    """The radius (python float or float64 (N,)) the box cull of a call uses."""
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
