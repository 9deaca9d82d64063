"""Shapes of tests/test_hip_views_scale.py (GPU) and tests/test_views_host.py (host): the seeded rows whose selection is
compared, entry by entry, with tests/views_reference.py.

view_scan_kernel (mvx_views.hip) is one workgroup of 1 024 threads; thread t owns per = ceil(M / 1024) consecutive counts of the
M = B * ntiles (view, tile) pairs, ntiles = ceil(N / 1024). Every scan row names the M and per it stands for, and the host module
asserts them, together with the one condition under which a rotated row may be compared exactly: no (view, atom) pair lies
within 1e-9 A of a cull bound (the device's quaternion product and numpy's may differ by rounding of order 1e-13 A at these
magnitudes), for every row, so that the GPU test skips no atom.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import views_reference as vr

CUBE = 40.0  # clouds are uniform in a cube of this edge, centred at the origin
VIEW_TILE = 1024  # mvx_views.h
SCAN_THREADS = 1024  # mvx_views.hip
THIN = (1200.0, 4.0, 4.0)  # the long thin box: x is the long edge
MARGIN = 1e-9  # A
TRANSFORM = dict(random_rotation=True, random_translation=1.0)


def cloud(seed, N, mode, C, radii_type, edge=CUBE):
    """(coords, channels, radii) as numpy arrays for one cloud of N atoms."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-edge / 2, edge / 2, (N, 3))
    if mode == "features":
        chan = rng.random((N, C)).astype(np.float32)
    elif mode == "types":
        chan = rng.integers(0, C, N).astype(np.int64)
    else:
        chan = None
    if radii_type == "scalar":
        radii = 1.5
    elif radii_type == "atom-wise":
        radii = rng.uniform(0.8, 2.2, N).astype(np.float32)
    else:
        radii = rng.uniform(0.8, 2.2, C).astype(np.float32)
    return xyz, chan, radii


def centers(seed, B, xyz):
    """View 0 is centred 1 000 A away (no atoms), view 1 on the cloud, the rest on atoms / random points of the cube."""
    rng = np.random.default_rng(seed + 1)
    cen = rng.uniform(-CUBE / 2, CUBE / 2, (B, 3))
    if xyz.shape[0]:
        pick = rng.integers(0, xyz.shape[0], B)
        cen[::2] = xyz[pick[::2]]
    if B >= 2:
        cen[0] = [1000.0, 0.0, 0.0]
        cen[1] = 0.0
    return cen


def thin_cloud(seed, N, order):
    """N atoms uniform in the THIN box; order "sorted": ascending x, so a view's atoms are a few consecutive whole tiles and
    every other tile is empty; "shuffled": every tile holds a few atoms of every view."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, (N, 3)) * np.array(THIN)
    if order == "sorted":
        xyz = xyz[np.argsort(xyz[:, 0], kind="stable")]
    return xyz


def thin_centers():
    """One view beyond the end of the box (no atoms), the rest on its long axis."""
    return np.array([[1000.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-431.3, 0.4, -0.2], [207.9, -0.3, 0.5], [593.0, 0.0, 0.0]])


@dataclass(frozen=True)
class ScanRow:
    id: str
    B: int
    N: int
    M: int  # B * ntiles: the counts view_scan_kernel scans
    per: int  # ceil(M / 1024): counts per thread
    radii: str = "scalar"  # scalar | atom-wise
    shape: str = "cube"  # cube | thin-shuffled | thin-sorted
    rotated: bool = True  # runs with identity views and with TRANSFORM (False: identity views only)
    D: int = 16
    res: float = 1.0


SCAN_ROWS = [
    ScanRow("B1024-N10", 1024, 10, 1024, 1),  # every thread busy; the last count of the whole scan feeds offsets[B]
    ScanRow("B1025-N10", 1025, 10, 1025, 2),  # odd M; half the threads idle
    ScanRow("B1100-N64", 1100, 64, 1100, 2),  # every piece crosses a view boundary
    ScanRow("B1100-N1100", 1100, 1100, 2200, 3, radii="atom-wise"),  # pieces start mid-view at alternating phase
    ScanRow("B345-N3000", 345, 3000, 1035, 2, radii="atom-wise"),  # per and ntiles coprime
    ScanRow("B5-N300000-shuffled", 5, 300_000, 1465, 2, shape="thin-shuffled"),  # tiles in gridDim.x; a view spans ~147 threads
    ScanRow("B5-N300000-sorted", 5, 300_000, 1465, 2, shape="thin-sorted"),  # runs of empty tiles, several whole tiles
    ScanRow("B65600-N40", 65_600, 40, 65_600, 65, rotated=False),  # views beyond 65 535 in gridDim.x
]
SCAN_CASES = [(row, rot) for row in SCAN_ROWS for rot in ((False, True) if row.rotated else (False,))]


def case_id(case):
    return f"{case[0].id}-{'rotated' if case[1] else 'identity'}"


def row_seed(row):
    return 1000 + SCAN_ROWS.index(row)


@functools.lru_cache(maxsize=None)
def row_inputs(row):
    """(coords (N, 3), centers (B, 3), radii: float | float32 (N,)) of a scan row."""
    seed = row_seed(row)
    if row.shape == "cube":
        xyz, _, radii = cloud(seed, row.N, "single", 1, row.radii)
        cen = centers(seed, row.B, xyz)
    else:
        xyz, cen, radii = thin_cloud(seed, row.N, row.shape[5:]), thin_centers(), 1.5
    for a in (xyz, cen):
        a.setflags(write=False)
    return xyz, cen, radii


def row_positions(row, rotated):
    """(B, N, 3): what view_positions gives for the row; the GPU test seeds numpy's RNG with the same row_seed(row)."""
    xyz, cen, _ = row_inputs(row)
    return vr.view_positions(xyz, cen, row_seed(row), **TRANSFORM) if rotated else vr.view_positions(xyz, cen)


@functools.lru_cache(maxsize=None)
def row_reference(row, rotated):
    """(index, offsets, smallest margin of any (view, atom) pair) of a scan row: computed once, shared, read-only."""
    _, _, radii = row_inputs(row)
    p = row_positions(row, rotated)
    index, offsets = vr.select_exact(p, row.res, row.D, row.radii, radii)
    least = float(vr.margin(p, row.res, row.D, row.radii, radii).min())
    for a in (index, offsets):
        a.setflags(write=False)
    return index, offsets, least


# ---- select_views against the reference for every radii source: N = 3000, B = 9 (tests 3e) ---------------------------------
@dataclass(frozen=True)
class SourceRow:
    id: str
    source: str  # views_reference.compares' name
    radii_type: str  # the voxelizer's
    mode: str  # single | types | features
    C: int = 1
    precision: int = 32
    N: int = 3000
    B: int = 9
    D: int = 16
    res: float = 1.0


SOURCE_ROWS = [
    SourceRow("scalar", "scalar", "scalar", "single"),
    SourceRow("atom-wise", "atom-wise", "atom-wise", "single"),
    SourceRow("by-type", "by-type", "channel-wise", "types", C=7),
    SourceRow("channel-features-p32", "channel-features", "channel-wise", "features", C=40),
    SourceRow("channel-features-p64", "channel-features", "channel-wise", "features", C=40, precision=64),
]
SOURCE_CASES = [(row, rot) for row in SOURCE_ROWS for rot in (False, True)]


def source_seed(row):
    return 2000 + SOURCE_ROWS.index(row)


@functools.lru_cache(maxsize=None)
def source_inputs(row):
    """(coords, centers, channels | None, radii) of a source row. Channel-wise feature radii have their largest value at
    channel 37; at precision 64 they are float64 values that float32 cannot hold."""
    seed = source_seed(row)
    xyz, chan, radii = cloud(seed, row.N, row.mode, row.C, row.radii_type)
    if row.source == "channel-features":
        radii = np.random.default_rng(seed + 2).uniform(0.8, 2.0, row.C)
        radii[37] = 2.2 + 1.0 / 3.0
        radii = radii.astype(np.float32 if row.precision == 32 else np.float64)
    return xyz, centers(seed, row.B, xyz), chan, radii


@functools.lru_cache(maxsize=None)
def source_reference(row, rotated):
    xyz, cen, chan, radii = source_inputs(row)
    p = vr.view_positions(xyz, cen, source_seed(row), **TRANSFORM) if rotated else vr.view_positions(xyz, cen)
    kw = dict(types=chan, num_channels=row.C) if row.mode == "types" else {}
    index, offsets = vr.select_exact(p, row.res, row.D, row.source, radii, row.precision, **kw)
    least = float(vr.margin(p, row.res, row.D, row.source, radii, row.precision, **kw).min())
    return index, offsets, least
