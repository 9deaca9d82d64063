"""Shapes of tests/test_hip_f64_sweep.py (GPU) and tests/test_f64_rows_host.py (host): one row per float64 kernel instantiation
(mvx_f64.hip: for_kernel64 / launch_mx64) on geometries dense enough to leave the one-round case of a slab's candidate line.

Every row declares the plan fields (mvx_plan_call, a pure host function) and the line form it stands for; the host module asserts
both without a GPU, so that a later change of the plan or of a geometry cannot silently empty the sweep. The candidate rule of
the pre-pass (mvx_device.h prep_atom, mvx_prep.hip xbin_kernel) is restated here as two bounds on the candidates per slab.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass

import numpy as np

F64_DENSE, F64_MX = 2, 3
RES, SIGMA = 0.5, 0.6
SUBX, SUBY, SUBZ = 2, 4, 8  # a slab is SUBX x SUBY x (SUBZ * nw) voxels (mvx_internal.h)
ONE_ROUND, LINE_CAP, XBIN_LDS = 63, 255, 1024  # primary line; line + extension; x-list entries xbin_kernel keeps in LDS


@dataclass(frozen=True)
class Geom:
    D: int
    atoms: int
    positions: str  # "normal:<std>" | "uniform"
    radius: float
    nw: int  # plan: waves (8-voxel z sub-tiles) per slab, chunks of a row along z, 16-byte stores
    nzc: int
    vec_store: int
    forms: tuple  # line forms the geometry must reach with the row's radii (see line_forms)


# res 0.5, sigma 0.6, positions from default_rng(1). Atom counts are chosen so that the forms hold with margin by the LOWER bound
# (tests/test_f64_rows_host.py): A 994 candidates in its densest slab and 1244 atoms on its longest x-list, B 28 ... 32 slabs between
# 64 and 255, C 1116 and slabs without any, D up to 92 in first chunks with work in the one-sub-tile second chunks, E at most 37.
GEOMS = {
    "A": Geom(24, 1500, "normal:1.2", 1.5, 3, 1, 1, ("xlist_long", "xlist")),
    "B": Geom(24, 600, "normal:2.5", 2.0, 3, 1, 1, ("extension",)),
    "C": Geom(40, 3000, "normal:2.0", 1.5, 5, 1, 1, ("xlist", "empty")),
    "D": Geom(72, 6500, "uniform", 1.5, 8, 2, 1, ("half_empty_chunk", "extension")),
    "E": Geom(33, 400, "uniform", 1.5, 5, 1, 0, ("one_round",)),
}


@dataclass(frozen=True)
class Row:
    id: str
    geom: str
    C: int
    route: int
    ct: int
    ncc: int
    mode: str = "features"  # features | types | single
    radii: str = "scalar"  # scalar | atom-wise | channel-wise
    density: str = "gaussian"
    blockdim: int | None = None
    lane_range: int = 0
    chanwise: bool = False  # the CHANWISE instantiations: channel-wise radii for features
    batch: bool = False  # also a row of test_row_in_a_batch

    @property
    def g(self) -> Geom:
        return GEOMS[self.geom]

    @property
    def nch(self) -> int:
        return 1 if self.mode == "single" else self.C

    @property
    def plan(self) -> dict:
        g = self.g
        return dict(route=self.route, ct=self.ct, ncc=self.ncc, nw=g.nw, nzc=g.nzc, vec_store=g.vec_store, lane_range=self.lane_range)

    @property
    def ncc16(self) -> int:
        """Channel chunks of the same call under debug_option("max_ct64", 16): the vector kernels, 16 channels per chunk."""
        return -(-self.C // 16)


def _r(geom, C, route, ct, ncc, mode="features", radii="scalar", density="gaussian", blockdim=None, lane_range=0, batch=False):
    chanwise = radii == "channel-wise" and mode == "features"
    id = "-".join([geom, {F64_DENSE: "dense", F64_MX: "mx"}[route], f"C{C}", mode, radii, density,
                   "bd" + ("8" if blockdim is None else str(blockdim))])
    return Row(id, geom, C, route, ct, ncc, mode, radii, density, blockdim, lane_range, chanwise, batch)


DN, MX = F64_DENSE, F64_MX
ROWS = [
    # ---- vector kernels, scalar / atom-wise radii, wave-uniform block cull: OpsF64<CT, GAUSS, false, false> --------------------------
    _r("A", 1, DN, 1, 1, batch=True),
    _r("B", 1, DN, 1, 1, mode="single", radii="atom-wise", density="binary"),
    _r("C", 4, DN, 4, 1, mode="types", batch=True),
    _r("A", 4, DN, 4, 1, radii="atom-wise", density="binary", blockdim=24),
    _r("B", 8, DN, 8, 1, batch=True),
    _r("C", 8, DN, 8, 1, radii="atom-wise", density="binary"),
    _r("A", 16, DN, 16, 1),
    _r("B", 16, DN, 16, 1, mode="types", radii="atom-wise", density="binary"),
    # ---- ... per-lane block ranges: OpsF64<CT, GAUSS, false, true> ---------------------------------------------------------------------
    _r("B", 1, DN, 1, 1, mode="single", blockdim=5, lane_range=1),
    _r("A", 1, DN, 1, 1, density="binary", blockdim=12, lane_range=1),
    _r("A", 4, DN, 4, 1, mode="types", radii="atom-wise", blockdim=5, lane_range=1),
    _r("C", 4, DN, 4, 1, density="binary", blockdim=12, lane_range=1),
    _r("C", 8, DN, 8, 1, blockdim=12, lane_range=1),
    _r("B", 8, DN, 8, 1, mode="types", density="binary", blockdim=5, lane_range=1),
    _r("B", 16, DN, 16, 1, radii="atom-wise", blockdim=5, lane_range=1),
    _r("A", 16, DN, 16, 1, density="binary", blockdim=12, lane_range=1),
    # ---- channel-wise radii for features: OpsF64<CT, GAUSS, true, true>, per-channel Tc / kc ---------------------------------------------
    _r("A", 1, DN, 1, 1, radii="channel-wise"),
    _r("B", 1, DN, 1, 1, radii="channel-wise", density="binary", blockdim=5, lane_range=1),
    _r("B", 4, DN, 4, 1, radii="channel-wise", blockdim=12, lane_range=1, batch=True),
    _r("C", 4, DN, 4, 1, radii="channel-wise", density="binary"),
    _r("C", 8, DN, 8, 1, radii="channel-wise", blockdim=5, lane_range=1),
    _r("A", 8, DN, 8, 1, radii="channel-wise", density="binary"),
    _r("A", 16, DN, 16, 1, radii="channel-wise", batch=True),
    _r("B", 16, DN, 16, 1, radii="channel-wise", density="binary", blockdim=12, lane_range=1),
    # (several chunks: the last chunk's channels are clamped at C - 1)
    _r("B", 40, DN, 16, 3, radii="channel-wise"),
    _r("A", 17, DN, 16, 2, radii="channel-wise", density="binary", blockdim=5, lane_range=1),
    # ---- matrix-core kernel: voxelize64_kernel<GAUSS, false> (each again through the vector kernels with ncc 2 ... 4) ---------------------
    _r("A", 32, MX, 32, 1, batch=True),
    _r("B", 17, MX, 32, 1, radii="atom-wise", batch=True),
    _r("C", 33, MX, 32, 2, batch=True),
    _r("A", 40, MX, 32, 2, mode="types"),
    _r("B", 64, MX, 32, 2),
    _r("B", 32, MX, 32, 1, density="binary"),
    _r("A", 33, MX, 32, 2, mode="types", radii="atom-wise", density="binary"),
    _r("B", 40, MX, 32, 2, radii="atom-wise", density="binary", blockdim=24),
    # ---- ... per-lane block ranges: voxelize64_kernel<GAUSS, true> ---------------------------------------------------------------------------
    _r("A", 32, MX, 32, 1, blockdim=5, lane_range=1),
    _r("B", 33, MX, 32, 2, radii="atom-wise", blockdim=12, lane_range=1),
    _r("C", 17, MX, 32, 1, blockdim=5, lane_range=1),
    _r("B", 40, MX, 32, 2, density="binary", blockdim=5, lane_range=1),
    _r("A", 64, MX, 32, 2, radii="atom-wise", density="binary", blockdim=12, lane_range=1),
    _r("C", 32, MX, 32, 1, mode="types", density="binary", blockdim=12, lane_range=1),
    # ---- types with channel-wise radii: a radius per atom, gathered by type (not the CHANWISE instantiations) ----------------------------------
    _r("B", 33, MX, 32, 2, mode="types", radii="channel-wise"),
    _r("A", 8, DN, 8, 1, mode="types", radii="channel-wise", density="binary"),
    # ---- rows cut along z, 8 + 1 sub-tiles: the last chunk's slabs run with seven of eight waves outside the grid --------------------------------
    _r("D", 4, DN, 4, 1, batch=True),
    _r("D", 16, DN, 16, 1, radii="atom-wise", blockdim=12, lane_range=1),
    _r("D", 17, MX, 32, 1, batch=True),
    _r("D", 32, MX, 32, 1, density="binary", blockdim=5, lane_range=1),
    _r("D", 8, DN, 8, 1, radii="channel-wise"),
    # ---- odd D and odd C, written into slice 1 of a batch grid: no 16-byte stores, the grid 8 bytes off 16-byte alignment ------------------------
    _r("E", 1, DN, 1, 1, mode="single", batch=True),
    _r("E", 7, DN, 8, 1, radii="atom-wise", density="binary", blockdim=5, lane_range=1),
    _r("E", 17, MX, 32, 1, batch=True),
    _r("E", 33, MX, 32, 2, radii="atom-wise", blockdim=12, lane_range=1),
    _r("E", 7, DN, 8, 1, radii="channel-wise"),
]
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)
BATCH_ROWS = [r for r in ROWS if r.batch]
BATCH_IDS = [r.id for r in BATCH_ROWS]


# ---- the molecules -------------------------------------------------------------------------------------------------------------------------
def geom_positions(g) -> np.ndarray:
    """The seeded cloud of a geometry (this table's or tests/narrow_rows.py's), read-only."""
    rng = np.random.default_rng(1)
    if g.positions == "uniform":
        W = RES * (g.D - 1)
        xyz = rng.uniform(-W / 2, W / 2, (g.atoms, 3))
    else:
        xyz = rng.normal(0.0, float(g.positions.split(":")[1]), (g.atoms, 3))
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def positions(geom: str) -> np.ndarray:
    return geom_positions(GEOMS[geom])


def make_molecule(row: Row) -> dict:
    """Coordinates, channels and radii of a row, as the voxelizer and the numpy port take them (float64 throughout). Radii other
    than scalar never exceed the geometry's radius and reach it, so the culls see the geometry the counts were made for."""
    g = row.g
    xyz = positions(row.geom)
    n = xyz.shape[0]
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    if row.mode == "features":
        chan = rng.random((n, row.C))
        chan[rng.random((n, row.C)) < 0.3] = 0.0
    elif row.mode == "types":
        chan = rng.integers(0, row.C, n).astype(np.int16)
        chan[0] = row.C - 1
    else:
        chan = None
    if row.radii == "scalar":
        radii = g.radius
    elif row.radii == "atom-wise":
        radii = g.radius * rng.uniform(0.9, 1.0, n)
        radii[n // 2] = g.radius
    else:
        radii = g.radius * rng.uniform(0.8, 1.0, row.C)
        radii[rng.integers(0, row.C)] = g.radius
    return dict(xyz=xyz, chan=chan, radii=radii)


def cull_radii(row: Row, mol: dict) -> np.ndarray:
    """The radius each atom is culled and binned with (mvx_box_cull.inc): its own, its type's, or the largest channel radius."""
    n = mol["xyz"].shape[0]
    if row.radii == "scalar":
        return np.full(n, float(mol["radii"]))
    if row.radii == "atom-wise":
        return np.asarray(mol["radii"], np.float64)
    if row.mode == "types":
        return np.asarray(mol["radii"], np.float64)[mol["chan"]]
    return np.full(n, float(np.max(mol["radii"])))


# ---- candidates per slab: two bounds -----------------------------------------------------------------------------------------------------------
def _block_interval(p, r, D, bd):
    """Voxel indices [vlo, vhi] of the reference blocks that admit an atom along one axis (mvx_device.h block_interval): block b
    admits iff (b == 0 or p > bounds[b - 1] - r) and (b == nb - 1 or p < bounds[b] + r), bounds[m] = axis[(m + 1) * bd] + res / 2."""
    nb = math.ceil(D / bd)
    if nb == 1:
        return np.zeros(p.shape, np.int64), np.full(p.shape, D - 1, np.int64)
    half = RES * (D - 1) / 2.0
    bounds = np.array([((m + 1) * bd * RES - half) + RES / 2.0 for m in range(nb - 1)])
    bhi = (p[:, None] > bounds[None, :] - r[:, None]).sum(axis=1)
    blo = (~(p[:, None] < bounds[None, :] + r[:, None])).sum(axis=1)
    return blo * bd, np.minimum((bhi + 1) * bd - 1, D - 1)


def slab_counts(xyz, r, D, nw, blockdim=None):
    """(lower, upper, xlower): candidates per slab [sx, sy, zc] of SUBX x SUBY x (SUBZ * nw) voxels bounded from both sides, and
    a lower bound on the atoms per (molecule, x-slab) list.

    upper: the pre-pass's own rule - the atom's axis-aligned box as a voxel index window (radius widened by 1e-6, as prep_atom
    does), cut to the admitted reference blocks, overlapping the slab on every axis. It can only over-count: the device clamps
    and compares the same integers.
    lower: the exact distance from the atom to the box of the slab's voxel centres that its admitted blocks leave, against a radius
    shrunk by 1e-9. A sphere that reaches that box reaches, on every axis, a stretch between two voxel centres of the slab that is
    at least one voxel long or ends on a centre (r >= res / 2), so its index window holds a voxel of the slab: a candidate."""
    bd = 8 if blockdim is None else blockdim
    half = RES * (D - 1) / 2.0
    steps = (SUBX, SUBY, SUBZ * nw)
    n = xyz.shape[0]
    assert (r >= RES / 2).all()
    rr = r * 1.000001 + 1e-9
    up_axes, dist_axes = [], []
    for a in range(3):
        p = xyz[:, a]
        lo = np.maximum(np.ceil((p - rr + half) / RES), 0).astype(np.int64)
        hi = np.minimum(np.floor((p + rr + half) / RES), D - 1).astype(np.int64)
        vlo, vhi = _block_interval(p, r, D, bd)
        lo, hi = np.maximum(lo, vlo), np.minimum(hi, vhi)
        ns = -(-D // steps[a])
        s_lo = np.arange(ns) * steps[a]
        s_hi = s_lo + steps[a] - 1
        up_axes.append((lo[:, None] <= s_hi[None, :]) & (hi[:, None] >= s_lo[None, :]) & (lo <= hi)[:, None])
        # the slab's stretch of voxel centres this atom's admitted blocks leave
        b_lo = np.maximum(s_lo[None, :], vlo[:, None])
        b_hi = np.minimum(np.minimum(s_hi, D - 1)[None, :], vhi[:, None])
        c_lo, c_hi = b_lo * RES - half, b_hi * RES - half
        d = np.maximum(np.maximum(c_lo - p[:, None], p[:, None] - c_hi), 0.0)
        d[b_lo > b_hi] = np.inf
        dist_axes.append(d)
    keep = up_axes[0].any(axis=1) & up_axes[1].any(axis=1) & up_axes[2].any(axis=1)
    upper = np.einsum("ai,aj,ak->ijk", *(u.astype(np.int64) for u in up_axes))
    d2 = dist_axes[0][:, :, None, None] ** 2 + dist_axes[1][:, None, :, None] ** 2 + dist_axes[2][:, None, None, :] ** 2
    rs = (r * (1.0 - 1e-9)) ** 2
    hit = d2 <= rs[:, None, None, None]
    lower = hit.sum(axis=0)
    xlower = hit.any(axis=(2, 3)).sum(axis=0)  # atoms that are candidates of some slab of the x-slab are on its list
    assert keep.sum() >= xlower.max() and lower.shape == upper.shape and (lower <= upper).all()
    return lower, upper, xlower


def line_forms(lower, upper, xlower, nw, D) -> set:
    """The line forms a molecule reaches for certain, from the two bounds."""
    forms = set()
    if (upper <= ONE_ROUND).all():
        forms.add("one_round")
    if ((lower > ONE_ROUND) & (upper <= LINE_CAP)).any():
        forms.add("extension")
    if (lower > LINE_CAP).any():
        forms.add("xlist")
    if (xlower > XBIN_LDS).any():
        forms.add("xlist_long")
    if (upper == 0).any():
        forms.add("empty")
    nsz = -(-D // SUBZ)
    if upper.shape[2] == 2 and nsz - nw == 1 and (lower[:, :, 1] > 0).any() and (lower[:, :, 0] > 0).any():
        forms.add("half_empty_chunk")  # rows of 8 + 1 sub-tiles: a second z chunk of one sub-tile, with work in both
    return forms


@functools.lru_cache(maxsize=None)
def row_forms(row: Row):
    mol = make_molecule(row)
    g = row.g
    lower, upper, xlower = slab_counts(mol["xyz"], cull_radii(row, mol), g.D, g.nw, row.blockdim)
    return line_forms(lower, upper, xlower, g.nw, g.D), lower, upper, xlower


# ---- the batch of test_row_in_a_batch: [small, row, empty, small] with per-molecule centres ------------------------------------------------------
def make_batch(row: Row) -> dict:
    mol = make_molecule(row)
    g = row.g
    rng = np.random.default_rng(zlib.crc32(("batch-" + row.id).encode()))
    W = RES * (g.D - 1)
    sizes = [37, mol["xyz"].shape[0], 0, 5]
    centers = rng.uniform(-1.0, 1.0, (4, 3))
    mols = []
    for b, n in enumerate(sizes):
        if b == 1:
            m = dict(mol)
        else:
            xyz = rng.uniform(-W / 2 - 1, W / 2 + 1, (n, 3))
            if row.mode == "features":
                chan = rng.random((n, row.C))
            elif row.mode == "types":
                chan = rng.integers(0, row.C, n).astype(np.int16)
                chan[:1] = row.C - 1  # (a one-molecule call takes its channel count from the largest type)
            else:
                chan = None
            radii = {"scalar": mol["radii"], "atom-wise": g.radius * rng.uniform(0.9, 1.0, n), "channel-wise": mol["radii"]}[row.radii]
            m = dict(xyz=xyz, chan=chan, radii=radii)
        m["xyz"] = m["xyz"] + centers[b]
        m["moved"] = m["xyz"] - centers[b]  # what the reference sees: coordinates after centring, as the pre-pass rounds them
        mols.append(m)
    return dict(sizes=sizes, centers=centers, mols=mols, offsets=np.cumsum([0] + sizes).astype(np.int64))
