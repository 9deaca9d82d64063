"""The shapes of the summed-grid sweep (tests/test_hip_sum_sweep.py on the GPU, tests/test_sum_sweep_host.py without one): the
branches of mvx_sum_body.inc that the eight rows of tests/sum_rows.py never enter - rows cut along z (P.nzc > 1), dimensions with
D % 8 == 4 (partial sub-tiles), the 1024-thread form past one round, blockdims other than 8 - and 48 seeded random draws.

A row is a tests/sum_rows.py Row with two more fields, and make() is sum_rows.make() itself with the z offset added: the row's
sum_rows fields are entered into sum_rows.BY_ID under the row's id (sum_rows.ROWS, the table its tests walk, is not touched), so
the generator, its draw order and the contract of the returned dict are the ones of tests/sum_rows.py.

  blockdim  the reference's block edge (None: 8)
  zshift    an offset in A added to every atom's z after centring: it puts a cluster on a z cut, or towards the half sub-tile at the
            end of a row

tests/test_sum_sweep_host.py asserts, with numpy and the culls of the pre-pass alone (tests/f64_rows.slab_counts), that every row
gets where its `reaches` says.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from tests import sum_rows as R
from tests.f64_rows import _block_interval, slab_counts
from tests.sum_rows import LINE_CAP, ONE_ROUND, RES, features_of, merged  # noqa: F401  (re-exported for the test modules)

XL_LDS = 1024  # x-list entries xbin_kernel keeps in LDS
SUBX, SUBY, SUBZ = 2, 4, 8

Row = collections.namedtuple("Row", R.Row._fields + ("blockdim", "zshift"))


def _row(id, D, C, mode, radii_type, density, sizes, radius, spread, seed, reaches, blockdim=None, zshift=0.0):
    return Row(id, D, C, mode, radii_type, density, tuple(sizes), radius, spread, seed, reaches, blockdim, zshift)


ROWS = [
    _row("tall", 72, 32, "features", "atom-wise", "gaussian", (300, 700, 2200), (1.35, 1.5), 2.0, 201,
         "nw 9; molecule 0 a slab over 63 and none over 255, molecule 1 a slab over 255, molecule 2 an x-list over 1024"),
    _row("cut96", 96, 2, "features", "scalar", "gaussian", (300, 1200, 40), 1.5, 2.0, 202,
         "nw 8, nzc 2 (8 + 4 waves): extension (molecule 0) and x-list (molecule 1) in both z chunks", zshift=8.25),
    _row("cut132", 132, 1, "single", "scalar", "binary", (300, 1200, 40), 1.5, 2.0, 203,
         "nw 9, nzc 2 (9 + 8 waves), the last sub-tile half outside: extension and x-list in both z chunks", zshift=3.25),
    _row("cut144", 144, 1, "single", "scalar", "gaussian", (300, 1200, 40), 1.5, 2.0, 204,
         "nw 8, nzc 3 (8 + 8 + 2): extension and x-list in chunks 1 and 2, chunk 0 has slabs without a candidate", zshift=28.25),
    _row("edge20", 20, 33, "features", "scalar", "gaussian", (60,) * 6, 1.2, "box", 205,
         "nw 3, nsy 5, two channel chunks; no molecule over 63, every slab non-empty, boxes that reach voxel 19 on each axis"),
    _row("edge20d", 20, 5, "features", "atom-wise", "gaussian", (40, 200, 700), (1.2, 1.5), 1.0, 206,
         "the same partial sub-tiles with the extension (molecule 1) and the x-list (molecule 2); the cluster 3 A up the z axis", zshift=3.0),
    _row("edge12", 12, 8, "types", "channel-wise", "binary", (0, 30, 30, 0, 30), (0.8, 1.6), "box", 207,
         "nw 2, nsx 6, nsy 3; empty molecules first and in the middle"),
    # (std 3.0 and 7 A up the z axis, with twice the atoms: a cluster of std 2.0 in the middle of a 21.5 A box has no atom near the
    # last y row or the last z sub-tile)
    _row("edge44", 44, 40, "features", "scalar", "gaussian", (400, 1000), 1.5, 3.0, 208,
         "nw 6; the extension (molecule 0) and a slab near the line cap (molecule 1)", zshift=7.0),
    _row("bd16", 40, 4, "features", "scalar", "gaussian", (300,) * 4, 1.5, "box", 209,
         "three blocks per axis (16 + 16 + 8); every molecule has an atom whose admitted blocks cut its voxel window", blockdim=16),
    _row("bd16u", 24, 8, "types", "channel-wise", "gaussian", (100,) * 5, (0.8, 1.6), "box", 210,
         "two unequal blocks (16 + 8); the same", blockdim=16),
    _row("bd24", 24, 1, "single", "atom-wise", "binary", (80, 80, 80), (1.0, 1.5), "box", 211,
         "one block: the blockdim-5000 grid bit for bit", blockdim=24),
]
ROW_IDS = [r.id for r in ROWS]
BY_ID = {r.id: r for r in ROWS}
assert not set(BY_ID) & set(R.ROW_IDS)

# ---- the random draws ----------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = list(range(7000, 7048))
SWEEP_D = (8, 12, 16, 20, 24, 28, 36, 44, 52, 72, 76)
SWEEP_C = (1, 3, 5, 8, 17, 32, 33, 40)
SERVED = [("features", "scalar"), ("features", "atom-wise"), ("types", "scalar"), ("types", "atom-wise"), ("types", "channel-wise"),
          ("single", "scalar"), ("single", "atom-wise")]  # (mode, radii type): what forward_sum serves
Draw = collections.namedtuple("Draw", "seed row weights K accumulate")


@functools.lru_cache(maxsize=None)
def draw(seed: int) -> Draw:
    """Draw `seed` of the random sweep: a row "draw<seed>" for make(), the weight kind (None | "mol" | "atom+"), the parts K of
    set_sum_parts and whether the call accumulates onto a start grid. Everything is drawn independently from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    D = int(rng.choice(SWEEP_D))
    C_ = int(rng.choice(SWEEP_C))
    mode, radii_type = SERVED[int(rng.integers(len(SERVED)))]
    if mode == "single":
        C_ = 1
    density = ("gaussian", "binary")[int(rng.integers(2))]
    blockdim = (None, 16, D)[int(rng.integers(3))]
    B = int(rng.integers(1, 10))
    sizes = [int(n) for n in rng.integers(0, 121, B)]
    if mode == "types" and sum(sizes) <= R.BAD_TYPE_ATOM:  # (make() gives atom 7 of a types row a type outside [0, C))
        sizes[-1] += R.BAD_TYPE_ATOM + 1
    spread = 1.0 if seed % 4 == 0 else "box"  # every fourth draw clustered
    radius = float(rng.uniform(1.0, 1.8)) if radii_type == "scalar" else (0.8, 1.6)
    weights = (None, "mol", "atom+")[int(rng.integers(3))]
    K = (1, 1, 2, 5)[int(rng.integers(4))]
    accumulate = bool(rng.integers(3) == 0)
    row = _row(f"draw{seed}", D, C_, mode, radii_type, density, sizes, radius, spread, seed, "random draw", blockdim)
    return Draw(seed, row, weights, K, accumulate)


def row_of(row_id: str) -> Row:
    return BY_ID[row_id] if row_id in BY_ID else draw(int(row_id[4:])).row


@functools.lru_cache(maxsize=None)
def make(row_id: str) -> dict:
    """The batch of a row or of a draw ("draw<seed>") as host arrays (never modified): sum_rows.make()'s dict, `row` being the
    row of this module, every atom's z moved by the row's zshift."""
    row = row_of(row_id)
    R.BY_ID.setdefault(row_id, R.Row(*row[:len(R.Row._fields)]))
    d = dict(R.make(row_id), row=row)
    if row.zshift:
        xyz = d["xyz"].copy()
        xyz[:, 2] += row.zshift
        d["xyz"] = xyz
    d["xyz"].setflags(write=False)
    return d


# ---- the plan and the candidates per slab -----------------------------------------------------------------------------------------
def nw_nzc(D: int):
    """(waves per slab, z chunks per row) of the summed call: plan_slabs (mvx_plan.hip) for the 32-channel binned plan - whole
    rows up to 16 sub-tiles unless D % 32 == 0, longer rows that are no multiples of 64 B in as few equal chunks as 16 waves allow,
    chunks of 8 otherwise."""
    nsz = -(-D // SUBZ)
    if nsz <= 8:
        nw = nsz
    elif nsz <= 16:
        nw = nsz if D % 32 != 0 else 8
    elif D % 16 != 0:
        k = -(-nsz // 16)
        nw = -(-nsz // k)
    else:
        nw = 8
    return nw, -(-nsz // nw)


def _kept(d: dict, lo: int, hi: int):
    """Positions (box coordinates) and radii of the atoms [lo, hi) that the pre-pass does not drop for their type."""
    row = d["row"]
    keep = np.ones(hi - lo, bool)
    if row.mode == "types":
        keep = (d["chan"][lo:hi] >= 0) & (d["chan"][lo:hi] < row.C)
    return merged(d)[lo:hi][keep], d["r_atom"][lo:hi][keep]


def counts(d: dict, lo: int, hi: int):
    """(lower, upper, xlower) of tests/f64_rows.slab_counts for the atoms [lo, hi) taken as one molecule in box coordinates, with
    the row's blockdim: candidates per slab [sx, sy, zc] bounded from both sides, and a lower bound on the x-lists."""
    row = d["row"]
    xyz, r = _kept(d, lo, hi)
    return slab_counts(xyz, r, row.D, nw_nzc(row.D)[0], row.blockdim)


def molecule_counts(d: dict, b: int):
    return counts(d, int(d["off"][b]), int(d["off"][b + 1]))


def reaches_the_partial_corner(d: dict) -> int:
    """How many atoms are, for certain, candidates of a slab in the last y row AND reach the last z sub-tile: the exact distance
    from the atom to the box of the voxel centres y >= SUBY (nsy - 1), z >= SUBZ (nsz - 1) (any x) against a radius shrunk by 1e-9,
    as slab_counts' lower bound does it: on every axis the stretch of those centres that the atom's admitted blocks leave."""
    row = d["row"]
    D, bd = row.D, 8 if row.blockdim is None else row.blockdim
    half = RES * (D - 1) / 2.0
    xyz, r = _kept(d, 0, d["N"])
    first = (0, SUBY * (-(-D // SUBY) - 1), SUBZ * (-(-D // SUBZ) - 1))
    d2 = np.zeros(xyz.shape[0])
    for a, v0 in enumerate(first):
        p = xyz[:, a]
        vlo, vhi = _block_interval(p, r, D, bd)
        b_lo, b_hi = np.maximum(v0, vlo), np.minimum(D - 1, vhi)
        gap = np.maximum(np.maximum(b_lo * RES - half - p, p - (b_hi * RES - half)), 0.0)
        gap[b_lo > b_hi] = np.inf
        d2 = d2 + gap ** 2
    return int((d2 <= (r * (1.0 - 1e-9)) ** 2).sum())


def window_cut_by_blocks(d: dict, b: int) -> int:
    """How many atoms of molecule b have, on some axis, a non-empty voxel window (the sphere's own, as prep_atom forms it) that
    the admitted reference blocks (mvx_device.h block_interval) make narrower: where the fold of the block cull into the candidate
    ranges changes what a slab sees."""
    row = d["row"]
    D, bd = row.D, 8 if row.blockdim is None else row.blockdim
    half = RES * (D - 1) / 2.0
    xyz, r = _kept(d, int(d["off"][b]), int(d["off"][b + 1]))
    rr = r * 1.000001 + 1e-9
    cut = np.zeros(xyz.shape[0], bool)
    inside = np.ones(xyz.shape[0], bool)
    for a in range(3):
        p = xyz[:, a]
        lo = np.maximum(np.ceil((p - rr + half) / RES), 0).astype(np.int64)
        hi = np.minimum(np.floor((p + rr + half) / RES), D - 1).astype(np.int64)
        vlo, vhi = _block_interval(p, r, D, bd)
        inside &= lo <= hi
        cut |= (lo <= hi) & ((vlo > lo) | (vhi < hi))
    return int((cut & inside).sum())


def sweep_coverage() -> dict:
    """What the 48 draws jointly reach: the sets of D, C and weight kinds, and the seeds of the draws that have a molecule with
    a slab over 63 candidates by slab_counts' lower bound."""
    over = []
    for s in SWEEP_SEEDS:
        d = make(f"draw{s}")
        if any(hi > lo and molecule_counts(d, b)[0].max() > ONE_ROUND for b, (lo, hi) in enumerate(zip(d["off"][:-1], d["off"][1:]))):
            over.append(s)
    dr = [draw(s) for s in SWEEP_SEEDS]
    return dict(D={x.row.D for x in dr}, C={x.row.C for x in dr}, weights={x.weights for x in dr}, K={x.K for x in dr},
                accumulate={x.accumulate for x in dr}, blockdim={"one" if x.row.blockdim == x.row.D else x.row.blockdim for x in dr},
                over_one_round=over)
