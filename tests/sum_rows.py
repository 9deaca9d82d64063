"""The shapes of the summed-grid tests (tests/test_hip_sum.py on the GPU, tests/test_sum_rows_host.py without one).

Every row is one batch for forward_sum: molecules stored back to back around centres of their own, res = 0.5, atoms drawn with a
fixed seed. `reaches` says what the row is there for; tests/test_sum_rows_host.py asserts, with numpy and the culls of the
pre-pass alone (tests/f64_rows.slab_counts), that the row really gets there.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from tests.f64_rows import slab_counts  # candidates per slab, bounded from both sides by the pre-pass's own culls

RES = 0.5
ONE_ROUND, LINE_CAP = 63, 255  # candidates a slab line / line + extension hold (mvx_device.h: SLOTS - 1, LINE_CAP)

Row = collections.namedtuple("Row", "id D C mode radii_type density sizes radius spread seed reaches")

ROWS = [
    Row("light", 16, 5, "features", "scalar", "gaussian", (0, 1, 3, 40, 0, 12, 25), 1.0, "box", 101,
        "one molecule outside the box; empty molecules first and in the middle"),
    Row("carry", 16, 32, "features", "atom-wise", "gaussian", (40,) * 12, (0.8, 1.6), 1.0, 102,
        "no molecule has a slab over 63 candidates; the batch has one over 255"),
    Row("rounds", 16, 32, "features", "scalar", "gaussian", (20, 300, 90), 1.5, "cluster", 103,
        "one molecule alone: a slab over 63 and one over 255"),
    Row("chunks", 24, 33, "features", "scalar", "gaussian", (30,) * 9, 1.0, "box", 104, "C = 32 + 1"),
    Row("wide", 24, 65, "features", "atom-wise", "gaussian", (50,) * 4, (0.8, 1.6), "box", 105, "three channel chunks"),
    Row("types", 24, 8, "types", "channel-wise", "gaussian", (60,) * 5, (0.8, 1.6), "box", 106, "one-hot rows; one type outside [0, C)"),
    Row("single", 40, 1, "single", "scalar", "binary", (80,) * 6, 1.2, "box", 107, "NW = 5, binary"),
    Row("long", 72, 4, "features", "scalar", "gaussian", (200,) * 3, 1.0, "box", 108, "a 9-wave slab (1024-thread form)"),
]
BY_ID = {r.id: r for r in ROWS}
ROW_IDS = [r.id for r in ROWS]
OUTSIDE_MOLECULE = 2  # `light`: the molecule of 3 atoms lies far outside the box
BAD_TYPE_ATOM = 7     # `types`: this atom's type is -1


@functools.lru_cache(maxsize=None)
def make(row_id: str) -> dict:
    """The batch of a row as host arrays (never modified): xyz (sumN, 3) float64 around the centres cen (B, 3), off (B + 1,),
    chan (features float32 (sumN, C) >= 0 | types int64 (sumN,) | None), radii (python float | (sumN,) | (C,) float32), q / t
    (explicit poses), and r_atom (sumN,) float64: every atom's own radius, as the culls see it."""
    row = BY_ID[row_id]
    rng = np.random.default_rng(row.seed)
    sizes = row.sizes
    B, N = len(sizes), int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    half = RES * (row.D - 1) / 2
    cen = rng.uniform(-25.0, 25.0, (B, 3))
    rel = []
    for b, n in enumerate(sizes):
        if row.spread == "box":
            p = rng.uniform(-half, half, (n, 3))
        elif row.spread == "cluster":  # within 1 A of the centre
            p = rng.uniform(-0.55, 0.55, (n, 3))
        else:
            p = rng.normal(0.0, float(row.spread), (n, 3))
        if row.id == "light" and b == OUTSIDE_MOLECULE:
            p = p + np.array([30.0, -28.0, 33.0])
        rel.append(p)
    xyz = np.concatenate([cen[b] + rel[b] for b in range(B)]).reshape(N, 3)
    if row.mode == "features":
        chan = rng.random((N, row.C)).astype(np.float32)
    elif row.mode == "types":
        chan = rng.integers(0, row.C, N)
        chan[BAD_TYPE_ATOM] = -1
    else:
        chan = None
    if row.radii_type == "scalar":
        radii = float(row.radius)
        r_atom = np.full(N, float(np.float32(radii)), np.float64)
    elif row.radii_type == "atom-wise":
        radii = rng.uniform(*row.radius, N).astype(np.float32)
        r_atom = radii.astype(np.float64)
    else:  # radii[types]
        radii = rng.uniform(*row.radius, row.C).astype(np.float32)
        r_atom = radii[np.clip(chan, 0, row.C - 1)].astype(np.float64)
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    t = rng.uniform(-0.5, 0.5, (B, 3))
    return dict(row=row, B=B, N=N, off=off, cen=cen, xyz=xyz, chan=chan, radii=radii, r_atom=r_atom, q=q, t=t)


def merged(d: dict) -> np.ndarray:
    """The ONE merged molecule concat_b(coords_b - c_b), formed in float64 as the device forms it."""
    lengths = np.diff(d["off"])
    return d["xyz"] - np.repeat(d["cen"], lengths, axis=0)


def features_of(d: dict) -> np.ndarray:
    """The weight rows w[n, c] of every atom as float32 features: the feature row, onehot(type) (zeros for a type outside
    [0, C)), or 1."""
    row = d["row"]
    if row.mode == "features":
        return d["chan"]
    if row.mode == "single":
        return np.ones((d["N"], 1), np.float32)
    w = np.zeros((d["N"], row.C), np.float32)
    ok = (d["chan"] >= 0) & (d["chan"] < row.C)
    w[np.nonzero(ok)[0], d["chan"][ok]] = 1.0
    return w


def nw_of(row: Row) -> int:
    """Waves per slab of the summed call: whole rows up to 16 sub-tiles (the 32-channel plan of the binned pipeline)."""
    nsz = -(-row.D // 8)
    return nsz if (nsz <= 8 or (nsz <= 16 and row.D % 32 != 0)) else 8


def counts(d: dict, lo: int, hi: int):
    """(lower, upper) candidates per slab of the atoms [lo, hi) taken as one molecule in box coordinates."""
    row = d["row"]
    keep = np.ones(hi - lo, bool)
    if row.mode == "types":
        keep = (d["chan"][lo:hi] >= 0) & (d["chan"][lo:hi] < row.C)  # (a type outside [0, C) is culled before anything else)
    lower, upper, _ = slab_counts(merged(d)[lo:hi][keep], d["r_atom"][lo:hi][keep], row.D, nw_of(row))
    return lower, upper
