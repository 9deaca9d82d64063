"""Shapes of tests/test_hip_narrow.py (GPU) and tests/test_narrow_rows_host.py (host): voxelize_narrow_kernel (mvx_slab.hip: chunks of
1 ... 8 channels, two or four z sub-tiles per wave) on geometries that leave the one-round case of a slab's candidate line.

The narrow kernel is an instantiation of mvx_slab_body.inc like every other batched kernel, but it is the only one whose waves
serve several sub-tiles: the staging's trips, the row filter's turns and the write-out's passes depend on the sub-tiles per wave.
The dense-cluster parity tests run at D = 24 - three sub-tiles per row, which neither 2 nor 4 divides - and never reach it.

Every geometry declares the line forms it stands for (tests/f64_rows.py slab_counts / line_forms, at the row's nw); the host module
asserts them and the plan fields without a GPU, so that neither a plan change nor a thinner geometry can silently empty the sweep.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

from tests import f64_rows as F

BINNED = 0
RES, SIGMA = F.RES, 0.6


@dataclass(frozen=True)
class Geom:
    D: int
    nw: int  # z sub-tiles per slab (plan)
    atoms: int
    positions: str  # "normal:<std>" | "uniform"
    radius: float  # scalar
    forms: tuple  # line forms the geometry must reach for certain


# res 0.5, positions from default_rng(1) (f64_rows.positions' rule). Measured with f64_rows.slab_counts: N32x at least 993 candidates
# in its densest slab and 1235 atoms on its longest x-list (beyond xbin_kernel's LDS copy); N16x one wave per workgroup at two
# sub-tiles per wave and rounds of 16 rows: many rounds; N48x three waves at two sub-tiles per wave; N32e 28 slabs between 64 and
# 255 candidates; N48o at most 18 candidates per slab.
GEOMS = {
    "N32x": Geom(32, 4, 1500, "normal:1.2", 1.5, ("xlist", "xlist_long", "extension", "empty")),
    "N16x": Geom(16, 2, 900, "normal:0.9", 1.5, ("xlist", "extension")),
    "N48x": Geom(48, 6, 1200, "normal:3.0", 2.0, ("xlist", "extension", "empty")),
    "N32e": Geom(32, 4, 500, "normal:2.5", 2.0, ("extension", "empty")),
    "N48o": Geom(48, 6, 600, "uniform", 1.0, ("one_round",)),
}


@dataclass(frozen=True)
class Config:
    name: str
    mode: str  # features | types | single
    C: int
    density: str

    @property
    def nch(self) -> int:
        return 1 if self.mode == "single" else self.C

    @property
    def exact(self) -> bool:
        return self.density == "binary" and self.mode != "features"


CONFIGS = [Config("single-binary", "single", 1, "binary"), Config("single-gaussian", "single", 1, "gaussian"),
           Config("types4-binary", "types", 4, "binary"), Config("feat5-gaussian", "features", 5, "gaussian")]
# ... and the remainder launch (c0 = 32) of 32 k + r channels on the narrow kernel, one and four channels wide
REMAINDERS = [Config("feat33-gaussian", "features", 33, "gaussian"), Config("feat36-gaussian", "features", 36, "gaussian")]


@dataclass(frozen=True)
class Row:
    geom: str
    cfg: Config

    @property
    def id(self) -> str:
        return f"{self.geom}-{self.cfg.name}"

    @property
    def g(self) -> Geom:
        return GEOMS[self.geom]

    @property
    def ct(self) -> int:
        """Channels per chunk of the launch that reaches the narrow kernel: the only launch, or the remainder's."""
        c = self.cfg.nch % 32
        return 1 if c == 1 else 4 if c <= 4 else 8

    @property
    def plan(self) -> dict:
        """Plan fields of the call (mvx_plan_call)."""
        p = dict(route=BINNED, nw=self.g.nw, nzc=1, vec_store=1, lane_range=0, grouped=0, nchunk=1)
        if self.cfg.nch > 32:
            p.update(ct=32, nfull=1, ct_rem=self.ct)
        else:
            p.update(ct=self.ct, ncc=1, ct_rem=0)
        return p

    @property
    def nsub(self) -> int:
        """Sub-tiles per wave the library's rule picks (mvx_slab.hip LaunchFn)."""
        return 4 if self.ct <= 4 and self.g.nw % 4 == 0 else 2

    @property
    def forced(self) -> tuple:
        """The "narrow_sub" values to compare against narrow_sub = 1 (voxelize_kernel's pair walk)."""
        return (2, 4) if self.ct <= 4 and self.g.nw % 4 == 0 else (2,)


ROWS = [Row(g, c) for g in GEOMS for c in CONFIGS] + [Row("N32x", c) for c in REMAINDERS]
ROW_IDS = [r.id for r in ROWS]
# channels-last grids (write_ndhwc_sets): four sub-tiles per wave for one channel only; 16-byte stores (C = 4) and element stores (C = 5)
CL_ROWS = [Row("N32x", CONFIGS[1]), Row("N32x", CONFIGS[2]), Row("N48o", CONFIGS[3])]
CL_IDS = [r.id for r in CL_ROWS]


def narrow_plan(plan: dict) -> dict:
    """The plan as the launch that reaches the narrow kernel sees it (batch_cut_rows.narrow_sub_tiles reads `ct`)."""
    return dict(plan, ct=plan["ct_rem"]) if plan["ct_rem"] else plan


@functools.lru_cache(maxsize=None)
def positions(geom: str) -> np.ndarray:
    return F.geom_positions(GEOMS[geom])


@functools.lru_cache(maxsize=None)
def geom_forms(geom: str):
    g = GEOMS[geom]
    lower, upper, xlower = F.slab_counts(positions(geom), np.full(g.atoms, g.radius), g.D, g.nw)
    return F.line_forms(lower, upper, xlower, g.nw, g.D), lower, upper, xlower


def channels(cfg: Config, n: int, rng) -> np.ndarray | None:
    if cfg.mode == "features":
        chan = rng.random((n, cfg.C)).astype(np.float32)
        chan[rng.random((n, cfg.C)) < 0.3] = 0.0
        return chan
    if cfg.mode == "types":
        chan = rng.integers(0, cfg.C, n).astype(np.int16)
        chan[:1] = cfg.C - 1
        return chan
    return None


@functools.lru_cache(maxsize=None)
def make_batch(row: Row) -> dict:
    """[a molecule with no atom inside the box, the row's molecule, a ten-atom one]: coordinates, channels, offsets."""
    g, cfg = row.g, row.cfg
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    W = RES * (g.D - 1)
    outside = rng.uniform(W / 2 + 2 * g.radius + 1, W / 2 + 2 * g.radius + 3, (25, 3)) * rng.choice([-1.0, 1.0], (25, 3))
    small = rng.uniform(-W / 2, W / 2, (10, 3))
    xyz = [outside, positions(row.geom), small]
    chan = [channels(cfg, x.shape[0], rng) for x in xyz]
    sizes = [x.shape[0] for x in xyz]
    return dict(xyz=xyz, chan=chan, sizes=sizes, offsets=np.cumsum([0] + sizes).astype(np.int64))
