"""Shapes of tests/test_hip_batch_cuts.py (GPU) and tests/test_batch_cuts_host.py (host): one row per kernel family that has to decode
"which molecule, which channels am I" when mvx_capi.hip cuts a forward_batch call into several launches.

Every row names the plan fields (mvx_plan_call, a pure host function) that make it the family it claims to be; the host module
asserts them without a GPU, so that a later retuning of the plan cannot silently move a row to another kernel. The rules of
mvx_plan.hip / mvx_capi.hip / mvx_slab.hip that decide how a call is cut are restated here in Python and checked against the
library on the host.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field

import numpy as np

BINNED, DIRECT, F64_DENSE, F64_MX = 0, 1, 2, 3
MALL_BUDGET = 288.0e6  # mvx_tuning.h
GRID_Y_MAX = 65535  # gridDim.y limit: (molecule, channel chunk) pairs per launch


@dataclass(frozen=True)
class Row:
    id: str
    D: int
    C: int
    plan: dict  # plan fields this row stands for (asserted against mvx_plan_call on the host)
    mode: str = "features"  # features | types | single
    radii: str = "scalar"  # scalar | atom-wise | channel-wise
    density: str = "gaussian"
    precision: int = 32
    blockdim: int | None = None
    bf16: bool = False
    cl: bool = False  # channels-last grid
    narrow_sub: int = 0  # "narrow_sub" option (0: the library's rule)
    narrow: int = -1  # sub-tiles per wave of voxelize_narrow_kernel this row reaches (0: it does not; -1: not asserted)
    misaligned: bool = False  # out_grid is a view 4 bytes off 16-byte alignment
    device: bool = True  # device-resident inputs (else numpy arrays staged by the library)
    batch: str = "ragged"  # ragged (16 molecules) | few (4 molecules, for big grids)
    chunks: tuple = ()  # values of the "chunks" option (side stream) to run besides the Infinity Cache budgets
    transform: bool = False  # random_translation / random_rotation per molecule
    n_radii: int = 0  # channel-wise radii: number of distinct values (0: every channel its own)


def _r(id, D, C, plan, **kw):
    return Row(id=id, D=D, C=C, plan=plan, **kw)


WIDE = dict(route=BINNED, ct=32, grouped=0, vec_store=1, lane_range=0)
ROWS = [
    # ---- wide + remainder launch: main launch of nfull chunks, second launch with ncc = 1 and c0 = nfull * ct ----------------
    _r("rem-C33", 32, 33, dict(WIDE, ncc=2, nfull=1, ct_rem=1, nw=4, nzc=1), chunks=(3,)),
    _r("rem-C40-host", 32, 40, dict(WIDE, ncc=2, nfull=1, ct_rem=8, nw=4, nzc=1), device=False, radii="atom-wise"),
    _r("rem-C65", 32, 65, dict(WIDE, ncc=3, nfull=2, ct_rem=1, nw=4, nzc=1), chunks=(4,)),
    # ---- two full chunks ------------------------------------------------------------------------------------------------------
    _r("full-C50-packed", 32, 50, dict(WIDE, ncc=2, nfull=2, ct_rem=0, cpad=64, weights_in_place=0), device=False),
    _r("full-C64-in-place", 32, 64, dict(WIDE, ncc=2, nfull=2, ct_rem=0, cpad=64, weights_in_place=1)),
    # ---- grouped launch (channel-wise feature radii) --------------------------------------------------------------------------
    _r("grouped-C40-3radii", 32, 40, dict(route=BINNED, grouped=1, ct=32, ncc=2, ct_rem=0, weights_in_place=1), radii="channel-wise",
       n_radii=3, chunks=(3,)),
    _r("grouped-C72-binary-host", 32, 72, dict(route=BINNED, grouped=1, ct=32, ncc=3, ct_rem=0), radii="channel-wise", density="binary",
       device=False),
    _r("grouped-C40-binary", 32, 40, dict(route=BINNED, grouped=1, ct=32, ncc=2), radii="channel-wise", density="binary", n_radii=3),
    _r("grouped-C72", 32, 72, dict(route=BINNED, grouped=1, ct=32, ncc=3), radii="channel-wise", chunks=(2,)),
    # ---- narrow multi-sub-tile kernel (the shared decode of mvx_slab_body.inc with NW / NSUB waves per workgroup) ---------------
    _r("narrow-single-D32", 32, 1, dict(route=BINNED, ct=1, ncc=1, nw=4, nzc=1, vec_store=1, lane_range=0), mode="single", narrow=4),
    _r("narrow-single-D40", 40, 1, dict(route=BINNED, ct=1, ncc=1, nw=4, nzc=2, vec_store=1, lane_range=0), mode="single",
       radii="atom-wise", narrow=4, device=False),
    _r("narrow-types-C4-D32", 32, 4, dict(route=BINNED, ct=4, ncc=1, nw=4, nzc=1, vec_store=1, lane_range=0), mode="types",
       density="binary", narrow=4),
    # (C = 4 at D = 40 keeps whole rows of five sub-tiles, which no multi-sub-tile kernel divides: D = 48, six sub-tiles, two per wave)
    _r("narrow-types-C4-D48", 48, 4, dict(route=BINNED, ct=4, ncc=1, nw=6, nzc=1, vec_store=1, lane_range=0), mode="types", narrow=2),
    _r("narrow-types-C4-sub2", 32, 4, dict(route=BINNED, ct=4, ncc=1, nw=4, nzc=1, vec_store=1, lane_range=0), mode="types",
       narrow_sub=2, narrow=2, radii="atom-wise"),
    _r("narrow-single-sub2", 32, 1, dict(route=BINNED, ct=1, ncc=1, nw=4, nzc=1, vec_store=1, lane_range=0), mode="single",
       density="binary", narrow_sub=2, narrow=2),
    _r("narrow-fallback-types-C4-sub4-D40", 40, 4, dict(route=BINNED, ct=4, ncc=1, nw=5, nzc=1, vec_store=1, lane_range=0), mode="types",
       narrow_sub=4, narrow=0),  # (five sub-tiles: the request cannot be met, voxelize_kernel's pair walk serves the row)
    # ---- narrow pair walk, 8 / 16 channels --------------------------------------------------------------------------------------
    _r("pair-C8", 32, 8, dict(route=BINNED, ct=8, ncc=1, nw=4, vec_store=1, lane_range=0), narrow=2),
    _r("pair-C16-host", 32, 16, dict(route=BINNED, ct=16, ncc=1, nw=4, vec_store=1, lane_range=0), narrow=0, device=False, radii="atom-wise"),
    # ---- run-wise write-out with XCD ranges (blockIdx.x remapped while blockIdx.y carries the chunk) ---------------------------
    _r("runs-D31-C32", 31, 32, dict(route=BINNED, ct=32, ncc=1, vec_store=0, xcd_ranges=1, nzc=1)),
    _r("runs-D31-C4-host", 31, 4, dict(route=BINNED, ct=4, ncc=1, vec_store=0, xcd_ranges=1, nzc=1), narrow=0, device=False),
    _r("runs-D50-C32", 50, 32, dict(route=BINNED, ct=32, ncc=1, vec_store=0, xcd_ranges=1, nzc=1, nw=7), radii="atom-wise"),
    _r("runs-D50-C4", 50, 4, dict(route=BINNED, ct=4, ncc=1, vec_store=0, xcd_ranges=1, nzc=1, nw=7), mode="types", narrow=0),
    _r("runs-D32-C33-misaligned", 32, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=0, xcd_ranges=1), misaligned=True),
    # ---- run-wise write-out, rows cut in z (no XCD ranges): big grids, a few molecules, one per chunk ---------------------------
    _r("runs-nzc-D130-C4", 130, 4, dict(route=BINNED, ct=4, ncc=1, vec_store=0, xcd_ranges=0, nzc=2, nw=9), batch="few", narrow=0),
    _r("runs-nzc-D130-C33", 130, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=0, xcd_ranges=0, nzc=2, nw=9),
       batch="few"),
    # ---- rows cut in z with vector stores -----------------------------------------------------------------------------------------
    _r("vec-nzc-D96-C16", 96, 16, dict(route=BINNED, ct=16, ncc=1, vec_store=1, nw=4, nzc=3), batch="few", device=False),
    _r("vec-nzc-D96-C33", 96, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=1, nw=8, nzc=2), batch="few"),
    # ---- per-lane block ranges ----------------------------------------------------------------------------------------------------
    _r("lanes-bd5-C33", 32, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, lane_range=1), blockdim=5),
    _r("lanes-bd12-C4-host", 32, 4, dict(route=BINNED, ct=4, ncc=1, lane_range=1), blockdim=12, mode="types", narrow=0, device=False),
    _r("lanes-bd12-C33", 32, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, lane_range=1), blockdim=12, density="binary"),
    _r("lanes-bd5-C4", 32, 4, dict(route=BINNED, ct=4, ncc=1, lane_range=1), blockdim=5, narrow=0),
    # ---- types with many channels (weights packed by prep_kernel from pa.first) ------------------------------------------------
    _r("types-C40-atomwise", 32, 40, dict(WIDE, ncc=2, nfull=1, ct_rem=8, weights_in_place=0), mode="types", radii="atom-wise",
       density="binary"),
    _r("types-C40-chanwise-host", 32, 40, dict(WIDE, ncc=2, nfull=1, ct_rem=8, weights_in_place=0), mode="types", radii="channel-wise",
       device=False),
    # ---- bfloat16 grids -------------------------------------------------------------------------------------------------------------
    _r("bf16-C33-D32", 32, 33, dict(WIDE, ncc=2, nfull=1, ct_rem=1), bf16=True),
    _r("bf16-C4-D32-host", 32, 4, dict(route=BINNED, ct=4, ncc=1, vec_store=1), bf16=True, mode="types", narrow=4, device=False),
    _r("bf16-C33-D31", 31, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=0, xcd_ranges=1), bf16=True),
    _r("bf16-C4-D31", 31, 4, dict(route=BINNED, ct=4, ncc=1, vec_store=0, xcd_ranges=1), bf16=True, narrow=0),
    # ---- channels-last grids ------------------------------------------------------------------------------------------------------
    _r("cl-f32-C33", 32, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=0, xcd_ranges=0), cl=True, chunks=(3,)),
    _r("cl-bf16-C33-host", 32, 33, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1, vec_store=0, xcd_ranges=0), cl=True, bf16=True,
       device=False),
    _r("cl-f32-C40", 32, 40, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=8, vec_store=1), cl=True),
    _r("cl-bf16-C40", 32, 40, dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=8, vec_store=1), cl=True, bf16=True, chunks=(2,)),
    _r("cl-f32-C72-D72", 72, 72, dict(route=BINNED, ct=32, ncc=3, nfull=2, ct_rem=8, vec_store=1, nw=5, nzc=2), cl=True, batch="few"),
    _r("cl-bf16-C72-D72", 72, 72, dict(route=BINNED, ct=32, ncc=3, nfull=2, ct_rem=8, vec_store=1, nw=5, nzc=2), cl=True, bf16=True,
       batch="few"),
    _r("cl-f32-C40-grouped", 32, 40, dict(route=BINNED, grouped=1, ct=32, ncc=2), cl=True, radii="channel-wise", n_radii=3),
    # ---- float64: every chunk's pre-pass first, then one launch (dense) or launch_mx64's own loop ---------------------------------
    _r("f64-dense-C16", 32, 16, dict(route=F64_DENSE, ct=16, ncc=1), precision=64, chunks=(2, 4)),
    _r("f64-dense-C40-chanwise-host", 32, 40, dict(route=F64_DENSE, ct=16, ncc=3, grouped=0), precision=64, radii="channel-wise",
       chunks=(3,), device=False),
    _r("f64-mx-C33", 32, 33, dict(route=F64_MX, ct=32, ncc=2), precision=64, chunks=(2, 4)),
    _r("f64-mx-C64-host", 32, 64, dict(route=F64_MX, ct=32, ncc=2), precision=64, chunks=(3,), radii="atom-wise", device=False),
    # ---- random transforms per molecule (the xforms array is indexed by the absolute molecule in prep_kernel) -------------------
    _r("xform-rem-C33", 32, 33, dict(WIDE, ncc=2, nfull=1, ct_rem=1), transform=True),
    _r("xform-narrow-types-C4-host", 32, 4, dict(route=BINNED, ct=4, ncc=1, nw=4), mode="types", transform=True, narrow=4, device=False),
]
ROW_IDS = [r.id for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)

RAGGED_SIZES = [0, 300, 1200, 45, 2200, 5, 1, 0, 300, 1200, 45, 1, 5, 300, 45, 0]  # first, last and a middle molecule empty
DENSE = 4  # the dense cluster: slab lines overflow into extension lines / the x-list inside a chunk with b0 > 0
FEW_SIZES = [400, 0, 250, 300]
SCALAR_RADIUS, SIGMA, RES = 1.1, 0.6, 0.5


def make_batch(row: Row) -> dict:
    """The molecules of a row: per-molecule coordinates (already moved by their centre), centres, channels and radii. Features,
    types and coordinates are random per molecule, so a grid written from another molecule's atoms cannot pass."""
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    sizes = list(RAGGED_SIZES if row.batch == "ragged" else FEW_SIZES)
    W = RES * (row.D - 1)
    coords = [rng.uniform(-W / 2 - 1, W / 2 + 1, (n, 3)) for n in sizes]
    if row.batch == "ragged":
        coords[DENSE] = rng.normal(0.0, 0.5, (sizes[DENSE], 3)) + rng.uniform(-W / 4, W / 4, 3)
    centers = rng.uniform(-1, 1, (len(sizes), 3))
    feats = [rng.random((n, row.C)).astype(np.float32) for n in sizes]
    types = [rng.integers(0, row.C, n).astype(np.int16) for n in sizes]
    r_atom = [rng.uniform(0.8, 1.6, n).astype(np.float32) for n in sizes]
    if row.n_radii:
        r_chan = rng.choice(np.linspace(1.0, 1.6, row.n_radii), row.C).astype(np.float32)
        r_chan[:row.n_radii] = np.linspace(1.0, 1.6, row.n_radii)
    else:
        r_chan = rng.uniform(0.8, 1.6, row.C).astype(np.float32)
    return dict(sizes=sizes, coords=coords, centers=centers, feats=feats, types=types, r_atom=r_atom, r_chan=r_chan,
                offsets=np.cumsum([0] + sizes).astype(np.int64))


def grid_codes(row):
    from molvoxel_amd.voxelizer.hip import _lib

    return (_lib.MVX_GRID_BF16 if row.bf16 else _lib.MVX_GRID_REAL, _lib.MVX_LAYOUT_NDHWC if row.cl else _lib.MVX_LAYOUT_NCDHW)


def host_plan(row: Row, sizes) -> dict:
    """mvx_plan_call for the row's batch as the library sees it without debug options (one launch per chunk of the plan)."""
    from molvoxel_amd.voxelizer.hip import _lib

    grid_type, layout = grid_codes(row)
    return _lib.plan_call(row.D, row.C, len(sizes), total_atoms=int(sum(sizes)), max_atoms=int(max(sizes)), mode=row.mode,
                          radii_type=row.radii, precision=row.precision, blockdim=row.blockdim or 8,
                          out_aligned16=not row.misaligned, grid_type=grid_type, layout=layout)


def narrow_sub_tiles(plan: dict, narrow_sub: int, cl: bool) -> int:
    """mvx_slab.hip LaunchFn restated: sub-tiles per wave of voxelize_narrow_kernel for the main launch of this plan, 0 when
    voxelize_kernel (or its run-wise variants) serves it."""
    ct = plan["ct"]
    if ct >= 16 or plan["lane_range"] or plan["grouped"]:
        return 0
    ct4 = 1 if cl else 4
    nsub = narrow_sub if narrow_sub > 0 else (4 if (ct <= ct4 and plan["nw"] % 4 == 0) else 2)
    if not (nsub > 1 and plan["nw"] % nsub == 0 and (plan["vec_store"] or cl)):
        return 0
    if nsub == 4:
        return 4 if ct <= ct4 else 0
    return 2


def prepass_bytes(plan: dict, B: int, C: int, total_atoms: int) -> float:
    """mvx_plan.hip: what a chunk's voxelize launch re-reads (records, keys, feature rows, slab lines)."""
    per_mol = plan["nsx"] * plan["nsy"] * plan["nzc"]
    return total_atoms * (64.0 + 8.0 + 4.0 * ((C + 3) // 4 * 4)) + float(B) * per_mol * 512.0


def expected_nchunk(plan: dict, B: int, C: int, total_atoms: int, precision: int = 32, budget_kb: int = 0, chunks: int = 1) -> int:
    """mvx_plan.hip "molecule chunks" restated: gridDim.y limit, Infinity Cache budget (float32 only; the "mall_budget_kb" option),
    the "chunks" option (side stream, B >= 4 * chunks)."""
    n = -(-B // (GRID_Y_MAX // plan["ncc"]))
    if precision == 32 and B > 0:
        budget = 1024.0 * budget_kb if budget_kb > 0 else MALL_BUDGET
        n = max(n, int(min(math.ceil(prepass_bytes(plan, B, C, total_atoms) / budget), max(1, B))))
    if chunks > 1 and B >= 4 * chunks:
        n = max(n, chunks)
    return max(n, 1)


def budget_for(plan: dict, B: int, C: int, total_atoms: int, nchunk: int) -> int:
    """A "mall_budget_kb" value that cuts the batch into `nchunk` chunks (the caller asserts expected_nchunk of it)."""
    return max(1, int(math.ceil(prepass_bytes(plan, B, C, total_atoms) / nchunk / 1024.0)))


def chunk_begin(B: int, nchunk: int, k: int) -> int:
    """mvx_capi.hip: first molecule of chunk k."""
    return B * k // nchunk


def expected_launches(plan: dict, nchunk: int) -> int:
    """Entries read_kernel_times_ms() returns for one call: one per voxelize launch of the float32 binned route (main + remainder
    per chunk; one grouped launch per chunk). Float64 calls time one bracket whatever the cut: the dense kernel is one launch and
    launch_mx64's bracket rides on its first launch only."""
    if plan["route"] in (F64_DENSE, F64_MX):
        return 1
    return nchunk * (1 + (plan["ct_rem"] != 0))


# ---- the division trick -----------------------------------------------------------------------------------------------------------
def umulhi_inverse(d: int) -> int:
    """mvx_capi.hip umulhi_inverse / mvx_prep.hip nsx_inv: ceil(2^32 / d); d == 1 is special-cased by the kernels (0xffffffff)."""
    return 0xFFFFFFFF if d == 1 else (0x100000000 + d - 1) // d


def umulhi(n: int, inv: int) -> int:
    assert 0 <= n < 1 << 32 and 0 <= inv < 1 << 32
    return (n * inv) >> 32


# ---- the gridDim.y limit for real (section B) ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Big:
    id: str
    D: int  # 8 for up to four channels (16 for the narrow-kernel rows: two sub-tiles per row), 4 above: outputs stay under 2 GB
    C: int
    B: int
    mode: str = "features"
    radii: str = "scalar"
    density: str = "gaussian"
    precision: int = 32
    bf16: bool = False
    cl: bool = False
    narrow: int = -1  # sub-tiles per wave of voxelize_narrow_kernel the call reaches (0: voxelize_kernel; -1: not asserted)
    plan: dict = field(default_factory=dict)


BIG = [
    Big("f32-single-65535", 8, 1, 65535, mode="single", narrow=0, plan=dict(route=BINNED, ct=1, ncc=1)),
    Big("f32-single-65536", 8, 1, 65536, mode="single", density="binary", narrow=0, plan=dict(route=BINNED, ct=1, ncc=1)),
    Big("f32-single-70001", 8, 1, 70001, mode="single", radii="atom-wise", narrow=0, plan=dict(route=BINNED, ct=1, ncc=1)),
    Big("f32-types-C4-65535", 8, 4, 65535, mode="types", density="binary", narrow=0, plan=dict(route=BINNED, ct=4, ncc=1)),
    Big("f32-types-C4-65536", 8, 4, 65536, mode="types", narrow=0, plan=dict(route=BINNED, ct=4, ncc=1)),
    Big("f32-types-C4-70001", 8, 4, 70001, mode="types", radii="atom-wise", narrow=0, plan=dict(route=BINNED, ct=4, ncc=1)),
    # voxelize_narrow_kernel takes the decode of mvx_slab_body.inc (blockIdx.y, b0, slab line address) with fewer waves than the
    # slab has sub-tiles: rows of one sub-tile (D = 8) never reach it, rows of two (D = 16) do, two sub-tiles per wave
    Big("f32-narrow-single-D16-65536", 16, 1, 65536, mode="single", narrow=2, plan=dict(route=BINNED, ct=1, ncc=1, nw=2, nzc=1, vec_store=1,
                                                                                     lane_range=0)),
    Big("f32-narrow-single-D16-70001", 16, 1, 70001, mode="single", radii="atom-wise", density="binary", narrow=2,
        plan=dict(route=BINNED, ct=1, ncc=1, nw=2, nzc=1, vec_store=1, lane_range=0)),
    Big("f32-rem-C33-65600", 4, 33, 65600, plan=dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=1)),
    Big("f32-rem-C65-32800", 4, 65, 32800, plan=dict(route=BINNED, ct=32, ncc=3, nfull=2, ct_rem=1)),
    Big("f32-grouped-C40-32800", 4, 40, 32800, radii="channel-wise", plan=dict(route=BINNED, grouped=1, ct=32, ncc=2)),
    Big("cl-bf16-C40-32800", 4, 40, 32800, bf16=True, cl=True, plan=dict(route=BINNED, ct=32, ncc=2, nfull=1, ct_rem=8)),
    Big("f64-mx-C33-32767", 4, 33, 32767, precision=64, plan=dict(route=F64_MX, ct=32, ncc=2)),
    Big("f64-mx-C33-32768", 4, 33, 32768, precision=64, plan=dict(route=F64_MX, ct=32, ncc=2)),
    Big("f64-mx-C33-40001", 4, 33, 40001, precision=64, radii="atom-wise", plan=dict(route=F64_MX, ct=32, ncc=2)),
    Big("f64-dense-C40-chanwise-21900", 4, 40, 21900, precision=64, radii="channel-wise", plan=dict(route=F64_DENSE, ct=16, ncc=3)),
    Big("f64-dense-C16-65600", 4, 16, 65600, precision=64, plan=dict(route=F64_DENSE, ct=16, ncc=1)),
]
BIG_IDS = [c.id for c in BIG]
MAX_OUTPUT_BYTES = 2 * 1024**3
SUB_BATCH = 4096  # molecules per call of the uncut comparison run: the regime the rest of the suite covers


def big_output_bytes(case: Big) -> int:
    return case.B * case.C * case.D**3 * (8 if case.precision == 64 else (2 if case.bf16 else 4))


def big_sizes(case: Big) -> np.ndarray:
    """0 ... 5 atoms per molecule, a sixth of the molecules empty (the first one among them)."""
    return ((np.arange(case.B, dtype=np.int64) * 7) % 6)


def big_host_plan(case: Big) -> dict:
    from molvoxel_amd.voxelizer.hip import _lib

    sizes = big_sizes(case)
    grid_type, layout = grid_codes(case)
    return _lib.plan_call(case.D, case.C, case.B, total_atoms=int(sizes.sum()), max_atoms=int(sizes.max()), mode=case.mode,
                          radii_type=case.radii, precision=case.precision, grid_type=grid_type, layout=layout)


def big_cut_points(case: Big, plan: dict) -> list:
    """First molecules of the launches a call is cut into. float32: chunk_begin of the plan's chunks. float64, either kernel:
    launch_slabs64's own loop, 65535 // ncc molecules per launch (the vector kernels' rows also keep the molecule after the
    first cut, from when they were one launch whose (molecule, chunk) ids crossed 65 535 there)."""
    if plan["route"] == F64_MX or plan["route"] == F64_DENSE:
        per = GRID_Y_MAX // plan["ncc"]
        return [k * per for k in range(1, -(-case.B // per))] + ([per + 1] if plan["route"] == F64_DENSE else [])
    return [chunk_begin(case.B, plan["nchunk"], k) for k in range(1, plan["nchunk"])]
