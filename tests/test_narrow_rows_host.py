"""Host half of tests/test_hip_narrow.py: no GPU, nothing is launched.

* every geometry of tests/narrow_rows.py reaches the line forms it names - one round, extension line, x-list, an x-list beyond
  xbin_kernel's LDS copy, empty slabs - by the two host-side bounds of tests/f64_rows.py at the row's sub-tiles per slab;
* mvx_plan_call gives every row the nw, ct (or remainder ct) and 16-byte stores that voxelize_narrow_kernel needs, and the
  launch rule (tests/batch_cut_rows.py narrow_sub_tiles: mvx_slab.hip LaunchFn restated) then picks the sub-tiles per wave the row
  expects, also under the "narrow_sub" values the GPU test forces;
* the table reaches both sub-tile counts, every narrow chunk width and one, two and three waves per workgroup.
"""
import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import batch_cut_rows as B
from tests import f64_rows as F
from tests import narrow_rows as R


def _host_plan(row, batch=1, layout=_lib.MVX_LAYOUT_NCDHW):
    g = row.g
    return _lib.plan_call(g.D, row.cfg.nch, batch, total_atoms=batch * g.atoms, max_atoms=g.atoms, mode=row.cfg.mode, radii_type="scalar",
                          layout=layout)


@pytest.mark.parametrize("geom", list(R.GEOMS))
def test_geometry_reaches_the_line_forms_it_names(geom):
    g = R.GEOMS[geom]
    forms, lower, upper, xlower = R.geom_forms(geom)
    assert set(g.forms) <= forms, (geom, sorted(forms), int(lower.max()), int(upper.max()), int(xlower.max()))
    assert lower.shape == (g.D // F.SUBX, g.D // F.SUBY, 1) and g.D == F.SUBZ * g.nw  # one slab per row of voxels
    if "one_round" in g.forms:
        assert forms <= {"one_round", "empty"}


def test_the_figures_the_geometries_were_chosen_for():
    _, lower, upper, xlower = R.geom_forms("N32x")
    assert lower.max() >= 993 and xlower.max() >= 1235
    _, lower, upper, _ = R.geom_forms("N16x")
    assert lower.max() > 16 * 16  # rounds of 16 rows (one wave, two sub-tiles): more than sixteen of them
    _, lower, upper, _ = R.geom_forms("N32e")
    assert int(((lower > F.ONE_ROUND) & (upper <= F.LINE_CAP)).sum()) >= 28 and upper.max() <= F.LINE_CAP
    _, lower, upper, _ = R.geom_forms("N48o")
    assert upper.max() <= 18


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row_reaches_the_narrow_kernel(row):
    p = _host_plan(row, 64)  # many such molecules: the binned route by the plan's own choice
    assert {k: p[k] for k in row.plan} == row.plan, (row.id, p)
    n = R.narrow_plan(p)
    assert n["ct"] == row.ct and B.narrow_sub_tiles(n, 0, False) == row.nsub, (row.id, p)
    assert B.narrow_sub_tiles(n, 1, False) == 0  # "narrow_sub" = 1: voxelize_kernel's pair walk
    for nsub in row.forced:
        assert B.narrow_sub_tiles(n, nsub, False) == nsub, (row.id, nsub)
    # the GPU test's own calls - the molecule alone, and second of three - are small enough for the one-launch route, which the
    # test switches off (debug_option("direct", 0)) and then asserts the whole plan; the slab shape does not depend on the route
    for batch, extra in ((1, 0), (3, 35)):
        q = _lib.plan_call(row.g.D, row.cfg.nch, batch, total_atoms=row.g.atoms + extra, max_atoms=row.g.atoms, mode=row.cfg.mode)
        assert q["route"] in (_lib.MVX_ROUTE_BINNED, _lib.MVX_ROUTE_DIRECT)
        assert all(q[k] == row.plan[k] for k in ("nw", "nzc", "vec_store", "lane_range", "grouped")), (row.id, q)


@pytest.mark.parametrize("row", R.CL_ROWS, ids=R.CL_IDS)
def test_channels_last_row_reaches_the_narrow_kernel(row):
    p = _host_plan(row, layout=_lib.MVX_LAYOUT_NDHWC)
    assert (p["nw"], p["ct"], p["lane_range"], p["grouped"]) == (row.g.nw, row.ct, 0, 0), (row.id, p)
    want = 4 if row.ct == 1 and row.g.nw % 4 == 0 else 2  # (four sub-tiles per wave for one channel only)
    assert B.narrow_sub_tiles(p, 0, True) == want
    assert p["vec_store"] == {1: 1, 4: 1, 5: 0}[row.cfg.nch]  # (16-byte stores where every voxel's channel run is 16-byte aligned)


def test_the_table_covers_the_narrow_kernel():
    assert {(r.ct, r.nsub) for r in R.ROWS} == {(1, 2), (1, 4), (4, 2), (4, 4), (8, 2)}
    assert {(r.ct, n) for r in R.ROWS for n in r.forced} == {(1, 2), (1, 4), (4, 2), (4, 4), (8, 2)}
    assert {r.g.nw // r.nsub for r in R.ROWS} >= {1, 2, 3}  # waves per workgroup
    assert {r.cfg.density for r in R.ROWS if r.ct == 1} == {r.cfg.density for r in R.ROWS if r.ct == 4} == {"binary", "gaussian"}
    assert {r.ct for r in R.ROWS if r.cfg.nch > 32} == {1, 4}
    reached = set().union(*(R.geom_forms(g)[0] for g in R.GEOMS))
    assert reached >= {"one_round", "extension", "xlist", "xlist_long", "empty"}
    assert {(B.narrow_sub_tiles(_host_plan(r, layout=_lib.MVX_LAYOUT_NDHWC), 0, True), r.cfg.nch) for r in R.CL_ROWS} == \
        {(4, 1), (2, 4), (2, 5)}


def test_a_thinner_geometry_loses_its_form():
    """The form check can fail: N32x thinned until no slab passes 255 candidates no longer is an x-list geometry."""
    g, keep = R.GEOMS["N32x"], 300
    lower, upper, xlower = F.slab_counts(R.positions("N32x")[:keep], np.full(keep, g.radius), g.D, g.nw)
    assert upper.max() <= F.LINE_CAP
    assert not F.line_forms(lower, upper, xlower, g.nw, g.D) & {"xlist", "xlist_long"}
