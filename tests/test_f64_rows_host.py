"""Host half of tests/test_hip_f64_sweep.py: no GPU, nothing is launched.

* every row of tests/f64_rows.py reaches the kernel it names (mvx_plan_call: route, ct, ncc, nw, nzc, vec_store, lane range);
* its molecule reaches the line form it names - one round, extension line, x-list, an x-list beyond xbin_kernel's LDS copy - by
  two host-side bounds on the candidates per slab, so that neither a plan change nor a thinner geometry can empty the sweep;
* every instantiation for_kernel64 / launch_mx64 can reach has a row on a geometry that leaves the one-round case;
* ct = 32 comes with the matrix-core route only (why there is no OpsF64<32, ...>).
"""
import itertools

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import f64_rows as R


def _host_plan(row, aligned=None):
    g = row.g
    return _lib.plan_call(g.D, row.nch, 1, total_atoms=g.atoms, mode=row.mode, radii_type=row.radii, precision=64,
                          blockdim=row.blockdim or 8, out_aligned16=(g.vec_store == 1) if aligned is None else aligned)


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row_reaches_the_kernel_and_the_line_form_it_names(row):
    p = _host_plan(row)
    assert {k: p[k] for k in row.plan} == row.plan, (row.id, p)
    assert p["grouped"] == 0 and p["nchunk"] == 1
    assert (p["route"] == R.F64_MX) == (row.C > 16 and not row.chanwise and row.mode != "single")
    if row.geom == "E":  # odd D: no 16-byte stores whatever the alignment; slice 1 of a batch grid is 8 bytes off
        assert _host_plan(row, aligned=True)["vec_store"] == 0 and (row.nch * row.g.D ** 3) % 2 == 1
    else:
        assert _host_plan(row, aligned=False)["vec_store"] == 0  # (what the plan would say of a misaligned grid)
    forms, lower, upper, xlower = R.row_forms(row)
    assert set(row.g.forms) <= forms, (row.id, sorted(forms), int(lower.max()), int(upper.max()), int(xlower.max()))
    if "one_round" in row.g.forms:
        assert forms == {"one_round"} or forms == {"one_round", "empty"}
    if row.g.nzc == 2:  # 8 + 1 sub-tiles: the second chunk holds one sub-tile
        assert -(-row.g.D // R.SUBZ) == 9 and row.g.nw == 8
    mol = R.make_molecule(row)
    r = R.cull_radii(row, mol)
    assert r.max() == row.g.radius and r.min() >= 0.8 * row.g.radius


def test_the_table_covers_what_the_dispatch_can_reach():
    assert 40 <= len(R.ROWS) <= 60
    # for_kernel64: CT x GAUSS x {(CHANWISE, LANE_RANGE)}; launch_voxelize64 forces LANE_RANGE for channel-wise radii
    dense = set(itertools.product((1, 4, 8, 16), (True, False), ((False, False), (False, True), (True, True))))
    mx = set(itertools.product((True, False), (False, True)))
    seen_dense, seen_mx, seen_alt = set(), set(), set()
    for row in R.ROWS:
        forms = R.row_forms(row)[0]
        if not forms & {"extension", "xlist"}:
            continue
        gauss = row.density == "gaussian"
        if row.route == R.F64_DENSE:
            seen_dense.add((row.ct, gauss, (row.chanwise, bool(row.chanwise or row.lane_range))))
        else:
            seen_mx.add((gauss, bool(row.lane_range)))
            seen_alt.add((16, gauss, (False, bool(row.lane_range))))  # the same call under max_ct64 = 16
    assert seen_dense == dense and seen_mx == mx and seen_alt <= dense
    mx_rows = [r for r in R.ROWS if r.route == R.F64_MX]
    assert {r.C for r in mx_rows} == {17, 32, 33, 40, 64} and {r.ncc for r in mx_rows} == {1, 2}
    assert {r.ncc16 for r in mx_rows} == {2, 3, 4}
    assert {r.blockdim for r in R.ROWS} >= {None, 5, 12} and any(r.blockdim == r.g.D for r in R.ROWS)
    assert {r.mode for r in R.ROWS} == {"features", "types", "single"}
    assert {r.radii for r in R.ROWS} == {"scalar", "atom-wise", "channel-wise"}
    for geom in R.GEOMS:  # test_row_in_a_batch: one row per geometry and route
        assert {r.route for r in R.BATCH_ROWS if r.geom == geom} == {R.F64_DENSE, R.F64_MX}, geom
    # every line form is reached on both routes
    for route in (R.F64_DENSE, R.F64_MX):
        reached = set().union(*(R.row_forms(r)[0] for r in R.ROWS if r.route == route))
        assert reached >= {"one_round", "extension", "xlist", "xlist_long", "empty", "half_empty_chunk"}, route


def test_a_thinner_geometry_loses_its_form():
    """The form check can fail: geometry A thinned until no slab passes 255 candidates no longer is an x-list geometry."""
    row = R.ROWS[0]
    assert row.geom == "A" and set(row.g.forms) <= R.row_forms(row)[0]
    g, keep = row.g, 300
    lower, upper, xlower = R.slab_counts(R.positions("A")[:keep], np.full(keep, g.radius), g.D, g.nw)
    assert upper.max() <= R.LINE_CAP
    forms = R.line_forms(lower, upper, xlower, g.nw, g.D)
    assert not forms & {"xlist", "xlist_long"} and not set(g.forms) <= forms


def test_the_bounds_bracket_a_brute_force_count():
    """slab_counts against both rules spelled out voxel by voxel on a small case: upper is the count of atoms whose window of
    voxel indices meets the slab; lower is at least the count of atoms that really hold a voxel centre of the slab inside their
    sphere (such a sphere reaches the slab's box) and at most upper."""
    rng = np.random.default_rng(3)
    D, nw, n = 17, 3, 60
    half = R.RES * (D - 1) / 2
    xyz = rng.uniform(-half - 1, half + 1, (n, 3))
    r = rng.uniform(0.5, 1.6, n)
    axis = np.arange(D) * R.RES - half
    for bd in (D, 5, 8):  # one reference block; blocks that cut sub-tiles; the default
        nb = -(-D // bd)
        bounds = [axis[b * bd] + R.RES / 2 for b in range(1, nb)]  # numpy/voxelizer.py:55
        blk = np.arange(D) // bd
        lower, upper, _ = R.slab_counts(xyz, r, D, nw, bd)
        owns = np.zeros(lower.shape, np.int64)  # atoms with an admitted voxel centre of the slab inside their sphere
        box = np.zeros(lower.shape, np.int64)  # atoms whose box of admitted voxel indices meets the slab
        for a in range(n):
            inside = []
            for k in range(3):
                p = xyz[a, k]
                admits = np.array([(b == 0 or p > bounds[b - 1] - r[a]) and (b == nb - 1 or p < bounds[b] + r[a]) for b in range(nb)])
                inside.append((np.abs(axis - p) <= r[a] * 1.000001 + 1e-9) & admits[blk])
            d2 = ((axis[:, None, None] - xyz[a, 0]) ** 2 + (axis[None, :, None] - xyz[a, 1]) ** 2) + (axis[None, None, :] - xyz[a, 2]) ** 2
            hit = (d2 <= r[a] ** 2 * (1 - 1e-8)) & inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]
            for sx, sy, sz in np.ndindex(*lower.shape):
                sl = (slice(2 * sx, 2 * sx + 2), slice(4 * sy, 4 * sy + 4), slice(8 * nw * sz, 8 * nw * (sz + 1)))
                owns[sx, sy, sz] += bool(hit[sl].any())
                box[sx, sy, sz] += bool(inside[0][sl[0]].any() and inside[1][sl[1]].any() and inside[2][sl[2]].any())
        assert np.array_equal(upper, box), bd
        assert (owns <= lower).all() and (lower <= upper).all() and owns.sum() > 0, bd


def test_chunks_of_32_channels_come_with_the_matrix_core_route_only():
    """There is no OpsF64<32, ...> (for_kernel64 names CT 1 / 4 / 8 / 16 only): the plan gives ct = 32 at precision 64 only on the
    matrix-core route, whose slabs have at most 8 waves (launch_voxelize64 then takes launch_mx64: not channel-wise, NW <= 8)."""
    n32 = 0
    for D, C_, radii, mode, bd in itertools.product((5, 16, 24, 33, 64, 72, 130, 1020), (1, 4, 16, 17, 32, 33, 64, 200),
                                                    ("scalar", "atom-wise", "channel-wise"), ("features", "types"), (8, 5)):
        p = _lib.plan_call(D, C_, 3, total_atoms=100, mode=mode, radii_type=radii, precision=64, blockdim=bd)
        chanwise = radii == "channel-wise" and mode == "features"
        assert (p["ct"] == 32) == (p["route"] == R.F64_MX) == (C_ > 16 and not chanwise), (D, C_, radii, mode, p)
        assert p["ct"] in (1, 4, 8, 16, 32) and p["nw"] <= 8 and p["grouped"] == 0
        n32 += p["ct"] == 32
    assert n32 > 100
