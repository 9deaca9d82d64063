"""Host half of tests/test_hip_sum_sweep.py: no GPU, nothing is launched.

* nw_nzc() of tests/sum_sweep_rows.py is the library's own plan of a 32-channel binned call (mvx_plan_call), row by row and over
  a range of dimensions;
* every row reaches what its `reaches` column says - per molecule and per z chunk, from the two bounds on the candidates per slab
  of tests/f64_rows.slab_counts with the row's blockdim: a lower bound proves that a form is reached, an upper bound that a line
  stays under a cap;
* the rows with D % 8 == 4 have an atom that is a candidate of a slab in the last y row and reaches the last z sub-tile;
* a thinned `tall` fails `tall`'s conditions, so the check can fail;
* the 48 random draws jointly reach every D, every C, every weight kind and a slab over 63 candidates.
"""
import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import sum_sweep_rows as S
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)

ONE, CAP = S.ONE_ROUND, S.LINE_CAP
Z_CHUNKS = {"cut96": (0, 1), "cut132": (0, 1), "cut144": (1, 2)}  # the z chunks condition Z names


def _plan(row, B=None):
    return _lib.plan_call(row.D, 32 * -(-row.C // 32), len(row.sizes) if B is None else B, total_atoms=10 ** 8, mode="features",
                          blockdim=row.blockdim or 8)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_the_rows_plan_is_the_librarys(row_id):
    row = S.BY_ID[row_id]
    p = _plan(row)
    assert p["route"] == _lib.MVX_ROUTE_BINNED and p["ct"] == 32 and p["ct_rem"] == 0 and p["vec_store"] == 1 and p["lane_range"] == 0, p
    assert (p["nw"], p["nzc"]) == S.nw_nzc(row.D) and p["ncc"] == -(-row.C // 32), (p, S.nw_nzc(row.D))
    assert (p["nsx"], p["nsy"]) == (-(-row.D // 2), -(-row.D // 4))
    _fake(dimension=row.D, blockdim=row.blockdim or 8, radii_type=row.radii_type)._sum_guard(None)  # the Python layer serves it


def test_the_table_reaches_the_plans_the_issue_names():
    got = {r.id: S.nw_nzc(r.D) for r in S.ROWS}
    assert got == {"tall": (9, 1), "cut96": (8, 2), "cut132": (9, 2), "cut144": (8, 3), "edge20": (3, 1), "edge20d": (3, 1),
                   "edge12": (2, 1), "edge44": (6, 1), "bd16": (5, 1), "bd16u": (3, 1), "bd24": (3, 1)}
    # the last z chunk: D = 96 four of eight waves, D = 132 eight of nine, D = 144 two of eight
    assert [-(-D // 8) - nw * (nzc - 1) for D, (nw, nzc) in ((96, got["cut96"]), (132, got["cut132"]), (144, got["cut144"]))] == [4, 8, 2]
    assert S.R.nw_of(S.R.Row("x", 132, *[None] * 9)) == 8  # (why sum_rows.nw_of does not serve here: it stops at 16 sub-tiles)
    for r in S.ROWS:
        assert r.D % 4 == 0 and r.id not in S.R.ROW_IDS
    assert [r.id for r in S.ROWS if r.D % 8 == 4] == ["cut132", "edge20", "edge20d", "edge12", "edge44"]
    assert {r.blockdim for r in S.ROWS} == {None, 16, 24}


def test_nw_nzc_restates_plan_slabs_for_every_dimension_a_sum_serves():
    for D in range(4, 260, 4):
        p = _lib.plan_call(D, 32, 3, total_atoms=10 ** 8, mode="features")
        assert p["route"] == _lib.MVX_ROUTE_BINNED and (p["nw"], p["nzc"]) == S.nw_nzc(D), (D, p)


# ---- the molecules -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_the_batch_is_sum_rows_batch_with_the_z_offset(row_id):
    d = S.make(row_id)
    row = d["row"]
    assert row is S.BY_ID[row_id] and d["B"] == len(row.sizes) and d["N"] == sum(row.sizes)
    assert d["xyz"].shape == (d["N"], 3) and d["off"][-1] == d["N"] and d["cen"].shape == (d["B"], 3)
    assert np.abs(d["cen"]).max() > 5.0  # (the centres matter: the merged molecule is not the coordinates themselves)
    base = S.R.make(row_id)
    assert np.array_equal(d["xyz"][:, :2], base["xyz"][:, :2]) and np.array_equal(d["xyz"][:, 2], base["xyz"][:, 2] + row.zshift)
    assert all(d[k] is base[k] for k in ("off", "cen", "chan", "radii", "r_atom"))
    assert d["r_atom"].min() >= 0.8 and d["r_atom"].max() <= 1.6


# ---- what every row must reach -----------------------------------------------------------------------------------------------
def _mol(d, b):
    lower, upper, xlower = S.molecule_counts(d, b)
    return lower, upper, xlower


def _extension(lower, upper):
    """A slab over 63 candidates and none over 255: rounds over the line and its extension, no x-list."""
    return lower.max() > ONE and upper.max() <= CAP


def tall_conditions(d):
    (l0, u0, _), (l1, _, _), (_, _, x2) = (_mol(d, b) for b in range(3))
    return {"molecule 0: extension": _extension(l0, u0), "molecule 1: x-list": l1.max() > CAP, "molecule 2: x-list over 1024": x2.max() > S.XL_LDS}


def test_tall_runs_the_1024_thread_form_past_one_round():
    d = S.make("tall")
    assert S.nw_nzc(72) == (9, 1) and d["row"].C == 32 and d["row"].radii_type == "atom-wise"
    assert 1.35 <= d["r_atom"].min() and d["r_atom"].max() <= 1.5
    got = tall_conditions(d)
    assert all(got.values()), got


def test_a_thinned_tall_fails_its_conditions():
    """The check can fail: every tenth atom of `tall` reaches none of the three forms."""
    d = S.make("tall")
    keep = np.concatenate([np.arange(lo, hi)[::10] for lo, hi in zip(d["off"][:-1], d["off"][1:])])
    sizes = [len(np.arange(lo, hi)[::10]) for lo, hi in zip(d["off"][:-1], d["off"][1:])]
    thin = dict(d, N=len(keep), off=np.concatenate([[0], np.cumsum(sizes)]), xyz=d["xyz"][keep], chan=d["chan"][keep],
                radii=d["radii"][keep], r_atom=d["r_atom"][keep])
    assert sizes == [30, 70, 220]
    got = tall_conditions(thin)
    assert not any(got.values()), got


@pytest.mark.parametrize("row_id", list(Z_CHUNKS))
def test_cut_rows_have_the_extension_and_the_x_list_in_every_named_z_chunk(row_id):
    d = S.make(row_id)
    nw, nzc = S.nw_nzc(d["row"].D)
    l0, u0, _ = _mol(d, 0)
    l1, _, _ = _mol(d, 1)
    assert l0.shape[2] == nzc > 1
    for zc in Z_CHUNKS[row_id]:
        assert _extension(l0[:, :, zc], u0[:, :, zc]), (zc, int(l0[:, :, zc].max()), int(u0[:, :, zc].max()))
        assert l1[:, :, zc].max() > CAP, (zc, int(l1[:, :, zc].max()))
    _, up, _ = S.counts(d, 0, d["N"])
    if row_id == "cut144":  # chunk 0: slabs without any candidate, in the whole batch
        assert (up[:, :, 0] == 0).any() and (up[:, :, 1] > 0).any() and (up[:, :, 2] > 0).any()
    # the cluster sits on the cut: voxel nw * 8 * zc of the last named chunk
    half = S.RES * (d["row"].D - 1) / 2
    assert d["row"].zshift == 8 * nw * Z_CHUNKS[row_id][-1] * S.RES - half


def test_edge20_has_light_lines_everywhere_and_reaches_the_last_voxels():
    d = S.make("edge20")
    row = d["row"]
    p = _plan(row)
    assert (p["nw"], p["nsy"], p["ncc"]) == (3, 5, 2) and d["B"] == 6
    for b in range(d["B"]):
        assert _mol(d, b)[1].max() <= ONE
    lower, _, _ = S.counts(d, 0, d["N"])
    assert lower.min() > 0  # every slab has a candidate
    half = S.RES * (row.D - 1) / 2
    rr = d["r_atom"] * 1.000001 + 1e-9
    hi = np.floor((S.merged(d) + rr[:, None] + half) / S.RES)
    assert (hi >= row.D - 1).any(axis=0).all()  # on each axis an atom whose box reaches the last voxel


def test_edge20d_has_the_extension_and_the_x_list():
    d = S.make("edge20d")
    (_, u0, _), (l1, u1, _), (l2, _, _) = (_mol(d, b) for b in range(3))
    assert u0.max() <= ONE and _extension(l1, u1) and l2.max() > CAP, (int(u0.max()), int(l1.max()), int(u1.max()), int(l2.max()))
    assert d["r_atom"].max() <= 1.5 and S.nw_nzc(20) == (3, 1)


def test_edge12_has_empty_molecules_first_and_in_the_middle():
    d = S.make("edge12")
    p = _plan(d["row"])
    assert (p["nw"], p["nsx"], p["nsy"]) == (2, 6, 3)
    assert list(np.diff(d["off"])) == [0, 30, 30, 0, 30]
    assert d["row"].mode == "types" and d["row"].density == "binary" and d["radii"].shape == (8,)
    assert S.counts(d, 0, d["N"])[0].min() > 0


def test_edge44_has_the_extension_and_a_slab_near_the_line_cap():
    d = S.make("edge44")
    (l0, u0, _), (l1, u1, _) = (_mol(d, b) for b in range(2))
    assert S.nw_nzc(44) == (6, 1) and _plan(d["row"])["ncc"] == 2
    assert _extension(l0, u0) and l0.max() < 128, (int(l0.max()), int(u0.max()))
    assert _extension(l1, u1) and l1.max() >= 200, (int(l1.max()), int(u1.max()))  # within the last quarter of the line's extension


@pytest.mark.parametrize("row_id", ["edge20", "edge20d", "edge12", "edge44"])
def test_edge_rows_have_a_candidate_in_the_last_y_row_and_the_half_sub_tile(row_id):
    d = S.make(row_id)
    assert d["row"].D % 8 == 4
    assert S.reaches_the_partial_corner(d) > 0
    empty = dict(d, xyz=d["xyz"] - np.array([0.0, 3.0, 3.0]))  # (the count can be zero: the same atoms 3 A further in)
    assert S.reaches_the_partial_corner(empty) < S.reaches_the_partial_corner(d)


@pytest.mark.parametrize("row_id, blocks", [("bd16", (16, 16, 8)), ("bd16u", (16, 8))])
def test_blockdim_16_rows_have_windows_cut_by_the_admitted_blocks(row_id, blocks):
    d = S.make(row_id)
    row = d["row"]
    assert row.blockdim == 16 and tuple(min(16, row.D - 16 * b) for b in range(-(-row.D // 16))) == blocks
    assert _plan(row)["lane_range"] == 0
    for b in range(d["B"]):
        assert S.window_cut_by_blocks(d, b) > 0, b
    # ... which blockdim 8 would cut elsewhere and one block nowhere
    assert S.window_cut_by_blocks(dict(d, row=row._replace(blockdim=row.D)), 0) == 0


def test_bd24_is_one_block():
    d = S.make("bd24")
    row = d["row"]
    assert row.blockdim == row.D == 24 and -(-row.D // row.blockdim) == 1 and row.density == "binary" and row.radii_type == "atom-wise"
    assert all(S.window_cut_by_blocks(d, b) == 0 for b in range(3))
    assert S.window_cut_by_blocks(dict(d, row=row._replace(blockdim=None)), 0) > 0  # (blocks of 8 would cut)


# ---- the random draws --------------------------------------------------------------------------------------------------------
def test_the_draws_jointly_reach_every_dimension_channel_count_and_weight_kind():
    assert len(S.SWEEP_SEEDS) == len(set(S.SWEEP_SEEDS)) == 48
    cov = S.sweep_coverage()
    assert cov["D"] == set(S.SWEEP_D) and cov["C"] == set(S.SWEEP_C) and cov["weights"] == {None, "mol", "atom+"}, cov
    assert cov["K"] == {1, 2, 5} and cov["accumulate"] == {False, True} and cov["blockdim"] == {None, 16, "one"}, cov
    assert cov["over_one_round"], cov
    for s in S.SWEEP_SEEDS:
        x = S.draw(s)
        row = x.row
        assert (row.mode, row.radii_type) in S.SERVED and 1 <= len(row.sizes) <= 9 and (row.spread == 1.0) == (s % 4 == 0)
        assert max(row.sizes) <= 120 + S.R.BAD_TYPE_ATOM + 1 and min(row.sizes) >= 0
        p = _plan(row)
        assert p["route"] == _lib.MVX_ROUTE_BINNED and p["lane_range"] == 0 and (p["nw"], p["nzc"]) == S.nw_nzc(row.D), (s, p)
        _fake(dimension=row.D, blockdim=row.blockdim or 8, radii_type=row.radii_type)._sum_guard(None)
