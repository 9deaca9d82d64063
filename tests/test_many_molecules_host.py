"""The cases of tests/test_hip_many_molecules.py checked on the host with the references alone (no GPU): the ladders hold what
they claim, the sample touches what it claims and the reference is non-zero there, the cuts partition the batch, the element
counts of the wide buffers are the powers of two named, and the budgets of the cut forward calls give the chunk counts claimed.
These are conditions on the inputs, not measurements."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cut_rows as R
from tests import many_molecules_rows as M

BOUNDARY_SIZES = {63, 64, 65, 255, 256, 257, 511, 512, 513}


@pytest.mark.parametrize("ladder, boundary", [(tuple(M.LADDER), BOUNDARY_SIZES), (tuple(M.THIN_LADDER), {63, 64, 65})],
                         ids=["ladder", "thin"])
def test_the_ladders_hold_what_they_claim(ladder, boundary):
    sizes = M.ladder_sizes(ladder)
    assert len(sizes) == M.B_LADDER == 3 * 64 + 11
    assert sizes[0] == 0 and sizes[-1] == 0
    runs = M.empty_runs(sizes)
    assert any(hi - lo + 1 >= 2 for lo, hi in runs)  # back-to-back empties
    assert boundary <= set(sizes) and {1, 2, 5} <= set(sizes)
    total = int(sum(sizes))
    assert (30000 < total < 36000) if len(ladder) == 17 else (3500 < total < 5000), total


def test_the_sample_rule():
    sizes = M.ladder_sizes(M.LADDER)
    mols = M.sample_molecules(sizes)
    assert len(mols) >= 40 and all(sizes[b] > 0 for b in mols)
    assert set(sizes[b] for b in mols) == set(sizes) - {0}  # every ladder size
    for lo, hi in M.empty_runs(sizes):
        assert lo == 0 or lo - 1 in mols
        assert hi == len(sizes) - 1 or hi + 1 in mols
    # (molecule 192 = 3 * 64 is empty, the first of a run: its exact zeros are checked with every empty molecule's, and its
    # neighbours 191 and 194 are in the sample)
    assert all(b in mols or sizes[b] == 0 for b in M.FIXED_MOLECULES) and [b for b in M.FIXED_MOLECULES if sizes[b] == 0] == [192]
    assert {191, 194} <= set(mols)
    full = [b for b, n in enumerate(sizes) if n]
    assert full[0] in mols and full[-1] in mols
    atoms = sum(len(M.sample_atoms(sizes[b])) for b in mols)
    assert atoms <= 2500, atoms
    assert np.array_equal(M.sample_atoms(65), np.arange(65))
    assert M.sample_atoms(513).tolist() == [0, 1, 2, 63, 64, 65, 255, 256, 257, 510, 511, 512]
    assert M.sample_atoms(300).tolist() == [0, 1, 2, 63, 64, 65, 255, 256, 257, 297, 298, 299]
    whole = M.whole_molecules(sizes)
    assert sorted(sizes[b] for b in whole) == sorted(set(sizes) - {0})


def test_the_rows_of_the_issue_are_present():
    have = {(r.entry, r.mode, r.C, r.radii, r.density, r.kind, r.transform) for r in M.ROWS}
    want = {("backward", "features", 33, "scalar", "gaussian", "f32", "pose"),
            ("backward", "features", 33, "channel-wise", "gaussian", "bf16", "rotation"),
            ("backward", "types", 5, "atom-wise", "gaussian", "f64", "pose"),
            ("backward", "single", 1, "scalar", "binary", "f32", "none"),
            ("backward_radii", "features", 5, "atom-wise", "gaussian", "f32", "pose"),
            ("score", "features", 33, "channel-wise", "gaussian", "f32", "pose"),
            ("score", "types", 5, "atom-wise", "binary", "bf16", "rotation"),
            ("score", "single", 1, "scalar", "gaussian", "f64", "pose"),
            ("pose", "features", 4, "scalar", "gaussian", "f32", "pose"),
            ("pose", "features", 4, "scalar", "gaussian", "f64", "pose"),
            ("forward", "features", 33, "scalar", "gaussian", "f32", "pose"),
            ("forward", "types", 4, "scalar", "gaussian", "f32", "pose")}
    assert want <= have
    assert {r.device_pose for r in M.FORWARD_ROWS if r.mode == "features"} == {True, False}
    assert {r.device_pose for r in M.FORWARD_ROWS if r.mode == "types"} == {True, False}
    assert {(r.radii, r.kind, r.mode) for r in M.SUM_ROWS} == {("scalar", "f32", "features"), ("channel-wise", "f64", "features"),
                                                              ("channel-wise", "f32", "types")}


@pytest.mark.parametrize("row", M.GRAD_ROWS, ids=M.GRAD_IDS)
def test_the_reference_is_non_zero_on_the_sample(row):
    """More than 30 % of the sampled atoms (the condition tests/test_hip_score.py uses) and every sampled whole molecule. A
    binary-density backward row has zero coordinate gradients by definition: there the share is taken on the atoms' scores
    against the same upstream, which are non-zero exactly where the atom reaches a voxel."""
    d = M.row_batch(row)
    ref = M.row_reference(row)
    assert d["chan"] is None or row.mode != "types" or (np.any(d["chan"] >= row.C) == row.beyond)
    if row.entry == "pose":
        assert len(ref["whole"]) == len(set(d["sizes"]) - {0})
        for b, o in ref["whole"].items():
            for name in ("center", "quaternion", "translation"):
                assert np.all(o[name][0] != 0) or d["sizes"][b] < 5, (b, name)
        return
    live = total = 0
    for b, (sel, o) in ref["atoms"].items():
        assert len(sel) == len(M.sample_atoms(int(d["sizes"][b]))) or b in ref["whole"]
        if row.entry == "score":
            rows = o[0]
        elif row.density == "binary":
            rows = M.score_rows(d, b, M.field_of(d, b), row.density, sel)[0]
        else:
            rows = np.abs(o["coords"][0]).sum(1)
        live += int(np.count_nonzero(rows))
        total += len(sel)
    assert total <= 2500 + sum(int(d["sizes"][b]) for b in ref["whole"])
    assert live > 0.3 * total, (live, total)
    for b, s in ref["whole"].items():
        assert s[2] != 0.0, b  # (every sampled whole molecule scores)


@pytest.mark.parametrize("row", M.SUM_ROWS, ids=M.SUM_IDS)
def test_the_call_wide_sums_are_non_zero(row):
    ref = M.sum_reference(row)
    assert set(ref) == {"scalar": {"sigma", "radius"}, "channel-wise": {"radii", "sigma"} if row.entry == "density" else {"radii"}}[row.radii]
    for k, (g, b) in ref.items():
        assert np.all(np.asarray(g) != 0) and np.all(np.asarray(b) > 0), k


def test_the_cuts_partition_the_batch():
    assert M.CUTS[0] == 0 and M.CUTS[-1] == M.B_LADDER and len(M.CUTS) == 7
    assert all(a < b for a, b in zip(M.CUTS, M.CUTS[1:]))
    assert {1, 2} <= {b - a for a, b in zip(M.CUTS, M.CUTS[1:])}
    sizes = M.huge_sizes()
    assert len(sizes) == M.HUGE_B and sizes[0] == 0 and sizes.max() == 5 and np.array_equal(sizes, (np.arange(M.HUGE_B) * 7) % 6)
    for lo, hi in M.HUGE_WINDOWS:
        assert 0 <= lo < hi <= M.HUGE_B
    assert M.HUGE_WINDOWS[0][0] == 0 and M.HUGE_WINDOWS[-1][1] == M.HUGE_B
    assert M.HUGE_WINDOWS[1][0] < 65535 < 65536 < M.HUGE_WINDOWS[1][1]
    picks = M.huge_molecules(sizes)
    assert set(M.HUGE_PICKS) <= set(picks) and any(sizes[b] > 0 for b in picks)
    for b in M.HUGE_PICKS:
        if sizes[b] == 0:
            assert any(sizes[n] > 0 and abs(n - b) <= 2 for n in picks)
    assert (M.HUGE_B + 63) // 64 == 1094  # workgroups of pose_resolve_kernel
    assert all(v < R.MAX_OUTPUT_BYTES for v in M.huge_bytes().values())


def test_the_tiny_totals():
    for total in M.TINY_TOTALS:
        sizes = M.tiny_sizes(total)
        assert len(sizes) == 3 and sum(sizes) == total and 0 in sizes
    assert {t for t in M.TINY_TOTALS if t < 32} and 32 in M.TINY_TOTALS and 33 in M.TINY_TOTALS


@pytest.mark.parametrize("case", M.WIDE, ids=M.WIDE_IDS)
def test_the_wide_buffers_pass_the_powers_of_two_named(case):
    per = case.C * case.D**3
    assert 256 * per == 1 << 31 and 512 * per == 1 << 32
    size = {"bf16": 2, "f32": 4}[case.kind]
    assert abs(case.B * per * size / 1e9 - 8.6) < 0.05
    if case.kind == "bf16":
        assert case.B == 513 and {511, 512} <= set(case.picks)
    else:
        assert case.B == 257 and 128 * per * 4 == 1 << 32 and 256 * per * 4 == 1 << 33
    assert {0, 127, 128, 255, 256} <= set(case.picks) and max(case.picks) < case.B
    d = M.wide_batch(case)
    half = M.RES * (case.D - 1) / 2.0
    for m in case.picks:  # all atoms but the first lie inside the box: every checked molecule's gradients are about something
        p = M.positions(d, m, m + 1)
        assert len(p) == case.atoms and np.all(np.abs(p[1:]) < half) and np.any(np.abs(p[0]) > half + 2.0), m


def test_the_record_layout_the_tests_build_by_hand():
    from molvoxel_amd.voxelizer.hip import _lib

    XF = M.XF
    assert XF.itemsize == C.sizeof(_lib.MvxXform) == 80
    for name in ("center", "quat", "trans", "flags", "center_ptr"):
        assert XF.fields[name][1] == getattr(_lib.MvxXform, name).offset, name


@pytest.mark.parametrize("row", M.CUT_ROWS, ids=M.CUT_IDS)
def test_the_budgets_give_the_chunk_counts_claimed(row):
    sizes = R.RAGGED_SIZES
    B, total = len(sizes), int(sum(sizes))
    p = R.host_plan(row, sizes)
    assert {k: p[k] for k in row.plan} == row.plan, p
    assert R.expected_nchunk(p, B, row.C, total) == 1  # uncut without options
    for n, kb in M.cut_budgets(row).items():
        assert R.expected_nchunk(p, B, row.C, total, 32, kb, 0) == n, (n, kb)
    assert R.expected_nchunk(p, B, row.C, total, 32, 0, 3) == 3
    d = M.cut_batch(row.id)
    assert d["B"] == 16 and d["N"] == total and d["sizes"][R.DENSE] == max(sizes)
    assert all(sizes[b] > 0 for b in M.CUT_ORACLE_MOLECULES)
