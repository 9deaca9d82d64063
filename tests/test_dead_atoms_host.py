"""The rows of tests/dead_atom_rows.py are what they claim to be - shown on the CPU, so that tests/test_hip_dead_atoms.py's
"dirty equals clean" is a statement about the reference's own rule and about live atoms that contribute something.

For every row: the dead kinds and positions are all there; the oracle's grid of the dirty batch (oracle/c_oracle, oracle/numpy_port
at precision 64, at the posed positions) is bit for bit the grid of the clean batch, which is non-zero in every channel; the live
molecules have non-zero gradient bounds; and two mutated references have teeth: dead atoms replaced by atoms at the molecule's
centre change the oracle grid, and one live atom deleted exceeds the bars of tests/tolerance.py.

The view selection (tests/views_reference.keep_mask, the text of mvx_box_cull.inc) is the box cull alone, rule step 1: it rejects
every dead coordinate, a NaN radius and every type outside [0, C), in every view. An atom-wise radius of 0 or -1 or an infinite one
on an atom inside the box passes that cull (p + r > lb and p - r < ub hold) and is dropped by step 2, the radius test - so such an
atom may be listed by select_views, as the documented superset allows, and still reaches no voxel. Asserted as such below.
"""
import numpy as np
import pytest

from tests import dead_atom_rows as R
from tests import entry_fuzz_rows as E
from tests import grad_reference as gr
from tests import pose_reference as pr
from tests import views_reference as vr
from tests import hip_support as hip
from tests.tolerance import GAUSS_TOL, P64_TOL, gaussian_excess


def _grids(d, kinds=None):
    """The oracle's grids of a batch. kinds (the row's dead_kind, for the dirty batch): at precision 64 the atoms with an infinite
    radius are left out - oracle/numpy_port divides by the radius and so gives such an atom the whole grid, exp(0) = 1 in every
    voxel, where oracle/c_oracle and the library (d2_threshold / d2_threshold64: r < 3e38, r < 1e300) drop it;
    test_an_infinite_radius_at_precision_64_is_dead_in_the_library_only pins that difference."""
    p = R.positions_of(d)
    out = []
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        drop = kinds[lo:hi] == "r inf" if (kinds is not None and d["precision"] == 64) else np.zeros(hi - lo, bool)
        if drop.any():
            out.append(R.oracle_grid(d, p, b, xyz=p[lo:hi][~drop], w=R.weights_of(d)[lo:hi][~drop], r_atom=d["r_atom"][lo:hi][~drop]))
        else:
            out.append(R.oracle_grid(d, p, b))
    return out


def test_an_infinite_radius_at_precision_64_is_dead_in_the_library_only():
    from oracle import numpy_port

    spec = numpy_port.GridSpec(0.5, 16, None)
    with np.errstate(all="ignore"):
        g = numpy_port.voxelize(spec, np.zeros((1, 3)), np.ones((1, 1)), np.array([np.inf]), radii_type="atom-wise", density="gaussian",
                                sigma=0.5, precision=64)
    assert (g == 1.0).all()


def test_the_rows_cover_every_kind_position_placement_and_shape():
    seen = set()
    for rid in R.ROW_IDS:
        r = R.row(rid)
        d, c = R.dirty(r), R.clean(r)
        live = R.live(r)
        assert r["B"] * r["C"] * r["D"] ** 3 <= E.WALK_ELEMENTS
        assert c["sizes"] == R.LIVE and c["N"] == int(live.sum()) and d["N"] == live.shape[0]
        assert np.array_equal(d["xyz"][live], c["xyz"], equal_nan=True)
        if d["chan"] is not None:
            assert np.array_equal(d["chan"][live], c["chan"])
        if r["radii_type"] == "atom-wise":
            assert np.array_equal(d["radii"][live], c["radii"]) and np.all(np.isfinite(c["radii"]) & (c["radii"] > 0))
        assert np.all(np.isfinite(c["xyz"]))
        assert set(r["dead_kind"][~live]) == set(R.kinds_of(r["mode"], r["radii_type"], r["C"])), rid
        assert d["sizes"][R.EMPTY_MOL] == 0
        off = d["off"]
        if r["placement"] == "call_tail":
            assert not live[int(np.flatnonzero(live)[-1]) + 1:].any() and int(np.flatnonzero(~live)[0]) > int(np.flatnonzero(live)[-1])
            assert d["sizes"][:R.LAST_MOL] == R.LIVE[:R.LAST_MOL]
        else:
            assert d["sizes"][R.ALL_DEAD_MOL] == R.ALL_DEAD and not live[off[R.ALL_DEAD_MOL]:off[R.ALL_DEAD_MOL + 1]].any()
            assert d["sizes"][R.ALL_DEAD_MOL - 1] > 0 and d["sizes"][R.ALL_DEAD_MOL + 1] > 0
        for b, slots in R.SLOTS.items():
            m = live[off[b]:off[b + 1]]
            if r["placement"] == "scattered":
                assert [int(i) for i in np.flatnonzero(~m)] == [s % m.shape[0] for s in slots]
                assert m.shape[0] > 256 or b != 2
            elif r["placement"] == "tail":  # every live atom keeps its place in the molecule
                assert m[:R.LIVE[b]].all() and not m[R.LIVE[b]:].any() and m.shape[0] == R.LIVE[b] + len(slots)
        if r["posed"]:
            assert sorted({round(float(np.linalg.norm(q)), 6) for q in r["q"]}) == [0.8, 1.0, 1.25]
            assert np.array_equal(r["cen"] * 8, np.round(r["cen"] * 8))
        seen.add((r["mode"], r["radii_type"], r["kind"], r["placement"], r["C"], r["pose"] if isinstance(r["pose"], str) else "rot", r["D"]))
    assert {(m, rt) for m, rt, *_ in seen} == {("features", "scalar"), ("features", "atom-wise"), ("features", "channel-wise"),
                                               ("types", "scalar"), ("types", "atom-wise"), ("types", "channel-wise"),
                                               ("single", "scalar"), ("single", "atom-wise")}
    assert {s[2] for s in seen} == {"f32", "bf16", "f64"} and {s[3] for s in seen} == set(R.PLACEMENTS)
    assert {s[4] for s in seen} == {1, 5, 33} and {s[5] for s in seen} == {"posed", "centred", "rot"} and {s[6] for s in seen} == {16, 20}
    d20 = [R.row(i) for i in R.ROW_IDS if R.row(i)["D"] == 20]
    assert all((r["res"], r["blockdim"], r["sigma"]) == (0.4, 5, 0.3) and not E.sums_supported(20, 5) for r in d20)


@pytest.mark.parametrize("row_id", R.ROW_IDS)
def test_the_oracle_gives_the_clean_grid_for_the_dirty_batch_and_the_mutants_do_not(row_id):
    r = R.row(row_id)
    d, c = R.dirty(r), R.clean(r)
    dirty, clean = _grids(d, r["dead_kind"]), _grids(c)
    for b in range(r["B"]):
        assert hip.same_bits(dirty[b], clean[b]), (row_id, b)
        for ch in range(r["C"]):  # every channel that has a live atom (all of them: dead_atom_rows._live_channels)
            assert R.LIVE[b] == 0 or clean[b][ch].any(), (row_id, b, ch)
        if R.LIVE[b] == 0:
            assert not clean[b].any()

    # teeth 1: the dead atoms as ordinary atoms at their molecule's centre - weight one in every channel (features), type 0, the
    # row's scalar or channel radii or an atom-wise radius of 2 res - change the oracle's grid
    live = R.live(r)
    p = R.positions_of(d)
    changed = 0
    for b in range(r["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        dead = ~live[lo:hi]
        if not dead.any():
            continue
        xyz = p[lo:hi].copy()
        xyz[dead] = 0.0  # (the centre of the box is the posed centre of the molecule, the translation aside)
        w = R.weights_of(d)[lo:hi].copy()
        w[dead] = 1.0 if r["mode"] != "types" else 0.0
        if r["mode"] == "types":
            w[dead, 0] = 1.0
        ra = None
        if d["r_atom"] is not None:
            ra = d["r_atom"][lo:hi].copy()
            if r["radii_type"] == "atom-wise":
                ra[dead] = 2.0 * r["res"]
            elif r["mode"] == "types" and r["radii_type"] == "channel-wise":
                ra[dead] = float(r["radii"][0])
            if r["radii_type"] == "scalar":
                ra = None
        mutant = R.oracle_grid(d, p, b, xyz=xyz, w=w, r_atom=ra)
        assert not hip.same_bits(mutant, clean[b]) and np.abs(mutant.astype(np.float64) - clean[b]).max() > 0.1, (row_id, b)
        changed += 1
    assert changed >= 1

    # teeth 2: one live atom deleted - the one nearest the box centre with a weight in its first non-zero channel - fails the bars
    pc = R.positions_of(c)
    tol = P64_TOL if r["precision"] == 64 else GAUSS_TOL
    for b in range(r["B"]):
        lo, hi = int(c["off"][b]), int(c["off"][b + 1])
        if hi == lo:
            continue
        n = int(np.argmin(np.abs(pc[lo:hi]).max(axis=1)))
        keep = np.ones(hi - lo, bool)
        keep[n] = False
        ra = None if c["r_atom"] is None or r["radii_type"] == "scalar" else c["r_atom"][lo:hi][keep]
        mutant = R.oracle_grid(c, pc, b, xyz=pc[lo:hi][keep], w=R.weights_of(c)[lo:hi][keep], r_atom=ra)
        membership = np.not_equal(mutant != 0, clean[b] != 0).any()
        assert membership or gaussian_excess(mutant, clean[b], tol) > 1.0 or \
            (r["density"] == "binary" and not np.array_equal(mutant, clean[b])), (row_id, b)


@pytest.mark.parametrize("row_id", [i for i in R.ROW_IDS if R.row(i)["density"] == "gaussian"])
def test_every_live_molecule_has_gradient_bounds_to_compare_against(row_id):
    """With the row's field as the upstream: non-zero bounds for dL/dcoords and, posed, for each of dL/dc, dL/dq and dL/dt."""
    r = R.row(row_id)
    c = R.clean(r)
    F = E.field_of(c)
    p = R.positions_of(c)
    w, types = E.reference_channels(c)
    for b in range(r["B"]):
        lo, hi, radii = E.molecule(c, b)
        if hi == lo:
            continue
        o = gr.reference(p[lo:hi], F if F.ndim == 4 else F[b], radii, c["radii_type"], w=None if w is None else w[lo:hi], mode=c["mode"],
                         types=None if types is None else types[lo:hi], res=c["res"], sigma=c["sigma"], blockdim=c["blockdim"],
                         density=c["density"], precision=c["precision"])
        gp, bp = o["coords"]
        assert (bp > 0).any(axis=1).sum() >= (hi - lo) // 2, (row_id, b)
        if r["posed"]:
            pose = pr.pose_grads(c["xyz"][lo:hi], c["cen"][b], c["q"][b], gp, bp)
            for name in ("center", "quaternion", "translation"):
                assert np.all(pose[name][1] > 0) and np.all(pose[name][0] != 0), (row_id, b, name)


@pytest.mark.parametrize("row_id", [i for i in R.ROW_IDS if R.row(i)["posed"]])
def test_the_float64_pose_reference_of_the_dirty_batch_is_not_a_reference(row_id):
    """Why the reference of a dirty call is the reference of the clean call: a zero gradient row times a NaN coordinate."""
    r = R.row(row_id)
    d = R.dirty(r)
    b = int(np.searchsorted(d["off"], int(np.flatnonzero(~np.isfinite(d["xyz"]).all(axis=1))[0]), side="right") - 1)
    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    with np.errstate(all="ignore"):
        o = pr.pose_grads(d["xyz"][lo:hi], d["cen"][b], d["q"][b], np.zeros((hi - lo, 3)), np.zeros((hi - lo, 3)))
    assert np.isnan(o["quaternion"][0]).any()


@pytest.mark.parametrize("cloud_id", R.CLOUD_IDS)
def test_the_box_cull_of_every_view_drops_the_dead_atoms_it_can_see(cloud_id):
    c = R.cloud(cloud_id)
    d, k = R.dirty_cloud(c), R.clean_cloud(c)
    live = R.live(c)
    assert [int(i) for i in np.flatnonzero(~live)] == sorted(s % live.shape[0] for s in R.CLOUD_SLOTS)
    assert set(c["dead_kind"][~live]) == set(R.kinds_of(c["mode"], c["radii_type"], c["C"]))
    types = d["chan"] if c["mode"] == "types" else None
    nc = c["C"] if c["mode"] == "types" else None
    with np.errstate(all="ignore"):
        p = pr.view_positions(d["xyz"], d["cen"], d["q"], d["t"])
        keep = vr.keep_mask(p, c["res"], c["D"], R.view_source(c), d["radii"], c["precision"], types=types, num_channels=nc)
    assert keep.shape == (c["B"], d["N"])
    # rule step 1 alone: a radius of 0, -1 or inf inside the box passes the box cull and falls to the radius test (module docstring)
    by_radius = np.isin(c["dead_kind"], ["r 0", "r -1", "r inf"])
    assert not keep[:, ~live & ~by_radius].any()
    pk = pr.view_positions(k["xyz"], k["cen"], k["q"], k["t"])
    keep_clean = vr.keep_mask(pk, c["res"], c["D"], R.view_source(c), k["radii"], c["precision"],
                              types=k["chan"] if c["mode"] == "types" else None, num_channels=nc)
    assert np.array_equal(keep[:, live], keep_clean)
    assert (keep_clean.sum(1) > 20).all() and (keep_clean.sum(1) < k["N"]).all()  # the cull keeps some live atoms and drops some
    if by_radius.any():  # ... and those atoms reach no voxel in any view: the oracle's grid of each of them alone is empty
        from oracle import c_oracle

        assert c["precision"] == 32
        for n in np.flatnonzero(by_radius):
            for b in range(c["B"]):
                with np.errstate(all="ignore"):
                    g = c_oracle.voxelize(p[b, n:n + 1], np.ones((1, 1), np.float32), d["radii"][n:n + 1], resolution=c["res"],
                                          dimension=c["D"], blockdim=c["blockdim"], radii_type="atom-wise", density="gaussian",
                                          sigma=c["sigma"])
                assert not g.any(), (cloud_id, int(n), b)
