"""Torsion coordinates on the GPU (apply_torsions, score_hessian_flex_posed_batch, flex_lm_step, refine_flex_posed_batch) on the
rows of tests/flex_rows.py: four cases with D = 16 at resolution 0.5 - base (features, 14 / 0 / 9 atoms with 4 / 0 / 2 torsions,
one branch, nesting depth 3), long (300 atoms, one torsion turning 150: past one round of the 256-lane loop), deep (a 35-atom chain
with 32 torsions: the top mask bit, the largest LDS system) and binary (zeros but scores).

To the bit: G[:, :6], H[:, :6, :6], the scores and the per-atom rows against score_hessian_posed_batch; T = 0 against it entirely;
H against its transpose; two runs; a molecule alone and in its batch; inert torsions (padding, an index of N_b, coincident axis
atoms) and an atom with a NaN coordinate against the call without them; apply_torsions on zero angles and untouched atoms;
flex_lm_step with T = 0 against lm_step on every row of tests/lm_rows.py, and its decisions, counters and copies against the
reference for T = 1, 4, 32.
Within a bar: G and H against tests/flex_reference.py fed the device's own atom_pos, atom_grad and atom_hess, (N_b + 128) 2^-53
times the bound (float64 sums of at most N_b terms with under 128 roundings per term and in the assembly); against the reference
fed tests/hessian_reference.py's rows, GRAD_REL * bound + GRAD_ABS (GRAD64_* at precision 64); apply_torsions against the
reference and the distances inside every rigid part of a moving set, 64 T 2^-53 L; the residual of the step, four times np.linalg.solve's own.
The refinement: 8 starts of the 14-atom molecule against its own grid, torsions off by 10 - 15 degrees and the pose by 5 degrees
and 0.2 A; the accepted score never decreases and every start ends above refine_posed_batch from the same start.

Figures printed with -s (MI355X; DESIGN.md section 28, profiles/r22_flex.txt). Worst |got - ref| over its bar: the reductions
against the device's own rows 0.0137 (base), 0.0020 (long), 0.0095 (deep); the values against the reference's rows 7.8e-4 (base),
2.0e-4 (long), 3.6e-4 (deep). apply_torsions against the reference, worst error / (64 T 2^-53 L): 0.067 (base), 0.064 (long),
0.278 (deep) - the deep figure exceeds 1/4: the coordinates are absolute, about 40 A from the origin, and each of the 32 turns
rounds at that magnitude while the bar scales with L, the reach of a set (about 3 A); k stays 64. Distances inside a rigid part:
0.027, 0.096, 0.0016 of the same bar. (A moving set with a set nested in it is not rigid as a whole - the inner set turns against
it -, so the distances are checked inside the atoms of one and the same mask.) flex_lm_step: residual ratios 0.21 ... 0.32 against
np.linalg.solve's own 0.352 (gamma 1.409), q2 within 0.125 of its bar. The refinement: steps taken 1, 3, 3, 7, 8, 4, 3, 2 (rigid
1, 1, 2, 1, 3, 4, 1, 2); scores 591.1 ... 616.5 -> 639.4 ... 642.7, the rigid refinement of the same starts ends at 633.4 ... 640.9.
41 cases in 2.8 s.
"""
import functools

import numpy as np
import pytest

from tests import flex_reference as fr
from tests import flex_rows as X
from tests import hessian_reference as hr
from tests import lm_reference as lm
from tests import lm_rows as R
from tests import pose_reference as pr
from tests import hip_support as hip
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
U = 2.0 ** -53
KW = dict(lam_down=R.LAM_DOWN, lam_up=R.LAM_UP, max_dropped=R.MAX_DROPPED)
CASES = ("base", "long", "deep", "binary")


def _vox(d):
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, X.D, d["radii_type"], d["density"], library="hip", precision=64 if d["kind"] == "f64" else 32)


def _field(d):
    """(device field in the grid type of the case, the float64 array the kernel reads)."""
    import torch

    Fd = torch.tensor(d["F"], device="cuda").to(torch.float64 if d["kind"] == "f64" else torch.float32)
    return Fd, Fd.to(torch.float64).cpu().numpy()


def _flex(vox, d, Fd, axes=None, moves=None, per_atom=True):
    """(scores, G, H, atom_grad, atom_hess, atom_pos) of the case's batch as host arrays."""
    out = vox.score_hessian_flex_posed_batch(hip.dev(d["xyz"]), d["off"], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"]),
                                             hip.dev(d["radii"]), Fd, d["axes"] if axes is None else axes,
                                             d["moves"] if moves is None else moves, per_atom=per_atom)
    return tuple(x.cpu().numpy() for x in out)


def _rigid(vox, d, Fd):
    out = vox.score_hessian_posed_batch(hip.dev(d["xyz"]), d["off"], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"]),
                                        hip.dev(d["radii"]), Fd, per_atom=True)
    return tuple(x.cpu().numpy() for x in out)


@functools.lru_cache(maxsize=None)
def _got(name):
    """The case's flex call and its rigid twin, computed once and left unchanged."""
    d = X.data(name)
    vox = _vox(d)
    Fd, _ = _field(d)
    return _flex(vox, d, Fd), _rigid(vox, d, Fd)


def _sub(d, b):
    """Molecule b of a batch as a batch of its own."""
    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    return dict(d, sizes=(hi - lo,), off=np.array([0, hi - lo], np.int64), xyz=d["xyz"][lo:hi], q=d["q"][b:b + 1], t=d["t"][b:b + 1],
                cen=d["cen"][b:b + 1], chan=None if d["chan"] is None else d["chan"][lo:hi],
                radii=d["radii"] if np.isscalar(d["radii"]) else d["radii"][lo:hi], B=1, N=hi - lo, axes=d["axes"][b:b + 1],
                moves=d["moves"][lo:hi])


def _pivots(d):
    return d["t"].astype(np.float32).astype(np.float64)


# ---- bit identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_twist_block_the_scores_and_the_rows_are_the_rigid_entrys_bits(name):
    d = X.data(name)
    (S, G, H, ag, ah, ap), (S6, tg, th, ag6, ah6) = _got(name)
    n = 6 + d["T"]
    assert G.shape == (d["B"], n) and H.shape == (d["B"], n, n) and ap.shape == (d["N"], 3)
    assert hip.same_bits(S, S6) and hip.same_bits(G[:, :6], tg) and hip.same_bits(H[:, :6, :6], th)
    assert hip.same_bits(ag, ag6) and hip.same_bits(ah, ah6)
    assert hip.same_bits(H, H.transpose(0, 2, 1))
    assert np.isfinite(G).all() and np.isfinite(H).all()
    # the positions the records hold: the reference's, to rounding of the pose arithmetic
    p = pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])
    assert np.abs(ap - p).max() <= 1e-5
    if name == "binary":  # zeros but scores
        assert not G.any() and not H.any() and S[0] != 0.0 and S[1] == 0.0
    elif name == "base":
        assert G[0, 6:].all() and H[0, 6:, 6:].diagonal().all() and not G[1].any() and not H[1].any()
        assert not G[2, 8:].any() and not H[2, 8:].any()  # (molecule 2 has two torsions: the padding is inert)


@pytest.mark.parametrize("name", ("base", "long"))
def test_no_torsions_give_the_rigid_entry_entirely(name):
    d = X.data(name)
    vox = _vox(d)
    Fd, _ = _field(d)
    S, G, H = _flex(vox, d, Fd, axes=np.zeros((d["B"], 0, 2), np.int32), per_atom=False)
    _, (S6, tg, th, _, _) = _got(name)
    assert hip.same_bits(S, S6) and hip.same_bits(G, tg) and hip.same_bits(H, th)


@pytest.mark.parametrize("name", ("base", "long", "deep"))
def test_two_runs_agree_and_a_molecule_alone_is_the_molecule_in_its_batch(name):
    d = X.data(name)
    vox = _vox(d)
    Fd, _ = _field(d)
    first, _ = _got(name)
    again = _flex(vox, d, Fd)
    for a, b in zip(first, again):
        assert hip.same_bits(a, b)
    for b in range(d["B"]):
        alone = _flex(vox, _sub(d, b), Fd)
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        assert hip.same_bits(alone[0][0], first[0][b]) and hip.same_bits(alone[1][0], first[1][b]) and hip.same_bits(alone[2][0], first[2][b])
        assert hip.same_bits(alone[5], first[5][lo:hi])


# ---- against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("base", "long", "deep"))
def test_the_reductions_against_the_reference_fed_the_devices_own_rows(name):
    d = X.data(name)
    (S, G, H, ag, ah, ap), _ = _got(name)
    piv = _pivots(d)
    worst = 0.0
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        rG, bG, rH, bH = fr.flex(ap[lo:hi], ag[lo:hi], ah[lo:hi], piv[b], d["axes"][b], d["moves"][lo:hi])
        bar = (hi - lo + 128) * U
        for got, ref, bound in ((G[b], rG, bG), (H[b], rH, bH)):
            assert not got[bound == 0.0].any()
            err = np.abs(got - ref)
            assert (err <= bar * bound).all(), (b, float((err / (bar * bound + 1e-300)).max()))
            worst = max(worst, float((err / (bar * bound + 1e-300)).max()))
    print(f"FLEX_REDUCTIONS {name}: worst |got - ref| / ((N_b + 128) 2^-53 bound) {worst:.3g}")


@pytest.mark.parametrize("name", ("base", "long", "deep"))
def test_the_values_against_the_reference_fed_the_reference_rows(name):
    d = X.data(name)
    (S, G, H, _, _, _), _ = _got(name)
    _, Fref = _field(d)
    rel, ab = (GRAD64_REL, GRAD64_ABS) if d["kind"] == "f64" else (GRAD_REL, GRAD_ABS)
    p = pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])
    piv = _pivots(d)
    worst = 0.0
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            assert not G[b].any() and not H[b].any()
            continue
        radii = d["radii"] if np.isscalar(d["radii"]) else d["radii"][lo:hi]
        ref = hr.reference(p[lo:hi], Fref, radii, d["radii_type"], w=None if d["chan"] is None else d["chan"][lo:hi], mode=d["mode"],
                           precision=64 if d["kind"] == "f64" else 32)
        rG, bG, rH, bH = fr.flex(p[lo:hi], ref["g"][0], ref["H"][0], piv[b], d["axes"][b], d["moves"][lo:hi], ref["g"][1], ref["H"][1])
        for got, want, bound in ((G[b], rG, bG), (H[b], rH, bH)):
            err = np.abs(got - want)
            assert (err <= rel * bound + ab).all(), (b, float((err / (rel * bound + ab)).max()))
            worst = max(worst, float((err / (rel * bound + ab)).max()))
    print(f"FLEX_VALUES {name}: worst |got - ref| / bar {worst:.3g}")


# ---- inert torsions and dead atoms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(-1, -1), (4, 14), (14, 4), (4, 4), (-3, 2)])
def test_an_inert_torsion_gives_exact_zeros_and_leaves_the_other_bits(bad):
    d = X.data("base")
    vox = _vox(d)
    Fd, _ = _field(d)
    axes = np.concatenate([d["axes"], np.full((3, 1, 2), -1, np.int32)], axis=1)
    axes[0, 4] = bad  # (molecule 0 has 14 atoms: 14 is the index N_b)
    moves = d["moves"].copy()
    moves[9:12] |= 1 << 4  # the fifth set is a live set: only its axis is not
    S, G, H = _flex(vox, d, Fd, axes=axes, moves=moves, per_atom=False)
    (S4, G4, H4, _, _, _), _ = _got("base")
    assert hip.same_bits(S, S4) and hip.same_bits(G[:, :10], G4) and hip.same_bits(H[:, :10, :10], H4)
    assert not G[:, 10].any() and not H[:, 10, :].any() and not H[:, :, 10].any()
    assert not np.signbit(G[:, 10]).any() and not np.signbit(H[:, 10, :]).any()
    # ... and apply_torsions turns nothing about it
    ang = np.random.default_rng(1).uniform(-1, 1, (3, 5))
    with_it = vox.apply_torsions(hip.dev(d["xyz"]), d["off"], axes, moves, ang).cpu().numpy()
    without = vox.apply_torsions(hip.dev(d["xyz"]), d["off"], d["axes"], d["moves"], ang[:, :4]).cpu().numpy()
    assert hip.same_bits(with_it, without)


def test_a_dead_atom_in_a_moving_set_gives_the_bits_of_the_call_without_it():
    d = X.data("base")
    vox = _vox(d)
    Fd, _ = _field(d)
    last = d["N"] - 1  # the last atom of the last molecule, in both of its sets (at the tail the live atoms keep their lanes)
    assert (int(d["moves"][last]) & 3) == 3
    xyz = d["xyz"].copy()
    xyz[last, 1] = np.nan
    S, G, H, ag, ah, ap = _flex(vox, dict(d, xyz=xyz), Fd)
    assert np.isfinite(S).all() and np.isfinite(G).all() and np.isfinite(H).all() and not ag[last].any() and not ah[last].any()
    off = d["off"].copy()
    off[-1] -= 1
    cut = dict(d, xyz=d["xyz"][:last], chan=d["chan"][:last], radii=d["radii"][:last], off=off, moves=d["moves"][:last], N=last)
    S2, G2, H2 = _flex(vox, cut, Fd, per_atom=False)
    assert hip.same_bits(S, S2) and hip.same_bits(G, G2) and hip.same_bits(H, H2)


# ---- apply_torsions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("base", "long", "deep"))
def test_apply_torsions_against_the_reference(name):
    """Measured worst error / bar with k = 64 (MI355X): base 0.067, long 0.064, deep 0.278. The deep case exceeds 1/4 (absolute
    coordinates about 40 A from the origin, 32 turns, L about 3 A); k is not raised."""
    d = X.data(name)
    vox = _vox(d)
    rng = np.random.default_rng(7)
    B, T = d["B"], d["T"]
    ang = rng.uniform(-np.pi, np.pi, (B, T))
    if name == "base":
        ang[0, 1] = 0.0  # an angle of exactly zero turns nothing
    xyz = hip.dev(d["xyz"])
    same = vox.apply_torsions(xyz, d["off"], d["axes"], d["moves"], np.zeros((B, T))).cpu().numpy()
    assert hip.same_bits(same, d["xyz"])
    got = vox.apply_torsions(xyz, d["off"], d["axes"], d["moves"], ang).cpu().numpy()
    again = vox.apply_torsions(xyz, d["off"], d["axes"], d["moves"], ang).cpu().numpy()
    assert hip.same_bits(got, again) and hip.same_bits(xyz.cpu().numpy(), d["xyz"])
    worst = worst_d = 0.0
    for b in range(B):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            continue
        p0, mv, ax = d["xyz"][lo:hi], d["moves"][lo:hi], d["axes"][b]
        ref = fr.apply_torsions(p0, ax, mv, ang[b])
        turned = np.zeros(hi - lo, bool)
        for k in range(T):
            if fr.axis(p0, ax[k]) is not None and ang[b, k] != 0.0:
                turned |= fr.bits(mv, k)
        assert hip.same_bits(got[lo:hi][~turned], p0[~turned])
        bar = 64 * T * U * fr.reach(p0, ax, mv)
        worst = max(worst, float(np.abs(got[lo:hi] - ref).max() / bar))
        # the distances inside every rigid part of a moving set - the atoms with one and the same mask, which turn together (a set
        # with a set nested in it is not rigid as a whole: the inner one turns against it)
        for m in np.unique(mv):
            sel = np.flatnonzero(mv == m)
            if sel.size < 2:
                continue
            before = np.linalg.norm(p0[sel][:, None] - p0[sel][None], axis=2)
            after = np.linalg.norm(got[lo:hi][sel][:, None] - got[lo:hi][sel][None], axis=2)
            worst_d = max(worst_d, float(np.abs(after - before).max() / bar))
    print(f"FLEX_APPLY {name}: worst error / (64 T 2^-53 L) {worst:.3g}, worst change of a distance inside a rigid part / bar {worst_d:.3g}")
    assert worst <= 1.0 and worst_d <= 1.0


# ---- flex_lm_step ---------------------------------------------------------------------------------------------------------------
NAMES = ("q", "t", "theta", "S", "G", "H", "lam", "taken", "dropped")


def _flex_state(s, trial, B, T):
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import FlexLMState

    t = {k: torch.tensor(np.ascontiguousarray(v), device="cuda") for k, v in s.items()}
    st = FlexLMState(t["q"], t["t"], t["theta"], t["S"], t["G"], t["H"], t["lam"], t["taken"], t["dropped"])
    st.q2, st.t2, st.theta2 = t["q2"], t["t2"], t["theta2"]
    st.x = torch.full((B, 6 + T), np.nan, dtype=torch.float64, device="cuda")
    return st, tuple(torch.tensor(np.ascontiguousarray(x), device="cuda") for x in trial)


@pytest.fixture(scope="module")
def vox():
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, 16, "scalar", "gaussian", library="hip")


@pytest.mark.parametrize("have_trial", [True, False])
@pytest.mark.parametrize("B", R.SIZES)
def test_flex_lm_step_without_torsions_is_lm_step_to_the_bit(vox, B, have_trial):
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import LMState

    s, trial = R.rows(B)
    t = {k: torch.tensor(v, device="cuda") for k, v in s.items()}
    a = LMState(t["q"], t["t"], t["S"], t["G"], t["H"], t["lam"], t["taken"], t["dropped"])
    a.q2, a.t2, a.xi = t["q2"], t["t2"], torch.full((B, 6), np.nan, dtype=torch.float64, device="cuda")
    dev_trial = tuple(torch.tensor(x, device="cuda") for x in trial)
    vox.lm_step(a, dev_trial if have_trial else None, **KW)
    zero = np.zeros((B, 0))
    b, _ = _flex_state(dict(s, theta=zero, theta2=zero), trial, B, 0)
    vox.flex_lm_step(b, dev_trial if have_trial else None, **KW)
    for k, k2 in (("q", "q"), ("t", "t"), ("S", "S"), ("G", "G"), ("H", "H"), ("lam", "lam"), ("taken", "taken"), ("dropped", "dropped"),
                  ("q2", "q2"), ("t2", "t2"), ("xi", "x")):
        assert hip.same_bits(getattr(a, k).cpu().numpy(), getattr(b, k2).cpu().numpy()), k


@pytest.mark.parametrize("have_trial", [True, False])
@pytest.mark.parametrize("T", X.LM_T)
def test_flex_lm_step_against_the_reference(vox, T, have_trial):
    B = X.LM_B
    s0, trial = X.lm_rows(T)
    st, dev_trial = _flex_state(s0, trial, B, T)
    vox.flex_lm_step(st, dev_trial if have_trial else None, **KW)
    got = {k: getattr(st, k).cpu().numpy() for k in NAMES + ("q2", "t2", "theta2", "x")}
    again, _ = _flex_state(s0, trial, B, T)
    vox.flex_lm_step(again, dev_trial if have_trial else None, **KW)
    for k in got:
        assert hip.same_bits(got[k], getattr(again, k).cpu().numpy()), k
    ref, rtrial = X.lm_reference_state(T)
    decisions = fr.step(ref, rtrial if have_trial else None, x_from=got["x"], **KW)
    for k in NAMES:  # decisions, damping, counters and the copied state: to the bit
        assert hip.same_bits(got[k], getattr(ref, k)), (k, np.argwhere(got[k] != getattr(ref, k))[:3].tolist())
    for b in range(B):
        kind = R.kind_of(B, b)
        if decisions[b] == "accept":
            assert hip.same_bits(got["theta"][b], s0["theta2"][b]) and hip.same_bits(got["H"][b], rtrial[2][b]) and got["taken"][b] == s0["taken"][b] + 1
        else:
            assert hip.same_bits(got["theta"][b], s0["theta"][b]) and hip.same_bits(got["H"][b], s0["H"][b]) and got["taken"][b] == s0["taken"][b]
        stays = kind in R.FAILS or kind == "finished" or (have_trial and kind == "dropped_last")
        if stays:  # no step: x = 0 and the state itself, to the bit
            assert not got["x"][b].any() and not np.signbit(got["x"][b]).any(), (b, kind)
            assert hip.same_bits(got["q2"][b], got["q"][b]) and hip.same_bits(got["t2"][b], got["t"][b]) and hip.same_bits(got["theta2"][b], got["theta"][b])
        else:
            assert got["x"][b].any() and np.isfinite(got["x"][b]).all(), (b, kind)
            assert hip.same_bits(got["theta2"][b], got["theta"][b] + got["x"][b, 6:])
        if kind == "omega_zero":
            assert not got["x"][b, 3:6].any() and hip.same_bits(got["q2"][b], got["q"][b])
    numpy_worst, cond = X.lm_numpy_residual()
    gamma = 4.0 * numpy_worst
    assert cond < 1e8
    worst = 0.0
    for b in range(B):
        if got["x"][b].any():
            worst = max(worst, fr.residual_ratio(got["H"][b], got["G"][b], got["lam"][b], got["x"][b]))
    qerr = np.abs(got["q2"] - ref.q2).max(axis=1) / (8 * EPS * np.linalg.norm(got["q"], axis=1))
    terr = np.abs(got["t2"] - ref.t2).max(axis=1) / (8 * EPS * (np.abs(got["t"]).max(axis=1) + np.abs(got["x"][:, :3]).max(axis=1) + 1e-300))
    print(f"FLEX_LM_STEP T {T} trial {int(have_trial)}: residual ratio {worst:.3f} (numpy {numpy_worst:.3f}, gamma {gamma:.3f}); "
          f"q2 error / bar {qerr.max():.3g}, t2 error / bar {terr.max():.3g}")
    assert worst <= gamma, (worst, gamma)
    assert (qerr <= 1.0).all() and (terr <= 1.0).all()
    assert hip.same_bits(got["theta2"], ref.theta2)


# ---- the refinement -----------------------------------------------------------------------------------------------------------
def test_refinement_with_torsions_ends_above_the_rigid_refinement_of_every_start():
    import molvoxel_amd as mv

    xyz, cen, W, rad, axes, moves = X.refine_molecule()
    q0, t0, th0 = X.refine_starts()
    B = X.REFINE_POSES
    vox = mv.create_voxelizer(0.5, X.D, "atom-wise", "gaussian", library="hip")
    off1 = np.array([0, 14], np.int64)
    ident = (hip.dev(np.array([[1.0, 0.0, 0.0, 0.0]])), hip.dev(np.zeros((1, 3))))
    field = vox.forward_posed_batch(hip.dev(xyz), off1, hip.dev(cen), ident[0], ident[1], hip.dev(W), hip.dev(rad))[0].clone()
    assert np.abs(field.cpu().numpy().astype(np.float64) - X.cpu_field()).max() <= 1e-4
    # B copies of the molecule, one per start
    off = 14 * np.arange(B + 1, dtype=np.int64)
    rep = lambda x: hip.dev(np.concatenate([x] * B))
    coords, chan, radii, cens = rep(xyz), rep(W), rep(rad), rep(cen)
    ax, mvs = np.concatenate([axes] * B), np.concatenate([moves] * B)
    kw = dict(steps=X.REFINE_ROUNDS, **KW)
    q, t, theta, S, info = vox.refine_flex_posed_batch(coords, off, cens, hip.dev(q0), hip.dev(t0), hip.dev(th0), chan, radii, field, ax, mvs, **kw)
    hist = info["score_history"].cpu().numpy()
    assert hist.shape == (X.REFINE_ROUNDS + 1, B) and tuple(theta.shape) == (B, 4) and info["evaluations"] == X.REFINE_ROUNDS + 1
    assert hip.same_bits(hist[-1], S.cpu().numpy())
    # the rigid refinement of the same starts: the start conformers, then refine_posed_batch
    start = vox.apply_torsions(coords, off, ax, mvs, hip.dev(th0))
    _, _, S6, info6 = vox.refine_posed_batch(start, off, cens, hip.dev(q0), hip.dev(t0), chan, radii, field, **kw)
    assert hip.same_bits(hist[0], info6["score_history"][0].cpu().numpy())  # (both start from the same evaluation)
    print(f"FLEX_REFINE taken {info['taken'].tolist()} (rigid {info6['taken'].tolist()}); score {hist[0].min():.1f} ... {hist[0].max():.1f} "
          f"-> {hist[-1].min():.1f} ... {hist[-1].max():.1f}, rigid -> {float(S6.min()):.1f} ... {float(S6.max()):.1f}")
    X.refine_conditions(hist, S.cpu().numpy(), S6.cpu().numpy())
