"""The rows tests/test_hip_lm_step.py runs through mvx_lm_step and tests/test_lm_host.py through numpy (no GPU needed here): for
every batch size one state and one trial whose poses cycle through every kind of row the step distinguishes, the measurement of
np.linalg.solve's own residual on these systems, and the molecule, field and starts of the refinement tests."""
import functools

import numpy as np

from tests import lm_reference as lm

SIZES = (1, 63, 64, 65, 257)
MAX_DROPPED = 3
LAM_DOWN, LAM_UP = 1.0 / 3.0, 10.0
KINDS = ("accepted", "dropped", "dropped_last", "finished", "nan_S2", "nan_H", "singular", "zero_H", "omega_zero", "omega_pi",
         "unnormalised")
# kinds whose step fails: xi = 0 and (q2, t2) = (q, t) (a finished row gives the same without a step)
FAILS = ("nan_H", "singular")


def _symmetric(rng):
    """A random symmetric 6x6 H with the eigenvalues of -H in +-[1, 1e3], either sign: indefinite, cond(-H + lam I) < 2e3 for
    the lam of these rows."""
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    e = rng.choice([-1.0, 1.0], 6) * 10.0 ** rng.uniform(0.0, 3.0, 6)
    H = -(Q * e) @ Q.T
    return 0.5 * (H + H.T)


def kind_of(B, b):
    return KINDS[(b + B) % len(KINDS)]


@functools.lru_cache(maxsize=None)
def rows(B, seed=7):
    """(state, trial) for a batch of B poses as read-only numpy arrays: state = dict(q, t, S, G, H, lam, taken, dropped, q2, t2),
    trial = (S2, G2, H2); row b is of kind kind_of(B, b)."""
    rng = np.random.default_rng(seed + B)
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    q2 = rng.standard_normal((B, 4))
    q2 /= np.linalg.norm(q2, axis=1)[:, None]
    t, t2 = rng.uniform(-2, 2, (B, 3)), rng.uniform(-2, 2, (B, 3))
    S = rng.uniform(10.0, 100.0, B)
    S2 = S + rng.uniform(0.1, 5.0, B)
    G, G2 = rng.standard_normal((B, 6)), rng.standard_normal((B, 6))
    H, H2 = np.array([_symmetric(rng) for _ in range(B)]), np.array([_symmetric(rng) for _ in range(B)])
    lam = 10.0 ** rng.uniform(-3.0, -1.0, B)
    taken = rng.integers(0, 5, B).astype(np.int32)
    dropped = rng.integers(0, MAX_DROPPED, B).astype(np.int32)
    for b in range(B):
        k = kind_of(B, b)
        if k in ("dropped", "dropped_last", "nan_H", "singular", "zero_H", "omega_zero", "omega_pi"):
            S2[b] = S[b] - rng.uniform(0.0, 5.0) * (b % 2)  # (a tie, S2 == S, is dropped as well)
            dropped[b] = MAX_DROPPED - 1 if k == "dropped_last" else 0
        if k == "finished":
            dropped[b] = MAX_DROPPED
        if k == "nan_S2":
            S2[b], dropped[b] = np.nan, 0
        if k == "nan_H":
            H[b][int(rng.integers(0, 6)), int(rng.integers(0, 6))] = np.nan
        if k == "singular":
            H[b], lam[b] = 0.0, 0.0
        if k == "zero_H":
            H[b] = 0.0
        if k == "omega_zero":  # a block-diagonal system with G_omega = 0: xi_omega is exactly 0
            H[b, :3, 3:], H[b, 3:, :3], G[b, 3:] = 0.0, 0.0, 0.0
        if k == "omega_pi":  # -H = I: xi = G / (1 + lam'), |omega| about pi - 1e-3
            H[b] = -np.eye(6)
            w = rng.standard_normal(3)
            G[b, 3:] = (1.0 + lam[b] * LAM_UP) * (np.pi - 1e-3) * w / np.linalg.norm(w)
        if k == "unnormalised":
            q[b] *= 1.7
            q2[b] *= 0.6
    state = dict(q=q, t=t, S=S, G=G, H=H, lam=lam, taken=taken, dropped=dropped, q2=q2, t2=t2)
    trial = (S2, G2, H2)
    for x in list(state.values()) + list(trial):
        x.setflags(write=False)
    return state, trial


def reference_state(B):
    """A fresh lm_reference.State of rows(B), with the trial pose in place."""
    s, trial = rows(B)
    st = lm.State(s["q"], s["t"], s["S"], s["G"], s["H"], s["lam"], s["taken"], s["dropped"])
    st.q2, st.t2 = s["q2"].copy(), s["t2"].copy()
    return st, trial


@functools.lru_cache(maxsize=None)
def numpy_residual():
    """(the largest ||A xi - G||_inf / (2^-52 (||A||_inf ||xi||_inf + ||G||_inf)) np.linalg.solve itself attains on the systems
    of every batch here, with and without a trial; the largest 2-norm condition number among them)."""
    worst, cond = 0.0, 0.0
    for B in SIZES:
        for have_trial in (True, False):
            st, trial = reference_state(B)
            lm.step(st, trial if have_trial else None, LAM_DOWN, LAM_UP, MAX_DROPPED)
            for b in range(B):
                if st.xi[b].any():
                    worst = max(worst, lm.residual_ratio(st.H[b], st.G[b], st.lam[b], st.xi[b]))
                    cond = max(cond, float(np.linalg.cond(st.lam[b] * np.eye(6) - st.H[b])))
    return worst, cond


# ---- the refinement tests: the molecule of tests/test_hip_score_hessian.py's Newton step (case "single", molecule 0), its own
# grid at the identity pose as the field, and 8 starts of at most 5 degrees and 0.3 A ------------------------------------------------
REFINE_POSES, REFINE_ROUNDS = 8, 12
REFINE_RADIUS = 1.25


@functools.lru_cache(maxsize=None)
def refine_starts(seed=11):
    """(q (8, 4) unit, t (8, 3)): rotations of 1 ... 5 degrees about random axes and shifts of 0.06 ... 0.3 A."""
    rng = np.random.default_rng(seed)
    B = REFINE_POSES
    axis = rng.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    ang = np.deg2rad(rng.uniform(1.0, 5.0, B))
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    d = rng.standard_normal((B, 3))
    t = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.06, 0.3, B)[:, None]
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def angle_deg(q):
    """(B,): the rotation angle of each quaternion, in degrees."""
    q = np.asarray(q, np.float64)
    return np.degrees(2.0 * np.arccos(np.minimum(1.0, np.abs(q[:, 0]) / np.linalg.norm(q, axis=1))))


def refine_conditions(history, taken, q0, t0, q, t):
    """The three conditions of the refinement tests, for every pose without exemption: the score history never decreases, every
    pose took a step, every pose ends with a smaller rotation angle and a smaller shift than it started with."""
    history = np.asarray(history)
    assert (np.diff(history, axis=0) >= 0).all(), np.argwhere(np.diff(history, axis=0) < 0)[:3].tolist()
    assert (np.asarray(taken) >= 1).all(), np.asarray(taken).tolist()
    a0, a1 = angle_deg(q0), angle_deg(q)
    s0, s1 = np.linalg.norm(t0, axis=1), np.linalg.norm(t, axis=1)
    assert (a1 < a0).all(), (a0.tolist(), a1.tolist())
    assert (s1 < s0).all(), (s0.tolist(), s1.tolist())
    return a0, a1, s0, s1


@functools.lru_cache(maxsize=None)
def refine_molecule():
    """(xyz (64, 3), centre (1, 3), D): molecule 0 of the `single` case of tests/test_hip_score_hessian.py."""
    from tests import test_hip_score_hessian as th

    d = th._sub(th._data("single"), 0)
    assert d["radii"] == REFINE_RADIUS and d["kind"] == "f64" and d["mode"] == "single"
    return d["xyz"], d["cen"], th.D


@functools.lru_cache(maxsize=None)
def cpu_field():
    """(1, D, D, D) float64: the molecule's own grid at the identity pose, from the reference's densities (precision 64)."""
    from tests import pose_reference as pr
    from tests.grad_reference import Geometry, atom_density

    xyz, cen, D = refine_molecule()
    geo = Geometry(D, 0.5, None, 0.5, "gaussian", 64)
    p = pr.positions(xyz, cen[0], [1.0, 0.0, 0.0, 0.0], np.zeros(3))
    F = np.zeros((1, D, D, D))
    r = np.full(1, REFINE_RADIUS)
    for n in range(p.shape[0]):
        ev = atom_density(geo, p[n], r, REFINE_RADIUS, "scalar")
        if ev is not None:
            F[(0,) + ev[0]] += ev[3][0]
    F.setflags(write=False)
    return F


def cpu_evaluate(q, t, bounds=False):
    """(S (B,), G (B, 6), H (B, 6, 6)) of the molecule under the poses (q, t) against cpu_field(), from tests/hessian_reference.py,
    about the default pivots (the translations rounded to float32). bounds: also (bG (B, 6), bH (B, 6, 6)), the sums of the
    absolute values of the terms of G and H."""
    from tests import hessian_reference as hr
    from tests import pose_reference as pr

    xyz, cen, _ = refine_molecule()
    F = cpu_field()
    B = len(q)
    S, G, H, bG, bH = np.zeros(B), np.zeros((B, 6)), np.zeros((B, 6, 6)), np.zeros((B, 6)), np.zeros((B, 6, 6))
    for b in range(B):
        p = pr.positions(xyz, cen[0], q[b], t[b])
        ref = hr.reference(p, F, REFINE_RADIUS, "scalar", mode="single", precision=64)
        piv = np.asarray(t[b], np.float64).astype(np.float32).astype(np.float64)
        S[b] = ref["s"][0].sum()
        G[b], bG[b], H[b], bH[b] = hr.twist(p, ref["g"][0], ref["H"][0], piv, ref["g"][1], ref["H"][1])
    return (S, G, H, bG, bH) if bounds else (S, G, H)


@functools.lru_cache(maxsize=None)
def cpu_refinement():
    """The CPU loop on the starts: (final state, score history (rounds + 1, 8), the first trial pose (q2, t2))."""
    q0, t0 = refine_starts()
    return lm.refine(cpu_evaluate, q0, t0, REFINE_ROUNDS, None, LAM_DOWN, LAM_UP, MAX_DROPPED)
