"""The rows of tests/test_hip_flex.py, as host arrays that are never modified (no GPU needed here: tests/test_flex_host.py runs
the refinement rows through numpy): the four cases, every one with D = 16 at resolution 0.5, the rows mvx_flex_lm_step is run on -
tests/lm_rows.py's kinds extended to n = 6 + T dimensions -, and the molecule, field and starts of the refinement test.

    case    mode      C  radii      atoms per molecule  torsions per molecule   grid
    base    features  5  atom-wise  14 / 0 / 9          4 / 0 / 2, padded to 4  f32   (one branch, nesting depth 3)
    long    single    1  scalar     300                 1, turning 150 atoms    f64   (past one round of 256 lanes, past one chunk)
    deep    single    1  scalar     35                  32: every inner bond    f32   (the top mask bit, the largest LDS system)
    binary  features  5  atom-wise  14 / 0 / 9          as base                 f32   (binary density: zeros but scores)
"""
import functools

import numpy as np

from tests import flex_reference as fr
from tests import lm_reference as lm
from tests import lm_rows as R

D = 16
CEN = np.array([30.0, -20.0, 12.0])
CASES = {
    "base": dict(mode="features", C=5, radii_type="atom-wise", sizes=(14, 0, 9), kind="f32", density="gaussian"),
    "long": dict(mode="single", C=1, radii_type="scalar", sizes=(300,), kind="f64", density="gaussian"),
    "deep": dict(mode="single", C=1, radii_type="scalar", sizes=(35,), kind="f32", density="gaussian"),
    "binary": dict(mode="features", C=5, radii_type="atom-wise", sizes=(14, 0, 9), kind="f32", density="binary"),
}


def _chain(rng, n, bond):
    p = np.zeros((n, 3))
    for i in range(1, n):
        d = rng.standard_normal(3)
        p[i] = p[i - 1] + bond * d / np.linalg.norm(d)
    return p - p.mean(axis=0)


def _molecules(name, rng):
    """Per molecule (local coordinates about the origin, axes (T_b, 2), moves (N_b,) int32)."""
    if name in ("base", "binary"):
        nine = np.zeros(9, np.uint32)
        nine[3:] |= 1
        nine[6:] |= 2
        return [(fr.tree_coords(rng, 14, bond=0.75), fr.TREE_AXES, fr.tree_moves(14)),
                (np.zeros((0, 3)), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)),
                (_chain(rng, 9, 0.8), np.array([[2, 3], [5, 6]], np.int32), nine.view(np.int32))]
    if name == "long":
        m = np.zeros(300, np.uint32)
        m[150:] = 1
        return [(rng.uniform(-3.0, 3.0, (300, 3)), np.array([[0, 150]], np.int32), m.view(np.int32))]
    m = np.zeros(35, np.uint32)  # deep: torsion k about (k + 1, k + 2) turns the atoms k + 2 .. 34
    for k in range(32):
        m[k + 2:] |= np.uint32(1 << k)
    return [(_chain(rng, 35, 0.45), np.stack([np.arange(1, 33), np.arange(2, 34)], axis=1).astype(np.int32), m.view(np.int32))]


@functools.lru_cache(maxsize=None)
def data(name, seed=41):
    """One batch of a case: offsets, centres, coordinates, poses, channels, radii, field, axes (B, T, 2) padded with -1, moves."""
    c = dict(CASES[name])
    rng = np.random.default_rng(seed)
    fp = np.float64 if c["kind"] == "f64" else np.float32
    mols = _molecules(name, rng)
    sizes, C_ = c["sizes"], c["C"]
    B, N = len(sizes), int(sum(sizes))
    assert [m[0].shape[0] for m in mols] == list(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cen = CEN + rng.normal(0.0, 0.4, (B, 3))
    xyz = np.concatenate([cen[b] + m[0] for b, m in enumerate(mols)]).reshape(N, 3)
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    t = rng.uniform(-0.4, 0.4, (B, 3))
    T = max(m[1].shape[0] for m in mols)
    axes = np.full((B, T, 2), -1, np.int32)
    for b, m in enumerate(mols):
        axes[b, :m[1].shape[0]] = m[1]
    moves = np.concatenate([m[2] for m in mols]).astype(np.int32)
    chan = rng.standard_normal((N, C_)).astype(fp) if c["mode"] == "features" else None
    radii = 1.25 if c["radii_type"] == "scalar" else rng.uniform(1.0, 1.5, N).astype(fp)
    F = rng.standard_normal((C_,) + (D,) * 3)
    out = dict(c, name=name, off=off, cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, F=F, B=B, N=N, T=T, axes=axes, moves=moves)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- mvx_flex_lm_step: lm_rows' kinds in n dimensions ---------------------------------------------------------------------------
LM_T = (1, 4, 32)
LM_B = 23  # two rows of every kind and one more


def _symmetric(rng, n):
    """lm_rows' matrices in n dimensions: the eigenvalues of -H in +-[1, 1e3], either sign."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    e = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(0.0, 3.0, n)
    H = -(Q * e) @ Q.T
    return 0.5 * (H + H.T)


@functools.lru_cache(maxsize=None)
def lm_rows(T, B=LM_B, seed=5):
    """(state, trial) as lm_rows.rows gives them, row b of kind lm_rows.kind_of(B, b), with theta, theta2 (B, T) and G, H of
    width n = 6 + T."""
    rng = np.random.default_rng(seed + T)
    n = 6 + T
    s6, _ = R.rows(B)
    st = {k: np.array(v) for k, v in s6.items() if k not in ("G", "H")}
    S, lam, dropped = st["S"], st["lam"], st["dropped"]
    S2 = S + rng.uniform(0.1, 5.0, B)
    G, G2 = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    H, H2 = np.array([_symmetric(rng, n) for _ in range(B)]), np.array([_symmetric(rng, n) for _ in range(B)])
    theta, theta2 = rng.uniform(-1, 1, (B, T)), rng.uniform(-1, 1, (B, T))
    for b in range(B):
        k = R.kind_of(B, b)
        if k in ("dropped", "dropped_last", "nan_H", "singular", "zero_H", "omega_zero", "omega_pi"):
            S2[b] = S[b] - rng.uniform(0.0, 5.0) * (b % 2)
            dropped[b] = R.MAX_DROPPED - 1 if k == "dropped_last" else 0
        if k == "finished":
            dropped[b] = R.MAX_DROPPED
        if k == "nan_S2":
            S2[b], dropped[b] = np.nan, 0
        if k == "nan_H":
            H[b][int(rng.integers(0, n)), int(rng.integers(0, n))] = np.nan
        if k == "singular":
            H[b], lam[b] = 0.0, 0.0
        if k == "zero_H":
            H[b] = 0.0
        if k == "omega_zero":  # omega decoupled with G_omega = 0: x_omega is exactly 0
            H[b, 3:6, :] = 0.0
            H[b, :, 3:6] = 0.0
            H[b, 3:6, 3:6] = -np.eye(3)
            G[b, 3:6] = 0.0
        if k == "omega_pi":
            H[b] = -np.eye(n)
            w = rng.standard_normal(3)
            G[b, 3:6] = (1.0 + lam[b] * R.LAM_UP) * (np.pi - 1e-3) * w / np.linalg.norm(w)
    st.update(G=G, H=H, theta=theta, theta2=theta2, dropped=dropped)
    trial = (S2, G2, H2)
    for x in list(st.values()) + list(trial):
        x.setflags(write=False)
    return st, trial


def lm_reference_state(T, B=LM_B):
    s, trial = lm_rows(T, B)
    st = fr.State(s["q"], s["t"], s["theta"], s["S"], s["G"], s["H"], s["lam"], s["taken"], s["dropped"])
    st.q2, st.t2, st.theta2 = s["q2"].copy(), s["t2"].copy(), s["theta2"].copy()
    return st, trial


@functools.lru_cache(maxsize=None)
def lm_numpy_residual():
    """(np.linalg.solve's own largest residual ratio on the systems of lm_rows(T) for T in LM_T, with and without a trial; the
    largest condition number among them), measured as lm_rows.numpy_residual measures it."""
    worst, cond = 0.0, 0.0
    for T in LM_T:
        for have_trial in (True, False):
            st, trial = lm_reference_state(T)
            fr.step(st, trial if have_trial else None, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED)
            for b in range(len(st.q)):
                if st.x[b].any():
                    worst = max(worst, fr.residual_ratio(st.H[b], st.G[b], st.lam[b], st.x[b]))
                    cond = max(cond, float(np.linalg.cond(st.lam[b] * np.eye(6 + T) - st.H[b])))
    return worst, cond


# ---- the refinement test: the 14-atom molecule of `base` against its own grid, 8 starts ---------------------------------------
REFINE_POSES, REFINE_ROUNDS = 8, 12
REFINE_SEED = 17


@functools.lru_cache(maxsize=None)
def refine_molecule():
    """Molecule 0 of `base`: (xyz (14, 3), centre (1, 3), features (14, 5) float32, radii (14,) float32, axes (1, 4, 2), moves)."""
    d = data("base")
    return d["xyz"][:14], d["cen"][:1], d["chan"][:14], d["radii"][:14], d["axes"][:1], d["moves"][:14]


@functools.lru_cache(maxsize=None)
def refine_starts(seed=REFINE_SEED):
    """(q (8, 4), t (8, 3), theta (8, 4)): rotations of 5 degrees about random axes, shifts of 0.2 A, torsions off by 10 ... 15
    degrees either way."""
    rng = np.random.default_rng(seed)
    B = REFINE_POSES
    ax = rng.standard_normal((B, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    ang = np.deg2rad(np.full(B, 5.0))
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * ax], axis=1)
    d = rng.standard_normal((B, 3))
    t = 0.2 * d / np.linalg.norm(d, axis=1)[:, None]
    theta = np.deg2rad(rng.uniform(10.0, 15.0, (B, 4))) * rng.choice([-1.0, 1.0], (B, 4))
    for x in (q, t, theta):
        x.setflags(write=False)
    return q, t, theta


@functools.lru_cache(maxsize=None)
def cpu_field():
    """(5, D, D, D) float64: the molecule's own grid at the identity pose, from the reference's densities (precision 32)."""
    from tests import pose_reference as pr
    from tests.grad_reference import Geometry, atom_density

    xyz, cen, W, rad, _, _ = refine_molecule()
    geo = Geometry(D, 0.5, None, 0.5, "gaussian", 32)
    p = pr.positions(xyz, cen[0], [1.0, 0.0, 0.0, 0.0], np.zeros(3))
    F = np.zeros((W.shape[1], D, D, D))
    for n in range(p.shape[0]):
        ev = atom_density(geo, p[n], rad[n:n + 1], float(rad[n]), "atom")
        if ev is not None:
            F[(slice(None),) + ev[0]] += W[n].astype(np.float64)[:, None, None, None] * ev[3][0]
    F = F.astype(np.float32).astype(np.float64)  # (the device field is float32)
    F.setflags(write=False)
    return F


def cpu_evaluate(q, t, theta=None, conformer=None):
    """(S, G, H) of the molecule at the poses (q, t): with theta (B, 4) in n = 10 coordinates, the conformer made from the
    reference one by these angles; without, the rigid 6 of tests/hessian_reference.py on `conformer` (B, 14, 3)."""
    from tests import hessian_reference as hr
    from tests import pose_reference as pr

    xyz, cen, W, rad, axes, moves = refine_molecule()
    F = cpu_field()
    B = len(q)
    n = 6 if theta is None else 6 + theta.shape[1]
    S, G, H = np.zeros(B), np.zeros((B, n)), np.zeros((B, n, n))
    for b in range(B):
        conf = conformer[b] if theta is None else cen[0] + fr.apply_torsions(xyz - cen[0], axes[0], moves, theta[b])
        p = pr.positions(conf, cen[0], q[b], t[b])
        ref = hr.reference(p, F, rad, "atom-wise", w=W, mode="features", precision=32)
        piv = np.asarray(t[b], np.float64).astype(np.float32).astype(np.float64)
        S[b] = ref["s"][0].sum()
        if theta is None:
            G[b], _, H[b], _ = hr.twist(p, ref["g"][0], ref["H"][0], piv)
        else:
            G[b], _, H[b], _ = fr.flex(p, ref["g"][0], ref["H"][0], piv, axes[0], moves)
    return S, G, H


@functools.lru_cache(maxsize=None)
def cpu_refinement():
    """The CPU loops on the starts: (flex state, flex score history, rigid state, rigid history) - the rigid loop is
    refine_posed_batch's on the start conformers."""
    q0, t0, th0 = refine_starts()
    xyz, cen, _, _, axes, moves = refine_molecule()
    st, hist = fr.refine(cpu_evaluate, q0, t0, th0, REFINE_ROUNDS, None, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED)
    conf = np.stack([cen[0] + fr.apply_torsions(xyz - cen[0], axes[0], moves, th0[b]) for b in range(len(q0))])
    rigid, rhist, _ = lm.refine(lambda q, t: cpu_evaluate(q, t, conformer=conf), q0, t0, REFINE_ROUNDS, None, R.LAM_DOWN, R.LAM_UP,
                                R.MAX_DROPPED)
    return st, hist, rigid, rhist


def refine_conditions(history, final, rigid_final):
    """The two conditions of the refinement tests, for every start without exemption: the accepted score never decreases, and
    every start ends above where the rigid refinement of the same start ends."""
    history = np.asarray(history)
    assert (np.diff(history, axis=0) >= 0).all(), np.argwhere(np.diff(history, axis=0) < 0)[:3].tolist()
    assert (np.asarray(final) > np.asarray(rigid_final)).all(), (np.asarray(final).tolist(), np.asarray(rigid_final).tolist())
