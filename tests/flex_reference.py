"""Torsion coordinates restated in numpy float64 (no GPU): the conformer C(theta) of mvx_apply_torsions, the gradient and
Hessian of mvx_score_hessian_flex_batch in x = (tau, omega, theta) from per-atom rows (on tests/hessian_reference.py), and
mvx_flex_lm_step with the refinement loop around it (on tests/lm_reference.py). Shared by tests/test_flex_host.py and
tests/test_hip_flex.py.

One molecule at a time: axes (T, 2) local atom indices (a_k, b_k), moves (N,) int32 read as 32 bits, angles (T,). A torsion is
inert when an axis index is outside [0, N), or the axis has no or no finite length."""
import numpy as np

from tests import hessian_reference as hr
from tests import lm_reference as lm

# A 12-atom tree with a branch and nesting depth 3: atoms 0-2 are the root; torsion 0 turns 3..11 about (2, 3), torsion 1 turns
# 5..8 about (4, 5), torsion 2 turns 7, 8 about (6, 7), torsion 3 - the branch - turns 9..11 about (4, 9).
TREE_AXES = np.array([[2, 3], [4, 5], [6, 7], [4, 9]], np.int32)
TREE_SETS = (range(3, 12), range(5, 9), range(7, 9), range(9, 12))


def tree_moves(n_atoms=12, sets=TREE_SETS):
    m = np.zeros(n_atoms, np.uint32)
    for k, s in enumerate(sets):
        m[list(s)] |= np.uint32(1 << k)
    return m.view(np.int32)


def tree_coords(rng, n_atoms=12, bond=1.5):
    """Positions for the tree: bonded atoms `bond` apart along a bent chain with the branch leaving atom 4; atoms past 11 join
    the root."""
    parent = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 4, 9, 10] + [0] * (n_atoms - 12)
    p = np.zeros((n_atoms, 3))
    for n in range(1, n_atoms):
        d = rng.standard_normal(3) + np.array([1.2, 0.0, 0.0]) * (1 if n < 9 else -1)
        p[n] = p[parent[n]] + bond * d / np.linalg.norm(d)
    return p - p.mean(axis=0)


def bits(moves, k):
    """(N,) bool: the atoms of set k."""
    return ((np.asarray(moves, np.int32).view(np.uint32) >> np.uint32(k)) & np.uint32(1)).astype(bool)


def axis(p, ax):
    """(p_b, unit axis) of the torsion ax = (a, b) at the positions p, or None: inert."""
    N = p.shape[0]
    a, b = int(ax[0]), int(ax[1])
    if not (0 <= a < N and 0 <= b < N):
        return None
    with np.errstate(all="ignore"):
        d = p[b] - p[a]
        len2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if not (len2 > 0.0) or not np.isfinite(len2):
        return None
    return p[b].copy(), d / np.sqrt(len2)


def rotate_about(p, pb, u, th):
    """The points p (M, 3) turned by th about the line through pb along the unit vector u (Rodrigues)."""
    v = p - pb
    return pb + (v * np.cos(th) + np.cross(u, v) * np.sin(th) + np.outer(v @ u, u) * (1.0 - np.cos(th)))


def apply_torsions(coords, axes, moves, angles, order=None, frozen_axes=False):
    """C(theta): for k in `order` (default 0 .. T-1) the atoms of set k are turned by angles[k] about the current axis
    (a_k, b_k) through b_k. frozen_axes: the axes of the input conformer are used throughout (with order T-1 .. 0 this is the
    same conformer). An angle of exactly 0 and an inert torsion turn nothing."""
    p = np.array(coords, np.float64).reshape(-1, 3)
    p0 = p.copy()
    T = len(axes)
    for k in (range(T) if order is None else order):
        ax = axis(p0 if frozen_axes else p, axes[k])
        if ax is None or angles[k] == 0.0:
            continue
        sel = bits(moves, k)
        with np.errstate(all="ignore"):
            p[sel] = rotate_about(p[sel], ax[0], ax[1], float(angles[k]))
    return p


def reach(coords, axes, moves):
    """L: the largest distance of an atom from the point b_k of a torsion that turns it."""
    p = np.asarray(coords, np.float64).reshape(-1, 3)
    L = 0.0
    for k in range(len(axes)):
        if axis(p, axes[k]) is not None and bits(moves, k).any():
            L = max(L, float(np.linalg.norm(p[bits(moves, k)] - p[int(axes[k][1])], axis=1).max()))
    return L


def _abs_cross(a, b):
    """The bound of a x b from bounds of |a| and |b|."""
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def flex(p, g, H, pivot, axes, moves, bg=None, bH=None):
    """Gradient (n,) and Hessian (n, n), n = 6 + T, of S = sum_n s_n(p_n) at x = 0 in x = (tau, omega, theta) with
    p_n(x) = exp([omega]x) (C(theta)_n - pivot) + pivot + tau, from the positions p (N, 3), gradients g (N, 3) and Hessians H
    (N, 6 | N, 3, 3) of the atoms. With r_n = p_n - pivot, J_n = [I | -[r_n]x], u_k the unit axis, s_k = ((p_b - pivot) x u_k, u_k)
    and, over the atoms of set k whose rows are not all zero, F_k = sum g_n, N_k = sum r_n x g_n, X_k = sum J_n^T H_n J_n,
    K_k = sum r_n g_n^T, c_k = tau_k x F_k + (K_k - tr(K_k) I) u_k:
      G[:6], Hx[:6, :6] = hessian_reference.twist       G[6 + k] = s_k . (F_k, N_k)       Hx[:6, 6 + k] = X_k s_k + (0, c_k)
      Hx[6 + k, 6 + l] = s_k^T X_l s_l + u_k . c_l for k = l or an ancestor of l (bit k of moves[b_l]), else 0; mirrored.
    Returns (G, bound of G, Hx, bound of Hx): the bounds are the same formulas on absolute values (bg, bH: default |g|, |H|)."""
    p, g = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(g, np.float64).reshape(-1, 3)
    H = np.asarray(H, np.float64)
    H = hr.full(H) if H.shape[-1] == 6 else H
    bg = np.abs(g) if bg is None else np.asarray(bg, np.float64).reshape(-1, 3)
    bH = np.abs(H) if bH is None else (hr.full(bH) if np.asarray(bH).shape[-1] == 6 else np.asarray(bH, np.float64))
    pivot = np.asarray(pivot, np.float64)
    T = len(axes)
    n = 6 + T
    G, bG, X, bX = np.zeros(n), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    G[:6], bG[:6], X[:6, :6], bX[:6, :6] = hr.twist(p, g, H, pivot, bg, bH)
    live = [n_ for n_ in range(p.shape[0]) if g[n_].any() or H[n_].any()]
    tors = [None] * T
    mv = np.asarray(moves, np.int32).view(np.uint32)
    for k in range(T):
        ax = axis(p, axes[k])
        if ax is None:
            continue
        pb, u = ax
        sel = bits(moves, k)
        F, bF, Nn, bN = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
        Xk, bXk, K, bK = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((3, 3)), np.zeros((3, 3))
        for a in live:
            if not sel[a]:
                continue
            r = p[a] - pivot
            ra = np.abs(r)
            J = np.concatenate([np.eye(3), -hr.cross_matrix(r)], axis=1)
            Ja = np.abs(J)
            F += g[a]
            bF += bg[a]
            Nn += np.cross(r, g[a])
            bN += _abs_cross(ra, bg[a])
            Xk += J.T @ H[a] @ J
            bXk += Ja.T @ bH[a] @ Ja
            K += np.outer(r, g[a])
            bK += np.outer(ra, bg[a])
        rb = pb - pivot
        tau, btau, ua = np.cross(rb, u), _abs_cross(np.abs(rb), np.abs(u)), np.abs(u)
        s, bs = np.concatenate([tau, u]), np.concatenate([btau, ua])
        c = np.cross(tau, F) + (K - np.trace(K) * np.eye(3)) @ u
        bc = _abs_cross(btau, bF) + (bK + np.trace(bK) * np.eye(3)) @ ua
        y, by = Xk @ s, bXk @ bs
        tors[k] = (s, bs, y, by, c, bc, int(mv[int(axes[k][1])]))
        G[6 + k], bG[6 + k] = s @ np.concatenate([F, Nn]), bs @ np.concatenate([bF, bN])
        col, bcol = y.copy(), by.copy()
        col[3:] += c
        bcol[3:] += bc
        X[:6, 6 + k] = X[6 + k, :6] = col
        bX[:6, 6 + k] = bX[6 + k, :6] = bcol
    for l in range(T):
        if tors[l] is None:
            continue
        _, _, y, by, c, bc, mb = tors[l]
        for k in range(l + 1):
            if tors[k] is None or not (mb >> k) & 1:
                continue
            s, bs = tors[k][0], tors[k][1]
            X[6 + k, 6 + l] = X[6 + l, 6 + k] = s @ y + s[3:] @ c
            bX[6 + k, 6 + l] = bX[6 + l, 6 + k] = bs @ by + bs[3:] @ bc
    return G, bG, X, bX


def positions(conformer, pivot, x):
    """p_n(x) = exp([omega]x) (C(theta)_n - pivot) + pivot + tau for the conformer C(theta) given."""
    R = hr.exp_so3(x[3:6])
    return (np.asarray(conformer) - pivot) @ R.T + pivot + x[:3]


# ---- the step and the loop in n = 6 + T dimensions -----------------------------------------------------------------------------
def solve(H, G, lam):
    """x of (-H + lam I) x = G, or None: a singular matrix or a non-finite component."""
    G = np.asarray(G, np.float64)
    n = G.shape[0]
    with np.errstate(all="ignore"):
        A = lam * np.eye(n) - np.asarray(H, np.float64).reshape(n, n)
        try:
            x = np.linalg.solve(A, G)
        except np.linalg.LinAlgError:
            return None
    return x if np.isfinite(x).all() else None


class State(lm.State):
    """lm_reference.State with theta (B, T), G (B, n) and H (B, n, n); after a step q2, t2, theta2 and x (B, n)."""

    def __init__(self, q, t, theta, S, G, H, lam, taken=None, dropped=None):
        B = len(q)
        self.q, self.t, self.S = np.array(q, np.float64), np.array(t, np.float64), np.array(S, np.float64)
        self.theta = np.array(theta, np.float64).reshape(B, -1)
        n = 6 + self.theta.shape[1]
        self.G, self.H, self.lam = np.array(G, np.float64).reshape(B, n), np.array(H, np.float64).reshape(B, n, n), np.array(lam, np.float64)
        self.taken = np.zeros(B, np.int32) if taken is None else np.array(taken, np.int32)
        self.dropped = np.zeros(B, np.int32) if dropped is None else np.array(dropped, np.int32)
        self.q2 = self.t2 = self.theta2 = self.x = None


def step(st, trial=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, x_from=None):
    """One mvx_flex_lm_step on `st`, in place: lm_reference.step with the angles next to the pose. x_from: (B, n) steps to use
    in place of the solve where the solve succeeds. Returns the per-pose decisions: 'accept' | 'drop' | None."""
    B, T = st.theta.shape
    n = 6 + T
    decisions = [None] * B
    q2, t2, th2, xs = np.empty((B, 4)), np.empty((B, 3)), np.empty((B, T)), np.zeros((B, n))
    for b in range(B):
        if trial is not None and st.dropped[b] < max_dropped:
            S2, G2, H2 = trial
            if S2[b] > st.S[b]:
                st.q[b], st.t[b], st.theta[b], st.S[b] = st.q2[b], st.t2[b], st.theta2[b], S2[b]
                st.G[b], st.H[b] = G2[b], np.asarray(H2[b]).reshape(n, n)
                st.lam[b] = st.lam[b] * lam_down
                st.taken[b] += 1
                st.dropped[b] = 0
                decisions[b] = "accept"
            else:
                st.lam[b] = st.lam[b] * lam_up
                st.dropped[b] += 1
                decisions[b] = "drop"
        q2[b], t2[b], th2[b] = st.q[b], st.t[b], st.theta[b]
        if st.dropped[b] >= max_dropped:
            continue
        x = solve(st.H[b], st.G[b], st.lam[b])
        if x is None or not (np.isfinite(st.q[b]).all() and np.isfinite(st.t[b]).all() and np.isfinite(st.theta[b]).all()
                             and np.isfinite(st.lam[b])):
            continue
        if x_from is not None:
            x = np.asarray(x_from[b], np.float64)
        with np.errstate(all="ignore"):
            qq, tt = lm.apply_twist(st.q[b], st.t[b], x[:6])
            hh = st.theta[b] + x[6:]
        if not (np.isfinite(qq).all() and np.isfinite(tt).all() and np.isfinite(hh).all()):
            continue
        q2[b], t2[b], th2[b], xs[b] = qq, tt, hh, x
    st.q2, st.t2, st.theta2, st.x = q2, t2, th2, xs
    return decisions


def residual_ratio(H, G, lam, x):
    """lm_reference.residual_ratio for an n-dimensional system."""
    n = np.asarray(G).shape[0]
    A = np.asarray(lam, np.longdouble) * np.eye(n, dtype=np.longdouble) - np.asarray(H, np.longdouble).reshape(n, n)
    xv, g = np.asarray(x, np.longdouble), np.asarray(G, np.longdouble)
    r = np.abs(A @ xv - g).max()
    scale = np.abs(A).sum(axis=1).max() * np.abs(xv).max() + np.abs(g).max()
    return float(r / (np.longdouble(2.0) ** -52 * scale))


def refine(evaluate, q, t, theta, steps, lam0=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3):
    """The loop of refine_flex_posed_batch on the CPU: evaluate(q, t, theta) -> (S (B,), G (B, n), H (B, n, n)). Returns
    (state, score_history (steps + 1, B))."""
    S, G, H = evaluate(np.asarray(q, np.float64), np.asarray(t, np.float64), np.asarray(theta, np.float64))
    B = len(S)
    lam = 1e-3 * np.abs(np.asarray(H).reshape(B, -1)).max(axis=1) if lam0 is None else np.broadcast_to(np.asarray(lam0, np.float64), (B,))
    st = State(q, t, theta, S, G, H, lam)
    kw = dict(lam_down=lam_down, lam_up=lam_up, max_dropped=max_dropped)
    history = np.empty((steps + 1, B))
    history[0] = st.S
    step(st, **kw)
    for r in range(steps):
        step(st, evaluate(st.q2, st.t2, st.theta2), **kw)
        history[r + 1] = st.S
    return st, history
