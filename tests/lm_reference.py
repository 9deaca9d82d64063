"""mvx_lm_step restated in numpy float64 (no GPU): the same per-pose state machine, np.linalg.solve for the 6x6 system with the
same failure rule, and apply_twist's formula. Shared by tests/test_lm_host.py (the reference itself and the CPU refinement loop)
and the GPU tests (tests/test_hip_lm_step.py)."""
import numpy as np


def hamilton(p, q):
    p0, p1, p2, p3 = p
    q0, q1, q2, q3 = q
    return np.array([p0 * q0 - p1 * q1 - p2 * q2 - p3 * q3,
                     p0 * q1 + p1 * q0 + p2 * q3 - p3 * q2,
                     p0 * q2 - p1 * q3 + p2 * q0 + p3 * q1,
                     p0 * q3 + p1 * q2 - p2 * q1 + p3 * q0])


def apply_twist(q, t, xi):
    """(q2, t2) of one pose moved by the twist xi = (tau, omega): u = (cos(|w|/2), 0.5 sinc(|w|/2) w), q2 = u (x) q, t2 = t + tau;
    w = 0 gives q2 = q exactly."""
    q, t, xi = (np.asarray(x, np.float64) for x in (q, t, xi))
    w = xi[3:]
    half = 0.5 * np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if half == 0.0:
        return q.copy(), t + xi[:3]
    v = 0.5 * (np.sin(half) / half) * w
    return hamilton((np.cos(half), v[0], v[1], v[2]), q), t + xi[:3]


def solve(H, G, lam):
    """xi of (-H + lam I) xi = G, or None: a singular matrix or a non-finite component."""
    with np.errstate(all="ignore"):
        A = lam * np.eye(6) - np.asarray(H, np.float64).reshape(6, 6)
        try:
            xi = np.linalg.solve(A, np.asarray(G, np.float64))
        except np.linalg.LinAlgError:
            return None
    return xi if np.isfinite(xi).all() else None


class State:
    """B poses as numpy arrays: q (B, 4), t (B, 3), S (B,), G (B, 6), H (B, 6, 6), lam (B,), taken, dropped (B,) int32; after a
    step q2 (B, 4), t2 (B, 3), xi (B, 6)."""

    def __init__(self, q, t, S, G, H, lam, taken=None, dropped=None):
        B = len(q)
        self.q, self.t, self.S = np.array(q, np.float64), np.array(t, np.float64), np.array(S, np.float64)
        self.G, self.H, self.lam = np.array(G, np.float64), np.array(H, np.float64).reshape(B, 6, 6), np.array(lam, np.float64)
        self.taken = np.zeros(B, np.int32) if taken is None else np.array(taken, np.int32)
        self.dropped = np.zeros(B, np.int32) if dropped is None else np.array(dropped, np.int32)
        self.q2 = self.t2 = self.xi = None

    def copy(self):
        out = State(self.q, self.t, self.S, self.G, self.H, self.lam, self.taken, self.dropped)
        if self.q2 is not None:
            out.q2, out.t2, out.xi = self.q2.copy(), self.t2.copy(), self.xi.copy()
        return out


def step(st, trial=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, xi_from=None):
    """One mvx_lm_step on `st`, in place. trial: (S2, G2, H2) evaluated at (st.q2, st.t2), or None. xi_from: (B, 6) twists to use
    in place of the solve where the solve succeeds (the kernel's own, to judge its q2 and t2). Returns the per-pose decisions:
    'accept' | 'drop' | None (no decision: no trial, or finished before the call)."""
    B = len(st.q)
    decisions = [None] * B
    q2, t2, xi = np.empty((B, 4)), np.empty((B, 3)), np.zeros((B, 6))
    for b in range(B):
        if trial is not None and st.dropped[b] < max_dropped:
            S2, G2, H2 = trial
            if S2[b] > st.S[b]:
                st.q[b], st.t[b], st.S[b], st.G[b], st.H[b] = st.q2[b], st.t2[b], S2[b], G2[b], np.asarray(H2[b]).reshape(6, 6)
                st.lam[b] = st.lam[b] * lam_down
                st.taken[b] += 1
                st.dropped[b] = 0
                decisions[b] = "accept"
            else:
                st.lam[b] = st.lam[b] * lam_up
                st.dropped[b] += 1
                decisions[b] = "drop"
        q2[b], t2[b] = st.q[b], st.t[b]
        if st.dropped[b] >= max_dropped:
            continue
        x = solve(st.H[b], st.G[b], st.lam[b])
        if x is None or not (np.isfinite(st.q[b]).all() and np.isfinite(st.t[b]).all() and np.isfinite(st.lam[b])):
            continue
        if xi_from is not None:
            x = np.asarray(xi_from[b], np.float64)
        with np.errstate(all="ignore"):
            qq, tt = apply_twist(st.q[b], st.t[b], x)
        if not (np.isfinite(qq).all() and np.isfinite(tt).all()):
            continue
        q2[b], t2[b], xi[b] = qq, tt, x
    st.q2, st.t2, st.xi = q2, t2, xi
    return decisions


def residual_ratio(H, G, lam, xi):
    """||A xi - G||_inf / (2^-52 (||A||_inf ||xi||_inf + ||G||_inf)) with A = -H + lam I, evaluated in np.longdouble."""
    A = np.asarray(lam, np.longdouble) * np.eye(6, dtype=np.longdouble) - np.asarray(H, np.longdouble).reshape(6, 6)
    x, g = np.asarray(xi, np.longdouble), np.asarray(G, np.longdouble)
    r = np.abs(A @ x - g).max()
    scale = np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(g).max()
    return float(r / (np.longdouble(2.0) ** -52 * scale))


def refine(evaluate, q, t, steps, lam0=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3):
    """The loop of refine_posed_batch on the CPU: evaluate(q (B, 4), t (B, 3)) -> (S (B,), G (B, 6), H (B, 6, 6)). Returns
    (state, score_history (steps + 1, B), the first trial pose (q2, t2))."""
    S, G, H = evaluate(np.asarray(q, np.float64), np.asarray(t, np.float64))
    B = len(S)
    lam = 1e-3 * np.abs(np.asarray(H).reshape(B, 36)).max(axis=1) if lam0 is None else np.broadcast_to(np.asarray(lam0, np.float64), (B,))
    st = State(q, t, S, G, H, lam)
    kw = dict(lam_down=lam_down, lam_up=lam_up, max_dropped=max_dropped)
    history = np.empty((steps + 1, B))
    history[0] = st.S
    step(st, **kw)
    first = (st.q2.copy(), st.t2.copy())
    for r in range(steps):
        step(st, evaluate(st.q2, st.t2), **kw)
        history[r + 1] = st.S
    return st, history, first
