"""The adjoint of the conformer C(theta) (mvx_apply_torsions_backward) restated in numpy float64 on top of tests/flex_reference.py
(no GPU), one molecule at a time. Shared by tests/test_torsion_grad_host.py and tests/test_hip_torsion_grad.py.

The forward is a program of T dependent turns; the adjoint runs it in reverse, k = T-1 .. 0. With c = cos theta_k, s = sin theta_k,
R = c I + s [u]x + (1 - c) u u^T about the unit axis u from p_a to p_b, for every atom n of set k whose current row ybar_n is not
all zero, w = y_n - p_b the position behind the turn and v = R^T w the position in front of it:
    theta_bar_k += ybar_n . (u x w)        xbar_n = R^T ybar_n        b_bar += ybar_n - R^T ybar_n
    u_bar += s (v x ybar_n) + (1 - c) ((u . v) ybar_n + (u . ybar_n) v)
and behind the sums d_bar = (u_bar - u (u . u_bar)) / |p_b - p_a|, xbar_b += b_bar + d_bar, xbar_a -= d_bar. An angle of exactly
0 moves neither positions nor rows (theta_bar_k is still formed); an inert torsion gives theta_bar_k = +0.0 and touches nothing.

Two forms: `stored` sweeps over the positions the forward stored in front of every turn (`stored_from`: the same sweep for a
conformer that is given, over its pre-images); `undone` starts from the conformer the forward returned and undoes the turns, as
the device does. Each returns (grad_coords (N, 3), grad_angles (T,), bound of
grad_coords, bound of grad_angles): the bounds are the same sweep on absolute values (|ybar|, the entries of |R|, |v|, |w|,
1 / |p_b - p_a|)."""
import numpy as np

from tests import flex_reference as fr

# The Adam loop of the refinement tests: learning rate and steps, chosen on the numpy loop of tests/test_torsion_grad_host.py
# (torch.optim.Adam's other defaults). Learning rates 0.01 ... 0.03 with 12 ... 20 steps all gain 22 or more on every start.
ADAM_LR, ADAM_STEPS = 0.01, 20


def bar_factor(n_atoms, axes):
    """(N_b + 128)(T_b + 1) 2^-53, the factor in front of the bound in |got - ref| <= factor * bound: float64 sums of at most
    N_b terms with under 128 roundings per term, compounded over at most T_b + 1 levels; T_b counts the torsions of the molecule
    that are not padding."""
    return (n_atoms + 128) * (int((np.asarray(axes)[:, 0] >= 0).sum()) + 1) * 2.0 ** -53


def forward_stored(coords, axes, moves, angles):
    """(C(theta), [positions in front of turn k for k = 0 .. T-1]): flex_reference.apply_torsions, turn by turn."""
    p = np.array(coords, np.float64).reshape(-1, 3)
    before = []
    for k in range(len(axes)):
        before.append(p.copy())
        ax = fr.axis(p, axes[k])
        if ax is None or angles[k] == 0.0:
            continue
        sel = fr.bits(moves, k)
        with np.errstate(all="ignore"):
            p[sel] = fr.rotate_about(p[sel], ax[0], ax[1], float(angles[k]))
    return p, before


def _rotation(u, th):
    c, s = np.cos(th), np.sin(th)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(u, u)


def _sweep(conformer, axes, moves, angles, grad, before=None):
    y = np.array(conformer, np.float64).reshape(-1, 3)  # the working positions
    g = np.array(grad, np.float64).reshape(-1, 3)  # the working rows
    bg = np.abs(g)
    T = len(axes)
    ga, bga = np.zeros(T), np.zeros(T)
    for k in range(T - 1, -1, -1):
        p_front = y if before is None else before[k]
        ax = fr.axis(p_front, axes[k])  # (a_k is in no later set and b_k is a fixed point: the axis in front of the turn)
        if ax is None:
            continue
        pb, u = ax
        ia, ib = int(axes[k][0]), int(axes[k][1])
        length = float(np.linalg.norm(p_front[ib] - p_front[ia]))
        th = float(angles[k])
        turn = th != 0.0
        R = _rotation(u, th) if turn else np.eye(3)
        Ra, ua = np.abs(R), np.abs(u)
        c1, s = 1.0 - np.cos(th), np.sin(th)
        bbar, ubar, bbb, bub = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
        for n in np.flatnonzero(fr.bits(moves, k)):
            with np.errstate(all="ignore"):
                w = y[n] - pb
                v = (before[k][n] - pb) if before is not None else (R.T @ w if turn else w)
                if turn:
                    y[n] = (pb + v) if before is None else before[k][n]
            if not g[n].any():
                continue
            yb, byb = g[n].copy(), bg[n].copy()
            ga[k] += yb @ np.cross(u, w)
            bga[k] += byb @ fr._abs_cross(ua, np.abs(w))
            if not turn:
                continue
            g[n], bg[n] = R.T @ yb, Ra.T @ byb
            bbar += yb - g[n]
            bbb += byb + bg[n]
            ubar += s * np.cross(v, yb) + c1 * ((u @ v) * yb + (u @ yb) * v)
            bub += abs(s) * fr._abs_cross(np.abs(v), byb) + abs(c1) * ((ua @ np.abs(v)) * byb + (ua @ byb) * np.abs(v))
        if turn:
            d = (ubar - u * (u @ ubar)) / length
            bd = (bub + ua * (ua @ bub)) / length
            g[ib] += bbar + d
            bg[ib] += bbb + bd
            g[ia] -= d
            bg[ia] += bd
    return g, ga, bg, bga


def stored(coords, axes, moves, angles, grad):
    """Form (a): the sweep over the positions the forward stored in front of every turn, made here from the reference conformer
    `coords`."""
    conformer, before = forward_stored(coords, axes, moves, angles)
    return _sweep(conformer, axes, moves, angles, grad, before)


def preimages(conformer, axes, moves, angles):
    """[positions in front of turn k for k = 0 .. T-1] that belong to a conformer which is given, not made here: its own
    pre-images, the turns taken back last first in np.longdouble and each result rounded to float64 once. (A forward run
    here from the reference coordinates ends at another conformer than the device's, apart by the forward's own rounding -
    up to 64 T 2^-53 L at the magnitude of the absolute coordinates -, and w = y_n - p_b taken between the two is off by
    that much on a bond length.)"""
    y = np.array(conformer, np.longdouble).reshape(-1, 3)
    T = len(axes)
    before = [None] * T
    for k in range(T - 1, -1, -1):
        if fr.axis(y.astype(np.float64), axes[k]) is not None and angles[k] != 0.0:  # (inert: decided in float64, as the forward does)
            ia, ib = int(axes[k][0]), int(axes[k][1])
            d = y[ib] - y[ia]
            u, pb = d / np.sqrt((d * d).sum()), y[ib].copy()
            c, s = np.cos(np.longdouble(angles[k])), np.sin(np.longdouble(angles[k]))
            sel = fr.bits(moves, k)
            with np.errstate(all="ignore"):
                v = y[sel] - pb
                y[sel] = pb + (v * c - np.cross(u[None], v) * s + (v @ u)[:, None] * u[None] * (1 - c))  # R^T: the turn by -theta_k
        before[k] = y.astype(np.float64)
    return before


def stored_from(conformer, axes, moves, angles, grad):
    """Form (a) fed a conformer that is given (the device's own): the sweep over its pre-images as the stored positions."""
    return _sweep(conformer, axes, moves, angles, grad, preimages(conformer, axes, moves, angles))


def undone(conformer, axes, moves, angles, grad):
    """Form (b): from the conformer the forward returned, the turns undone inside the sweep - the device's program."""
    return _sweep(conformer, axes, moves, angles, grad, None)


def shortcut_angles(conformer, axes, moves, grad):
    """theta_bar_k = u_k . sum over M_k of (C_n - C_{b_k}) x g_n on the final conformer and the upstream rows (the torque about
    the final axis; a turn of a nested set about an axis inside set k does not change it)."""
    C_, g = np.asarray(conformer, np.float64).reshape(-1, 3), np.asarray(grad, np.float64).reshape(-1, 3)
    out = np.zeros(len(axes))
    for k in range(len(axes)):
        ax = fr.axis(C_, axes[k])
        if ax is None:
            continue
        sel = fr.bits(moves, k) & g.any(axis=1)
        out[k] = ax[1] @ np.cross(C_[sel] - ax[0], g[sel]).sum(axis=0)
    return out
