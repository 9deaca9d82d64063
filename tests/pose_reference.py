"""float64 restatement of explicit rigid poses (forward_posed_batch / forward_posed_views, mvx_pose_grad_batch).

Positions: a pose (c, q, t) maps x to p = q (x - c) conj(q) + float32(t): the centre subtracted, the sandwich product in
_quaternion.rotate's operation order (the library is built without fused multiply-adds, so these are the kernel's doubles), the
translation rounded to float32 as the record stores it and added once. q is used as given: M(q) scales by |q|^2.

Chain rule: with G_n = dL/dp_n and its bound b_n (tests/grad_reference.reference on the posed positions, without `rot`) and
x'_n = x_n - c:
    dL/dt   = sum_n G_n                          bound sum_n b_n                  (straight through the float32 rounding)
    dL/dq_k = sum_n G_n . (dM/dq_k x'_n)         bound sum_n b_n . |dM/dq_k x'_n|
    dL/dc   = -sum_n M^T G_n                     bound sum_n |M|^T b_n
"""
import numpy as np

from molvoxel_amd.voxelizer.hip import _quaternion


def rotation(q):
    """M(q), the matrix of x -> q x conj(q) (make_xform_f32 writes it out); M M^T = |q|^4 I."""
    q0, q1, q2, q3 = (float(v) for v in q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def rotation_derivatives(q):
    """(4, 3, 3): dM/dq_k."""
    q0, q1, q2, q3 = (float(v) for v in q)
    return 2.0 * np.array([[[q0, -q3, q2], [q3, q0, -q1], [-q2, q1, q0]],
                           [[q1, q2, q3], [q2, -q1, -q0], [q3, q0, -q1]],
                           [[-q2, q1, q0], [q1, q2, q3], [-q0, q3, -q2]],
                           [[-q3, -q0, q1], [q0, -q3, q2], [q1, q2, q3]]])


def positions(xyz, center, quaternion, translation, round_translation=True):
    """(N, 3) float64: the atoms as the kernels see them under the pose."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    c = np.zeros(3) if center is None else np.asarray(center, np.float64).reshape(3)
    t = np.asarray(translation, np.float64).reshape(3)
    if round_translation:
        t = t.astype(np.float32).astype(np.float64)
    q = tuple(float(v) for v in np.asarray(quaternion, np.float64).reshape(4))
    return _quaternion.rotate(xyz - c, q) + t


def batch_positions(xyz, offsets, centers, quaternions, translations):
    """positions() molecule by molecule for atoms stored back to back."""
    out = np.empty((int(offsets[-1]), 3))
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        out[lo:hi] = positions(xyz[lo:hi], None if centers is None else centers[b], quaternions[b], translations[b])
    return out


def view_positions(xyz, centers, quaternions, translations):
    """(B, N, 3): one shared cloud under B poses."""
    return np.stack([positions(xyz, centers[b], quaternions[b], translations[b]) for b in range(len(quaternions))])


def pose_grads(xyz, center, quaternion, G, b):
    """{"center": (3,), "quaternion": (4,), "translation": (3,)} as (value, bound) pairs from per-atom dL/dp = G (N, 3) with
    bounds b (N, 3) on the sums of the absolute values of their terms."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    c = np.zeros(3) if center is None else np.asarray(center, np.float64).reshape(3)
    G, b = np.asarray(G, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    xp = xyz - c
    M, dM = rotation(quaternion), rotation_derivatives(quaternion)
    dq, bq = np.zeros(4), np.zeros(4)
    for k in range(4):
        v = xp @ dM[k].T  # rows dM/dq_k x'_n
        dq[k] = (G * v).sum()
        bq[k] = (b * np.abs(v)).sum()
    return {"translation": (G.sum(0), b.sum(0)),
            "quaternion": (dq, bq),
            "center": (-(G @ M).sum(0), (b @ np.abs(M)).sum(0))}


def from_coords_grad(xyz, center, quaternion, gc):
    """The same three gradients from the call's own dL/dcoords = M^T dL/dp (gc, (N, 3)): dL/dp_n = M gc_n / |q|^4, evaluated
    in float64. Returns (value, sum of the absolute values of the terms) pairs, the scale of a summation-order tolerance."""
    M = rotation(quaternion)
    n4 = float(np.sum(np.asarray(quaternion, np.float64) ** 2)) ** 2
    gc = np.asarray(gc, np.float64).reshape(-1, 3)
    G = gc @ M.T / n4
    A = np.abs(gc) @ np.abs(M).T / n4
    out = pose_grads(xyz, center, quaternion, G, A)
    out["center"] = (-gc.sum(0), np.abs(gc).sum(0))
    return out
