"""Quaternion helpers for the host side of the HIP backend.

RNG-order and arithmetic-order compatible with the reference (molvoxel/voxelizer/numpy/_quaternion.py:13-50):
a uniform unit quaternion from three np.random.rand draws, rotation as q * (0, p) * q^-1 evaluated
with the same products and the same left-to-right sums, so seeded results are identical. The device
applies the same expression tree in fp64 (csrc/mvx_device.h: apply_xform).
"""
from __future__ import annotations

import math

import numpy as np

TWO_PI = 2 * math.pi


def random_quaternion():
    """Draws exactly three uniforms from the global numpy RNG (_quaternion.py:13-21)."""
    u1, u2, u3 = np.random.rand(3)
    a, b = math.sqrt(1 - u1), math.sqrt(u1)
    return (a * math.sin(TWO_PI * u2), a * math.cos(TWO_PI * u2), b * math.sin(TWO_PI * u3), b * math.cos(TWO_PI * u3))


def _hamilton(p, q):
    p0, p1, p2, p3 = p
    q0, q1, q2, q3 = q
    return (
        p0 * q0 - p1 * q1 - p2 * q2 - p3 * q3,
        p0 * q1 + p1 * q0 + p2 * q3 - p3 * q2,
        p0 * q2 - p1 * q3 + p2 * q0 + p3 * q1,
        p0 * q3 + p1 * q2 - p2 * q1 + p3 * q0,
    )


def rotate(points: np.ndarray, quaternion) -> np.ndarray:
    """(N, 3) -> (N, 3): q * (0, p) * conj(q) (_quaternion.py:45-50)."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    conj = (quaternion[0], quaternion[1] * -1, quaternion[2] * -1, quaternion[3] * -1)
    _, rx, ry, rz = _hamilton(_hamilton(quaternion, (np.zeros_like(x), x, y, z)), conj)
    return np.stack([rx, ry, rz], axis=-1)


def apply_twist(quaternions, translations, twist):
    """(q', t') of the poses (quaternions (B, 4), translations (B, 3)) moved by the twists xi = (tau, omega) (B, 6) that
    score_hessian_posed_batch differentiates along: q' = u (x) q with u = (cos(|w|/2), sin(|w|/2) w/|w|) the unit quaternion of
    the rotation vector w = omega, and t' = t + tau. With the pivot at the image of the centre (the default of
    score_hessian_posed_batch) the posed atoms move to p' = exp([omega]x) (p - t) + t + tau exactly; q is used as given (an
    unnormalised q keeps its norm). Torch ops in float64 on the inputs' device; safe at |w| = 0."""
    import torch

    def as_f64(x, like=None):
        x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))
        return x.to(dtype=torch.float64) if like is None else x.to(device=like.device, dtype=torch.float64)

    q = as_f64(quaternions)
    t, xi = as_f64(translations, q), as_f64(twist, q)
    tau, w = xi[:, :3], xi[:, 3:]
    half = 0.5 * torch.linalg.vector_norm(w, dim=1, keepdim=True)
    # sin(|w|/2) w/|w| = 0.5 sinc(|w|/2) w, with torch.sinc(x) = sin(pi x) / (pi x) and sinc(0) = 1
    v = 0.5 * torch.sinc(half / math.pi) * w
    u = (torch.cos(half)[:, 0], v[:, 0], v[:, 1], v[:, 2])
    return torch.stack(_hamilton(u, (q[:, 0], q[:, 1], q[:, 2], q[:, 3])), dim=1), t + tau
