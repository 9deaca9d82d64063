"""Pose refinement by damped Newton steps: the ligand, target and start of examples/refine_pose.py, second order.

    python examples/refine_pose_newton.py [steps]

The target is the 10GS ligand's grid in its crystal pose; the start is that pose perturbed by a rotation of about 20 degrees and
a shift of about 0.7 A. Instead of Adam on the squared grid difference, this maximises the score S = sum(target * grid(q, t)) by
Levenberg-Marquardt steps on the six degrees of freedom of the rigid pose: `score_hessian_posed_batch` returns S with its
gradient G and Hessian Hxi under a twist xi = (tau, omega) about the image of the centre - one more walk of the atoms' boxes,
no grid -, the step solves (-Hxi + lambda I) xi = G, and `apply_twist` moves the pose. lambda is multiplied by 10 when the score
does not rise (the step is dropped) and divided by 3 when it does. At most 40 evaluations, fewer when three steps in a row are
dropped (refine_pose.py takes 300 Adam steps). The run ends with refine_pose.py's own assertion on the squared grid
difference, computed once. Needs an MI355X.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import molvoxel_amd  # noqa: E402
from molvoxel_amd.etc import mol as M  # noqa: E402
from molvoxel_amd.voxelizer.hip.voxelizer import apply_twist  # noqa: E402


def main(steps=40):
    import torch

    ligand = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    vox = molvoxel_amd.create_voxelizer(resolution=0.5, dimension=48, density_type="gaussian", library="hip")
    dev = vox.device
    xyz = torch.as_tensor(np.asarray(ligand.coords, np.float64), device=dev)
    offsets = np.array([0, xyz.shape[0]], np.int64)
    center = xyz.mean(0, keepdim=True)                                # (1, 3): the pose rotates about the centroid
    identity = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev, dtype=torch.float64)
    zero = torch.zeros((1, 3), device=dev, dtype=torch.float64)

    def grid_of(q, t):  # channels=None: one density channel, scalar radius 1.5
        return vox.forward_posed_batch(xyz, offsets, center, q / q.norm(dim=1, keepdim=True), t, None, 1.5)

    def score_of(q, t):  # (scores (1,), twist_grad (1, 6), twist_hess (1, 6, 6)) against the target, without a grid
        return vox.score_hessian_posed_batch(xyz, offsets, center, q, t, None, 1.5, target[0])

    def report(step, S, q, t, lam, note=""):
        off = 2.0 * math.degrees(math.acos(min(1.0, abs(float(q[0, 0] / q.norm())))))
        print(f"step {step:3d}: score {float(S):12.5f}   rotation off by {off:6.3f} deg   shift off by {float(t.norm()):.4f} A"
              f"   lambda {lam:9.3g}{note}")

    target = grid_of(identity, zero)
    angle = math.radians(20.0)
    axis = np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)
    q = torch.tensor([[math.cos(angle / 2), *(math.sin(angle / 2) * axis)]], device=dev, dtype=torch.float64)
    t = torch.tensor([[0.4, -0.5, 0.3]], device=dev, dtype=torch.float64)
    S, G, H = score_of(q, t)
    lam = 1e-3 * float(H.abs().max())
    eye = torch.eye(6, device=dev, dtype=torch.float64)
    report(0, S[0], q, t, lam)
    taken = dropped = 0
    for step in range(1, steps + 1):
        xi = torch.linalg.solve(-H[0] + lam * eye, G[0])
        q2, t2 = apply_twist(q, t, xi[None])
        S2, G2, H2 = score_of(q2, t2)
        if float(S2[0]) > float(S[0]):
            q, t, S, G, H = q2, t2, S2, G2, H2
            lam /= 3.0
            taken, dropped = taken + 1, 0
            report(step, S[0], q, t, lam)
        else:
            lam *= 10.0
            dropped += 1
            report(step, S[0], q, t, lam, "   (no rise: step dropped)")
        if dropped == 3:  # three damped steps in a row find no rise: what is left is the truncation at the radius, held fixed
            break
    print(f"{taken} Newton steps taken in {step} evaluations")
    loss = ((grid_of(q, t) - target) ** 2).sum()
    assert float(loss) < 0.05 * float((target ** 2).sum()), "the refinement did not come back to the crystal pose"


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
