"""Many poses refined together by damped Newton steps: examples/refine_pose_newton.py for 256 starts at once.

    python examples/refine_poses_newton.py [steps]

The ligand, the target and the first start are those of refine_pose_newton.py (the 10GS ligand's grid in its crystal pose; a
rotation of 20 degrees and a shift of about 0.7 A); 255 more starts are drawn within 20 degrees and 0.7 A. `refine_posed_views`
takes the ligand once and the 256 poses: every round is one `score_hessian_posed_views` - the scores of all poses with their twist
gradients and Hessians, no grid - and one `lm_step`, which accepts or drops each pose's step on the device, each pose with a
damping of its own; no value comes to the host inside the loop. Prints how many poses end within 0.1 degrees and 0.01 A of the
crystal pose and ends, for pose 0, with refine_pose_newton.py's own assertion on the squared grid difference. Needs an MI355X.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import molvoxel_amd  # noqa: E402
from molvoxel_amd.etc import mol as M  # noqa: E402


def main(steps=40, poses=256):
    import torch

    ligand = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    vox = molvoxel_amd.create_voxelizer(resolution=0.5, dimension=48, density_type="gaussian", library="hip")
    dev = vox.device
    xyz = torch.as_tensor(np.asarray(ligand.coords, np.float64), device=dev)
    offsets = np.array([0, xyz.shape[0]], np.int64)
    center = xyz.mean(0, keepdim=True)                                # (1, 3): the poses rotate about the centroid
    identity = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev, dtype=torch.float64)
    zero = torch.zeros((1, 3), device=dev, dtype=torch.float64)

    def grid_of(q, t):  # channels=None: one density channel, scalar radius 1.5
        return vox.forward_posed_batch(xyz, offsets, center, q / q.norm(dim=1, keepdim=True), t, None, 1.5)

    target = grid_of(identity, zero)
    # pose 0: refine_pose_newton.py's start; the others: random axes, angles up to 20 degrees, shifts up to 0.7 A
    rng = np.random.default_rng(0)
    axis = rng.standard_normal((poses, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.radians(rng.uniform(0.0, 20.0, poses))
    shift = rng.standard_normal((poses, 3))
    shift *= (rng.uniform(0.0, 0.7, poses) / np.linalg.norm(shift, axis=1))[:, None]
    axis[0], angle[0], shift[0] = np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0), math.radians(20.0), [0.4, -0.5, 0.3]
    q0 = torch.tensor(np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis], axis=1), device=dev)
    t0 = torch.tensor(shift, device=dev)

    q, t, S, info = vox.refine_posed_views(xyz, center.repeat(poses, 1), q0, t0, None, 1.5, target[0], steps=steps)

    def off(q, t):  # (degrees, Angstrom) from the crystal pose
        w = (q[:, 0] / q.norm(dim=1)).abs().clamp(max=1.0)
        return torch.rad2deg(2.0 * torch.acos(w)), t.norm(dim=1)

    (a0, s0), (a1, s1) = off(q0, t0), off(q, t)
    home = int(((a1 < 0.1) & (s1 < 0.01)).sum())
    hist = info["score_history"]
    print(f"{poses} poses, {info['evaluations']} evaluations: start off by up to {float(a0.max()):.2f} deg / {float(s0.max()):.3f} A")
    print(f"score of pose 0: {float(hist[0, 0]):.5f} -> {float(S[0]):.5f}; it took {int(info['taken'][0])} steps and ends "
          f"{float(a1[0]):.3f} deg / {float(s1[0]):.4f} A off")
    print(f"steps taken per pose: {float(info['taken'].double().mean()):.1f} on average, {int(info['taken'].max())} at most; "
          f"{int((info['dropped'] >= 3).sum())} poses finished")
    print(f"{home} of {poses} poses end within 0.1 deg and 0.01 A of the crystal pose")
    loss = ((grid_of(q[:1], t[:1]) - target) ** 2).sum()
    assert float(loss) < 0.05 * float((target ** 2).sum()), "the refinement of pose 0 did not come back to the crystal pose"


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
