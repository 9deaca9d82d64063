"""A flexible ligand refined by damped Newton steps in pose and torsion angles: examples/refine_poses_newton.py with rotatable bonds.

    python examples/refine_flex_newton.py [steps] [poses]

The target is the 10GS ligand's grid in its crystal pose and conformer (one density channel, radius 1.5). `torsion_tree` finds the
ligand's rotatable bonds - single, on no ring, not terminal - and the atoms each one turns. Every start perturbs all of them: the
torsion angles by up to 10 degrees, the pose by up to 5 degrees and 0.3 A. `refine_flex_posed_batch` then refines the 6 + T
coordinates of all starts together: every round is one `apply_torsions`, one `score_hessian_flex_posed_batch` - scores, gradients
and (6 + T) x (6 + T) Hessians, no grid - and one `flex_lm_step`, which accepts or drops each start's step on the device. The rigid
`refine_posed_batch` from the same starts, which cannot mend the conformer, is printed next to it. The measure of "refined back"
is the score against the crystal grid, not the angles: the ligand's ends are symmetric groups (a carboxylate, a phenyl ring), and
one density channel cannot tell such a group from itself half a turn on, so a start may settle at the equivalent conformer near
180 degrees. The angles are therefore printed as their distance from the nearest multiple of 180 degrees. Needs an MI355X.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import molvoxel_amd  # noqa: E402
from molvoxel_amd.etc import mol as M  # noqa: E402


def main(steps=40, poses=64):
    import torch

    ligand = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    axes, moves = M.torsion_tree(ligand)
    T, n = axes.shape[0], ligand.num_atoms
    vox = molvoxel_amd.create_voxelizer(resolution=0.5, dimension=48, density_type="gaussian", library="hip")
    dev = vox.device
    xyz = torch.as_tensor(np.asarray(ligand.coords, np.float64), device=dev)
    center = xyz.mean(0, keepdim=True)
    identity = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev, dtype=torch.float64)
    zero = torch.zeros((1, 3), device=dev, dtype=torch.float64)
    target = vox.forward_posed_batch(xyz, np.array([0, n], np.int64), center, identity, zero, None, 1.5)[0].clone()

    rng = np.random.default_rng(0)
    axis = rng.standard_normal((poses, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.radians(rng.uniform(0.0, 5.0, poses))
    shift = rng.standard_normal((poses, 3))
    shift *= (rng.uniform(0.0, 0.3, poses) / np.linalg.norm(shift, axis=1))[:, None]
    q0 = torch.tensor(np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis], axis=1), device=dev)
    t0 = torch.tensor(shift, device=dev)
    theta0 = torch.tensor(np.radians(rng.uniform(-10.0, 10.0, (poses, T))), device=dev)

    # one copy of the ligand per start: the batch form (views cull atoms, and an axis atom may be culled)
    coords, offsets = xyz.repeat(poses, 1), np.arange(poses + 1, dtype=np.int64) * n
    centers = center.repeat(poses, 1)
    all_axes, all_moves = np.tile(axes[None], (poses, 1, 1)), np.tile(moves, poses)
    q, t, theta, S, info = vox.refine_flex_posed_batch(coords, offsets, centers, q0, t0, theta0, None, 1.5, target, all_axes, all_moves,
                                                       steps=steps)
    start = vox.apply_torsions(coords, offsets, all_axes, all_moves, theta0)
    _, _, S_rigid, info_rigid = vox.refine_posed_batch(start, offsets, centers, q0, t0, None, 1.5, target, steps=steps)
    best = float((target.double() ** 2).sum())  # the score of the crystal pose and conformer against its own grid
    hist = info["score_history"]
    print(f"{n} atoms, {T} torsions, {poses} starts, {info['evaluations']} evaluations of {6 + T} coordinates")
    print(f"score / crystal score: start {float(hist[0].mean()) / best:.4f} on average, rigid refinement {float(S_rigid.mean()) / best:.4f}, "
          f"with torsions {float(S.mean()) / best:.4f} (worst start {float(S.min()) / best:.4f})")
    print(f"steps taken per start: {float(info['taken'].double().mean()):.1f} with torsions, "
          f"{float(info_rigid['taken'].double().mean()):.1f} rigid")
    left = torch.rad2deg(theta)
    fold = (left - 180.0 * torch.round(left / 180.0)).abs()  # from the nearest multiple of 180 degrees (symmetric end groups)
    print(f"torsion angles left, from the nearest multiple of 180 degrees: median {float(fold.median()):.2f}, largest "
          f"{float(fold.max()):.2f} degrees (started at up to {float(torch.rad2deg(theta0.abs().max())):.2f}); "
          f"{int((left.abs() > 90.0).sum())} of {left.numel()} settled half a turn on")
    assert bool((S >= S_rigid).all()), "a start ended below its rigid refinement"
    assert float(S.mean()) > 0.98 * best, "the refinement did not come back to the crystal conformer"


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
