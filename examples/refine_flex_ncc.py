"""A flexible ligand fitted into a density map with a torch optimiser: examples/refine_pose_ncc.py with rotatable bonds.

    python examples/refine_flex_ncc.py [steps] [poses]

The target is the 10GS ligand's grid in its crystal pose and conformer (one density channel, radius 1.5). `torsion_tree` finds the
ligand's 15 rotatable bonds and the atoms each one turns. Every start perturbs all of them: the torsion angles by up to 15
degrees, the pose by up to 10 degrees and 0.5 A. The loss is -NCC, built from the moments of the posed conformer's grid,

    conformer = apply_torsions(coords, offsets, axes, moves, theta)
    m = moments_posed_batch(conformer, offsets, centers, q / |q|, t, None, 1.5, target=target)
    NCC = m[..., 2] / sqrt(m[..., 1] * sum(target ** 2))

on a voxelizer made with `moments_grad=True` and `torsion_grad=True`: `apply_torsions` is then part of the autograd graph, and
`torch.optim.Adam([q, t, theta])` refines the poses and the torsion angles of all starts together. Every step is one
`apply_torsions`, one `moments_posed_batch` and one `backward()` - no grid of the ligand is written, and the turns are not rebuilt
from torch operations: the backward pass of the conformer is one launch (mvx_apply_torsions_backward). Next to it the rigid run
from the same starts - the start conformers, `Adam([q, t])` -, which cannot mend the conformer. NCC cannot tell a symmetric end
group (a carboxylate, a phenyl ring) from itself half a turn on, so the measure is the NCC, not the angles. Needs an MI355X.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import molvoxel_amd  # noqa: E402
from molvoxel_amd.etc import mol as M  # noqa: E402


def main(steps=300, poses=16):
    import torch

    ligand = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    axes, moves = M.torsion_tree(ligand)
    T, n = axes.shape[0], ligand.num_atoms
    vox = molvoxel_amd.create_voxelizer(resolution=0.5, dimension=48, density_type="gaussian", library="hip", differentiable=True,
                                        moments_grad=True, torsion_grad=True)
    dev = vox.device
    xyz = torch.as_tensor(np.asarray(ligand.coords, np.float64), device=dev)
    center = xyz.mean(0, keepdim=True)
    identity = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev, dtype=torch.float64)
    zero = torch.zeros((1, 3), device=dev, dtype=torch.float64)
    with torch.no_grad():
        target = vox.forward_posed_batch(xyz, np.array([0, n], np.int64), center, identity, zero, None, 1.5)[0].clone()
    tt = (target.double() ** 2).sum()

    rng = np.random.default_rng(0)
    axis = rng.standard_normal((poses, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.radians(rng.uniform(0.0, 10.0, poses))
    shift = rng.standard_normal((poses, 3))
    shift *= (rng.uniform(0.0, 0.5, poses) / np.linalg.norm(shift, axis=1))[:, None]
    q0 = torch.tensor(np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis], axis=1), device=dev)
    t0 = torch.tensor(shift, device=dev)
    theta0 = torch.tensor(np.radians(rng.uniform(-15.0, 15.0, (poses, T))), device=dev)

    # one copy of the ligand per start: the batch form (views cull atoms, and an axis atom may be culled)
    coords, offsets = xyz.repeat(poses, 1), np.arange(poses + 1, dtype=np.int64) * n
    centers = center.repeat(poses, 1)
    all_axes = torch.tensor(np.tile(axes[None], (poses, 1, 1)), device=dev)
    all_moves = torch.tensor(np.tile(moves, poses), device=dev)

    def ncc(conformer, q, t):
        m = vox.moments_posed_batch(conformer, offsets, centers, q / q.norm(dim=1, keepdim=True), t, None, 1.5, target=target)
        return m[:, 0, 2] / torch.sqrt(m[:, 0, 1] * tt)

    def refine(flexible):
        q, t = q0.clone().requires_grad_(), t0.clone().requires_grad_()
        theta = theta0.clone().requires_grad_(flexible)
        start_conformer = vox.apply_torsions(coords, offsets, all_axes, all_moves, theta0)
        conformer = (lambda: vox.apply_torsions(coords, offsets, all_axes, all_moves, theta)) if flexible else (lambda: start_conformer)
        opt = torch.optim.Adam([q, t, theta] if flexible else [q, t], lr=0.01)
        first = None
        for _ in range(steps):
            opt.zero_grad()
            value = ncc(conformer(), q, t)
            first = value.detach().clone() if first is None else first
            (-value.sum()).backward()
            opt.step()
        with torch.no_grad():
            return first, ncc(conformer(), q, t), theta.detach()

    start, rigid, _ = refine(False)
    _, flex, theta = refine(True)
    print(f"{n} atoms, {T} torsions, {poses} starts, {steps} Adam steps on -NCC")
    print(f"NCC: start {float(start.mean()):.4f} on average (worst {float(start.min()):.4f}), rigid {float(rigid.mean()):.4f} "
          f"(worst {float(rigid.min()):.4f}), with torsions {float(flex.mean()):.4f} (worst {float(flex.min()):.4f})")
    left = torch.rad2deg(theta)
    fold = (left - 180.0 * torch.round(left / 180.0)).abs()
    print(f"torsion angles left, from the nearest multiple of 180 degrees: median {float(fold.median()):.2f}, largest "
          f"{float(fold.max()):.2f} degrees (started at up to {float(torch.rad2deg(theta0.abs().max())):.2f})")
    assert bool((flex > start).all()), "a start ended below where it began"
    assert float(flex.mean()) > float(rigid.mean()), "the torsions did not help"


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
