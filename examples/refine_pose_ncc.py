"""Pose refinement on normalised cross-correlation, without a grid: the 10GS ligand, rotated and shifted, is moved back onto
its own density map.

    python examples/refine_pose_ncc.py [steps] [--views]

examples/refine_pose.py with another loss. The target is the ligand's grid in its crystal pose; the start is that pose perturbed
by a rotation of about 20 degrees and a shift of about 0.7 A. `torch.optim.Adam([q, t])` minimises -NCC, and NCC is built from the
moments of the posed ligand's grid, m = `moments_posed_batch(..., target=target)` on a voxelizer made with `moments_grad=True`:

    NCC = m[..., 2] / sqrt(m[..., 1] * sum(target ** 2))

Every step is one `moments_posed_batch` and one `backward()`. No grid of the posed ligand is written for autograd and no grid of
dL/dgrid exists: the backward walk forms its upstream from the moments' gradients (mvx_moments_backward_batch). The quaternion is
normalised in torch before the call (autograd carries the normalisation). Needs an MI355X (the HIP backend has no CPU path).

--views: the same refinement through `moments_posed_views`, which takes the ligand as ONE shared cloud and the pose as a view of
it (here a single one; B poses under refinement are B rows of `centers`, `q` and `t`, and the ligand is still handed over once).
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import molvoxel_amd  # noqa: E402
from molvoxel_amd.etc import mol as M  # noqa: E402


def main(steps=300, views=False):
    import torch

    ligand = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    vox = molvoxel_amd.create_voxelizer(resolution=0.5, dimension=48, density_type="gaussian", library="hip", differentiable=True,
                                        moments_grad=True)
    dev = vox.device
    xyz = torch.as_tensor(np.asarray(ligand.coords, np.float64), device=dev)
    offsets = np.array([0, xyz.shape[0]], np.int64)
    center = xyz.mean(0, keepdim=True)                                # (1, 3): the pose rotates about the centroid
    identity = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev, dtype=torch.float64)
    zero = torch.zeros((1, 3), device=dev, dtype=torch.float64)

    with torch.no_grad():  # channels=None: one density channel, scalar radius 1.5
        target = vox.forward_posed_batch(xyz, offsets, center, identity, zero, None, 1.5)[0]
    tt = (target.double() ** 2).sum()

    def ncc_of(q, t):
        qn = q / q.norm(dim=1, keepdim=True)
        if views:
            m = vox.moments_posed_views(xyz, center, qn, t, None, 1.5, target=target)
        else:
            m = vox.moments_posed_batch(xyz, offsets, center, qn, t, None, 1.5, target=target)
        return (m[..., 2] / torch.sqrt(m[..., 1] * tt)).sum()

    angle = math.radians(20.0)
    axis = np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)
    q = torch.tensor([[math.cos(angle / 2), *(math.sin(angle / 2) * axis)]], device=dev, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[0.4, -0.5, 0.3]], device=dev, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([q, t], lr=0.01)
    for step in range(steps + 1):
        opt.zero_grad()
        ncc = ncc_of(q, t)
        (-ncc).backward()
        if step % 50 == 0 or step == steps:
            qn = (q / q.norm()).detach()
            off = 2.0 * math.degrees(math.acos(min(1.0, abs(float(qn[0, 0])))))
            print(f"step {step:4d}: NCC {float(ncc):8.5f}   rotation off by {off:6.2f} deg   shift off by {float(t.norm()):.3f} A")
        opt.step()
    assert float(ncc) > 0.97, "the refinement did not come back to the crystal pose"


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:] if a != "--views"][:1], views="--views" in sys.argv[1:])
