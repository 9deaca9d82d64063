#!/usr/bin/env python3
"""One pose-refinement step (forward + backward to dL/dq, dL/dt) through the posed entries against the torch-ops way.

    python3 tools/rate_pose.py [--rounds 9] [--inner 5] [--rows ligand,cfg2x64]

Rows
  ligand    64 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5:
            `forward_posed_views` (one shared cloud) and `forward_posed_batch` on the cloud repeated 64 times
  cfg2x64   64 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each: `forward_posed_batch`
Each is compared with the only way to do it without the posed entries: the poses applied to the B copies with torch ops
(M(q) (x - c) + t as tensors), `forward_batch` on the result, autograd back through the torch ops. Same loss (<grid, G> with a
fixed G), same leaves (q, t), both paths in one process: warm-up, then interleaved rounds of `inner` steps with a device
synchronisation around each window; medians per step. The q and t gradients of the two paths are compared before timing.
Kernel time of pose_grad_kernel alone: run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rotation(q):
    """(B, 3, 3) M(q) with torch ops (q as given: scales by |q|^2)."""
    import torch

    q0, q1, q2, q3 = q.unbind(1)
    rows = [q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
            2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1),
            2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def poses(B, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q, rng.uniform(-1.0, 1.0, (B, 3)).astype(np.float32).astype(np.float64)


def build(row, B):
    """(voxelizer, {name: step()}, leaves) - step() runs forward + backward and leaves the gradients in q.grad / t.grad."""
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W
    from molvoxel_amd.etc import mol as M

    if row == "ligand":
        lig = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
        clouds = [np.asarray(lig.coords, np.float64)] * B
        feats = [np.random.default_rng(1).random((clouds[0].shape[0], 8)).astype(np.float32)] * B
        D, radius = 48, 1.5
    else:
        wl = W.cfg2(batch=B)
        clouds, feats, D, radius = [wl.coords[i] for i in range(B)], [wl.channels[i] for i in range(B)], wl.dimension, 1.0
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True)
    dev = vox.device
    sizes = [c.shape[0] for c in clouds]
    offsets = np.cumsum([0] + sizes).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    qn, tn = poses(B)
    q = torch.tensor(qn, device=dev, requires_grad=True)
    t = torch.tensor(tn, device=dev, requires_grad=True)
    owner = torch.repeat_interleave(torch.arange(B, device=dev), torch.as_tensor(sizes, device=dev))
    C_ = f.shape[1]
    G = torch.randn((B, C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def finish(grid):
        q.grad = t.grad = None
        (grid * G).sum().backward()

    def posed_batch():
        finish(vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius))

    def torch_ops():
        p = torch.einsum("nij,nj->ni", rotation(q)[owner], xyz - cen[owner]) + t[owner]
        finish(vox.forward_batch(p, offsets, None, f, radius))

    steps = {"posed_batch": posed_batch, "torch_ops": torch_ops}
    if row == "ligand":
        x1, f1 = xyz[:sizes[0]].clone(), f[:sizes[0]].clone()
        steps["posed_views"] = lambda: finish(vox.forward_posed_views(x1, cen, q, t, f1, radius))
    return vox, steps, (q, t), dict(B=B, atoms=int(offsets[-1]), C=C_, D=D)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--rows", default="ligand,cfg2x64")
    a = ap.parse_args()
    for row in a.rows.split(","):
        vox, steps, (q, t), shape = build(row, a.poses)
        grads = {}
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            grads[name] = (q.grad.clone(), t.grad.clone())
        agree = {name: max(float((g[0] - grads["torch_ops"][0]).abs().max() / grads["torch_ops"][0].abs().max()),
                           float((g[1] - grads["torch_ops"][1]).abs().max() / grads["torch_ops"][1].abs().max()))
                 for name, g in grads.items() if name != "torch_ops"}
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # interleaved: one window of each per round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    step()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / a.inner)
        med = {name: statistics.median(v) for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()},
                              min_ms={k: round(min(v), 4) for k, v in times.items()},
                              over_torch_ops={k: round(v / med["torch_ops"], 3) for k, v in med.items() if k != "torch_ops"},
                              grad_rel_diff_vs_torch_ops={k: float(f"{v:.3g}") for k, v in agree.items()},
                              rounds=a.rounds, inner=a.inner)), flush=True)
        del vox, steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
