#!/usr/bin/env python3
"""What torsion angles cost inside autograd: 1024 poses of the 10GS ligand, one first-order step with and without torsions, and
the same step with the conformer built from torch operations.

    python3 tools/rate_torsion_grad.py [--rounds 7] [--window 0.5] [--poses 1024]

The ligand (tests/golden/10gs, 33 atoms, the 15 torsions molvoxel_amd.etc.mol.torsion_tree finds) with 8 synthetic feature
channels, 48^3 at 0.5 A, radius 1.5, repeated once per pose; the field is its own grid at the identity pose; the starts lie within
5 degrees, 0.3 A and 10 degrees per torsion (seeded, tools/rate_flex.py's). Rows, all on the same poses:
  apply        apply_torsions, plain values                                        (mvx_apply_torsions)
  backward     apply_torsions_backward alone, on a fixed upstream                  (mvx_apply_torsions_backward)
  step_rigid   score_posed_batch(coords, q, t).sum().backward(): gradients for q and t, no torsions (the baseline step)
  step_flex    score_posed_batch(apply_torsions(coords, theta), q, t).sum().backward() on a torsion_grad voxelizer: gradients for
               q, t and theta
  step_torch   the same step with the conformer built in the tool from torch operations - T Rodrigues updates on a (B, n, 3)
               tensor, each a handful of small kernels, replayed backwards by autograd - on the same voxelizer
One process; every form is warmed, then the forms alternate round by round; each window repeats its form until it has run for at
least `--window` seconds and is timed with device events; medians and the spread (max - min) / median over the rounds."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rate_refine import starts  # noqa: E402
from tools.rate_score import window  # noqa: E402


def torch_conformer(xyz, axes1, moves1, theta):
    """C(theta) of B copies of one molecule from torch operations: xyz (n, 3), theta (B, T) -> (B * n, 3)."""
    import torch

    B, T = theta.shape
    p = xyz[None].expand(B, -1, -1)
    bits = torch.as_tensor(np.asarray(moves1, np.int32).view(np.uint32).astype(np.int64), device=xyz.device)
    for k in range(T):
        a, b = int(axes1[k, 0]), int(axes1[k, 1])
        pb = p[:, b:b + 1]
        u = pb - p[:, a:a + 1]
        u = u / u.norm(dim=2, keepdim=True)
        c, s = torch.cos(theta[:, k])[:, None, None], torch.sin(theta[:, k])[:, None, None]
        v = p - pb
        turned = pb + (v * c + torch.cross(u.expand_as(v), v, dim=2) * s + u * ((v * u).sum(dim=2, keepdim=True) * (1.0 - c)))
        p = torch.where((((bits >> k) & 1) != 0)[None, :, None], turned, p)
    return p.reshape(-1, 3)


def build(B):
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd.etc import mol as M

    lig = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    axes1, moves1 = M.torsion_tree(lig)
    cloud = np.asarray(lig.coords, np.float64)
    n, T = cloud.shape[0], axes1.shape[0]
    feats = np.random.default_rng(1).random((n, 8)).astype(np.float32)
    vox = mv.create_voxelizer(0.5, 48, "scalar", "gaussian", library="hip", differentiable=True, torsion_grad=True)
    dev = vox.device
    xyz, f = torch.as_tensor(cloud, device=dev), torch.as_tensor(feats, device=dev)
    cen = xyz.mean(0, keepdim=True).repeat(B, 1)
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device=dev)
    with torch.no_grad():
        field = vox.forward_posed_batch(xyz, np.array([0, n], np.int64), cen[:1], ident,
                                        torch.zeros((1, 3), dtype=torch.float64, device=dev), f, 1.5)[0].clone()
    qn, tn = starts(B)
    q = torch.tensor(qn, device=dev).requires_grad_()
    t = torch.tensor(tn, device=dev).requires_grad_()
    theta = torch.tensor(np.radians(np.random.default_rng(2).uniform(-10.0, 10.0, (B, T))), device=dev).requires_grad_()
    coords, feat = xyz.repeat(B, 1), f.repeat(B, 1)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    axes = torch.tensor(np.tile(axes1[None], (B, 1, 1)), device=dev)
    moves = torch.tensor(np.tile(moves1, B), device=dev)
    th0 = theta.detach()
    conformer = vox.apply_torsions(coords, offsets, axes, moves, th0)
    upstream = torch.tensor(np.random.default_rng(3).standard_normal((B * n, 3)), device=dev)

    def step(conf):
        for x in (q, t, theta):
            x.grad = None
        vox.score_posed_batch(conf(), offsets, cen, q, t, feat, 1.5, field).sum().backward()

    forms = {
        "apply": lambda: vox.apply_torsions(coords, offsets, axes, moves, th0),
        "backward": lambda: vox.apply_torsions_backward(conformer, offsets, axes, moves, th0, upstream),
        "step_rigid": lambda: step(lambda: coords),
        "step_flex": lambda: step(lambda: vox.apply_torsions(coords, offsets, axes, moves, theta)),
        "step_torch": lambda: step(lambda: torch_conformer(xyz, axes1, moves1, theta)),
    }
    # the two conformers and the two angle gradients agree: the torch form is the same function
    step(lambda: vox.apply_torsions(coords, offsets, axes, moves, theta))
    g_hip = theta.grad.clone()
    step(lambda: torch_conformer(xyz, axes1, moves1, theta))
    agree = dict(conformer=float((torch_conformer(xyz, axes1, moves1, th0) - conformer).abs().max()),
                 theta_grad=float((theta.grad - g_hip).abs().max() / g_hip.abs().max()))
    return vox, forms, dict(B=B, atoms=n, T=T, C=8, D=48), agree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--poses", type=int, default=1024)
    a = ap.parse_args()
    vox, forms, shape, agree = build(a.poses)
    for step in forms.values():
        for _ in range(a.warmup):
            step()
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, step in forms.items():  # alternating: one window of each form per round
            times[name].append(window(step, a.window))
    med = {name: statistics.median(v) for name, v in times.items()}
    spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
    print(json.dumps(dict(row=f"ligand{a.poses}", **shape, ms={k: round(v, 4) for k, v in med.items()},
                          spread={k: round(v, 4) for k, v in spread.items()},
                          step_flex_over_rigid=round(med["step_flex"] / med["step_rigid"], 4),
                          step_torch_over_flex=round(med["step_torch"] / med["step_flex"], 4),
                          max_abs_conformer_difference=agree["conformer"], relative_theta_grad_difference=agree["theta_grad"],
                          rounds=a.rounds, window_s=a.window)), flush=True)


if __name__ == "__main__":
    main()
