#!/usr/bin/env python3
"""What torsion coordinates cost next to the rigid refinement: one evaluation of 1024 poses of the 10GS ligand with and without
torsions, the two step kernels, and one round of each loop.

    python3 tools/rate_flex.py [--rounds 7] [--window 0.5] [--steps 12] [--poses 1024]

The ligand (tests/golden/10gs, 33 atoms, the 15 torsions molvoxel_amd.etc.mol.torsion_tree finds) with 8 synthetic feature
channels, 48^3 at 0.5 A, radius 1.5, repeated once per pose; the field is its own grid at the identity pose; the starts lie within
5 degrees, 0.3 A and 10 degrees per torsion (seeded). Rows, all on the same poses:
  eval_rigid   score_hessian_posed_batch                      (the baseline: the rigid evaluation as it was)
  eval_flex0   score_hessian_flex_posed_batch with T = 0      (the rigid values through the new entry)
  eval_flex    score_hessian_flex_posed_batch with the torsions: the public entry, which copies axes and masks to the host and
               asserts the tree rules on every call (check_torsions: one synchronisation)
  eval_loop    the same evaluation as the refinement loop makes it: the tree was checked once, before the loop
  apply        apply_torsions
  step_rigid   lm_step without a trial                         (the baseline step)
  step_flex    flex_lm_step without a trial, n = 6 + T
  round_rigid  refine_posed_batch, per round                   (the baseline loop)
  round_flex   refine_flex_posed_batch, per round: apply_torsions + evaluation + step
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


def build(B, steps):
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd.etc import mol as M
    from molvoxel_amd.voxelizer.hip.voxelizer import FlexLMState, LMState

    lig = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    axes1, moves1 = M.torsion_tree(lig)
    cloud = np.asarray(lig.coords, np.float64)
    n, T = cloud.shape[0], axes1.shape[0]
    feats = np.random.default_rng(1).random((n, 8)).astype(np.float32)
    vox = mv.create_voxelizer(0.5, 48, "scalar", "gaussian", library="hip")
    dev = vox.device
    xyz, f = torch.as_tensor(cloud, device=dev), torch.as_tensor(feats, device=dev)
    cen = xyz.mean(0, keepdim=True).repeat(B, 1)
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device=dev)
    field = vox.forward_posed_batch(xyz, np.array([0, n], np.int64), cen[:1], ident, torch.zeros((1, 3), dtype=torch.float64, device=dev),
                                    f, 1.5)[0].clone()
    qn, tn = starts(B)
    q0, t0 = torch.tensor(qn, device=dev), torch.tensor(tn, device=dev)
    th0 = torch.tensor(np.radians(np.random.default_rng(2).uniform(-10.0, 10.0, (B, T))), device=dev)
    coords, feat = xyz.repeat(B, 1), f.repeat(B, 1)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    axes = torch.tensor(np.tile(axes1[None], (B, 1, 1)), device=dev)
    moves = torch.tensor(np.tile(moves1, B), device=dev)
    none = torch.zeros((B, 0, 2), dtype=torch.int32, device=dev)
    kw = dict(steps=steps)
    flex_eval = lambda ax: vox.score_hessian_flex_posed_batch(coords, offsets, cen, q0, t0, feat, 1.5, field, ax, moves)
    S6, G6, H6 = vox.score_hessian_posed_batch(coords, offsets, cen, q0, t0, feat, 1.5, field)
    S, G, H = flex_eval(axes)
    lam = lambda Hx: 1e-3 * Hx.abs().reshape(B, -1).amax(dim=1)
    rigid = LMState(q0.clone(), t0.clone(), S6, G6, H6, lam(H6))
    flex = FlexLMState(q0.clone(), t0.clone(), th0.clone(), S, G, H, lam(H))
    forms = {
        "eval_rigid": lambda: vox.score_hessian_posed_batch(coords, offsets, cen, q0, t0, feat, 1.5, field),
        "eval_flex0": lambda: flex_eval(none),
        "eval_flex": lambda: flex_eval(axes),
        "eval_loop": lambda: vox._score_hessian_flex(coords, offsets, cen, feat, 1.5, field, axes, moves, posed=(q0, t0), checked=True),
        "apply": lambda: vox.apply_torsions(coords, offsets, axes, moves, th0),
        "step_rigid": lambda: vox.lm_step(rigid),
        "step_flex": lambda: vox.flex_lm_step(flex),
        "round_rigid": lambda: vox.refine_posed_batch(coords, offsets, cen, q0, t0, feat, 1.5, field, **kw),
        "round_flex": lambda: vox.refine_flex_posed_batch(coords, offsets, cen, q0, t0, th0, feat, 1.5, field, axes, moves, **kw),
    }
    return vox, forms, dict(B=B, atoms=n, T=T, C=8, D=48, steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--poses", type=int, default=1024)
    a = ap.parse_args()
    vox, forms, shape = build(a.poses, a.steps)
    for step in forms.values():
        for _ in range(a.warmup):
            step()
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, step in forms.items():  # alternating: one window of each form per round
            ms = window(step, a.window)
            times[name].append(ms / (a.steps + 1) if name.startswith("round_") else ms)
    med = {name: statistics.median(v) for name, v in times.items()}
    spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
    print(json.dumps(dict(row=f"ligand{a.poses}", **shape, ms={k: round(v, 4) for k, v in med.items()},
                          spread={k: round(v, 4) for k, v in spread.items()},
                          eval_flex_over_rigid=round(med["eval_flex"] / med["eval_rigid"], 4),
                          eval_loop_over_rigid=round(med["eval_loop"] / med["eval_rigid"], 4),
                          eval_flex0_over_rigid=round(med["eval_flex0"] / med["eval_rigid"], 4),
                          step_flex_over_rigid=round(med["step_flex"] / med["step_rigid"], 4),
                          round_flex_over_rigid=round(med["round_flex"] / med["round_rigid"], 4),
                          rounds=a.rounds, window_s=a.window)), flush=True)


if __name__ == "__main__":
    main()
