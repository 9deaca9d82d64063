#!/usr/bin/env python3
"""One scoring-and-gradient step of B poses of ONE shared cloud against a fixed field grid, forward + backward to the gradients
of the shared coordinates and features and of every pose: the views form against the repeated cloud.

    python3 tools/rate_score_views.py [--rounds 7] [--window 0.5] [--rows ligand1024,pocket256]

Rows (tests/golden/10gs)
  ligand1024  the 10GS ligand under 1024 poses, 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5, centred on the ligand
  pocket256   the 10GS pocket seen from 256 boxes centred on its first 256 atoms, each with a pose of its own, 32 synthetic
              feature channels, 64^3 at 0.5 A, radius 1.5
Forms, on the same seeded inputs and the same leaves (coords, features, q, t), one (C, D, D, D) field shared by all poses
  views   A: score_posed_views(...).sum().backward()             selection, gather, one walk, mvx_views_reduce onto the atoms
  batch   B: score_posed_batch on coords.repeat(B, 1) / features.repeat(B, 1), .sum().backward()   (autograd sums the copies)
One process; every shape is warmed, then the two forms alternate round by round; each window repeats the step until it has
run for at least `--window` seconds and is timed with device events; medians per step and the spread (max - min) / median over
the rounds. Memory: torch.cuda.max_memory_allocated over one warmed step of each form, above the inputs. The gradients of the
two forms are compared before timing (coordinates and features: sums in another order; poses: another grouping of the score)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.rate_score import poses, window  # noqa: E402

ROWS = {"ligand1024": ("ligand", 1024), "pocket256": ("pocket", 256)}


def build(what, B):
    """(voxelizer, {form: step()}, leaves, shape) - step() runs forward + backward and leaves the gradients in the leaves."""
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd.etc import mol as M

    gold = os.path.join(ROOT, "tests", "golden", "10gs")
    if what == "ligand":
        cloud = np.asarray(M.read_sdf(os.path.join(gold, "10gs_ligand.sdf"))[0].coords, np.float64)
        C_, D = 8, 48
        centers = np.repeat(cloud.mean(0)[None], B, 0)
    else:
        cloud = np.asarray(M.read_pdb(os.path.join(gold, "10gs_pocket_nowater.pdb")).coords, np.float64)
        C_, D = 32, 64
        centers = cloud[:B].copy()
    N = cloud.shape[0]
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True)
    dev = vox.device
    xyz = torch.tensor(cloud, device=dev, requires_grad=True)
    f = torch.tensor(np.random.default_rng(1).random((N, C_)).astype(np.float32), device=dev, requires_grad=True)
    cen = torch.as_tensor(centers, device=dev)
    qn, tn = poses(B)
    q = torch.tensor(qn, device=dev, requires_grad=True)
    t = torch.tensor(tn, device=dev, requires_grad=True)
    leaves = (xyz, f, q, t)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    field = torch.randn((C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    _, off = vox.select_posed_views(xyz.detach(), cen, q.detach(), t.detach(), radii=1.5)

    def clear():
        for x in leaves:
            x.grad = None

    def views():
        clear()
        vox.score_posed_views(xyz, cen, q, t, f, 1.5, field).sum().backward()

    def batch():
        clear()
        vox.score_posed_batch(xyz.repeat(B, 1), offsets, cen, q, t, f.repeat(B, 1), 1.5, field).sum().backward()

    kept = np.diff(off)
    return vox, {"views": views, "batch": batch}, leaves, dict(B=B, atoms=N, C=C_, D=D, kept_min=int(kept.min()),
                                                               kept_median=int(np.median(kept)), kept_max=int(kept.max()))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand1024,pocket256")
    a = ap.parse_args()
    for row in a.rows.split(","):
        what, B = ROWS[row]
        vox, steps, leaves, shape = build(what, B)
        grads, peak = {}, {}
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            grads[name] = [x.grad.clone() for x in leaves]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        agree = max(float((gv - gb).abs().max() / gb.abs().max()) for gv, gb in zip(grads["views"], grads["batch"]))
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              views_over_batch=round(med["views"] / med["batch"], 4),
                              peak_mib_above_inputs={k: round(v, 2) for k, v in peak.items()},
                              grad_rel_diff=float(f"{agree:.3g}"), rounds=a.rounds, window_s=a.window)), flush=True)
        del vox, steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
