#!/usr/bin/env python3
"""One scoring step of B poses against a fixed field grid, forward + backward to dL/dq and dL/dt: the fused score entry
against today's path through the grids.

    python3 tools/rate_score.py [--rounds 7] [--window 0.5] [--rows ligand,cfg2x64,ligand1024]

Rows (those of tools/rate_pose.py, plus the ligand at 1024 poses)
  ligand      64 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
  cfg2x64     64 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each
  ligand1024  the ligand row with 1024 poses
Forms, on the same seeded inputs and the same leaves (q, t), one (C, D, D, D) field shared by all poses
  score   A: score_posed_batch(...).sum().backward()                  one walk of the atoms' boxes over the field, no grid
  grids   B: forward_posed_batch, (grid * field).sum(dim=(1, 2, 3, 4)), .sum().backward()
One process; every shape is warmed, then the two forms alternate round by round; each window repeats the step until it has
run for at least `--window` seconds and is timed with device events; medians per step and the spread (max - min) / median over
the rounds. Memory: torch.cuda.max_memory_allocated over one warmed step of each form. The q and t gradients of the two forms
are compared before timing. Kernel times of score_kernel / score_reduce_kernel alone: run this script under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"ligand": ("ligand", 64), "cfg2x64": ("cfg2", 64), "ligand1024": ("ligand", 1024)}


def poses(B, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q, rng.uniform(-1.0, 1.0, (B, 3)).astype(np.float32).astype(np.float64)


def build(what, B):
    """(voxelizer, {form: step()}, leaves, shape) - step() runs forward + backward and leaves the gradients in q.grad / t.grad."""
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W
    from molvoxel_amd.etc import mol as M

    if what == "ligand":
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
    C_ = f.shape[1]
    field = torch.randn((C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def score():
        q.grad = t.grad = None
        vox.score_posed_batch(xyz, offsets, cen, q, t, f, radius, field).sum().backward()

    def grids():
        q.grad = t.grad = None
        grid = vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius)
        (grid * field).sum(dim=(1, 2, 3, 4)).sum().backward()

    return vox, {"score": score, "grids": grids}, (q, t), dict(B=B, atoms=int(offsets[-1]), C=C_, D=D)


def window(step, seconds):
    """ms per step over a window of at least `seconds`, by device events around the whole window."""
    import torch

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, inner = 0, 1
    start.record()
    while True:
        for _ in range(inner):
            step()
        n += inner
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= seconds * 1e3:
            return ms / n
        inner = max(1, min(4 * n, int(n * (seconds * 1e3 - ms) / max(ms, 1e-3)) + 1))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand,cfg2x64,ligand1024")
    a = ap.parse_args()
    for row in a.rows.split(","):
        what, B = ROWS[row]
        vox, steps, (q, t), shape = build(what, B)
        grads, peak = {}, {}
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            grads[name] = (q.grad.clone(), t.grad.clone())
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        agree = max(float((grads["score"][i] - grads["grids"][i]).abs().max() / grads["grids"][i].abs().max()) for i in (0, 1))
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              score_over_grids=round(med["score"] / med["grids"], 4),
                              peak_mib_above_inputs={k: round(v, 2) for k, v in peak.items()},
                              grad_rel_diff=float(f"{agree:.3g}"), rounds=a.rounds, window_s=a.window)), flush=True)
        del vox, steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
