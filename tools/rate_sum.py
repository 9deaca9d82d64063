#!/usr/bin/env python3
"""One summed grid of B poses: forward_posed_sum against today's path through the B grids, and a field-gradient step of the score
path against the path through the grids.

    python3 tools/rate_sum.py [--rounds 7] [--window 0.5] [--rows ligand1024,cfg2x64,cfg2x256]

Rows (those of tools/rate_score.py)
  ligand1024  1024 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
  cfg2x64     64 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each
  cfg2x256    256 of them
Forms, on the same seeded inputs, one float32 weight per pose
  sum      A: forward_posed_sum(..., weights=w)                                    one (C, D, D, D) grid, written once
  grids    B: (forward_posed_batch(...) * w[:, None, None, None, None]).sum(0)     B grids, then a torch reduction
  (unweighted, the reduction of form B is .sum(0) alone: `--unweighted`)
Field-gradient step, one (C, D, D, D) field that requires grad, shared by all poses
  fsum     A: score_posed_batch(...).sum().backward() on a field_grad voxelizer    one walk over the field, then one summed grid
  fgrids   B: (forward_posed_batch(...) * field).sum(dim=(1, 2, 3, 4)).sum().backward()
One process; every shape is warmed, then the forms alternate round by round; each window repeats the step until it has run for at
least `--window` seconds and is timed with device events; medians per step and the spread (max - min) / median over the rounds.
Memory: torch.cuda.max_memory_allocated over one warmed step of each form. The results of the two forms are compared before
timing. Kernel times of voxelize_sum_kernel alone: run this script under `rocprofv3 --kernel-trace --stats` in a run of its own.
At most slabs x channel chunks workgroups run in form A (D = 48: 24 x 12 = 288, D = 64: 32 x 16 = 512), whatever B is."""
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

ROWS = {"ligand1024": ("ligand", 1024), "cfg2x64": ("cfg2", 64), "cfg2x256": ("cfg2", 256)}


def build(what, B, weighted):
    """({form: step()}, results, shape) - step() leaves its result (the summed grid, or the field's gradient) in results[form]."""
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
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True, field_grad=True)
    dev = vox.device
    sizes = [c.shape[0] for c in clouds]
    offsets = np.cumsum([0] + sizes).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    qn, tn = poses(B)
    q, t = torch.tensor(qn, device=dev), torch.tensor(tn, device=dev)
    C_ = f.shape[1]
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(B, device=dev, generator=gen) if weighted else None
    field = torch.randn((C_, D, D, D), device=dev, generator=gen).requires_grad_()
    res = {}

    def fsum():
        field.grad = None
        vox.score_posed_batch(xyz, offsets, cen, q, t, f, radius, field).sum().backward()
        res["fsum"] = field.grad

    def fgrids():
        field.grad = None
        grid = vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius)
        (grid * field).sum(dim=(1, 2, 3, 4)).sum().backward()
        res["fgrids"] = field.grad

    def sum_():
        res["sum"] = vox.forward_posed_sum(xyz, offsets, cen, q, t, f, radius, weights=w)

    def grids():
        grid = vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius)
        res["grids"] = grid.sum(0) if w is None else (grid * w[:, None, None, None, None]).sum(0)

    return {"sum": sum_, "grids": grids, "fsum": fsum, "fgrids": fgrids}, res, dict(B=B, atoms=int(offsets[-1]), C=C_, D=D)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand1024,cfg2x64,cfg2x256")
    ap.add_argument("--unweighted", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rate_sum.py measures on the GPU"
    for row in a.rows.split(","):
        what, B = ROWS[row]
        steps, res, shape = build(what, B, not a.unweighted)
        peak, kept = {}, {}
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            kept[name] = res[name].detach().clone()
            res.clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            res.clear()
        agree = {pair: float((kept[pair[0]] - kept[pair[1]]).abs().max() / kept[pair[1]].abs().max()) for pair in (("sum", "grids"), ("fsum", "fgrids"))}
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
                res.clear()
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, weighted=not a.unweighted, step_ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              sum_over_grids=round(med["sum"] / med["grids"], 4), fsum_over_fgrids=round(med["fsum"] / med["fgrids"], 4),
                              peak_mib_above_inputs={k: round(v, 2) for k, v in peak.items()},
                              rel_diff={"/".join(k): float(f"{v:.3g}") for k, v in agree.items()}, rounds=a.rounds, window_s=a.window)),
              flush=True)
        del steps, res, kept
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
