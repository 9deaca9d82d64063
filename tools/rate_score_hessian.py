#!/usr/bin/env python3
"""One second-order evaluation of B poses against a fixed field grid - scores, twist gradients and twist Hessians - against
the first-order step it extends.

    python3 tools/rate_score_hessian.py [--rounds 7] [--window 0.5] [--rows ligand1024,cfg2x64]

Rows (those of tools/rate_score.py)
  ligand1024  1024 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
  cfg2x64     64 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each
Forms, on the same seeded inputs, one (C, D, D, D) field shared by all poses
  hessian  A: score_hessian_posed_batch(...)                          one walk: S, G (B, 6) and Hxi (B, 6, 6), no autograd
  score    B: score_posed_batch(...).sum().backward()                 one walk: S, then dS/dq and dS/dt through autograd
The Hessian call does strictly more than the score's walk (eleven lane partials against four, and a 27-value reduction per
molecule); it has no autograd graph to record. One process; every shape is warmed, then the two forms alternate round by round;
each window repeats the step until it has run for at least `--window` seconds and is timed with device events; medians per step
and the spread (max - min) / median over the rounds. The scores of the two forms are compared bit for bit before timing."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rate_score import ROWS, poses, window  # noqa: E402


def build(what, B):
    """(voxelizer, {form: step()}, compare(), shape)"""
    import numpy as np
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
    offsets = np.cumsum([0] + [c.shape[0] for c in clouds]).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    qn, tn = poses(B)
    q = torch.tensor(qn, device=dev, requires_grad=True)
    t = torch.tensor(tn, device=dev, requires_grad=True)
    C_ = f.shape[1]
    field = torch.randn((C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    out = {}

    def hessian():
        out["hessian"] = vox.score_hessian_posed_batch(xyz, offsets, cen, q, t, f, radius, field)

    def score():
        q.grad = t.grad = None
        out["score"] = vox.score_posed_batch(xyz, offsets, cen, q, t, f, radius, field)
        out["score"].sum().backward()

    def compare():
        S, G, H = out["hessian"]
        assert torch.equal(S, out["score"].detach()), "the scores of the two forms differ"
        assert torch.equal(H, H.transpose(1, 2)) and bool(torch.isfinite(G).all())
        # dS/dt = G_tau: the twist's translation is the pose's
        return float((G[:, :3] - t.grad).abs().max() / t.grad.abs().max())

    return vox, {"hessian": hessian, "score": score}, compare, dict(B=B, atoms=int(offsets[-1]), C=C_, D=D)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand1024,cfg2x64")
    a = ap.parse_args()
    for row in a.rows.split(","):
        what, B = ROWS[row]
        vox, steps, compare, shape = build(what, B)
        for step in steps.values():
            for _ in range(a.warmup):
                step()
        agree = compare()
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              hessian_over_score=round(med["hessian"] / med["score"], 4),
                              grad_t_rel_diff=float(f"{agree:.3g}"), rounds=a.rounds, window_s=a.window)), flush=True)
        del vox, steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
