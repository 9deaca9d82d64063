#!/usr/bin/env python3
"""Per-channel moments of B poses: moments_posed_batch against the path it replaces, the B grids and torch reductions over them.

    python3 tools/rate_moments.py [--rounds 7] [--window 0.5] [--rows cfg2x256,ligand1024] [--out profiles/r15_moments.txt]

Rows (those of tools/rate_sum.py)
  cfg2x256    256 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each
  ligand1024  1024 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
Forms, on the same seeded inputs and one seeded float32 target (C, D, D, D)
  moments     A: moments_posed_batch(...)                                       (B, C, 2) float64, no grid
  moments_t   A: moments_posed_batch(..., target=t)                             (B, C, 3)
  forward     forward_posed_batch(...) alone                                    the B float32 grids, nothing reduced
  grids       B: g = forward_posed_batch(...).double(); [g.sum, (g * g).sum] over the voxels
  grids_t     B: the same and (g * t.double()).sum
One process; every shape is warmed, then the forms alternate round by round; each window repeats the step until it has run for at
least `--window` seconds and is timed with device events; medians per step and the spread (max - min) / median over the rounds.
The results of the two paths are compared before timing (largest |A - B| over the largest |B| per moment). Bytes: what each
path has to move through device memory at least, from the shapes - A: the slab partials written and read once (B slabs K C
doubles, twice), the moments, the target once; B: the grids written once and read once per reduction pass that torch runs over them
(.double(): 4 read + 8 written per voxel value; every sum 8 read; every product 16 read + 8 written) - not a measurement.
Kernel times of moments_kernel alone: run this script under `rocprofv3 --kernel-trace --stats` in a run of its own."""
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
FORMS = ("moments", "moments_t", "forward", "grids", "grids_t")


def build(what, B):
    """({form: step()}, results, shape) - step() leaves its result in results[form]."""
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
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    dev = vox.device
    sizes = [c.shape[0] for c in clouds]
    offsets = np.cumsum([0] + sizes).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    qn, tn = poses(B)
    q, t = torch.tensor(qn, device=dev), torch.tensor(tn, device=dev)
    C_ = f.shape[1]
    target = torch.randn((C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    res = {}

    def moments():
        res["moments"] = vox.moments_posed_batch(xyz, offsets, cen, q, t, f, radius)

    def moments_t():
        res["moments_t"] = vox.moments_posed_batch(xyz, offsets, cen, q, t, f, radius, target=target)

    def forward():
        res["forward"] = vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius)

    def reduce(with_target):
        g = vox.forward_posed_batch(xyz, offsets, cen, q, t, f, radius).double()
        out = [g.sum(dim=(2, 3, 4)), (g * g).sum(dim=(2, 3, 4))]
        if with_target:
            out.append((g * target.double()).sum(dim=(2, 3, 4)))
        return torch.stack(out, dim=-1)

    def grids():
        res["grids"] = reduce(False)

    def grids_t():
        res["grids_t"] = reduce(True)

    steps = dict(moments=moments, moments_t=moments_t, forward=forward, grids=grids, grids_t=grids_t)
    plan = None
    moments()
    plan = vox.last_plan()
    return steps, res, dict(B=B, atoms=int(offsets[-1]), C=C_, D=D, slabs=plan["nsx"] * plan["nsy"] * plan["nzc"], nchunk=plan["nchunk"])


def least_bytes(shape):
    """form -> bytes through device memory at least, from the shapes (see the module's docstring)."""
    B, C_, D, TS = shape["B"], shape["C"], shape["D"], shape["slabs"]
    vox = B * C_ * D ** 3
    a = lambda K: 2 * B * TS * K * C_ * 8 + B * C_ * K * 8  # noqa: E731
    grid, dbl = 4 * vox, 12 * vox
    return dict(moments=a(2), moments_t=a(3) + 4 * C_ * D ** 3, forward=grid, grids=grid + dbl + 8 * vox + 32 * vox,
                grids_t=grid + dbl + 8 * vox + 32 * vox + 32 * vox)


def table(rows):
    lines = ["moments_posed_batch against forward_posed_batch and float64 torch reductions over its grids (tools/rate_moments.py)",
             "ms per step: median over the rounds of windows timed with device events (spread = (max - min) / median); GB: least bytes",
             "through device memory by the shapes, not measured; agree: largest |moments - reduced grids| / largest |reduced grids|", ""]
    head = f"{'row':<11}{'B':>5}{'C':>4}{'D':>4}{'chunks':>7}  " + "".join(f"{n + ' ms':>14}{'spread':>8}{'GB':>8}" for n in FORMS)
    lines.append(head)
    for r in rows:
        lines.append(f"{r['row']:<11}{r['B']:>5}{r['C']:>4}{r['D']:>4}{r['nchunk']:>7}  " +
                     "".join(f"{r['step_ms'][n]:>14.4f}{r['spread'][n]:>8.3f}{r['least_gb'][n]:>8.3f}" for n in FORMS))
    lines.append("")
    for r in rows:
        m = r["step_ms"]
        lines.append(f"{r['row']}: moments / forward = {m['moments'] / m['forward']:.3f}, moments / grids = {m['moments'] / m['grids']:.3f}, "
                     f"moments_t / grids_t = {m['moments_t'] / m['grids_t']:.3f}; agree {r['agree']}")
    return "\n".join(lines) + "\n"


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="cfg2x256,ligand1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_moments.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rate_moments.py measures on the GPU"
    done = []
    for row in a.rows.split(","):
        what, B = ROWS[row]
        steps, res, shape = build(what, B)
        kept = {}
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            if name != "forward":
                kept[name] = res[name].detach().clone()
            res.clear()
        torch.cuda.synchronize()
        agree = {f"{x}/{y}": [float(f"{float((kept[x][..., k] - kept[y][..., k]).abs().max() / kept[y][..., k].abs().max()):.3g}")
                              for k in range(kept[x].shape[-1])] for x, y in (("moments", "grids"), ("moments_t", "grids_t"))}
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
                res.clear()
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        done.append(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()}, spread={k: round(v, 4) for k, v in spread.items()},
                         least_gb={k: round(v / 1e9, 4) for k, v in least_bytes(shape).items()}, agree=agree, rounds=a.rounds, window_s=a.window))
        print(json.dumps(done[-1]), flush=True)
        del steps, res, kept
        torch.cuda.empty_cache()
    text = table(done)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
