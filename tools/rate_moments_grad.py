#!/usr/bin/env python3
"""One optimisation step on normalised cross-correlation: through the moments (moments_grad=True) against through the grids.

    python3 tools/rate_moments_grad.py [--rounds 7] [--window 0.5] [--rows cfg2x256,ligand1024] [--scratch-kb 0,262144,16777216]
                                       [--out profiles/r16_moments_grad.txt]

--scratch-kb: one run of every row per value of the "mgrad_scratch_kb" option (0: the library's bound of 1 GiB of grids per
molecule chunk; a value above the call's grids: the forward's own cut alone). profiles/r16_moments_grad.txt: 0,262144,16777216.

Rows (those of tools/rate_moments.py)
  cfg2x256    256 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3), one pose each
  ligand1024  1024 poses of the 10GS ligand (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
Forms, on the same seeded inputs, poses (q, t require grad) and one seeded float32 target (C, D, D, D); the loss is
-sum_{b,c} m2 / sqrt(m1 * sum t^2 + 1e-6)
  moments  m = moments_posed_batch(..., target=t) on a moments_grad voxelizer; loss; backward()
           (mvx_moments_batch, then per molecule chunk forward + mvx_moments_backward_batch's walk, then mvx_pose_grad_batch)
  grids    g = forward_posed_batch(...).double() on a differentiable voxelizer; m from torch reductions; loss; backward()
           (autograd materialises dL/dgrid for all B grids before mvx_backward_batch runs)
One process, a voxelizer per form; every form is warmed, then the forms alternate round by round; each window repeats the step
until it has run for at least `--window` seconds and is timed with device events; medians per step and the spread (max - min) /
median over the rounds. The gradients of the two forms are compared before timing (largest |A - B| / largest |B|).
Peak device memory of one step, per form, measured on a warmed voxelizer: the peak of torch's allocator over the step above
what was allocated before it, plus what the library holds itself (device memory in use that torch has not reserved; the
library's buffers live as long as the handle, so their size after the step is their peak)."""
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

ROWS = {"ligand1024": ("ligand", 1024), "ligand64": ("ligand", 64), "cfg2x64": ("cfg2", 64), "cfg2x256": ("cfg2", 256)}
FORMS = ("moments", "grids")


def _held_by_library(torch):
    free, total = torch.cuda.mem_get_info()
    return (total - free) - torch.cuda.memory_reserved()


def build(what, B, scratch_kb=0):
    """({form: step()}, leaves, shape, the two voxelizers) - step() leaves the gradients in q.grad / t.grad. scratch_kb: the
    "mgrad_scratch_kb" option of the moments form's voxelizer (0: the library's bound of 1 GiB of grids per molecule chunk)."""
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
    vm = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True, moments_grad=True)
    vg = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True)
    if scratch_kb:
        vm.debug_option("mgrad_scratch_kb", scratch_kb)
    dev = vm.device
    sizes = [c.shape[0] for c in clouds]
    offsets = np.cumsum([0] + sizes).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    qn, tn = poses(B)
    q = torch.tensor(qn, device=dev, requires_grad=True)
    t = torch.tensor(tn, device=dev, requires_grad=True)
    C_ = f.shape[1]
    target = torch.randn((C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    tt = (target.double() ** 2).sum(dim=(1, 2, 3))

    def loss_of(m):
        return -(m[..., 2] / torch.sqrt(m[..., 1] * tt + 1e-6)).sum()

    def moments():
        q.grad = t.grad = None
        loss_of(vm.moments_posed_batch(xyz, offsets, cen, q, t, f, radius, target=target)).backward()

    def grids():
        q.grad = t.grad = None
        g = vg.forward_posed_batch(xyz, offsets, cen, q, t, f, radius).double()
        m = torch.stack([g.sum(dim=(2, 3, 4)), (g * g).sum(dim=(2, 3, 4)), (g * target.double()).sum(dim=(2, 3, 4))], dim=-1)
        loss_of(m).backward()

    return dict(moments=moments, grids=grids), (q, t), dict(B=B, atoms=int(offsets[-1]), C=C_, D=D), (vm, vg)


def peak_memory(torch, step):
    """(bytes torch's allocator peaked at above its level before the step, bytes the library holds after it) for one more step."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    torch.cuda.empty_cache()
    return peak, _held_by_library(torch)


def table(rows):
    lines = ["one step on -NCC of B poses against a target: through the moments (moments_grad) and through the grids (tools/rate_moments_grad.py)",
             "ms per step: median over the rounds of windows timed with device events (spread = (max - min) / median); peak GB: torch's",
             "allocator over one step plus the library's own buffers of that form's voxelizer; agree: largest |moments - grids| / largest |grids|", ""]
    head = f"{'row':<11}{'B':>5}{'C':>4}{'D':>4}{'scratch MB':>11}{'chunks':>7}  " + "".join(f"{n + ' ms':>12}{'spread':>8}{'torch GB':>10}{'lib GB':>8}" for n in FORMS)
    lines.append(head)
    for r in rows:
        lines.append(f"{r['row']:<11}{r['B']:>5}{r['C']:>4}{r['D']:>4}{r['scratch_mb']:>11}{r['nchunk']:>7}  " +
                     "".join(f"{r['step_ms'][n]:>12.3f}{r['spread'][n]:>8.3f}{r['torch_gb'][n]:>10.3f}{r['lib_gb'][n]:>8.3f}" for n in FORMS))
    lines.append("")
    for r in rows:
        m, tg, lg = r["step_ms"], r["torch_gb"], r["lib_gb"]
        lines.append(f"{r['row']} ({r['nchunk']} chunks): moments / grids = {m['moments'] / m['grids']:.3f} in time, "
                     f"{(tg['moments'] + lg['moments']) / (tg['grids'] + lg['grids']):.3f} in peak memory; "
                     f"grids of one chunk {r['chunk_grids_gb']:.3f} GB against {r['all_grids_gb']:.3f} GB for B grids; agree dq {r['agree'][0]}, dt {r['agree'][1]}")
    return "\n".join(lines) + "\n"


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="cfg2x256,ligand1024")
    ap.add_argument("--scratch-kb", default="0", help="comma list of mgrad_scratch_kb values, one run of every row each (0: the library's 1 GiB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_moments_grad.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rate_moments_grad.py measures on the GPU"
    done = []
    for row, scratch_kb in [(r, int(k)) for r in a.rows.split(",") for k in a.scratch_kb.split(",")]:
        what, B = ROWS[row]
        torch.cuda.empty_cache()
        idle = _held_by_library(torch)  # (the runtime's own and, from the second row on, nothing of the previous row's voxelizers)
        steps, (q, t), shape, voxs = build(what, B, scratch_kb)
        shape["scratch_mb"] = (scratch_kb or 1 << 20) // 1024
        kept, torch_gb, lib_gb = {}, {}, {}
        held = idle
        for name, step in steps.items():
            for _ in range(a.warmup):
                step()
            kept[name] = (q.grad.detach().clone(), t.grad.detach().clone())
            peak, now = peak_memory(torch, step)
            torch_gb[name], lib_gb[name] = peak / 1e9, (now - held) / 1e9  # (this form's voxelizer alone: the other's buffers are in `held`)
            held = now
        shape["nchunk"] = voxs[0].last_plan()["nchunk"]
        q.grad = t.grad = None
        rel = lambda x, y: float(f"{float((x - y).abs().max() / y.abs().max()):.3g}")  # noqa: E731
        agree = [rel(kept["moments"][0], kept["grids"][0]), rel(kept["moments"][1], kept["grids"][1])]
        times = {name: [] for name in steps}
        for _ in range(a.rounds):
            for name, step in steps.items():  # alternating: one window of each form per round
                times[name].append(window(step, a.window))
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        one = 4.0 * shape["C"] * shape["D"] ** 3 / 1e9
        done.append(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()}, spread={k: round(v, 4) for k, v in spread.items()},
                         torch_gb={k: round(v, 4) for k, v in torch_gb.items()}, lib_gb={k: round(v, 4) for k, v in lib_gb.items()},
                         chunk_grids_gb=round(one * -(-B // shape["nchunk"]), 4), all_grids_gb=round(one * B, 4), agree=agree,
                         rounds=a.rounds, window_s=a.window))
        print(json.dumps(done[-1]), flush=True)
        del steps, kept, voxs, q, t
        torch.cuda.empty_cache()
    text = table(done)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
