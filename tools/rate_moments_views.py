#!/usr/bin/env python3
"""The moments of B views of ONE shared cloud, forward alone and as one optimisation step on -NCC with backward(): the views form
(moments_posed_views, the cloud handed over once) against the repeated cloud (moments_posed_batch on B copies).

    python3 tools/rate_moments_views.py [--rounds 7] [--window 0.5] [--rows ligand1024,pocket256] [--out profiles/r19_moments_views.txt]

Rows (tests/golden/10gs), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
  ligand1024  the 10GS ligand under 1024 poses about its centroid, one (C, D, D, D) target shared by all poses
  pocket256   the 10GS pocket seen from 256 boxes centred on its first 256 atoms, each with a pose of its own and a target of its
              own: (B, C, D, D, D) in the views form. moments_posed_batch has no target per molecule: its form of this row reads
              the first view's target for every molecule - the same arithmetic, one target's worth of reads kept in cache
Forms, on the same seeded inputs and poses (q, t require grad); the loss is -sum_{b,c} m2 / sqrt(m1 * sum t_b^2 + 1e-6)
  views   moments_posed_views(xyz, ...)                 selection, gather, one walk; backward: the rows, mvx_views_reduce, poses
  batch   moments_posed_batch(xyz.repeat(B, 1), ...)    the B copies are made inside the timed step, as a caller has to make them
Per form `forward` (no graph) and `step` (forward, loss, backward()) on a moments_grad voxelizer of its own. One process; every
shape is warmed, then the two forms alternate round by round; each window repeats the step until it has run for at least
`--window` seconds and is timed with device events; medians and the spread (max - min) / median over the rounds. Peak device
memory of one step as tools/rate_moments_grad.py measures it: torch's allocator over the step above what was allocated before
it, plus what the library holds itself. The pose gradients of the two forms are compared before timing where both read the same
targets (largest |views - batch| / largest |batch|)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rate_moments_grad import _held_by_library, peak_memory  # noqa: E402
from tools.rate_score import poses, window  # noqa: E402

ROWS = {"ligand1024": ("ligand", 1024), "ligand64": ("ligand", 64), "pocket256": ("pocket", 256), "pocket16": ("pocket", 16)}
FORMS = ("views", "batch")
C_, D, RADIUS = 8, 48, 1.5


def build(what, B):
    """({form: {"forward": fn, "step": fn}}, leaves, shape, the two voxelizers) - step() leaves the gradients in q.grad / t.grad."""
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd.etc import mol as M

    gold = os.path.join(ROOT, "tests", "golden", "10gs")
    if what == "ligand":
        cloud = np.asarray(M.read_sdf(os.path.join(gold, "10gs_ligand.sdf"))[0].coords, np.float64)
        centers = np.repeat(cloud.mean(0)[None], B, 0)
    else:
        cloud = np.asarray(M.read_pdb(os.path.join(gold, "10gs_pocket_nowater.pdb")).coords, np.float64)
        centers = cloud[:B].copy()
    per_view = what == "pocket"
    N = cloud.shape[0]
    vox = {name: mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True, moments_grad=True) for name in FORMS}
    dev = vox["views"].device
    xyz = torch.as_tensor(cloud, device=dev)
    f = torch.as_tensor(np.random.default_rng(1).random((N, C_)).astype(np.float32), device=dev)
    cen = torch.as_tensor(centers, device=dev)
    qn, tn = poses(B)
    q = torch.tensor(qn, device=dev, requires_grad=True)
    t = torch.tensor(tn, device=dev, requires_grad=True)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    target = torch.randn(((B,) if per_view else ()) + (C_, D, D, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    tt = (target.double() ** 2).sum(dim=(-3, -2, -1))
    shared = target[0] if per_view else target  # (what the batch form can be given)
    tt_shared = tt[0] if per_view else tt
    _, off = vox["views"].select_posed_views(xyz, cen, q.detach(), t.detach(), radii=RADIUS)

    def loss_of(m, tt):
        return -(m[..., 2] / torch.sqrt(m[..., 1] * tt + 1e-6)).sum()

    def views(qq, tq):
        return vox["views"].moments_posed_views(xyz, cen, qq, tq, f, RADIUS, target=target)

    def batch(qq, tq):
        return vox["batch"].moments_posed_batch(xyz.repeat(B, 1), offsets, cen, qq, tq, f.repeat(B, 1), RADIUS, target=shared)

    def step_of(fn, tt):
        def step():
            q.grad = t.grad = None
            loss_of(fn(q, t), tt).backward()
        return step

    forms = {"views": {"forward": lambda: views(q.detach(), t.detach()), "step": step_of(views, tt)},
             "batch": {"forward": lambda: batch(q.detach(), t.detach()), "step": step_of(batch, tt_shared)}}
    kept = np.diff(off)
    shape = dict(B=B, atoms=N, C=C_, D=D, per_view_targets=per_view, kept_min=int(kept.min()), kept_median=int(np.median(kept)),
                 kept_max=int(kept.max()))
    return forms, (q, t), shape, vox


def table(rows):
    lines = ["moments of B views of one cloud: the views form (moments_posed_views) and the repeated cloud (moments_posed_batch on B copies)",
             "(tools/rate_moments_views.py). ms: median over the rounds of windows timed with device events (spread = (max - min) / median);",
             "forward = the moments alone, step = forward, -NCC, backward() to dq, dt. peak GB of one step: torch's allocator plus the",
             "library's own buffers of that form's voxelizer. agree: largest |views - batch| / largest |batch| of dq, dt (n/a where the",
             "batch form cannot read one target per view and is timed on the first view's target)", ""]
    lines.append(f"{'row':<11}{'B':>5}{'atoms':>6}{'kept':>6}{'targets':>9}  " +
                 "".join(f"{n + ' fwd ms':>15}{'spread':>8}{n + ' step ms':>15}{'spread':>8}{'peak GB':>9}" for n in FORMS))
    for r in rows:
        lines.append(f"{r['row']:<11}{r['B']:>5}{r['atoms']:>6}{r['kept_median']:>6}{'per view' if r['per_view_targets'] else 'shared':>9}  " +
                     "".join(f"{r['forward_ms'][n]:>15.3f}{r['forward_spread'][n]:>8.3f}{r['step_ms'][n]:>15.3f}{r['step_spread'][n]:>8.3f}"
                             f"{r['torch_gb'][n] + r['lib_gb'][n]:>9.3f}" for n in FORMS))
    lines.append("")
    for r in rows:
        fw, st = r["forward_ms"], r["step_ms"]
        mem = {n: r["torch_gb"][n] + r["lib_gb"][n] for n in FORMS}
        lines.append(f"{r['row']}: views / batch = {fw['views'] / fw['batch']:.3f} forward, {st['views'] / st['batch']:.3f} per step, "
                     f"{mem['views'] / mem['batch']:.3f} in peak memory (torch {r['torch_gb']}, library {r['lib_gb']}); "
                     f"backward chunks {r['nchunk']}; agree {r['agree']}")
    return "\n".join(lines) + "\n"


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand1024,pocket256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_moments_views.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rate_moments_views.py measures on the GPU"
    done = []
    for row in a.rows.split(","):
        what, B = ROWS[row]
        forms, (q, t), shape, vox = build(what, B)
        torch.cuda.empty_cache()
        held = _held_by_library(torch)  # (the runtime's own, both handles as made, and the selection build() ran for the shape)
        kept, torch_gb, lib_gb = {}, {}, {}
        for name in FORMS:
            for _ in range(a.warmup):
                forms[name]["forward"]()
                forms[name]["step"]()
            kept[name] = (q.grad.detach().clone(), t.grad.detach().clone())
            peak, now = peak_memory(torch, forms[name]["step"])
            torch_gb[name], lib_gb[name] = peak / 1e9, (now - held) / 1e9  # (this form's voxelizer alone: the other's buffers are in `held`)
            held = now
        shape["nchunk"] = {name: vox[name].last_plan()["nchunk"] for name in FORMS}
        q.grad = t.grad = None
        rel = lambda x, y: float(f"{float((x - y).abs().max() / y.abs().max()):.3g}")  # noqa: E731
        agree = "n/a" if shape["per_view_targets"] else [rel(kept["views"][0], kept["batch"][0]), rel(kept["views"][1], kept["batch"][1])]
        times = {(name, k): [] for name in FORMS for k in ("forward", "step")}
        for _ in range(a.rounds):
            for key in times:  # alternating: one window of each form and kind per round
                times[key].append(window(forms[key[0]][key[1]], a.window))
        med = {key: statistics.median(v) for key, v in times.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in times.items()}
        pick = lambda src, kind: {n: round(src[(n, kind)], 4) for n in FORMS}  # noqa: E731
        done.append(dict(row=row, **shape, forward_ms=pick(med, "forward"), forward_spread=pick(spread, "forward"),
                         step_ms=pick(med, "step"), step_spread=pick(spread, "step"),
                         torch_gb={k: round(v, 4) for k, v in torch_gb.items()}, lib_gb={k: round(v, 4) for k, v in lib_gb.items()},
                         agree=agree, rounds=a.rounds, window_s=a.window))
        print(json.dumps(done[-1]), flush=True)
        del forms, kept, vox, q, t
        torch.cuda.empty_cache()
    text = table(done)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
