#!/usr/bin/env python3
"""Damped Newton refinement of B poses of ONE cloud together: what a round - one second-order evaluation and one
Levenberg-Marquardt step - costs in the views form, on the repeated cloud, and with the step done by torch ops.

    python3 tools/rate_refine.py [--rounds 7] [--window 0.5] [--steps 12] [--rows ligand1024,cfg2x64]

Rows
  ligand1024  the 10GS ligand (tests/golden/10gs) under 1024 poses, 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
  cfg2x64     molecule 0 of the cfg-2 workload (4 000 atoms, 32 channels, 64^3, radius 1.0) under 64 poses
The field is the cloud's own grid at the identity pose; the starts lie within 5 degrees and 0.3 A of it (seeded).
Whole refinements of `--steps` rounds from the same starts, so that every repetition does the same work (poses finish and stop
solving as they do in use); reported per round, i.e. per (steps + 1) evaluations and steps:
  views_lm     a: refine_posed_views                               score_hessian_posed_views + lm_step
  batch_lm     b: refine_posed_batch on coords.repeat(B, 1)         score_hessian_posed_batch + lm_step
  batch_torch  c: (b)'s evaluations with the step done by torch.linalg.solve_ex (torch.linalg.solve without the error check that
                  synchronises), apply_twist and torch.where, no host read
and the pieces alone, on the start state (which they leave as it is):
  eval_views, eval_batch   one evaluation
  step_lm                  lm_step without a trial: the solve and the twist of every pose, one launch
  step_torch               the same by torch.linalg.solve_ex and apply_twist
One process; every form is warmed, then the forms alternate round by round; each window repeats its form until it has run for at
least `--window` seconds and is timed with device events; medians and the spread (max - min) / median over the rounds. Before
timing the final scores of the three refinements are compared."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rate_score import window  # noqa: E402

ROWS = {"ligand1024": ("ligand", 1024), "cfg2x64": ("cfg2", 64)}
LAM_DOWN, LAM_UP, MAX_DROPPED = 1.0 / 3.0, 10.0, 3


def starts(B, seed=0):
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.deg2rad(rng.uniform(1.0, 5.0, B))
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    d = rng.standard_normal((B, 3))
    return q, d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.06, 0.3, (B, 1))


def build(what, B, steps):
    """(voxelizer, {form: step()}, compare(), shape)"""
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W
    from molvoxel_amd.etc import mol as M
    from molvoxel_amd.voxelizer.hip.voxelizer import LMState, apply_twist

    if what == "ligand":
        lig = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
        cloud = np.asarray(lig.coords, np.float64)
        feats = np.random.default_rng(1).random((cloud.shape[0], 8)).astype(np.float32)
        D, radius = 48, 1.5
    else:
        wl = W.cfg2(batch=1)
        cloud, feats, D, radius = np.asarray(wl.coords[0], np.float64), np.asarray(wl.channels[0], np.float32), wl.dimension, 1.0
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    dev = vox.device
    n = cloud.shape[0]
    xyz, f = torch.as_tensor(cloud, device=dev), torch.as_tensor(feats, device=dev)
    cen = xyz.mean(0, keepdim=True).repeat(B, 1)
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device=dev)
    field = vox.forward_posed_batch(xyz, np.array([0, n], np.int64), cen[:1], ident, torch.zeros((1, 3), dtype=torch.float64, device=dev),
                                    f, radius)[0].clone()
    qn, tn = starts(B)
    q0, t0 = torch.tensor(qn, device=dev), torch.tensor(tn, device=dev)
    xyz_rep, f_rep = xyz.repeat(B, 1), f.repeat(B, 1)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    kw = dict(steps=steps, lam_down=LAM_DOWN, lam_up=LAM_UP, max_dropped=MAX_DROPPED)
    eye = torch.eye(6, dtype=torch.float64, device=dev)
    out = {}

    def eval_views(q=q0, t=t0):
        return vox.score_hessian_posed_views(xyz, cen, q, t, f, radius, field)

    def eval_batch(q=q0, t=t0):
        return vox.score_hessian_posed_batch(xyz_rep, offsets, cen, q, t, f_rep, radius, field)

    def views_lm():
        out["views_lm"] = vox.refine_posed_views(xyz, cen, q0, t0, f, radius, field, **kw)

    def batch_lm():
        out["batch_lm"] = vox.refine_posed_batch(xyz_rep, offsets, cen, q0, t0, f_rep, radius, field, **kw)

    def torch_step(q, t, G, H, lam, done):
        """xi of the undone poses and the trial pose: a failed solve (a non-finite xi) and a finished pose stay."""
        xi = torch.linalg.solve_ex(lam[:, None, None] * eye - H, G)[0]  # (solve without its error check, which reads the host)
        ok = torch.isfinite(xi).all(dim=1) & ~done
        xi = torch.where(ok[:, None], xi, torch.zeros_like(xi))
        return apply_twist(q, t, xi)

    def batch_torch():
        """refine_posed_batch's loop with the bookkeeping in torch: masks and torch.where instead of host reads."""
        q, t = q0.clone(), t0.clone()
        S, G, H = eval_batch(q, t)
        lam = 1e-3 * H.abs().reshape(B, 36).amax(dim=1)
        dropped = torch.zeros(B, dtype=torch.int32, device=dev)
        taken = torch.zeros_like(dropped)
        q2, t2 = torch_step(q, t, G, H, lam, dropped >= MAX_DROPPED)
        for _ in range(steps):
            S2, G2, H2 = eval_batch(q2, t2)
            live = dropped < MAX_DROPPED
            acc = live & (S2 > S)
            rej = live & ~acc
            q, t = torch.where(acc[:, None], q2, q), torch.where(acc[:, None], t2, t)
            S, G, H = torch.where(acc, S2, S), torch.where(acc[:, None], G2, G), torch.where(acc[:, None, None], H2, H)
            lam = torch.where(acc, lam * LAM_DOWN, torch.where(rej, lam * LAM_UP, lam))
            taken = taken + acc.to(torch.int32)
            dropped = torch.where(acc, torch.zeros_like(dropped), dropped + rej.to(torch.int32))
            q2, t2 = torch_step(q, t, G, H, lam, dropped >= MAX_DROPPED)
        out["batch_torch"] = (q, t, S, dict(taken=taken, dropped=dropped))

    S0, G0, H0 = eval_batch()
    lam0 = 1e-3 * H0.abs().reshape(B, 36).amax(dim=1)
    state = LMState(q0.clone(), t0.clone(), S0, G0, H0, lam0)
    none = torch.zeros(B, dtype=torch.bool, device=dev)

    def step_lm():
        vox.lm_step(state, lam_down=LAM_DOWN, lam_up=LAM_UP, max_dropped=MAX_DROPPED)

    def step_torch():
        out["step_torch"] = torch_step(q0, t0, G0, H0, lam0, none)

    def compare():
        (qv, tv, Sv, iv), (qb, tb, Sb, ib), (qt, tt, St, it) = out["views_lm"], out["batch_lm"], out["batch_torch"]
        step_torch()
        step_lm()
        return dict(views_vs_batch_score_rel=float(((Sv - Sb).abs() / Sb.abs()).max()),
                    lm_vs_torch_score_rel=float(((Sb - St).abs() / Sb.abs()).max()),
                    taken_mean=float(ib["taken"].double().mean()), finished=int((ib["dropped"] >= MAX_DROPPED).sum()),
                    taken_same_as_torch=int((ib["taken"] == it["taken"]).sum()),
                    first_trial_q_diff=float((state.q2 - out["step_torch"][0]).abs().max()),
                    score_start=float(S0.mean()), score_end=float(Sb.mean()))

    forms = {"views_lm": views_lm, "batch_lm": batch_lm, "batch_torch": batch_torch, "eval_views": eval_views, "eval_batch": eval_batch,
             "step_lm": step_lm, "step_torch": step_torch}
    return vox, forms, compare, dict(B=B, atoms=n, C=int(f.shape[1]), D=D, steps=steps)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rows", default="ligand1024,cfg2x64")
    a = ap.parse_args()
    whole = ("views_lm", "batch_lm", "batch_torch")
    for row in a.rows.split(","):
        what, B = ROWS[row]
        vox, forms, compare, shape = build(what, B, a.steps)
        for step in forms.values():
            for _ in range(a.warmup):
                step()
        agree = compare()
        times = {name: [] for name in forms}
        for _ in range(a.rounds):
            for name, step in forms.items():  # alternating: one window of each form per round
                ms = window(step, a.window)
                times[name].append(ms / (a.steps + 1) if name in whole else ms)
        med = {name: statistics.median(v) for name, v in times.items()}
        spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
        print(json.dumps(dict(row=row, **shape, ms={k: round(v, 4) for k, v in med.items()},
                              spread={k: round(v, 4) for k, v in spread.items()},
                              views_over_batch=round(med["views_lm"] / med["batch_lm"], 4),
                              torch_over_lm_round=round(med["batch_torch"] / med["batch_lm"], 4),
                              torch_over_lm_step=round(med["step_torch"] / med["step_lm"], 4),
                              agree={k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in agree.items()},
                              rounds=a.rounds, window_s=a.window)), flush=True)
        del vox, forms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
