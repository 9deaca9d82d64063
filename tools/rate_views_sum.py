#!/usr/bin/env python3
"""One summed grid of B views of ONE shared cloud (forward_views_sum / forward_posed_views_sum), with and without the split of the
sum into parts (set_sum_parts), against the forms that existed before them.

    python3 tools/rate_views_sum.py [--rounds 7] [--window 0.5] [--rows ligand1024,pocket256,cfg2x256] [--pocket-k K]

Rows
  ligand1024  1024 poses of the 10GS ligand (tests/golden/10gs, 33 atoms), 8 synthetic feature channels, 48^3 at 0.5 A, radius 1.5
      A/K   forward_posed_views_sum on a voxelizer with set_sum_parts(K), K = 1, 2, 4, 8, 16
      B     forward_posed_sum on the cloud repeated 1024 times (parts = 1): the form the summed grid had before
      C     forward_posed_views(...).sum(0): through the 1024 grids
  pocket256   256 boxes of the 10GS pocket centred on its first 256 atoms, 32 synthetic channels, 64^3 at 0.5 A, radius 1.5
      A/K   forward_views_sum, K = 1 and the K with the smallest median of the ligand row (or --pocket-k)
      C     forward_views(...).sum(0)
  cfg2x256    256 molecules of the cfg-2 workload (4 000 atoms, 32 channels, 64^3): a batch that fills the card without parts
      S/K   forward_sum, K = 1, 2, 4
One process, one card; every form is warmed, then the forms alternate round by round; each window repeats the step until it has
run for at least `--window` seconds and is timed with device events (tools/rate_score.window); medians per step and the spread
(max - min) / median over the rounds. Memory: torch.cuda.max_memory_allocated above the inputs over one warmed step of each form,
plus the partial grids the library holds outside torch's allocator (G x C x D^3 x 4 bytes, computed). Before timing, every form's
result is compared with the row's first form. No default is chosen from these numbers."""
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

LIGAND_KS, CFG2_KS = (1, 2, 4, 8, 16), (1, 2, 4)


def _vox(D, K):
    import molvoxel_amd as mv

    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    if K > 1:
        vox.set_sum_parts(K)
    return vox


def _partial_mib(B, K, C_, D):
    if K <= 1:
        return 0.0
    q = -(-B // K)
    return -(-B // q) * C_ * D ** 3 * 4 / 2 ** 20


def ligand(B=1024):
    import torch

    from molvoxel_amd.etc import mol as M

    lig = M.read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    cloud = np.asarray(lig.coords, np.float64)
    N, C_, D, radius = cloud.shape[0], 8, 48, 1.5
    vox = {K: _vox(D, K) for K in LIGAND_KS}
    dev = vox[1].device
    xyz = torch.as_tensor(cloud, device=dev)
    f = torch.as_tensor(np.random.default_rng(1).random((N, C_)).astype(np.float32), device=dev)
    cen = torch.as_tensor(np.repeat(cloud.mean(0)[None], B, axis=0), device=dev)
    qn, tn = poses(B)
    q, t = torch.tensor(qn, device=dev), torch.tensor(tn, device=dev)
    rep_xyz, rep_f = xyz.repeat(B, 1), f.repeat(B, 1)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    forms = {f"A/{K}": (lambda K=K: vox[K].forward_posed_views_sum(xyz, cen, q, t, f, radius)) for K in LIGAND_KS}
    forms["B"] = lambda: vox[1].forward_posed_sum(rep_xyz, offsets, cen, q, t, rep_f, radius)
    forms["C"] = lambda: vox[1].forward_posed_views(xyz, cen, q, t, f, radius).sum(0)
    extra = {f"A/{K}": _partial_mib(B, K, C_, D) for K in LIGAND_KS}
    return forms, extra, dict(B=B, atoms=N, C=C_, D=D)


def pocket(B=256, ks=(1,)):
    import torch

    from molvoxel_amd.etc import mol as M

    pk = M.read_pdb(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_pocket_nowater.pdb"))
    N, C_, D, radius = pk.coords.shape[0], 32, 64, 1.5
    vox = {K: _vox(D, K) for K in ks}
    dev = vox[ks[0]].device
    xyz = torch.as_tensor(np.asarray(pk.coords, np.float64), device=dev)
    f = torch.as_tensor(np.random.default_rng(0).random((N, C_)).astype(np.float32), device=dev)
    cen = xyz[:B].clone()
    forms = {f"A/{K}": (lambda K=K: vox[K].forward_views_sum(xyz, cen, f, radius)) for K in ks}
    forms["C"] = lambda: vox[ks[0]].forward_views(xyz, cen, f, radius).sum(0)
    return forms, {f"A/{K}": _partial_mib(B, K, C_, D) for K in ks}, dict(B=B, atoms=N, C=C_, D=D)


def cfg2(B=256):
    import torch

    from molvoxel_amd import workloads as W

    wl = W.cfg2(batch=B)
    clouds, feats, D = [wl.coords[i] for i in range(B)], [wl.channels[i] for i in range(B)], wl.dimension
    vox = {K: _vox(D, K) for K in CFG2_KS}
    dev = vox[1].device
    offsets = np.cumsum([0] + [c.shape[0] for c in clouds]).astype(np.int64)
    xyz = torch.as_tensor(np.concatenate(clouds), device=dev)
    f = torch.as_tensor(np.concatenate(feats), device=dev)
    cen = torch.as_tensor(np.stack([c.mean(0) for c in clouds]), device=dev)
    forms = {f"S/{K}": (lambda K=K: vox[K].forward_sum(xyz, offsets, cen, f, 1.0)) for K in CFG2_KS}
    C_ = int(f.shape[1])
    return forms, {f"S/{K}": _partial_mib(B, K, C_, D) for K in CFG2_KS}, dict(B=B, atoms=int(offsets[-1]), C=C_, D=D)


def measure(row, forms, extra, shape, a):
    """One JSON line for a row; returns the medians (ms per step) of its forms."""
    import torch

    peak, kept = {}, {}
    for name, step in forms.items():
        for _ in range(a.warmup):
            out = step()
        kept[name] = out.detach().clone()
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20 + extra.get(name, 0.0)
    first = next(iter(forms))
    scale = float(kept[first].abs().max())
    rel = {name: float(f"{float((kept[name] - kept[first]).abs().max()) / scale:.3g}") for name in forms if name != first}
    kept.clear()
    torch.cuda.empty_cache()
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, step in forms.items():  # alternating: one window of each form per round
            times[name].append(window(step, a.window))
    med = {name: statistics.median(v) for name, v in times.items()}
    spread = {name: (max(v) - min(v)) / med[name] for name, v in times.items()}
    print(json.dumps(dict(row=row, **shape, step_ms={k: round(v, 4) for k, v in med.items()},
                          spread={k: round(v, 4) for k, v in spread.items()},
                          peak_mib_above_inputs={k: round(v, 2) for k, v in peak.items()},
                          max_rel_diff_to_first_form=rel, rounds=a.rounds, window_s=a.window)), flush=True)
    return med


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="ligand1024,pocket256,cfg2x256")
    ap.add_argument("--pocket-k", type=int, default=0, help="the K > 1 of the pocket row (default: the best K of the ligand row)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rate_views_sum.py measures on the GPU"
    best = a.pocket_k
    for row in a.rows.split(","):
        if row == "ligand1024":
            med = measure(row, *ligand(), a)
            if not best:
                best = min(LIGAND_KS, key=lambda K: med[f"A/{K}"])
            b = med["B"]
            print(json.dumps(dict(row=row, baseline="B", over_B={k: round(v / b, 4) for k, v in med.items()},
                                  over_C={k: round(v / med["C"], 4) for k, v in med.items()})), flush=True)
        elif row == "pocket256":
            ks = (1,) if best in (0, 1) else (1, best)
            med = measure(row, *pocket(ks=ks), a)
            print(json.dumps(dict(row=row, over_C={k: round(v / med["C"], 4) for k, v in med.items()})), flush=True)
        elif row == "cfg2x256":
            med = measure(row, *cfg2(), a)
            print(json.dumps(dict(row=row, over_K1={k: round(v / med["S/1"], 4) for k, v in med.items()})), flush=True)
        else:
            raise SystemExit(f"unknown row {row}")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
