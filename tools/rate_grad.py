#!/usr/bin/env python3
"""Backward pass against the forward voxelize kernel (differentiable=True; DESIGN.md "Backward pass").

    python3 tools/rate_grad.py [--steps 20] [--rounds 3] [--rows cfg2x256,cfg4x128,ligands_cfg3x256] [--order 1|0]

(--order: the "grad_order" option - 0 the caller's order (the default), 1 atoms in spatial order, XCD by XCD)

One process per run. Per row:
  fwd kernel ms   voxelize launches of one forward call (HIP events, mvx_set_profiling), summed
  bwd ms          one mvx_backward_batch call (HIP events around it on the caller's stream: offsets upload, prep_kernel and
                  grad_kernel; the profiling ring does not see it)
  bwd/fwd         the ratio the backward's performance bar is stated in (target <= 3, goal <= 2)
  G TB/s          bytes of G (one read of the grid) over bwd ms
Kernel times of prep_kernel and grad_kernel alone come from a separate run of this script under
`rocprofv3 --kernel-trace --stats`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows():
    from molvoxel_amd import workloads as W

    return {
        "cfg2x256": (W.cfg2(batch=256), 256),
        "cfg4x128": (W.cfg4(batch=128), 128),
        "ligands_cfg3x256": (W.cfg3(batch=256), 256),
    }


def setup(wl, B, order):
    import torch

    import molvoxel_amd

    kw = {"sigma": wl.sigma} if wl.density == "gaussian" else {}
    if wl.blockdim is not None:
        kw["blockdim"] = wl.blockdim
    vox = molvoxel_amd.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, wl.density, library="hip",
                                        differentiable=True, **kw)
    vox.debug_option("grad_order", order)
    ids = list(range(B))
    coords = [wl.coords[i] - wl.centers[i] for i in ids]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords]).astype(np.int64)
    c = vox.asarray(np.concatenate(coords), "coords").requires_grad_(True)
    if wl.mode == "features":
        chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features").requires_grad_(True)
    else:
        chan = torch.as_tensor(np.concatenate([wl.channels[i] for i in ids]).astype(np.int32), device=vox.device)
    radii = wl.radii[0]
    if not np.isscalar(radii):
        radii = vox.asarray(np.concatenate([wl.radii[i] for i in ids]), "radii")
    grid = vox.forward_batch(c, offsets, None, chan, radii, num_channels=wl.num_channels)
    G = torch.randn_like(grid)
    fn = grid.grad_fn
    spec = fn.spec
    cs, fs = spec.coords, (spec.channels if spec.mode == "features" else None)  # the call's record: the arrays as the library read them
    fwd = lambda: vox.forward_batch(c.detach(), offsets, None, chan.detach(), radii, num_channels=wl.num_channels)
    bwd = lambda: vox._backward(spec, cs, fs, G, wl.mode == "features")
    return vox, fwd, bwd, G.numel() * G.element_size()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", default=",".join(rows()))
    ap.add_argument("--order", type=int, default=0)
    args = ap.parse_args()
    table = rows()
    for name in args.rows.split(","):
        wl, B = table[name]
        vox, fwd, bwd, gbytes = setup(wl, B, args.order)
        for _ in range(args.warmup):
            fwd()
            bwd()
        torch.cuda.synchronize()
        f_ms, b_ms = [], []
        for _ in range(args.rounds):
            vox.set_profiling(True)
            for _ in range(args.steps):
                fwd()
            torch.cuda.synchronize()
            f_ms.append(float(np.sum(vox.read_kernel_times_ms())) / args.steps)
            vox.set_profiling(False)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                bwd()
            b.record()
            b.synchronize()
            b_ms.append(a.elapsed_time(b) / args.steps)
        f, bk = float(np.median(f_ms)), float(np.median(b_ms))
        print(json.dumps(dict(row=name, order=args.order, molecules=B, D=wl.dimension, C=wl.num_channels, mode=wl.mode,
                              fwd_kernel_ms=round(f, 4), bwd_ms=round(bk, 4), bwd_over_fwd=round(bk / f, 2),
                              G_TBps=round(gbytes / (bk * 1e-3) / 1e12, 3))), flush=True)
        del vox, fwd, bwd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
