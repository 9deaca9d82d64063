#!/usr/bin/env python3
"""Backward pass with radius gradients against the backward without them (radii_grad=True; DESIGN.md "Backward pass").

    python3 tools/rate_grad_radii.py [--steps 20] [--rounds 3] [--rows cfg2x256,cfg4x128] [--radii atom,channel]

Per row the workload's molecules with radii of their own kind:
  atom      one radius per atom, all 1.0 (the radius of the cfg workloads), on an atom-wise voxelizer
  channel   channel-wise radii, 4 distinct values over the channels (features mode only)
and, on one voxelizer and the same upstream gradient G, two timings (HIP events on the caller's stream, one call each):
  bwd ms        mvx_backward_batch: coordinate and feature gradients
  bwd+r ms      mvx_backward_radii_batch: the same outputs plus dL/dradii
  ratio         bwd+r / bwd (target <= 1.10 for one radius per atom)
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

    return {"cfg2x256": (W.cfg2(batch=256), 256), "cfg4x128": (W.cfg4(batch=128), 128)}


def setup(wl, B, kind):
    import torch

    import molvoxel_amd

    kw = {"sigma": wl.sigma} if wl.density == "gaussian" else {}
    if wl.blockdim is not None:
        kw["blockdim"] = wl.blockdim
    rt = "atom-wise" if kind == "atom" else "channel-wise"
    vox = molvoxel_amd.create_voxelizer(wl.resolution, wl.dimension, rt, wl.density, library="hip", differentiable=True,
                                        radii_grad=True, **kw)
    ids = list(range(B))
    coords = [wl.coords[i] - wl.centers[i] for i in ids]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords]).astype(np.int64)
    c = vox.asarray(np.concatenate(coords), "coords").requires_grad_(True)
    if wl.mode == "features":
        chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features").requires_grad_(True)
    else:
        chan = torch.as_tensor(np.concatenate([wl.channels[i] for i in ids]).astype(np.int32), device=vox.device)
    C_ = wl.num_channels if wl.num_channels is not None else (chan.shape[1] if chan.ndim == 2 else int(chan.max()) + 1)
    if kind == "atom":
        radii = torch.ones(int(offsets[-1]), device=vox.device, requires_grad=True)
    else:
        radii = torch.as_tensor(np.resize(np.array([1.0, 1.2, 1.5, 1.8], np.float32), C_), device=vox.device).requires_grad_(True)
    grid = vox.forward_batch(c, offsets, None, chan, radii, num_channels=wl.num_channels)
    G = torch.randn_like(grid)
    fn = grid.grad_fn
    spec = fn.spec
    cs, fs = spec.coords, (spec.channels if spec.mode == "features" else None)  # the call's record: the arrays as the library read them
    feat = wl.mode == "features"
    bwd = lambda: vox._backward(spec, cs, fs, G, feat)  # noqa: E731
    bwd_r = lambda: vox._backward(spec, cs, fs, G, feat, True)  # noqa: E731
    return vox, bwd, bwd_r, C_


def timed(fn, steps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default=",".join(rows()))
    ap.add_argument("--radii", default="atom,channel")
    args = ap.parse_args()
    table = rows()
    for name in args.rows.split(","):
        wl, B = table[name]
        for kind in args.radii.split(","):
            if kind == "channel" and wl.mode != "features":
                continue
            vox, bwd, bwd_r, C_ = setup(wl, B, kind)
            for _ in range(args.warmup):
                bwd()
                bwd_r()
            torch.cuda.synchronize()
            t0, t1 = [], []
            for _ in range(args.rounds):
                t0.append(timed(bwd, args.steps))
                t1.append(timed(bwd_r, args.steps))
            b0, b1 = float(np.median(t0)), float(np.median(t1))
            print(json.dumps(dict(row=name, radii=kind, molecules=B, D=wl.dimension, C=C_, mode=wl.mode, bwd_ms=round(b0, 4),
                                  bwd_radii_ms=round(b1, 4), ratio=round(b1 / b0, 3))), flush=True)
            del vox, bwd, bwd_r
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
