#!/usr/bin/env python3
"""Backward pass with sigma / scalar-radius gradients against the backward without them (sigma_grad=True; DESIGN.md
"Sigma and scalar-radius gradients").

    python3 tools/rate_grad_density.py [--steps 20] [--rounds 3]

Rows, each on one voxelizer, the same inputs and the same upstream gradient G (HIP events on the caller's stream, one call each):
  cfg2x256 scalar    scalar radius 1.0: base mvx_backward_batch; mvx_backward_density_batch with sigma alone, with the scalar
                     radius alone, with both
  cfg4x128 atom      one radius per atom (all 1.0): base mvx_backward_batch; density entry with sigma
  cfg2x256 channel   channel-wise features, 4 distinct radii: base mvx_backward_radii_batch (it already pays for the second
                     walk); density entry with radii and sigma
  ratio              new / base. No target was fixed in advance; a row above 1.10 is reported as such.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(wl, B, kind):
    import torch

    import molvoxel_amd

    kw = {"sigma": wl.sigma} if wl.density == "gaussian" else {}
    if wl.blockdim is not None:
        kw["blockdim"] = wl.blockdim
    rt = {"scalar": "scalar", "atom": "atom-wise", "channel": "channel-wise"}[kind]
    vox = molvoxel_amd.create_voxelizer(wl.resolution, wl.dimension, rt, wl.density, library="hip", differentiable=True,
                                        radii_grad=True, sigma_grad=True, **kw)
    ids = list(range(B))
    coords = [wl.coords[i] - wl.centers[i] for i in ids]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords]).astype(np.int64)
    c = vox.asarray(np.concatenate(coords), "coords").requires_grad_(True)
    chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features").requires_grad_(True)
    C_ = chan.shape[1]
    if kind == "scalar":
        radii = 1.0
    elif kind == "atom":
        radii = torch.ones(int(offsets[-1]), device=vox.device, requires_grad=True)
    else:
        radii = torch.as_tensor(np.resize(np.array([1.0, 1.2, 1.5, 1.8], np.float32), C_), device=vox.device).requires_grad_(True)
    grid = vox.forward_batch(c, offsets, None, chan, radii)
    G = torch.randn_like(grid)
    fn = grid.grad_fn
    spec = fn.spec
    cs, fs = spec.coords, (spec.channels if spec.mode == "features" else None)  # the call's record: the arrays as the library read them
    call = lambda *need: (lambda: vox._backward(spec, cs, fs, G, True, *need))  # noqa: E731
    # (need_radii, need_sigma, need_rscalar)
    if kind == "scalar":
        return C_, call(), {"sigma": call(False, True, False), "radius": call(False, False, True), "sigma+radius": call(False, True, True)}
    if kind == "atom":
        return C_, call(), {"sigma": call(False, True, False)}
    return C_, call(True), {"radii+sigma": call(True, True, False)}


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

    from molvoxel_amd import workloads as W

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for name, make, B, kind in (("cfg2x256", W.cfg2, 256, "scalar"), ("cfg4x128", W.cfg4, 128, "atom"),
                                ("cfg2x256", W.cfg2, 256, "channel")):
        wl = make(batch=B)
        C_, base, new = setup(wl, B, kind)
        fns = [base] + list(new.values())
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(args.rounds):  # base and new interleaved round by round: drift hits both alike
            for t, fn in zip(times, fns):
                t.append(timed(fn, args.steps))
        med = [float(np.median(t)) for t in times]
        for what, m in zip(new, med[1:]):
            print(json.dumps(dict(row=name, radii=kind, grads=what, molecules=B, D=wl.dimension, C=C_, base_ms=round(med[0], 4),
                                  new_ms=round(m, 4), ratio=round(m / med[0], 3))), flush=True)
        del base, new, fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
