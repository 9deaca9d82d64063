#!/usr/bin/env python3
"""Same-box A/B of bfloat16 grids against float32 grids (grid_dtype="bfloat16"; DESIGN.md "bfloat16 grids").

    python3 tools/rate_bf16.py [--steps 20] [--rounds 3] [--rows cfg2x256,...] [--lib path/to/libmvx_hip.so]

(--lib: an A/B variant of the library, e.g. one built by tools/ab_build.sh with other pacing constants)

One process, the float32 and bfloat16 handles alternating round by round on the same inputs. Per row and form:
  kernel ms  voxelize launches of one call (HIP events on the launch stream, mvx_set_profiling), summed
  step ms    one call end to end (HIP events around `steps` calls on the caller's stream)
  TB/s       bytes / kernel time, bytes per molecule = e * C * D^3 + 156 * N, e = 4 or 2
and the form users run without the option: the float32 call followed by .to(torch.bfloat16) (step only).
Kernel times from rocprofv3 come from a separate run of this script under `rocprofv3 --kernel-trace --stats`.
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
        "cfg2x256": (W.cfg2(batch=256), list(range(256)), "batch"),
        "cfg3x256": (W.cfg3(batch=256), list(range(256)), "batch"),
        "single_cfg2x64": (W.cfg2(batch=64), list(range(64)), "single"),
        "cfg2_pocket_per_call": (W.cfg2(batch=1), [0], "call"),
        "cfg4x128": (W.cfg4(batch=128), list(range(128)), "batch"),
        "cfg5x4": (W.cfg5(batch=4), list(range(4)), "batch"),
        "D49_runs_x64": (W.cfg2(batch=64, dimension=49, n_atoms=int(round(4000 * (48 / 63.0) ** 3))), list(range(64)), "batch"),
        # per-lane index ranges (blockdim 5): the twins that carry the run-wise write-out and spill more scalar registers
        "bd5_cfg2x64": (_blockdim(W.cfg2(batch=64), 5), list(range(64)), "batch"),
        "bd5_cfg3x256": (_blockdim(W.cfg3(batch=256), 5), list(range(256)), "batch"),
    }


def _blockdim(wl, bd):
    wl.blockdim = bd
    return wl


def make_step(wl, ids, kind, bf16):
    import torch

    import molvoxel_amd

    kw = {"sigma": wl.sigma} if wl.density == "gaussian" else {}
    if wl.blockdim is not None:
        kw["blockdim"] = wl.blockdim
    if bf16:
        kw["grid_dtype"] = "bfloat16"
    vox = molvoxel_amd.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, wl.density, library="hip", **kw)
    coords = [wl.coords[i] - wl.centers[i] for i in ids]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords]).astype(np.int64)
    d_coords = vox.asarray(np.concatenate(coords), "coords")
    chan, nch = None, wl.num_channels
    if kind == "single":
        nch = 1
    elif wl.mode == "features":
        chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features")
    else:
        chan = torch.as_tensor(np.concatenate([wl.channels[i] for i in ids]).astype(np.int32), device=vox.device)
    radii = wl.radii[ids[0]]
    if not np.isscalar(radii):
        radii = vox.asarray(np.concatenate([wl.radii[i] for i in ids]), "radii")
    out = vox.get_empty_grid(nch, batch_size=len(ids))
    if kind == "call":
        call = lambda: vox.forward(d_coords, None, chan, radii, out_grid=out[0])
    else:
        call = lambda: vox.forward_batch(d_coords, offsets, None, chan, radii, num_channels=nch, out_grid=out)
    atoms = int(offsets[-1])
    nbytes = (2 if bf16 else 4) * len(ids) * nch * wl.dimension ** 3 + 156 * atoms
    return vox, call, nbytes


def timed(vox, step, steps, kernel):
    import torch

    if kernel:
        vox.set_profiling(True)
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = float(np.sum(vox.read_kernel_times_ms())) / steps
        vox.set_profiling(False)
        return ms
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", default=",".join(rows()))
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        from molvoxel_amd.voxelizer.hip import _lib

        _lib.LIB_PATH = os.path.abspath(args.lib)
    table = rows()
    for name in args.rows.split(","):
        wl, ids, kind = table[name]
        forms = {"f32": make_step(wl, ids, kind, False), "bf16": make_step(wl, ids, kind, True)}
        f32_step = forms["f32"][1]
        forms["f32+cast"] = (forms["f32"][0], lambda: f32_step().to(torch.bfloat16), forms["f32"][2])
        for _, step, _ in forms.values():
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        res = {k: dict(kernel=[], step=[]) for k in forms}
        for _ in range(args.rounds):  # A/B alternating, same inputs, same process
            for k, (vox, step, _) in forms.items():
                res[k]["step"].append(timed(vox, step, args.steps, False))
                if k != "f32+cast":
                    res[k]["kernel"].append(timed(vox, step, args.steps, True))
        out = dict(row=name, molecules=len(ids), D=wl.dimension)
        for k, (_, _, nbytes) in forms.items():
            st = float(np.median(res[k]["step"]))
            out[f"{k}_step_ms"] = round(st, 4)
            if res[k]["kernel"]:
                km = float(np.median(res[k]["kernel"]))
                out[f"{k}_kernel_ms"] = round(km, 4)
                out[f"{k}_TBps"] = round(nbytes / (km * 1e-3) / 1e12, 3)
        out["bf16/f32 kernel"] = round(out["bf16_kernel_ms"] / out["f32_kernel_ms"], 3)
        out["bf16/f32 step"] = round(out["bf16_step_ms"] / out["f32_step_ms"], 3)
        out["(f32+cast)/bf16 step"] = round(out["f32+cast_step_ms"] / out["bf16_step_ms"], 2)
        print(json.dumps(out), flush=True)
        del forms, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
