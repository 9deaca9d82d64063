#!/usr/bin/env python3
"""Same-box A/B of channels-last grids (grid_layout="channels_last") against the path without the option.

    python3 tools/rate_channels_last.py [--steps 20] [--rounds 3] [--rows cfg2x256,...] [--dtypes f32,bf16]

One process, the forms alternating round by round on the same inputs. Per row, element type and form:
  direct     the channels-last voxelizer: forward_batch / forward writes NDHWC
  two-pass   the baseline: the contiguous voxelizer's call followed by .contiguous(memory_format=torch.channels_last_3d)
  ncdhw      the contiguous voxelizer's call alone (no conversion: what the kernels cost in the other layout)
  step ms    one call end to end (HIP events around `steps` calls on the caller's stream)
  kernel ms  voxelize launches of one call (HIP events on the launch stream, mvx_set_profiling), summed - direct and ncdhw
  TB/s       grid and input bytes / kernel time, bytes per molecule = e * C * D^3 + 156 * N, e = 4 or 2
WRITE_SIZE comes from a separate run of one row under `rocprofv3 --pmc WRITE_SIZE` (--pmc-run: one warm-up call and one
call of the direct form, nothing else).
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
        "cfg4x128": (W.cfg4(batch=128), list(range(128)), "batch"),
        "cfg3x256": (W.cfg3(batch=256), list(range(256)), "batch"),
        "D49x64": (W.cfg2(batch=64, dimension=49, n_atoms=int(round(4000 * (48 / 63.0) ** 3))), list(range(64)), "batch"),
        "cfg2_pocket_per_call": (W.cfg2(batch=1), [0], "call"),
    }


def make_step(wl, ids, kind, bf16, channels_last):
    import torch

    import molvoxel_amd

    kw = {"sigma": wl.sigma} if wl.density == "gaussian" else {}
    if wl.blockdim is not None:
        kw["blockdim"] = wl.blockdim
    if bf16:
        kw["grid_dtype"] = "bfloat16"
    if channels_last:
        kw["grid_layout"] = "channels_last"
    vox = molvoxel_amd.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, wl.density, library="hip", **kw)
    coords = [wl.coords[i] - wl.centers[i] for i in ids]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords]).astype(np.int64)
    d_coords = vox.asarray(np.concatenate(coords), "coords")
    nch = wl.num_channels
    if wl.mode == "features":
        chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features")
    else:
        chan = torch.as_tensor(np.concatenate([wl.channels[i] for i in ids]).astype(np.int32), device=vox.device)
    radii = wl.radii[ids[0]]
    if not np.isscalar(radii):
        radii = vox.asarray(np.concatenate([wl.radii[i] for i in ids]), "radii")
    out = vox.get_empty_grid(nch, batch_size=len(ids))
    if kind == "call":
        call = lambda: vox.forward(d_coords, None, chan, radii, out_grid=out[0]).unsqueeze(0)  # noqa: E731
    else:
        call = lambda: vox.forward_batch(d_coords, offsets, None, chan, radii, num_channels=nch, out_grid=out)  # noqa: E731
    nbytes = (2 if bf16 else 4) * len(ids) * nch * wl.dimension ** 3 + 156 * int(offsets[-1])
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
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--pmc-run", action="store_true", help="one warm-up call and one call of the direct form of the first row")
    args = ap.parse_args()
    table = rows()
    for name in args.rows.split(","):
        wl, ids, kind = table[name]
        for dt in args.dtypes.split(","):
            bf16 = dt == "bf16"
            direct = make_step(wl, ids, kind, bf16, True)
            if args.pmc_run:
                for _ in range(2):
                    g = direct[1]()
                torch.cuda.synchronize()
                print(json.dumps(dict(row=name, dtype=dt, grid_bytes=g.numel() * g.element_size(), launches_per_call=1)), flush=True)
                return
            plain = make_step(wl, ids, kind, bf16, False)
            plain_step = plain[1]
            forms = {"direct": direct, "ncdhw": plain,
                     "two-pass": (plain[0], lambda: plain_step().contiguous(memory_format=torch.channels_last_3d), plain[2])}
            assert torch.equal(forms["direct"][1](), forms["two-pass"][1]()), "the direct writer and the baseline disagree"
            assert forms["direct"][1]().is_contiguous(memory_format=torch.channels_last_3d)
            for _, step, _ in forms.values():
                for _ in range(args.warmup):
                    step()
            torch.cuda.synchronize()
            res = {k: dict(kernel=[], step=[]) for k in forms}
            for _ in range(args.rounds):  # interleaved: same inputs, same process
                for k, (vox, step, _) in forms.items():
                    res[k]["step"].append(timed(vox, step, args.steps, False))
                    if k != "two-pass":
                        res[k]["kernel"].append(timed(vox, step, args.steps, True))
            out = dict(row=name, dtype=dt, molecules=len(ids), D=wl.dimension, C=wl.num_channels)
            for k, (_, _, nbytes) in forms.items():
                out[f"{k}_step_ms"] = round(float(np.median(res[k]["step"])), 4)
                out[f"{k}_step_ms_rounds"] = [round(x, 4) for x in res[k]["step"]]
                if res[k]["kernel"]:
                    km = float(np.median(res[k]["kernel"]))
                    out[f"{k}_kernel_ms"] = round(km, 4)
                    out[f"{k}_TBps"] = round(nbytes / (km * 1e-3) / 1e12, 3)
            out["direct/two-pass step"] = round(out["direct_step_ms"] / out["two-pass_step_ms"], 3)
            out["ndhwc/ncdhw kernel"] = round(out["direct_kernel_ms"] / out["ncdhw_kernel_ms"], 3)
            print(json.dumps(out), flush=True)
            del forms, res, direct, plain
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
