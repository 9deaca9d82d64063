"""forward_views against forward_batch on the repeated cloud, each as a whole call.

    python3 tools/rate_views.py [--views 256] [--rounds 9]

Cloud: the 10GS pocket of tests/golden/10gs with 32 synthetic feature channels; views centred on the first `views` atoms;
64^3 grids at 0.5 A, scalar radius 1.5. Each variant (no transform; random_rotation=True) is warmed up, then timed in interleaved
rounds (views call, repeated-cloud call, views call, ...) with a device synchronisation around every call; medians are reported
with the ratio and the survivor count per view."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd.etc import mol as M

    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    pocket = M.read_pdb(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_pocket_nowater.pdb"))
    N, B, C = pocket.coords.shape[0], a.views, 32
    vox = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip", output="torch")
    xyz = torch.as_tensor(pocket.coords, device=vox.device)
    feat = torch.as_tensor(np.random.default_rng(0).random((N, C)).astype(np.float32), device=vox.device)
    cen = xyz[:B].clone()
    rep_xyz, rep_feat = xyz.repeat(B, 1), feat.repeat(B, 1)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    out = vox.get_empty_grid(C, batch_size=B)
    _, off = vox.select_views(xyz, cen, radii=1.5)
    cnt = np.diff(off)
    print(f"cloud {N} atoms, {B} views, {C} channels, 64^3 at 0.5 A; survivors per view: min {cnt.min()} median "
          f"{int(np.median(cnt))} max {cnt.max()} (repeated cloud: {N} rows per view)")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for rot in (False, True):
        kw = dict(random_rotation=True) if rot else {}
        views = lambda: vox.forward_views(xyz, cen, feat, 1.5, out_grid=out, **kw)  # noqa: E731
        batch = lambda: vox.forward_batch(rep_xyz, offsets, cen, rep_feat, 1.5, out_grid=out, **kw)  # noqa: E731
        for _ in range(3):
            views(), batch()
        tv, tb = [], []
        for _ in range(a.rounds):
            tv.append(timed(views))
            tb.append(timed(batch))
        mv_, mb = statistics.median(tv), statistics.median(tb)
        print(f"random_rotation={rot}: forward_views {mv_:.3f} ms, forward_batch(repeated) {mb:.3f} ms, "
              f"ratio views/batch {mv_ / mb:.3f} (medians of {a.rounds} interleaved rounds; min {min(tv):.3f} / {min(tb):.3f})")


if __name__ == "__main__":
    main()
