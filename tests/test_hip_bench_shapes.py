"""Parity at the exact launch shapes that are benchmarked (bench.py, bench_configs.py).

The headline number is one forward_batch of 256 cfg-2 molecules on device tensors (gridDim.y = 256, 1.02 M atoms);
the ligand row is cfg-4 x 128 (ragged 40-60 atoms), the stress row cfg-5 x 4. Here those very calls are checked:
first / middle / last molecule of each batch against the CPU oracle (membership identical + the north-star bar as written:
|out - ref| <= 1e-5 absolute on the full array),
molecule 0 against the reference's golden samples, and every other molecule by property: its slice of the batch grid
equals the same molecule's single-call grid bit for bit (what the reference's own harness asserts,
test/test_time_numpy.py:65-69, restated for batches).
"""
import numpy as np
import pytest

from tests import goldens
from tests.tolerance import NORTH_STAR_ABS, assert_north_star

pytestmark = pytest.mark.gpu

Z_BIG, IDX_BIG = goldens.load("big_cases.npz")


def _oracle(wl, i):
    from oracle import c_oracle

    return c_oracle.voxelize(wl.coords[i] - wl.centers[i].reshape(1, 3), wl.channels[i], wl.radii[i],
                             resolution=wl.resolution, dimension=wl.dimension, radii_type=wl.radii_type,
                             density=wl.density, sigma=wl.sigma, num_channels=wl.num_channels)


def _batch_call(vox, wl, ids):
    coords = np.concatenate([wl.coords[i] - wl.centers[i] for i in ids])
    offsets = np.cumsum([0] + [wl.coords[i].shape[0] for i in ids]).astype(np.int64)
    d_coords = vox.asarray(coords, "coords")
    d_chan = vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features")
    radii = wl.radii[ids[0]]
    if not np.isscalar(radii):
        radii = vox.asarray(np.concatenate([wl.radii[i] for i in ids]), "radii")
    out = vox.get_empty_grid(wl.num_channels, batch_size=len(ids))
    out.fill_(float("nan"))  # every voxel must be overwritten
    got = vox.forward_batch(d_coords, offsets, None, d_chan, radii, out_grid=out)
    assert got is out
    return out, d_coords, d_chan, radii, offsets


def _check_batch(mv, wl, ids, oracle_ids, single_ids):
    import torch

    vox = mv.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, wl.density, library="hip", sigma=wl.sigma)
    out, d_coords, d_chan, radii, offsets = _batch_call(vox, wl, ids)
    assert not torch.isnan(out).any()
    worst = 0.0
    for b in oracle_ids:
        worst = max(worst, assert_north_star(out[b].cpu().numpy(), _oracle(wl, ids[b])))
    print(f"{wl.name} x {len(ids)}: max |out - oracle| = {worst:.3g} (bar {NORTH_STAR_ABS:g})")
    one = vox.get_empty_grid(wl.num_channels)
    for b in single_ids:
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        r = radii if np.isscalar(radii) else radii[lo:hi]
        vox.forward_features(d_coords[lo:hi], None, d_chan[lo:hi], r, out_grid=one)
        assert torch.equal(out[b], one), f"batch slice {b} differs from the single call"
    return out


def test_cfg2_x256_the_headline_launch():
    """bench.py's step: 256 cfg-2 molecules (seeds 0, 1000, ...), device tensors, one forward_batch."""
    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W

    wl = W.cfg2(batch=256)
    out = _check_batch(mv, wl, list(range(256)), oracle_ids=(0, 128, 255), single_ids=range(0, 256, 5))
    # molecule 0 is the BASELINE seed-0 molecule: the reference's own samples
    case = next(c for c in IDX_BIG if c["id"] == "cfg2_features_gaussian")
    flat = out[0].reshape(-1).cpu().numpy()
    idx, val = Z_BIG[f"{case['id']}/sample_idx"], Z_BIG[f"{case['id']}/sample_val"]
    assert np.abs(flat[idx] - val).max() <= NORTH_STAR_ABS  # the reference's own values
    assert int(np.count_nonzero(flat)) == case["nonzero"]


def test_cfg4_x128_ragged_ligands():
    """cfg-4's per-GPU share: 128 ligands of 40-60 atoms, C = 16, one forward_batch."""
    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W

    wl = W.cfg4(batch=128)
    out = _check_batch(mv, wl, list(range(128)), oracle_ids=(0, 64, 127), single_ids=range(128))
    for k in range(8):  # the reference's goldens for the first 8 ligands (same seed-4 stream)
        case = next(c for c in IDX_BIG if c["id"] == f"cfg4_features_gaussian_m{k}")
        flat = out[k].reshape(-1).cpu().numpy()
        idx, val = Z_BIG[f"{case['id']}/sample_idx"], Z_BIG[f"{case['id']}/sample_val"]
        assert np.abs(flat[idx] - val).max() <= NORTH_STAR_ABS
        assert int(np.count_nonzero(flat)) == case["nonzero"]


def test_cfg5_x4_high_resolution():
    """cfg-5 x 4: 128^3, sigma 1.0, atom-wise radii, N = 10 000, C = 32 (1.07 GB of grids)."""
    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W

    wl = W.cfg5(batch=4)
    out = _check_batch(mv, wl, [0, 1, 2, 3], oracle_ids=(0, 3), single_ids=(0, 1, 2, 3))
    case = next(c for c in IDX_BIG if c["id"] == "cfg5_features_gaussian")
    flat = out[0].reshape(-1).cpu().numpy()
    idx, val = Z_BIG[f"{case['id']}/sample_idx"], Z_BIG[f"{case['id']}/sample_val"]
    assert np.abs(flat[idx] - val).max() <= NORTH_STAR_ABS  # the reference's own values
    assert int(np.count_nonzero(flat)) == case["nonzero"]


def test_bench_spot_check_helper():
    """The post-timing spot check bench.py runs (outside the timed region) passes on a correct grid and fails on a
    corrupted one."""
    import molvoxel_amd as mv
    import bench
    from molvoxel_amd import workloads as W

    wl = W.cfg2(batch=3)
    vox = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", library="hip")
    out, *_ = _batch_call(vox, wl, [0, 1, 2])
    coords = [wl.coords[i] for i in range(3)]
    feats = [wl.channels[i] for i in range(3)]
    verdict, worst = bench.parity_spot(out, coords, feats, picks=(0, 2))
    assert verdict == "ok" and 0 < worst <= 5e-6
    out[2, 5, 10, 10, 10] += 1.0
    assert bench.parity_spot(out, coords, feats, picks=(0, 2))[0].startswith("FAIL")


def test_plain_bench_run_and_its_dumped_outputs(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` without --full: the headline fields only, `ms_per_step` over the
    K timed steps, and the dumped grids are what the timed path computed (molecule 0 against the CPU oracle)."""
    import json
    import os
    import subprocess
    import sys

    import bench

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(bench.ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "8",
                          "--prewarm", "5", "--dump-outputs", str(tmp_path)], cwd=bench.ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "molecules/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 8 * 1e3 / rec["ms_per_step"]) <= 1e-9 * rec["value"]
    assert not {"roofline", "parity_spot", "cpu_baseline"} & set(rec)
    names = sorted(os.listdir(tmp_path))
    assert names == ["channel_sums.npy", "grid_first.npy", "grid_sample.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in names) <= 64 * 2**20
    first = np.load(tmp_path / "grid_first.npy")
    _, coords, feats = bench.make_batch(1, 0)
    from oracle import c_oracle

    assert_north_star(first, c_oracle.voxelize(coords[0], feats[0], 1.0, dimension=64))
    sums = np.load(tmp_path / "channel_sums.npy")
    assert sums.dtype == np.float64 and sums.shape == (8, 32)
    assert np.allclose(sums[0], first.astype(np.float64).sum(axis=(1, 2, 3)), rtol=1e-9)
    sample = np.load(tmp_path / "grid_sample.npy")
    idx = np.sort(np.random.default_rng(0).integers(0, 8 * 32 * 64**3, size=bench.DUMP_SAMPLE))
    in_first = idx < first.size
    assert sample.dtype == np.float32 and np.array_equal(sample[in_first], first.reshape(-1)[idx[in_first]])


def test_pacing_guard_rows_are_recorded(record_property):
    """The store pacing of the slab kernels is tuned to launch shapes (mvx_tuning.h): this test records - it does not
    assert a rate, boxes of the pool differ by +-2 % and short runs sit on the clock ramp - the kernel's fraction of the
    HBM peak at cfg-2 x 16 / 64 / 96 / 256 and cfg-4 x 128, so that a drifted threshold is visible in the test report
    (`bench_configs.py --pacing` is the same table with settled clocks). Only gross cliffs fail it."""
    import bench_configs

    rows = bench_configs.pacing_rows(steps=10, warmup=30)
    for r in rows:
        record_property(r["config"], round(r["of_peak"], 3))
        print(f'{r["config"]}: kernel {r["kernel_ms"]:.3f} ms = {r["of_peak"]:.3f} of peak')
    by = {r["config"]: r["of_peak"] for r in rows}
    assert by["pacing guard: cfg2 x256"] > 0.6 and by["pacing guard: cfg2 x64"] > 0.55 and by["pacing guard: cfg4 ligands x128"] > 0.6


def test_per_molecule_call_kernel_times_are_recorded(record_property):
    """One molecule per forward() call (the reference's unit of work): records the launch's duration by HIP events for cfg-2 and
    cfg-3 - voxelize_pair_kernel, 14 us and 7 us when this was written (20 us / 10 us with the kernel it replaced) - so that a
    regression of the per-molecule path shows in the test report. Only a gross cliff fails it."""
    import bench_configs
    from molvoxel_amd import workloads as W

    rows = [bench_configs.run("cfg2 single call", W.cfg2(), [0], steps=60, warmup=30),
            bench_configs.run("cfg3 single call", W.cfg3(), [0], steps=60, warmup=30)]
    for r in rows:
        record_property(r["config"], round(1e3 * r["kernel_ms"], 1))
        print(f'{r["config"]}: kernel {1e3 * r["kernel_ms"]:.1f} us, call {1e3 * r["ms_per_call"]:.1f} us')
    assert rows[0]["kernel_ms"] < 0.030 and rows[1]["kernel_ms"] < 0.020
