"""bfloat16 grids (grid_dtype="bfloat16"): bit for bit the float32 grid of the same call, converted by torch.

Every case runs one float32 and one bfloat16 voxelizer on the same inputs and compares the bfloat16 grid's bits with
`grid32.to(torch.bfloat16)` (round to nearest, ties to even). The bfloat16 grid is pre-filled with garbage: every element
must be written. Routes (one launch / binned), kernels (matrix-core, candidate pairs, narrow, per-lane ranges, grouped
channel-wise radii, run-wise write-out) and write-out paths (vector stores, runs, unaligned grids) are all reached.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _vox(bf16, *args, **kw):
    import molvoxel_amd as mv

    if bf16:
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(*args, library="hip", **kw)


def _garbage(grid):
    import torch

    g = torch.Generator(device=grid.device).manual_seed(grid.numel() % 1000)
    grid.view(torch.int16).copy_(torch.randint(-32768, 32767, grid.shape, dtype=torch.int16, device=grid.device, generator=g))
    return grid


def assert_bits(g16, g32):
    import torch

    assert g16.dtype == torch.bfloat16 and g32.dtype == torch.float32 and g16.shape == g32.shape
    exp = g32.to(torch.bfloat16)
    same = g16.view(torch.int16) == exp.view(torch.int16)
    if not bool(same.all()):
        bad = (~same).nonzero()[:5].tolist()
        raise AssertionError(f"{int((~same).sum())} elements differ, first at {bad}: "
                             f"{[float(g16[tuple(i)]) for i in bad]} vs {[float(exp[tuple(i)]) for i in bad]}")


def _molecule(rng, D, res, N, C_, spread=1.0):
    W = res * (D - 1)
    xyz = rng.uniform(-W / 2 * spread, W / 2 * spread, (N, 3))
    feats = rng.random((N, C_)).astype(np.float32)
    types = rng.integers(0, C_, N).astype(np.int16)
    if N:
        types[0] = C_ - 1
    return xyz, feats, types


def _both(call, *args, direct=None, **kw):
    """call(vox, out_grid) with a float32 and a bfloat16 voxelizer; returns (bfloat16 grid, float32 grid)."""
    out = []
    for bf16 in (False, True):
        v = _vox(bf16, *args, **kw)
        if direct is not None:
            v.debug_option("direct", direct)
        out.append(call(v, bf16))
    return out[1], out[0]


def _check_forward(D=48, res=0.5, C_=8, N=600, mode="features", radii_type="scalar", density="gaussian", blockdim=None,
                   direct=None, seed=0, center=None):
    rng = np.random.default_rng(seed)
    xyz, feats, types = _molecule(rng, D, res, N, C_)
    radii = {"scalar": 1.5, "atom-wise": rng.uniform(0.8, 2.0, N).astype(np.float32),
             "channel-wise": rng.choice([1.0, 1.5, 2.0], C_).astype(np.float32)}[radii_type]
    extra = {} if blockdim is None else {"blockdim": blockdim}

    def call(v, bf16):
        nch = 1 if mode == "single" else C_
        grid = v.get_empty_grid(nch)
        if bf16:
            _garbage(grid)
        else:
            grid.fill_(7.0)
        r = radii if np.isscalar(radii) else v.asarray(radii, "radii")
        c = v.asarray(xyz, "coords")
        if mode == "features":
            got = v.forward_features(c, center, v.asarray(feats, "features"), r, out_grid=grid)
        elif mode == "types":
            got = v.forward_types(c, center, v.asarray(types, "types"), r, out_grid=grid)
        else:
            got = v.forward_single(c, center, r, out_grid=grid)
        assert got is grid
        return got

    g16, g32 = _both(call, res, D, radii_type, density, direct=direct, **extra)
    assert_bits(g16, g32)
    return g16, g32


def _batch(vox, wl, ids, bf16):
    coords = np.concatenate([wl.coords[i] - wl.centers[i] for i in ids])
    offsets = np.cumsum([0] + [wl.coords[i].shape[0] for i in ids]).astype(np.int64)
    radii = wl.radii[ids[0]]
    if not np.isscalar(radii):
        radii = vox.asarray(np.concatenate([wl.radii[i] for i in ids]), "radii")
    out = vox.get_empty_grid(wl.num_channels, batch_size=len(ids))
    _garbage(out) if bf16 else out.fill_(float("nan"))
    got = vox.forward_batch(vox.asarray(coords, "coords"), offsets, None,
                            vox.asarray(np.concatenate([wl.channels[i] for i in ids]), "features"), radii, out_grid=out)
    assert got is out
    return out


def _check_workload(wl, ids, direct=None):
    g16, g32 = _both(lambda v, bf16: _batch(v, wl, ids, bf16), wl.resolution, wl.dimension, wl.radii_type, wl.density,
                     sigma=wl.sigma, direct=direct)
    for b in range(len(ids)):  # (per molecule: no second full-size temporary)
        assert_bits(g16[b], g32[b])
    return g16


def test_cfg2_x256_headline():
    from molvoxel_amd import workloads as W

    g16 = _check_workload(W.cfg2(batch=256), list(range(256)))
    assert g16.shape == (256, 32, 64, 64, 64)


@pytest.mark.parametrize("direct", [None, 0])
def test_single_pocket_and_single_ligand(direct):
    from molvoxel_amd import workloads as W

    _check_workload(W.cfg2(batch=1), [0], direct=direct)
    _check_workload(W.cfg4(batch=4), [2], direct=direct)


def test_cfg5_high_resolution():
    from molvoxel_amd import workloads as W

    _check_workload(W.cfg5(batch=1), [0])


@pytest.mark.parametrize("C_", [1, 4, 5, 8, 16, 33])
@pytest.mark.parametrize("direct", [None, 0])
def test_channel_counts(C_, direct):
    _check_forward(C_=C_, direct=direct, seed=C_)


@pytest.mark.parametrize("mode", ["features", "types", "single"])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("radii_type", ["scalar", "atom-wise", "channel-wise"])
def test_modes_densities_radii(mode, density, radii_type):
    if mode == "single" and radii_type == "channel-wise":
        pytest.skip("channel-wise radii have no single mode (as in the reference)")
    for direct in (None, 0):
        _check_forward(C_=32 if radii_type == "channel-wise" else 6, mode=mode, density=density, radii_type=radii_type,
                       direct=direct, seed=11)


@pytest.mark.parametrize("blockdim", [5, 12])
@pytest.mark.parametrize("C_", [4, 32])
def test_blockdims_with_per_lane_ranges(blockdim, C_):
    for direct in (None, 0):
        _check_forward(C_=C_, blockdim=blockdim, direct=direct, seed=blockdim)


@pytest.mark.parametrize("D", [48, 49, 63, 65, 96, 120, 128])
@pytest.mark.parametrize("C_", [4, 32])
def test_dimensions(D, C_):
    N = 300 if D > 64 else 600
    _check_forward(D=D, C_=C_, N=N, direct=0, seed=D)
    if D <= 64:
        _check_forward(D=D, C_=C_, N=N, seed=D)


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("D, C_", [(64, 32), (64, 4), (48, 1), (49, 8)])
def test_grids_off_alignment(offset, D, C_):
    """A slice of a larger bfloat16 tensor, 2 or 4 bytes off alignment: written in place, run by run."""
    import torch

    rng = np.random.default_rng(D + C_)
    xyz, feats, _ = _molecule(rng, D, 0.5, 500, C_)
    for direct in (None, 0):
        grids = []
        for bf16 in (False, True):
            v = _vox(bf16, 0.5, D)
            v.debug_option("direct", direct if direct is not None else -1)
            n = C_ * D ** 3
            if bf16:
                big = _garbage(torch.empty(n + 8, dtype=torch.bfloat16, device=v.device))
                grid = big[offset:offset + n].view(C_, D, D, D)
                assert grid.is_contiguous() and grid.data_ptr() % 8 == 2 * offset
            else:
                grid = v.get_empty_grid(C_)
            got = v.forward_features(v.asarray(xyz, "coords"), None, v.asarray(feats, "features"), 1.5, out_grid=grid)
            assert got is grid
            if bf16:  # nothing outside the slice was touched
                fresh = _garbage(torch.empty_like(big)).view(torch.int16)
                assert torch.equal(big[:offset].view(torch.int16), fresh[:offset])
                assert torch.equal(big[offset + n:].view(torch.int16), fresh[offset + n:])
            grids.append(got)
        assert_bits(grids[1], grids[0])


def test_forward_batch_with_random_transforms():
    """forward_batch draws one transform per molecule from numpy's global RNG: same seed, same draws for both."""
    rng = np.random.default_rng(5)
    D, C_, B = 48, 8, 6
    sizes = [0, 40, 300, 1200, 7, 600]
    coords = np.concatenate([rng.uniform(-10, 10, (n, 3)) for n in sizes])
    feats = rng.random((coords.shape[0], C_)).astype(np.float32)
    offsets = np.cumsum([0] + sizes)
    centers = rng.uniform(-2, 2, (B, 3))

    def call(v, bf16):
        np.random.seed(123)
        out = v.get_empty_grid(C_, batch_size=B)
        _garbage(out) if bf16 else out.fill_(3.0)
        return v.forward_batch(v.asarray(coords, "coords"), offsets, centers, v.asarray(feats, "features"), 1.4,
                               out_grid=out, random_translation=1.0, random_rotation=True)

    for direct in (None, 0, 1):
        g16, g32 = _both(call, 0.5, D, direct=direct)
        assert_bits(g16, g32)


def test_rounding_midpoints_and_subnormals():
    """Binary density, atoms far apart: a voxel holds exactly one atom's feature. 1 + 2^-8 and 1 + 3 * 2^-8 lie on bfloat16
    midpoints (ties to even: down / up); float32 subnormals become bfloat16 subnormals (or zero) as torch rounds them."""
    import torch

    D, C_ = 32, 8
    g = np.arange(4) * 8.0 - 12.0
    xyz = np.array([[x, y, z] for x in g for y in g for z in g])  # 64 atoms 8 A apart, radius 1 A: the 8 at +-4 A lie in the 15.5 A box
    vals = np.array([1 + 2 ** -8, 1 + 3 * 2 ** -8, 1 + 2 ** -7 + 2 ** -9, 2 ** -149, 1e-39, 5.877472e-39, 3.4e38, -1 - 2 ** -8],
                    dtype=np.float32)
    feats = np.stack([np.roll(vals, i) for i in range(xyz.shape[0])])[:, :C_].astype(np.float32)
    for direct in (None, 0):
        def call(v, bf16):
            grid = v.get_empty_grid(C_)
            _garbage(grid) if bf16 else grid.fill_(7.0)
            return v.forward_features(v.asarray(xyz, "coords"), None, v.asarray(feats, "features"), 1.0, out_grid=grid)

        g16, g32 = _both(call, 0.5, D, "scalar", "binary", direct=direct)
        assert_bits(g16, g32)
        present = set(np.unique(g32.cpu().numpy()).tolist())
        assert float(vals[0]) in present and float(vals[4]) in present  # the midpoints and subnormals reached the grid
        assert torch.equal(g16[g32 == float(vals[0])], torch.ones_like(g16[g32 == float(vals[0])]))  # tie to even: 1.0


@pytest.mark.parametrize("seed", range(50))
def test_random_configurations(seed):
    """Configurations drawn by the parity fuzzer's case generator (tests/test_hip_fuzz.py)."""
    from tests.test_hip_fuzz import _draw

    case = _draw(seed)
    if case["N"] == 0 and case["mode"] == "types":
        pytest.skip("max(types) of an empty array")
    extra = {} if case["blockdim"] is None else {"blockdim": case["blockdim"]}
    nch = {"features": case["C"], "types": case["C"], "single": 1}[case["mode"]]

    def call(v, bf16):
        coords = v.asarray(case["xyz"], "coords")
        chan = None if case["chan"] is None else v.asarray(case["chan"], case["mode"])
        radii = case["radii"] if np.isscalar(case["radii"]) else v.asarray(case["radii"], "radii")
        center = None if case["center"] is None else v.asarray(case["center"], "center")
        grid = v.get_empty_grid(nch)
        _garbage(grid) if bf16 else grid.fill_(7.0)
        return v.forward(coords, center, chan, radii, out_grid=grid)

    for direct in (0, 1):
        g16, g32 = _both(call, case["res"], case["D"], case["radii_type"], case["density"], sigma=case["sigma"], direct=direct,
                         **extra)
        assert_bits(g16, g32)


def test_interface_keeps_the_option():
    import torch

    v = _vox(True, 0.5, 32)
    assert v.grid_dtype == torch.bfloat16 and v.get_empty_grid(3).dtype == torch.bfloat16
    assert v.get_empty_grid(3, batch_size=2).shape == (2, 3, 32, 32, 32)
    assert v.to(v.device).grid_dtype == torch.bfloat16
    assert _vox(False, 0.5, 32).grid_dtype == torch.float32
    # a float32 out_grid, or a numpy one, takes the copy path: the values are the bfloat16 grid's
    xyz = np.random.default_rng(1).uniform(-6, 6, (50, 3))
    ref = v.forward_single(v.asarray(xyz, "coords"), None, 1.5)
    f32 = torch.empty(1, 32, 32, 32, device=v.device)
    assert v.forward_single(v.asarray(xyz, "coords"), None, 1.5, out_grid=f32) is f32
    assert torch.equal(f32, ref.float())
    host = np.zeros((1, 32, 32, 32), np.float32)
    v.forward_single(xyz, None, 1.5, out_grid=host)
    assert np.array_equal(host, ref.float().cpu().numpy())


def test_bf16_kernel_resources():
    """Registers, spills and scratch of every bfloat16 twin against its float32 kernel (tools/regs.py):
    * VGPRs: at most 64 for the slab kernels (their launch bounds); the one-launch pair kernels, whose float32 forms already
      use 91-128 under launch_bounds(1024), at most as many as their float32 twin;
    * no scratch wherever the float32 twin has none;
    * twins without the run-wise write-out (aligned-grid slab kernels, narrow kernels): exactly the float32 spills and scratch;
    * twins that carry the bfloat16 store_runs (run-wise, per-lane-range and pair kernels) spill more scalar registers
      (16-17 in the slab kernels, up to 34 in the pair kernels; to VGPR lanes, no scratch) and voxelize_kernel<32, false, true, 1024, false, __bf16> 13 more
      VGPRs (8 -> 56 B of scratch): pinned at the measured bound (rates: profiles/r05_bf16.txt)."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import regs

    res = regs.kernel_resources()
    # bfloat16 kernel -> its float32 twin: the same instantiation with the grid type float
    twins = {k: k[: -len("__bf16>")] + "float>" for k in res if k.startswith("voxelize_") and k.endswith(", __bf16>")}
    assert len(twins) >= 100, len(twins)
    for k, twin in twins.items():
        r, t = res[k], res[twin]
        pair = twin.startswith("voxelize_pair_kernel<")
        assert r["vgpr"] <= (t["vgpr"] if pair else 64), (twin, r, t)
        if t["scratch"] == 0:
            assert r["scratch"] == 0, (twin, r, t)
        runs = pair or twin.startswith(("voxelize_runs_kernel<", "voxelize_pair_runs_kernel<")) or \
            (twin.startswith("voxelize_kernel<") and twin.split(", ")[2] == "true")
        if not runs:
            assert (r["vspill"], r["sspill"], r["scratch"]) == (t["vspill"], t["sspill"], t["scratch"]), (twin, r, t)
        else:
            assert r["vspill"] <= t["vspill"] + 13 and r["sspill"] <= t["sspill"] + 40 and r["scratch"] <= t["scratch"] + 48, (twin, r, t)

