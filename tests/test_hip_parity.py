"""Parity of the HIP path (through the Python operator API and the C ABI) with the reference.

Compared against (a) the committed goldens produced by the imported reference numpy backend and
(b) the CPU oracle on the same seeded inputs.
Bar (BASELINE.json north_star): binary bit-exact; Gaussian <= 1e-5 abs. The tests use a tighter
5e-6 for Gaussian; membership (which voxels are non-zero) must be identical in every case.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import goldens
from tests.tolerance import GAUSS_TOL, NORTH_STAR_ABS, P64_TOL, assert_exact, assert_gaussian, assert_north_star

pytestmark = pytest.mark.gpu

Z_SMALL, IDX_SMALL = goldens.load("small_cases.npz")
Z_BIG, IDX_BIG = goldens.load("big_cases.npz")
Z_API, IDX_API = goldens.load("api_cases.npz")
Z_P64, IDX_P64 = goldens.load("p64_cases.npz")
Z_DENSE, IDX_DENSE = goldens.load("dense_cases.npz")


@pytest.fixture(scope="module")
def mv():
    import molvoxel_amd

    return molvoxel_amd


def _make(mv, case_or_kw, **over):
    kw = dict(case_or_kw)
    kw.update(over)
    extra = {}
    if kw.get("blockdim") is not None:
        extra["blockdim"] = kw["blockdim"]
    if kw["density"] == "gaussian":
        extra["sigma"] = kw["sigma"]
    return mv.create_voxelizer(kw["resolution"], kw["dimension"], kw["radii_type"], kw["density"], "hip",
                               output="numpy", **extra)


def _compare(out, ref, exact):
    assert out.shape == ref.shape and out.dtype == np.float32
    if exact:
        assert_exact(out, ref)
    else:
        assert_gaussian(out, ref)  # tests/tolerance.py: membership identical, |d| <= 5e-6 * max(1, |ref|) per voxel


@pytest.mark.parametrize("route", ["binned", "direct"])
@pytest.mark.parametrize("case", IDX_SMALL, ids=[c["id"] for c in IDX_SMALL])
def test_small_golden(mv, case, route):
    """Every small golden through both routes of the library: the binned three-launch pipeline and the
    single-launch direct kernel (what per-molecule calls take by default)."""
    coords, chan, radii = goldens.small_case_inputs(Z_SMALL, case)
    ref = Z_SMALL[f"{case['id']}/out"]
    v = _make(mv, case)
    v.debug_option("direct", 1 if route == "direct" else 0)
    out = v.forward(coords, None, chan, radii)
    _compare(out, ref, exact=(case["density"] == "binary" and case["mode"] != "features"))
    if case["density"] == "binary" and case["mode"] == "features":
        # binary features: sums of the same float32 feature values; only the summation order may differ
        assert np.abs(out - ref).max() <= 1e-6


def _workload(case):
    from molvoxel_amd import workloads as W

    name = case["workload"]
    if name == "cfg1":
        pc = np.load(goldens.GOLD + "/pointcloud_10gs.npz")
        return W.cfg1(pc["ligand_xyz"], pc["ligand_feat5"])
    if name == "cfg4":
        return W.cfg4(batch=8)
    return getattr(W, name)()


@pytest.mark.parametrize("case", IDX_BIG, ids=[c["id"] for c in IDX_BIG])
def test_baseline_configs_golden_and_oracle(mv, case, record_property):
    """BASELINE.json configs at full size: golden sha/samples from the reference + full-array oracle compare.
    Gaussian configs are held to the north-star bar as written: |out - ref| <= 1e-5 ABSOLUTE on the full array
    (numpy/voxelizer.py:557-560 is the chain being matched), max |d| recorded as a test property."""
    from oracle import c_oracle

    wl = _workload(case)
    i = case["molecule"]
    _, mode, density = case["id"].split("_")[:3]
    chan = None if mode == "single" else wl.channels[i]
    v = mv.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, density, "hip", output="numpy",
                            **({"sigma": wl.sigma} if density == "gaussian" else {}))
    out = v.forward(wl.coords[i], wl.centers[i], chan, wl.radii[i])
    assert list(out.shape) == case["shape"]
    assert int(np.count_nonzero(out)) == case["nonzero"]
    if case["exact"]:
        assert hashlib.sha256(out.tobytes()).hexdigest() == case["sha256"]
    idx, val = Z_BIG[f"{case['id']}/sample_idx"], Z_BIG[f"{case['id']}/sample_val"]
    assert np.abs(out.reshape(-1)[idx] - val).max() <= (0 if case["exact"] else GAUSS_TOL)  # the reference's own values
    sums = out.reshape(out.shape[0], -1).sum(axis=1, dtype=np.float64)
    assert np.allclose(sums, Z_BIG[f"{case['id']}/chan_sums"], rtol=2e-6, atol=1e-3)
    # full-array comparison with the CPU oracle (itself pinned to the reference by test_oracle_golden.py)
    xyz = wl.coords[i] - wl.centers[i].reshape(1, 3)
    ora = c_oracle.voxelize(xyz, chan, wl.radii[i], resolution=wl.resolution, dimension=wl.dimension,
                            radii_type=wl.radii_type, density=density, sigma=wl.sigma, num_channels=out.shape[0])
    if case["exact"]:
        assert_exact(out, ora)
    else:
        worst = assert_north_star(out, ora)
        record_property("max_abs_err", worst)
        print(f"{case['id']}: max |out - oracle| = {worst:.3g} (bar {NORTH_STAR_ABS:g}), max value {float(ora.max()):.3g}")


@pytest.mark.parametrize("case", IDX_DENSE, ids=[c["id"] for c in IDX_DENSE])
def test_dense_golden_against_the_reference(mv, case, record_property):
    """Dense clusters voxelized by the reference itself (sums up to ~200, BLAS summation order): the HIP path against
    those arrays under the one tolerance rule; the measured error is reported as a test property."""
    from tests.tolerance import gaussian_excess

    cid = case["id"]
    xyz, ref = Z_DENSE[f"{cid}/coords"], Z_DENSE[f"{cid}/out"]
    chan = Z_DENSE[f"{cid}/chan"] if f"{cid}/chan" in Z_DENSE.files else None
    rad = case["scalar_radius"] if case["scalar_radius"] is not None else Z_DENSE[f"{cid}/radii"]
    v = mv.create_voxelizer(0.5, case["dimension"], case["radii_type"], case["density"], "hip", output="numpy",
                            **({"sigma": case["sigma"]} if case["density"] == "gaussian" else {}))
    out = v.forward(xyz, None, chan, rad)
    if case["density"] == "binary":
        assert_exact(out, ref)
        return
    assert_gaussian(out, ref)
    d = np.abs(out - ref)
    record_property("max_abs_err", float(d.max()))
    record_property("max_rel_err", float((d / np.maximum(1.0, np.abs(ref))).max()))
    print(f"{cid}: max abs {d.max():.3g}, max |d|/max(1,|ref|) {(d / np.maximum(1.0, np.abs(ref))).max():.3g}, "
          f"rule excess {gaussian_excess(out, ref):.3f}")


def test_api_cases(mv):
    """End-to-end calls recorded through the reference's public API (centring, seeded random transform,
    out_grid reuse with an extra channel, radii_type / density_type switches)."""
    z = Z_API
    xyz, types, center = z["sys_xyz"], z["sys_types"], z["center"]
    pc = np.load(goldens.GOLD + "/pointcloud_10gs.npz")
    lig, lig_f = pc["ligand_xyz"], pc["ligand_feat5"]

    v = mv.create_voxelizer(0.5, 32, library="hip", output="numpy")
    g = v.get_empty_grid(10)
    out = v.forward(xyz, center, types, 1.0, out_grid=g)
    assert out is g  # in-place contract (reference test/test_run_numpy.py:46)
    _compare(out, z["a0/out"], False)

    np.random.seed(123)
    out = v.forward(xyz, center, types, 1.0, random_translation=0.5, random_rotation=True)
    _compare(out, z["a1/out"], False)

    v.radii_type = "channel-wise"
    _compare(v.forward(xyz, center, types, z["a2/r_chan"]), z["a2/out"], False)
    v.radii_type = "atom-wise"
    _compare(v.forward(xyz, center, types, z["a2/r_chan"][types]), z["a3/out"], False)
    v.radii_type = "scalar"
    v.density_type = "binary"
    _compare(v.forward(xyz, center, types, 1.5), z["a4/out"], True)

    v2 = mv.create_voxelizer(0.5, 32, library="hip", output="numpy")
    _compare(v2.forward(lig, center, lig_f, 1.0), z["a5/out"], False)
    _compare(v2.forward(lig, center, None, 1.0), z["a6/out"], False)
    _compare(v2.forward(lig.astype(np.float32), None, lig_f, 1.0), z["a7/out"], False)


def test_determinism_and_types_equals_onehot_features(mv):
    """The reference's own assertions (test/test_time_numpy.py:65-69): repeated calls agree, and
    forward_types equals forward_features on one-hot features, to 1e-5."""
    from molvoxel_amd import workloads as W

    wl = W.cfg3()
    v = mv.create_voxelizer(0.5, 48, "scalar", "gaussian", "hip", output="numpy")
    t = wl.channels[0]
    a = v.forward(wl.coords[0], wl.centers[0], t, 1.0)
    b = v.forward(wl.coords[0], wl.centers[0], t, 1.0)
    assert np.array_equal(a, b)
    onehot = np.eye(4, dtype=np.float32)[t]
    c = v.forward(wl.coords[0], wl.centers[0], onehot, 1.0)
    assert np.abs(a - c).max() < 1e-5


def test_c_abi_direct_host_pointers(mv):
    """Call the C ABI directly (no Python operator layer): mvx_create / mvx_forward_types / mvx_destroy."""
    from molvoxel_amd import workloads as W
    from molvoxel_amd.voxelizer.hip import _lib
    from oracle import c_oracle

    lib = _lib.load()
    wl = W.cfg3()
    cfg = _lib.MvxConfig(0.5, 0.5, 48, 8, _lib.MVX_BINARY, 0, 32, 0)
    h = _lib.Handle()
    _lib.check(lib.mvx_create(C.byref(cfg), C.byref(h)))
    xyz = np.ascontiguousarray(wl.coords[0])
    types = np.ascontiguousarray(wl.channels[0], dtype=np.int32)
    out = np.full((4, 48, 48, 48), np.nan, dtype=np.float32)
    _lib.check(lib.mvx_forward_types(h, xyz.ctypes.data, types.ctypes.data, None, 1.0, _lib.MVX_RADII_SCALAR,
                                     xyz.shape[0], 4, None, out.ctypes.data, _lib.MVX_HOST, _lib.MVX_HOST, None))
    ref = c_oracle.voxelize(xyz, types, 1.0, dimension=48, density="binary", num_channels=4)
    assert np.array_equal(out, ref)
    # error path: channel-wise radii are rejected for forward_single with the reference's message
    rc = lib.mvx_forward_single(h, xyz.ctypes.data, xyz.ctypes.data, 1.0, _lib.MVX_RADII_CHANNEL, xyz.shape[0], None,
                                out.ctypes.data, _lib.MVX_HOST, _lib.MVX_HOST, None)
    assert rc == -1 and b"Channel-Wise" in lib.mvx_last_error()
    _lib.check(lib.mvx_destroy(h))


def test_batch_matches_per_molecule_and_ragged_empty(mv):
    """forward_batch (one launch) == per-molecule calls; ragged sizes incl. an empty molecule."""
    from molvoxel_amd import workloads as W

    wl = W.cfg4(batch=6)
    coords = [c for c in wl.coords]
    feats = [f for f in wl.channels]
    coords[2] = coords[2][:0]  # empty molecule
    feats[2] = feats[2][:0]
    offsets = np.cumsum([0] + [c.shape[0] for c in coords])
    v = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip", output="numpy")
    out = v.forward_batch(np.concatenate(coords), offsets, None, np.concatenate(feats), 1.0)
    assert out.shape == (6, 16, 64, 64, 64)
    for b in range(6):
        one = v.forward(coords[b], None, feats[b], 1.0) if coords[b].shape[0] else np.zeros_like(out[b])
        assert np.array_equal(out[b], one)
    assert not out[2].any()


def test_torch_device_tensors_zero_copy(mv):
    """torch CUDA tensors in and out (data_ptr hand-off on the current stream); same bits as the host path."""
    import torch

    from molvoxel_amd import workloads as W

    wl = W.cfg2(n_atoms=500, channels=32)
    vt = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip")
    vn = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip", output="numpy")
    coords = vt.asarray(wl.coords[0], "coords")
    feats = vt.asarray(wl.channels[0], "features")
    center = vt.asarray(wl.centers[0], "center")
    assert coords.is_cuda and coords.dtype == torch.float64 and feats.dtype == torch.float32
    grid = vt.get_empty_grid(32)
    out = vt.forward(coords, center, feats, 1.0, out_grid=grid)
    assert out is grid and out.is_cuda
    host = vn.forward(wl.coords[0], wl.centers[0], wl.channels[0], 1.0)
    assert np.array_equal(out.cpu().numpy(), host)


def test_size_independent_properties_full_size(mv):
    """cfg-2 size: linearity in the features, channel permutation, and Gaussian <= binary support."""
    from molvoxel_amd import workloads as W

    wl = W.cfg2()
    xyz, f = wl.coords[0], wl.channels[0]
    v = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip", output="numpy")
    a = v.forward(xyz, None, f, 1.0)
    # scaling by a power of two is exact in float32
    assert np.array_equal(v.forward(xyz, None, f * np.float32(2.0), 1.0), a * np.float32(2.0))
    perm = np.random.default_rng(0).permutation(32)
    assert np.array_equal(v.forward(xyz, None, f[:, perm], 1.0), a[perm])
    # each channel is independent of the others: C=32 result restricted to 4 channels == C=4 result
    assert np.array_equal(v.forward(xyz, None, np.ascontiguousarray(f[:, :4]), 1.0), a[:4])
    v.density_type = "binary"
    s_bin = v.forward(xyz, None, None, 1.0)
    v.density_type = "gaussian"
    s_gau = v.forward(xyz, None, None, 1.0)
    assert np.array_equal(s_bin != 0, s_gau != 0)
    assert s_bin.sum() == float(np.count_nonzero(s_bin)) or s_bin.max() > 1  # integer counts
    assert np.array_equal(s_bin, np.round(s_bin))


def test_blockdim_modes(mv):
    """blockdim emulation: default 8 reproduces the reference's block-cull artefact, blockdim=dimension removes it."""
    from oracle import c_oracle

    rng = np.random.default_rng(9)
    D = 32
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2, W_ / 2, (500, 3))
    for bd in (8, 32, 16, 5, 12):
        v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy", blockdim=bd)
        out = v.forward(xyz, None, None, 1.0)
        ref = c_oracle.voxelize(xyz, None, 1.0, dimension=D, blockdim=bd, density="binary")
        assert np.array_equal(out, ref), f"blockdim={bd}"
    one = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy", blockdim=D).forward(xyz, None, None, 1.0)
    eight = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy").forward(xyz, None, None, 1.0)
    assert (one != eight).sum() > 0  # ~0.5 % of voxels differ


def test_many_channels_and_odd_dimension(mv):
    """C > 32 (several channel chunks) and a dimension that is not a multiple of 4 (scalar-store path)."""
    from oracle import c_oracle

    rng = np.random.default_rng(3)
    for D, C_ in ((30, 70), (17, 3), (64, 40)):
        W_ = 0.5 * (D - 1)
        xyz = rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (300, 3))
        f = rng.random((300, C_)).astype(np.float32)
        v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", output="numpy")
        out = v.forward(xyz, None, f, 1.25)
        ref = c_oracle.voxelize(xyz, f, 1.25, dimension=D)
        _compare(out, ref, False)


def test_dense_cluster_exceeds_candidate_capacity(mv):
    """Thousands of atoms inside one slab: exercises the multi-round scan and chunked LDS staging."""
    from oracle import c_oracle

    rng = np.random.default_rng(4)
    xyz = rng.normal(scale=0.8, size=(3000, 3))
    t = rng.integers(0, 3, 3000)
    v = mv.create_voxelizer(0.5, 24, "scalar", "binary", "hip", output="numpy")
    ref = c_oracle.voxelize(xyz, t, 1.0, dimension=24, density="binary", num_channels=3)
    for route in (0, 1):  # binned: slabs beyond 255 candidates walk their x-list; direct: many rounds per slab
        v.debug_option("direct", route)
        assert np.array_equal(v.forward(xyz, None, t, 1.0), ref)
    f = rng.random((3000, 32)).astype(np.float32)
    vg = mv.create_voxelizer(0.5, 24, "scalar", "gaussian", "hip", output="numpy")
    vg.debug_option("direct", 1)
    outd = vg.forward(xyz, None, f, 1.0).copy()
    vg.debug_option("direct", 0)
    outg = vg.forward(xyz, None, f, 1.0)
    assert np.array_equal(outd, outg)
    refg = c_oracle.voxelize(xyz, f, 1.0, dimension=24)
    assert_gaussian(outg, refg)  # sums of ~1000 terms: the relative branch of the rule


def test_medium_density_multi_round_slab_lines(mv):
    """64 < candidates per slab <= 255: the slab line is consumed in several rounds of 64 entries."""
    from oracle import c_oracle

    rng = np.random.default_rng(11)
    D = 32
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2, W_ / 2, (2000, 3))
    t = rng.integers(0, 5, 2000)
    v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy")
    v.debug_option("direct", 0)
    out = v.forward(xyz, None, t, 1.5)
    assert np.array_equal(out, c_oracle.voxelize(xyz, t, 1.5, dimension=D, density="binary", num_channels=5))
    f = rng.random((2000, 32)).astype(np.float32)
    vg = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", output="numpy")
    vg.debug_option("direct", 0)
    outg = vg.forward(xyz, None, f, 1.5)
    refg = c_oracle.voxelize(xyz, f, 1.5, dimension=D)
    assert_gaussian(outg, refg)  # sums of up to ~60 terms


@pytest.mark.parametrize("D,C_,mode", [(72, 4, "types"), (88, 1, "single"), (88, 4, "types"), (100, 3, "features"), (104, 4, "features"),
                                       (112, 1, "single"), (120, 4, "types"), (120, 2, "features"), (40, 1, "single"), (56, 1, "single")])
def test_long_rows_in_chunks_for_one_and_four_channel_launches(mv, D, C_, mode):
    """plan_slabs: launches of one or four channels per workgroup cut rows of 9 ... 15 sub-tiles into chunks of eight (four at
    D = 72) so that the multi-sub-tile kernel applies - pieces that share 64-byte blocks with their neighbours; forward_single
    cuts rows of five / seven sub-tiles (D = 40, 56) into chunks of four. Against the oracle, Gaussian and binary."""
    from oracle import c_oracle

    rng = np.random.default_rng(7000 + 10 * D + C_)
    n = int(4000 * (D / 64.0) ** 3)
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2, W_ / 2, (n, 3))
    for density in ("gaussian", "binary"):
        v = mv.create_voxelizer(0.5, D, "scalar", density, "hip", output="numpy", sigma=0.6)
        if mode == "single":
            out = v.forward_single(xyz, None, 1.0)
            ref = c_oracle.voxelize(xyz, None, 1.0, dimension=D, density=density, sigma=0.6)
        elif mode == "types":
            t = rng.integers(0, C_, n)
            t[0] = C_ - 1
            out = v.forward_types(xyz, None, t, 1.0)
            ref = c_oracle.voxelize(xyz, t, 1.0, dimension=D, density=density, sigma=0.6, num_channels=C_)
        else:
            f = rng.random((n, C_)).astype(np.float32)
            out = v.forward_features(xyz, None, f, 1.0)
            ref = c_oracle.voxelize(xyz, f, 1.0, dimension=D, density=density, sigma=0.6)
        _compare(out, ref, density == "binary" and mode != "features")


@pytest.mark.parametrize("C_,mode", [(1, "single"), (4, "types"), (8, "features"), (16, "features"), (40, "features")])
def test_rows_of_twelve_sub_tiles_in_chunks_of_four(mv, C_, mode):
    """D = 96: narrow launches cut the row into three chunks of four sub-tiles (plan_slabs), 32-channel chunks into 8 + 4;
    C = 40 keeps the 8 + 4 plan for its 32-channel launch and its 8-channel remainder launch alike. Against the oracle."""
    from oracle import c_oracle

    rng = np.random.default_rng(960 + C_)
    D, n = 96, 5000
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2, W_ / 2, (n, 3))
    for density in ("gaussian", "binary"):
        v = mv.create_voxelizer(0.5, D, "scalar", density, "hip", output="numpy", sigma=0.6)
        if mode == "single":
            out = v.forward_single(xyz, None, 1.25)
            ref = c_oracle.voxelize(xyz, None, 1.25, dimension=D, density=density, sigma=0.6)
        elif mode == "types":
            t = rng.integers(0, C_, n)
            out = v.forward_types(xyz, None, t, 1.25)
            ref = c_oracle.voxelize(xyz, t, 1.25, dimension=D, density=density, sigma=0.6, num_channels=C_)
        else:
            f = rng.random((n, C_)).astype(np.float32)
            out = v.forward_features(xyz, None, f, 1.25)
            ref = c_oracle.voxelize(xyz, f, 1.25, dimension=D, density=density, sigma=0.6)
        _compare(out, ref, density == "binary" and mode != "features")  # (binary features: sums of float32 products, the Gaussian rule)


@pytest.mark.parametrize("variant", ["plain", "lane_range", "channel_wise", "runs", "six_waves", "nine_waves"])
def test_candidate_counts_around_the_rounds_staged_together(mv, variant):
    """The 32-channel kernels stage the first TWO rounds of a slab's line at once (stage_first_rounds: rows 0 .. 2 RW - 1 of
    the row region) and walk the second round without a barrier; a third round goes through the row region again. A cluster
    of exactly k atoms inside one sub-tile makes k the candidate count of that slab: every count around RW and 2 RW (RW = 64
    rows, 48 on the six-wave slabs of a 48^3 grid), in every kernel family that shares the staging - plain, per-lane ranges
    (blockdim 5), grouped channel-wise radii, the run-wise write-out (D = 50), slabs of six and of nine waves. Binned route
    against the oracle and, bit for bit, against the one-launch route."""
    from oracle import c_oracle

    D = {"runs": 50, "six_waves": 48, "nine_waves": 72}.get(variant, 64)
    RW = 48 if variant == "six_waves" else 64
    kw = {"blockdim": 5} if variant == "lane_range" else {}
    rt = "channel-wise" if variant == "channel_wise" else "scalar"
    rng = np.random.default_rng(sum(map(ord, variant)))
    vox = mv.create_voxelizer(0.5, D, rt, "gaussian", "hip", output="numpy", sigma=0.8, **kw)
    for k in (RW - 2, RW - 1, RW, RW + 1, RW + 9, 2 * RW - 1, 2 * RW, 2 * RW + 1, 2 * RW + 17, 3 * RW + 5):
        c0 = rng.uniform(-3.0, 3.0, 3)
        xyz = np.concatenate([c0 + rng.uniform(-0.2, 0.2, (k, 3)), rng.uniform(-0.25 * D, 0.25 * D, (40, 3))])
        f = rng.random((len(xyz), 32)).astype(np.float32)
        radii = np.linspace(0.8, 1.4, 32)[rng.permutation(32)] if rt == "channel-wise" else 1.0
        radii = np.round(radii * 4) / 4 if rt == "channel-wise" else radii  # a few distinct radii: grouped slots
        ref = c_oracle.voxelize(xyz, f, radii, dimension=D, density="gaussian", sigma=0.8, radii_type=rt, blockdim=kw.get("blockdim"))
        vox.debug_option("direct", 0)
        out = vox.forward(xyz, None, f, radii).copy()
        assert_gaussian(out, ref)
        if rt != "channel-wise":  # (channel-wise features never take the one-launch route)
            vox.debug_option("direct", 1)
            assert np.array_equal(vox.forward(xyz, None, f, radii), out), f"routes disagree at {k} candidates"


@pytest.mark.parametrize("D,C_,blockdim", [(70, 16, None), (120, 16, None), (70, 32, 5), (120, 32, 5), (72, 32, None), (100, 8, None)])
def test_whole_row_slabs_of_long_rows_with_more_than_64_candidates(mv, D, C_, blockdim):
    """Rows of 65 ... 128 voxels stay in one slab of 9 ... 16 waves (plan_slabs). A round still holds 64 rows: the staging
    step's slot wave + u * NW runs past 63 for the larger u there and must skip those slots (a guard the 8-wave kernels do
    not need) - slabs with 64 ... 255 candidates (radius 2.0 A on the 0.5 A grid) take several rounds over line and
    extension. Batched (binned route), Gaussian and binary, against the oracle."""
    from oracle import c_oracle

    rng = np.random.default_rng(D * 100 + C_)
    W_ = 0.5 * (D - 1)
    n = int(9000 * (D / 70.0) ** 3)  # ~150 candidates per slab at a 2.0 A radius
    xyz = rng.uniform(-W_ / 2, W_ / 2, (n, 3))
    f = rng.random((n, C_)).astype(np.float32)
    extra = {"blockdim": blockdim} if blockdim else {}
    for density in ("gaussian", "binary"):
        v = mv.create_voxelizer(0.5, D, "scalar", density, "hip", output="numpy", sigma=0.7, **extra)
        v.debug_option("direct", 0)
        out = v.forward(xyz, None, f, 2.0)
        ref = c_oracle.voxelize(xyz, f, 2.0, dimension=D, density=density, sigma=0.7, blockdim=blockdim)
        assert_gaussian(out, ref)  # (binary features too: sums of ~150 float32 products, the relative branch of the rule)


def test_long_x_list_beyond_lds_copy(mv):
    """An x-slab list longer than the binning pass's LDS copy (1024 entries): its tail is re-read from L2."""
    from oracle import c_oracle

    rng = np.random.default_rng(13)
    D = 64
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2, W_ / 2, (9000, 3))
    xyz[:, 0] = rng.uniform(-0.4, 0.4, 9000)  # a plate: every atom in the same two or three x-slabs
    t = rng.integers(0, 4, 9000)
    v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy")
    ref = c_oracle.voxelize(xyz, t, 1.0, dimension=D, density="binary", num_channels=4)
    for route in (0, 1):  # direct: three scan segments of 4096 atoms, hundreds of candidates per slab
        v.debug_option("direct", route)
        assert np.array_equal(v.forward(xyz, None, t, 1.0), ref)


@pytest.mark.parametrize("n", [2049, 4096, 4097, 6144, 6145, 8192, 8193, 10000, 10241, 12288, 12289, 16385, 20000])
def test_binning_of_one_large_molecule_at_every_chunk_configuration(mv, n):
    """One large molecule on the binned route takes the 1024-thread binning configuration (xbin_kernel<1024, ., CH, 1>,
    CH = 4 / 6 / 8 / 10 / 12 / 16 chunks of 1024 atoms in flight; above 16 384 atoms several rounds): atom counts either side
    of every CH boundary, against the direct kernel bit for bit and against the oracle."""
    from oracle import c_oracle

    rng = np.random.default_rng(n)
    D = 48
    W_ = 0.5 * (D - 1)
    xyz = rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3))
    f = rng.random((n, 8)).astype(np.float32)
    r = rng.uniform(0.6, 1.2, n).astype(np.float32)
    v = mv.create_voxelizer(0.5, D, "atom-wise", "gaussian", "hip", output="numpy", sigma=0.8)
    v.debug_option("direct", 0)
    binned = v.forward(xyz, None, f, r).copy()
    v.debug_option("direct", 1)
    assert np.array_equal(v.forward(xyz, None, f, r), binned)
    if n in (4097, 10000, 16385):
        assert_gaussian(binned, c_oracle.voxelize(xyz, f, r, dimension=D, sigma=0.8, radii_type="atom-wise"))


@pytest.mark.parametrize("D,B", [(96, 1), (100, 1), (100, 3), (128, 2)])
def test_binning_of_large_molecules_on_grids_with_many_slabs_per_x_slab(mv, D, B):
    """Grids above 64 voxels have several slabs per z row and 48-64 slabs per x-slab: one or a few large molecules take
    the 1024-thread binning configuration with one line per wave and several blocks per x-slab (B = 1) or four lines
    per wave (small batches); 100 is not a multiple of the slab sizes. Binned route against the direct kernel bit for
    bit, molecule 0 against the oracle."""
    from oracle import c_oracle

    rng = np.random.default_rng(1000 * D + B)
    W_ = 0.5 * (D - 1)
    n = 3000
    xyz = [rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)) for _ in range(B)]
    f = [rng.random((n, 4)).astype(np.float32) for _ in range(B)]
    off = np.arange(B + 1, dtype=np.int64) * n
    v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", output="numpy", sigma=0.7)
    v.debug_option("direct", 0)
    binned = v.forward_batch(np.concatenate(xyz), off, None, np.concatenate(f), 1.4).copy()
    v.debug_option("direct", 1)
    assert np.array_equal(v.forward_batch(np.concatenate(xyz), off, None, np.concatenate(f), 1.4), binned)
    assert_gaussian(binned[0], c_oracle.voxelize(xyz[0], f[0], 1.4, dimension=D, sigma=0.7))


@pytest.mark.parametrize("D", [18, 50])
def test_even_dimension_that_is_not_a_multiple_of_four(mv, D):
    """Rows of such grids start on 8-byte, not 16-byte, boundaries: the write-out takes the element-by-element path
    (both routes, a slice of a batch grid as out_grid included)."""
    from oracle import c_oracle

    rng = np.random.default_rng(D)
    W_ = 0.5 * (D - 1)
    n = 700
    xyz = rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3))
    f = rng.random((n, 5)).astype(np.float32)
    ref = c_oracle.voxelize(xyz, f, 1.1, dimension=D)
    v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip")
    grid = v.get_empty_grid(5, batch_size=3)
    dx, df = v.asarray(xyz, "coords"), v.asarray(f, "features")
    for route in (0, 1):
        v.debug_option("direct", route)
        grid.fill_(7.0)
        out = v.forward(dx, None, df, 1.1, out_grid=grid[1])
        assert out.data_ptr() == grid[1].data_ptr()
        assert_gaussian(out.cpu().numpy(), ref)
        assert float(grid[0].min()) == 7.0 and float(grid[2].max()) == 7.0  # neighbours untouched


def test_ragged_batch_with_one_large_molecule(mv):
    """Packed x-list regions: a 5000-atom molecule next to tiny ones in one launch."""
    from oracle import c_oracle

    rng = np.random.default_rng(12)
    D = 24
    W_ = 0.5 * (D - 1)
    sizes = [3, 5000, 0, 17, 1]
    coords = [rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)) for n in sizes]
    types = [rng.integers(0, 3, n) for n in sizes]
    offsets = np.cumsum([0] + sizes)
    v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip", output="numpy")
    out = v.forward_batch(np.concatenate(coords), offsets, None, np.concatenate(types), 1.0, num_channels=3)
    for b, n in enumerate(sizes):
        ref = c_oracle.voxelize(coords[b], types[b], 1.0, dimension=D, density="binary", num_channels=3) if n else 0
        assert np.array_equal(out[b], ref + np.zeros_like(out[b])), b


def test_pipelined_chunks_match_single_stream(mv):
    """Batches of >= 8 molecules are cut into chunks whose pre-pass runs on a side stream (debug option "chunks"); results
    must not depend on the chunk count, and every chunk count must match the oracle (ragged sizes, empty
    molecules, a dense cluster whose slabs walk their x-lists, random transforms)."""
    from oracle import c_oracle

    rng = np.random.default_rng(21)
    D = 32
    W_ = 0.5 * (D - 1)
    sizes = [40, 0, 700, 3, 1500, 0, 0, 90, 2500, 1, 33, 400, 0, 64, 65, 1000, 7]
    coords = [rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)) for n in sizes]
    coords[4] = rng.normal(0.0, 0.4, (sizes[4], 3))  # dense cluster: hundreds of candidates per slab
    feats = [rng.random((n, 7)).astype(np.float32) for n in sizes]
    radii = [rng.uniform(0.8, 1.6, n).astype(np.float32) for n in sizes]
    offsets = np.cumsum([0] + sizes)
    outs = {}
    for chunks in (1, 2, 3, 5):
        v = mv.create_voxelizer(0.5, D, "atom-wise", "gaussian", "hip", sigma=0.7, output="numpy")
        v.debug_option("chunks", chunks)
        for _ in range(2):  # the second call reuses the workspace the first call's launches read
            outs[chunks] = v.forward_batch(np.concatenate(coords), offsets, None, np.concatenate(feats), np.concatenate(radii))
    for chunks in (2, 3, 5):
        assert np.array_equal(outs[chunks], outs[1]), chunks
    for b, n in enumerate(sizes):
        if n == 0:
            assert not outs[1][b].any()
            continue
        ref = c_oracle.voxelize(coords[b], feats[b], radii[b], dimension=D, radii_type="atom-wise", density="gaussian", sigma=0.7)
        _compare(outs[1][b], ref, exact=False)  # (b == 4: sums of hundreds of terms, relative branch of the rule)


def test_transform_objects_on_device(mv):
    """T / RandomTransform on torch CUDA tensors equal the seeded reference results (goldens)."""
    import torch

    z, idx = goldens.load("transform_cases.npz")
    xyz, center = z["coords"], z["center"]
    tx = torch.as_tensor(xyz, device="cuda")
    rt_mod = __import__("molvoxel_amd.voxelizer.hip.transform", fromlist=["x"])
    for case in idx:
        np.random.seed(case["seed"])
        if case["id"].startswith("t"):
            out = rt_mod.do_random_transform(tx, center if case["use_center"] else None,
                                             case["random_translation"], case["random_rotation"])
            assert np.array_equal(np.random.rand(2), z[f"{case['id']}/next_rand"])
        else:
            T = mv.create_random_transform(case["random_translation"], case["random_rotation"], "hip").get_transform()
            out = T(tx, center)
        assert np.array_equal(out.cpu().numpy(), z[f"{case['id']}/out"]), case["id"]


@pytest.mark.parametrize("case", IDX_P64, ids=[c["id"] for c in IDX_P64])
def test_precision64_golden(mv, case):
    """precision=64 handles (numpy/voxelizer.py:33-34): float64 features / radii in, float64 grids out."""
    coords, chan, radii = goldens.small_case_inputs(Z_P64, case)
    ref = Z_P64[f"{case['id']}/out"]
    extra = {} if case["blockdim"] is None else {"blockdim": case["blockdim"]}
    v = mv.create_voxelizer(case["resolution"], case["dimension"], case["radii_type"], case["density"], "hip",
                            sigma=case["sigma"], precision=64, output="numpy", **extra)
    out = v.forward(coords, None, chan, radii)
    assert out.dtype == np.float64 and out.shape == ref.shape
    assert np.array_equal(out != 0, ref != 0), f"membership differs in {(np.not_equal(out != 0, ref != 0)).sum()} voxels"
    if case["density"] == "binary" and case["mode"] != "features":
        assert np.array_equal(out, ref)
    else:
        assert np.abs(out - ref).max() <= P64_TOL * max(1.0, float(np.abs(ref).max()))


def test_precision64_full_size_device_tensors_and_batch(mv):
    """cfg-2-sized float64 run (two channel chunks of 16) on torch tensors against the numpy port; batch form;
    same out_grid object back; float32 handles are unaffected."""
    import torch

    from molvoxel_amd import workloads as W
    from oracle import numpy_port

    wl = W.cfg2(batch=3)
    v = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip", precision=64)
    assert v.get_empty_grid(2).dtype == torch.float64 and v.asarray([1.0], "radii").dtype == torch.float64
    coords = [v.asarray(wl.coords[i], "coords") for i in range(3)]
    feats = [v.asarray(wl.channels[i], "features") for i in range(3)]
    grid = v.get_empty_grid(32)
    out = v.forward_features(coords[0], None, feats[0], 1.0, out_grid=grid)
    assert out is grid and out.dtype == torch.float64
    spec = numpy_port.GridSpec(0.5, 64)
    ref = numpy_port.voxelize(spec, wl.coords[0], wl.channels[0], 1.0, precision=64)
    got = out.cpu().numpy()
    assert np.array_equal(got != 0, ref != 0)
    assert np.abs(got - ref).max() <= P64_TOL * max(1.0, float(np.abs(ref).max()))
    offsets = np.arange(4, dtype=np.int64) * 4000
    batch = v.forward_batch(torch.cat(coords), offsets, None, torch.cat(feats), 1.0)
    assert batch.dtype == torch.float64 and torch.equal(batch[0], out)
    for b in (1, 2):
        assert torch.equal(batch[b], v.forward_features(coords[b], None, feats[b], 1.0))
    # types: sums of float64 densities in atom order, exactly what the reference's loop does (:364-365)
    vt = mv.create_voxelizer(0.5, 48, "atom-wise", "binary", "hip", precision=64, output="numpy")
    w3 = W.cfg3()
    rad = np.full(w3.coords[0].shape[0], 1.25)
    ref_t = numpy_port.voxelize(numpy_port.GridSpec(0.5, 48), w3.coords[0], w3.channels[0], rad, radii_type="atom-wise",
                                density="binary", precision=64)
    assert np.array_equal(vt.forward_types(w3.coords[0], None, w3.channels[0], rad), ref_t)


def test_offsets_cache_across_calls_and_streams(mv):
    """The device copy of the batch offsets is reused while they do not change (and only on the stream that uploaded
    them): same offsets, different offsets of the same length, a transform in between, another stream."""
    import torch

    rng = np.random.default_rng(31)
    D = 24
    W_ = 0.5 * (D - 1)
    v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip")

    def batch(sizes):
        coords = rng.uniform(-W_ / 2, W_ / 2, (sum(sizes), 3))
        types = rng.integers(0, 3, sum(sizes))
        offsets = np.cumsum([0] + sizes)
        out = v.forward_batch(v.asarray(coords, "coords"), offsets, None, v.asarray(types, "types"), 1.0, num_channels=3)
        for b in range(len(sizes)):
            lo, hi = offsets[b], offsets[b + 1]
            one = v.forward_types(v.asarray(coords[lo:hi], "coords"), None, v.asarray(types[lo:hi], "types"), 1.0,
                                  out_grid=v.get_empty_grid(3)) if hi > lo else torch.zeros_like(out[b])
            assert torch.equal(out[b], one), (sizes, b)

    batch([10, 20, 30])
    batch([10, 20, 30])  # cached offsets
    batch([30, 20, 10])  # same length, different content
    v.transform_class(0.5, True).forward(v.asarray(rng.uniform(-1, 1, (5, 3)), "coords"), None)  # other user of the handle
    batch([30, 20, 10])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        batch([30, 20, 10])  # same offsets, other stream: uploaded again
        batch([5, 5, 50])
    torch.cuda.synchronize()


def test_device_types_caches_follow_in_place_writes_and_new_tensors(mv):
    """The cached (min, max) / int32 copy of a device `types` tensor must not outlive its content: in-place writes
    bump torch's version counter; a new tensor is a new object even when the allocator hands back the same address."""
    import torch

    from oracle import c_oracle

    rng = np.random.default_rng(8)
    D = 16
    xyz = rng.uniform(-3, 3, (40, 3))
    v = mv.create_voxelizer(0.5, D, "scalar", "binary", "hip")
    coords = v.asarray(xyz, "coords")
    t_np = rng.integers(0, 3, 40)
    types = v.asarray(t_np, "types")

    def check(t_dev, t_host):
        out = v.forward_types(coords, None, t_dev, 1.0).cpu().numpy()
        assert np.array_equal(out, c_oracle.voxelize(xyz, t_host, 1.0, dimension=D, density="binary"))

    check(types, t_np)
    check(types, t_np)  # served from the caches
    types[5] = 6  # in place: more channels now
    t_np = t_np.copy()
    t_np[5] = 6
    check(types, t_np)
    addr = types.data_ptr()
    del types
    for _ in range(4):  # fresh tensors, very likely at the address just freed
        t_np = rng.integers(0, 5, 40)
        fresh = v.asarray(t_np, "types")
        check(fresh, t_np)
        same_addr = fresh.data_ptr() == addr
        del fresh
    assert isinstance(same_addr, bool)


def test_argument_dtypes_and_layouts_are_normalised(mv):
    """What the reference's asarray/_dtypechange would accept (numpy/voxelizer.py:562-583): float32 coords, float64
    features, int64 types, Fortran-ordered arrays, a non-contiguous or wrongly typed out_grid (still the object
    returned, filled through a temporary)."""
    import torch

    from oracle import c_oracle

    rng = np.random.default_rng(17)
    D = 20
    xyz32 = rng.uniform(-4, 4, (60, 3)).astype(np.float32)
    feats64 = np.asfortranarray(rng.random((60, 6)))
    types64 = rng.integers(0, 4, 60).astype(np.int64)
    v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", output="numpy")
    ref_f = c_oracle.voxelize(xyz32.astype(np.float64), feats64.astype(np.float32), 1.0, dimension=D)
    ref_t = c_oracle.voxelize(xyz32.astype(np.float64), types64, 1.0, dimension=D)
    _compare(v.forward_features(xyz32, None, feats64, 1.0), ref_f, exact=False)
    _compare(v.forward_types(xyz32, None, types64, 1.0), ref_t, exact=False)
    big = np.zeros((6, D, D, 2 * D), np.float32)
    view = big[..., ::2]  # non-contiguous
    assert v.forward_features(xyz32, None, feats64, 1.0, out_grid=view) is view
    _compare(np.ascontiguousarray(view), ref_f, exact=False)
    out64 = np.empty((6, D, D, D), np.float64)  # wrong dtype: converted on the way back
    assert v.forward_features(xyz32, None, feats64, 1.0, out_grid=out64) is out64
    assert np.abs(out64 - ref_f).max() <= GAUSS_TOL
    vt = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip")  # torch in / out
    tview = torch.zeros((6, D, D, 2 * D), device=vt.device)[..., ::2]
    got = vt.forward_features(torch.as_tensor(xyz32), None, torch.as_tensor(feats64), 1.0, out_grid=tview)
    assert got is tview
    _compare(tview.contiguous().cpu().numpy(), ref_f, exact=False)


def test_reference_readme_quick_start(mv):
    """README.md:48-98 of the reference with `library='hip'`: the 10gs ligand through forward_single / forward_types /
    forward_features, once with numpy arrays (boolean feature matrix included) and once with float32 / int64 CUDA
    tensors."""
    import os

    import torch

    from molvoxel_amd.etc import mol as M
    from oracle import c_oracle

    lig = M.read_sdf(os.path.join(goldens.GOLD, "10gs", "10gs_ligand.sdf"))[0]
    channels = {"C": 0, "N": 1, "O": 2, "S": 3}
    coords = lig.coords
    center = coords.mean(axis=0)
    atom_types = np.array([channels[a.GetSymbol()] for a in lig.atoms()])
    atom_features = np.array([[a.GetSymbol() == "C", a.GetSymbol() == "N", a.GetSymbol() == "O", a.GetSymbol() == "S",
                               a.GetIsAromatic()] for a in lig.atoms()])  # bool (V, 5)
    assert atom_features.dtype == bool
    voxelizer = mv.create_voxelizer(library="hip", output="numpy")  # defaults: 0.5, 64, scalar, gaussian sigma 0.5
    moved = coords - center
    ref = {
        "single": c_oracle.voxelize(moved, None, 1.0, dimension=64),
        "types": c_oracle.voxelize(moved, atom_types, 1.0, dimension=64),
        "features": c_oracle.voxelize(moved, atom_features.astype(np.float32), 1.0, dimension=64),
    }
    img = {
        "single": voxelizer.forward_single(coords, center, 1.0),
        "types": voxelizer.forward_types(coords, center, atom_types, 1.0),
        "features": voxelizer.forward_features(coords, center, atom_features, 1.0),
    }
    assert img["single"].shape == (1, 64, 64, 64) and img["types"].shape == (4, 64, 64, 64) and img["features"].shape == (5, 64, 64, 64)
    for k in ref:
        _compare(img[k], ref[k], exact=False)
    # "PyTorch - Cuda Available" (README.md:84-98)
    vt = mv.create_voxelizer(library="hip", device="cuda")
    tc = torch.FloatTensor(coords).to("cuda")
    tcen = torch.FloatTensor(center).to("cuda")
    ttypes = torch.LongTensor(atom_types).to("cuda")
    tfeat = torch.FloatTensor(atom_features.astype(np.float32)).to("cuda")
    moved32 = tc.double().cpu().numpy() - tcen.double().cpu().numpy()  # what float32 inputs mean in float64
    out = vt.forward_features(tc, tcen, tfeat, 1.0)
    assert out.is_cuda and tuple(out.shape) == (5, 64, 64, 64)
    _compare(out.cpu().numpy(), c_oracle.voxelize(moved32, atom_features.astype(np.float32), 1.0, dimension=64), exact=False)
    _compare(vt.forward_types(tc, tcen, ttypes, 1.0).cpu().numpy(), c_oracle.voxelize(moved32, atom_types, 1.0, dimension=64), exact=False)
    _compare(vt.forward_single(tc, tcen, 1.0).cpu().numpy(), c_oracle.voxelize(moved32, None, 1.0, dimension=64), exact=False)


def test_out_grid_slices_of_a_batch_grid_with_odd_dimension(mv):
    """The reference harness writes molecule i into `out_grid=grid[i]` (test/test_time_numpy.py:11-15). With D = 33,
    C = 10, float32, slice 1 starts 1 437 480 B into the grid: 8 mod 16. Such slices take the scalar-store path."""
    import torch

    from oracle import c_oracle

    rng = np.random.default_rng(41)
    for D, C_ in ((33, 10), (17, 3), (64, 5)):
        W_ = 0.5 * (D - 1)
        v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip")
        grid = v.get_empty_grid(C_, batch_size=3)
        grid.fill_(7.0)
        mols = [(rng.uniform(-W_ / 2, W_ / 2, (120, 3)), rng.random((120, C_)).astype(np.float32)) for _ in range(3)]
        for i, (xyz, f) in enumerate(mols):
            got = v.forward(v.asarray(xyz, "coords"), None, v.asarray(f, "features"), 1.0, out_grid=grid[i])
            assert got.data_ptr() == grid[i].data_ptr()
        for i, (xyz, f) in enumerate(mols):
            assert_gaussian(grid[i].cpu().numpy(), c_oracle.voxelize(xyz, f, 1.0, dimension=D))
        # a float32 view that is only 4-byte aligned (one element into a larger buffer)
        flat = torch.empty(C_ * D**3 + 1, dtype=torch.float32, device=v.device)
        view = flat[1:].view(C_, D, D, D)
        v.forward(v.asarray(mols[0][0], "coords"), None, v.asarray(mols[0][1], "features"), 1.0, out_grid=view)
        assert torch.equal(view, grid[0])


def test_interleaved_calls_on_two_streams_without_synchronisation(mv):
    """One handle, two torch streams, no torch.cuda.synchronize() between calls: the handle's workspace is shared,
    so a call on another stream must first wait for the previous stream's launches (include/mvx.h, conventions)."""
    import torch

    from molvoxel_amd import workloads as W
    from oracle import c_oracle

    wl = W.cfg2(batch=4, n_atoms=3000)
    v = mv.create_voxelizer(0.5, 64, "scalar", "gaussian", "hip")
    coords = [v.asarray(wl.coords[i], "coords") for i in range(4)]
    feats = [v.asarray(wl.channels[i], "features") for i in range(4)]
    big_c, big_f = torch.cat(coords), torch.cat(feats)
    off = np.arange(5, dtype=np.int64) * 3000
    # expected grids: the same calls one at a time, checked against the oracle
    exp_batch = v.forward_batch(big_c, off, None, big_f, 1.0).clone()
    exp_single = [v.forward_features(coords[i], None, feats[i], 1.0).clone() for i in range(4)]
    torch.cuda.synchronize()
    for i in range(4):
        assert_gaussian(exp_single[i].cpu().numpy(), c_oracle.voxelize(wl.coords[i], wl.channels[i], 1.0, dimension=64))
        assert torch.equal(exp_batch[i], exp_single[i])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(8):
        i = rep % 4
        with torch.cuda.stream(s1):  # a long batch call ...
            gb = v.forward_batch(big_c, off, None, big_f, 1.0)
        with torch.cuda.stream(s2):  # ... and at once a single call on another stream, same handle
            g1 = v.forward_features(coords[i], None, feats[i], 1.0)
        outs.append((i, gb, g1))
    torch.cuda.synchronize()
    for i, gb, g1 in outs:
        assert torch.equal(g1, exp_single[i])
        assert torch.equal(gb, exp_batch)


@pytest.mark.parametrize("mode,radii_type,C_", [("features", "scalar", 33), ("features", "channel-wise", 40),
                                                ("types", "channel-wise", 40), ("types", "atom-wise", 33),
                                                ("features", "atom-wise", 48)])
def test_precision64_more_than_32_channels(mv, mode, radii_type, C_):
    """float64 workgroups take 16 channels (32 for Gaussian grids of more than 16 channels): C > 32 means several
    chunks (packed double weights, Cpad = 48, channel-wise radii clamped at C - 1 in the last chunk)."""
    from oracle import numpy_port

    rng = np.random.default_rng(64 + C_)
    D = 20
    W_ = 0.5 * (D - 1)
    n = 150
    xyz = rng.uniform(-W_ / 2 - 0.5, W_ / 2 + 0.5, (n, 3))
    chan = rng.random((n, C_)) if mode == "features" else rng.integers(0, C_, n)
    if mode == "types":
        chan[0] = C_ - 1
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(0.8, 1.8, n), "channel-wise": rng.uniform(0.8, 1.8, C_)}[radii_type]
    for density in ("gaussian", "binary"):
        v = mv.create_voxelizer(0.5, D, radii_type, density, "hip", sigma=0.6, precision=64, output="numpy")
        out = v.forward(xyz, None, chan, radii)
        ref = numpy_port.voxelize(numpy_port.GridSpec(0.5, D), xyz, chan, radii, radii_type=radii_type, density=density,
                                  sigma=0.6, precision=64, num_channels=C_)
        assert out.dtype == np.float64 and out.shape == ref.shape
        if density == "binary" and mode == "types":
            assert_exact(out, ref)
        else:
            assert_gaussian(out, ref, P64_TOL)
        # Gaussian grids of more than 16 channels take 32 channels per workgroup on 4-wave slabs by default; the
        # 16-channel form (what binary grids use) is one debug option away and must agree in every voxel
        v.debug_option("max_ct64", 16)
        narrow = v.forward(xyz, None, chan, radii)
        assert np.array_equal(narrow != 0, out != 0)
        assert np.abs(narrow - out).max() <= 1e-13 * max(1.0, np.abs(out).max())


def test_forward_batch_rejects_short_arrays(mv):
    """forward_batch applies the per-molecule argument checks to the concatenated arrays (the library reads sumN rows)."""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-3, 3, (30, 3))
    off = np.array([0, 10, 30])
    v = mv.create_voxelizer(0.5, 16, "scalar", "gaussian", "hip", output="numpy")
    with pytest.raises(AssertionError, match="atom features does not match number of atoms"):
        v.forward_batch(xyz, off, None, rng.random((29, 4)).astype(np.float32), 1.0)
    with pytest.raises(AssertionError, match="types does not match dimension"):
        v.forward_batch(xyz, off, None, rng.integers(0, 3, 29), 1.0)
    with pytest.raises(AssertionError, match="radii should be scalar"):
        v.forward_batch(xyz, off, None, rng.random((30, 4)).astype(np.float32), np.ones(30, np.float32))
    v.radii_type = "atom-wise"
    with pytest.raises(AssertionError, match="radii should be Array"):
        v.forward_batch(xyz, off, None, rng.random((30, 4)).astype(np.float32), 1.0)
    with pytest.raises(AssertionError, match="number of atoms"):
        v.forward_batch(xyz, off, None, rng.random((30, 4)).astype(np.float32), np.ones(29, np.float32))
    v.radii_type = "channel-wise"
    with pytest.raises(AssertionError, match="number of channels"):
        v.forward_batch(xyz, off, None, rng.random((30, 4)).astype(np.float32), np.ones(3, np.float32))
    with pytest.raises(AssertionError, match="Channel-Wise Radii Type is not supported"):
        v.forward_batch(xyz, off, None, None, np.ones(1, np.float32))
    with pytest.raises(AssertionError, match="number of channels"):
        v.forward_batch(xyz, off, None, np.full(30, 3), np.ones(3, np.float32), num_channels=4)
    # fewer radii than channels is fine for types as long as every type has one (extra channels stay zero)
    out = v.forward_batch(xyz, off, None, rng.integers(0, 3, 30), np.ones(3, np.float32), num_channels=5)
    assert out.shape == (2, 5, 16, 16, 16) and not out[:, 3:].any()


def test_overlapped_prepass_equals_serial_calls(mv):
    """mvx_set_overlap: the pre-pass of call k+1 runs on the side stream under call k's voxelize launches, on the
    other workspace set. A loop of batched calls with changing inputs, offsets, operators and radii kinds - and no host
    synchronisation between calls - must give exactly the grids of the serial handle."""
    import torch

    rng = np.random.default_rng(99)
    D = 32
    W_ = 0.5 * (D - 1)

    def make(sizes, mode, C_):
        coords = rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (sum(sizes), 3))
        chan = rng.random((sum(sizes), C_)).astype(np.float32) if mode == "features" else rng.integers(0, C_, sum(sizes))
        return coords, chan, np.cumsum([0] + sizes)

    jobs = [make([700, 900, 40, 0, 1300, 800, 650, 2000, 300, 1100, 5, 900], "features", 8),
            make([1500, 600, 700, 900, 40, 1300, 800, 650, 2000, 300, 1100, 400], "features", 8),
            make([300, 200, 400, 900, 100, 1300, 800, 650, 600, 300, 1100, 700], "types", 5),
            make([2500] + [350] * 11, "features", 33)]
    for radii_type in ("scalar", "atom-wise", "channel-wise"):
        serial = mv.create_voxelizer(0.5, D, radii_type, "gaussian", "hip", sigma=0.6)
        fast = mv.create_voxelizer(0.5, D, radii_type, "gaussian", "hip", sigma=0.6, overlap_prepass=True)
        for v in (serial, fast):
            v.debug_option("direct", 0)
        dev = []
        for coords, chan, off in jobs:
            C_ = chan.shape[1] if chan.ndim == 2 else int(chan.max()) + 1
            radii = {"scalar": 1.2, "atom-wise": serial.asarray(rng.uniform(0.8, 1.7, coords.shape[0]), "radii"),
                     "channel-wise": serial.asarray(rng.uniform(0.8, 1.7, C_), "radii")}[radii_type]
            dev.append((serial.asarray(coords, "coords"), serial.asarray(chan, "features" if chan.ndim == 2 else "types"), off, radii, C_))
        torch.cuda.synchronize()  # the inputs are complete before the loop starts: the overlap contract
        order = [0, 1, 0, 2, 3, 3, 1, 2, 0, 0, 3, 1]
        want = [serial.forward_batch(dev[j][0], dev[j][2], None, dev[j][1], dev[j][3], num_channels=dev[j][4]).clone() for j in order]
        got = [fast.forward_batch(dev[j][0], dev[j][2], None, dev[j][1], dev[j][3], num_channels=dev[j][4]).clone() for j in order]
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), (radii_type, k, order[k])
        # a single-molecule call (direct kernel) and a transform in between do not disturb the sets
        one = fast.forward_features(dev[0][0][:700], None, dev[0][1][:700], dev[0][3] if radii_type != "atom-wise" else dev[0][3][:700])
        assert torch.equal(one, want[0][0])
        assert torch.equal(fast.forward_batch(dev[1][0], dev[1][2], None, dev[1][1], dev[1][3], num_channels=dev[1][4]), want[1])


def test_views_between_overlapped_batches_leave_the_overlap_as_it_was(mv):
    """forward_views on a handle with mvx_set_overlap: its compact batch must not overlap its pre-pass (the gathered rows are made
    on the caller's stream a moment before), and that is a property of the one call - the forward_batch calls around it overlap
    as before, on alternating workspace sets. forward_batch and forward_views alternate on device tensors with no host
    synchronisation by the caller in between; every result must equal the serial handle's.

    D = 16 at 0.5 A, C = 8 features; two batches of 4 molecules of 40 ... 120 atoms (B > 1, one chunk, the one-launch route
    switched off: the smallest batch on the overlapped binned route); 4 views of a 300-atom cloud, one of them empty."""
    import torch

    rng = np.random.default_rng(7)
    D, C_ = 16, 8
    half = 0.5 * (D - 1) / 2
    serial = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.6)
    fast = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.6, overlap_prepass=True)
    for v in (serial, fast):
        v.debug_option("direct", 0)
    batches = []
    for sizes in ([40, 120, 75, 90], [110, 45, 60, 100]):
        n = sum(sizes)
        batches.append((serial.asarray(rng.uniform(-half - 1, half + 1, (n, 3)), "coords"),
                        serial.asarray(rng.random((n, C_)).astype(np.float32), "features"), np.cumsum([0] + sizes)))
    cloud = rng.uniform(-10.0, 10.0, (300, 3))
    centers = cloud[rng.integers(0, 300, 4)] + rng.normal(0.0, 0.5, (4, 3))
    centers[2] = 60.0  # (a view of empty space)
    cloud, centers = serial.asarray(cloud, "coords"), torch.tensor(centers, device="cuda")
    cloud_feat = serial.asarray(rng.random((300, C_)).astype(np.float32), "features")
    torch.cuda.synchronize()  # the inputs are complete before the loop starts: the overlap contract

    def run(v, job):
        if job == "views":
            return v.forward_views(cloud, centers, cloud_feat, 1.2).clone()
        coords, feat, off = batches[job]
        return v.forward_batch(coords, off, None, feat, 1.2).clone()

    order = [0, "views", 1, "views", 0, 0, "views", "views", 1, 0]
    want = [run(serial, job) for job in order]
    got = [run(fast, job) for job in order]
    torch.cuda.synchronize()
    assert fast.last_plan() == serial.last_plan()
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.shape == ((4, C_, D, D, D)) and torch.equal(a, b), (k, order[k])
    views = want[1]
    assert not views[2].any() and all(views[i].any() for i in (0, 1, 3)) and all(w.any() for w in want)


@pytest.mark.parametrize("C_,distinct,D,blockdim", [(32, 4, 32, None), (40, 2, 32, None), (12, 9, 24, None), (32, 1, 32, None),
                                                    (7, 3, 27, 5), (64, 8, 16, None), (33, 33, 16, None), (32, 32, 24, None),
                                                    (70, 31, 16, None), (40, 40, 16, None), (96, 96, 16, None), (45, 45, 20, 5)])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
def test_channel_wise_features_grouped_by_radius(mv, C_, distinct, D, blockdim, density):
    """Channel-wise radii for features (numpy/voxelizer.py:213-224): channels that share a radius share the membership test
    and the density. chan_aux_kernel numbers the distinct radii of every chunk of 32 channels on the device (slots, by
    descending radius: at most 32 per chunk, so any number of channels and of distinct radii - 40 / 40, 96 / 96 here - runs
    grouped; there is no per-channel kernel any more) and the grouped launch evaluates one threshold test and one density
    per slot and candidate on the matrix-core path, stopping at the first slot no lane hits. Every shape against the
    oracle, and batched against per-molecule calls bit for bit (both grouped: channel-wise features never take the
    one-launch route); chunks that hold several slots, radii that recur in several chunks."""
    from oracle import c_oracle

    rng = np.random.default_rng(1000 * C_ + distinct)
    W_ = 0.5 * (D - 1)
    sizes = [900, 30, 0, 1400]
    off = np.cumsum([0] + sizes)
    xyz = rng.uniform(-W_ / 2 - 1.5, W_ / 2 + 1.5, (off[-1], 3))
    feat = (rng.random((off[-1], C_)) - 0.25).astype(np.float32)
    pool = rng.uniform(0.7, 1.9, distinct).astype(np.float32)
    radii = pool[rng.integers(0, distinct, C_)]
    radii[:distinct] = pool  # every value occurs
    extra = {"blockdim": blockdim} if blockdim else {}
    v = mv.create_voxelizer(0.5, D, "channel-wise", density, "hip", output="numpy", sigma=0.6, **extra)
    v.debug_option("direct", 0)
    got = v.forward_batch(xyz, off, None, feat, radii)
    one = mv.create_voxelizer(0.5, D, "channel-wise", density, "hip", output="numpy", sigma=0.6, **extra)
    one.debug_option("direct", 1)
    for b in range(len(sizes)):
        lo, hi = off[b], off[b + 1]
        ref = c_oracle.voxelize(xyz[lo:hi], feat[lo:hi], radii, resolution=0.5, dimension=D, radii_type="channel-wise",
                                density=density, sigma=0.6, num_channels=C_, blockdim=blockdim)
        if density == "binary":
            assert np.array_equal(got[b] != 0, ref != 0) and np.abs(got[b] - ref).max() <= 1e-6
        else:
            assert_gaussian(got[b], ref)
        if hi > lo:
            assert np.array_equal(got[b], one.forward_features(xyz[lo:hi], None, feat[lo:hi], radii)), b


def test_per_molecule_calls_with_overlap_enabled_wait_for_their_converted_inputs(mv):
    """overlap_prepass concerns batched calls only (mvx.h: "the batched three-launch path"). A per-molecule forward() on
    such a handle - binned route (a cfg-5-sized molecule), float32 device coords and a float32 device centre that this
    layer converts to float64 ON the caller's stream right before the call - must not read them from a side stream that
    never waited: same grid as a serial handle, call after call, with no synchronisation in between."""
    import torch

    rng = np.random.default_rng(321)
    D, N, C_ = 96, 9000, 8
    W_ = 0.5 * (D - 1)
    serial = mv.create_voxelizer(0.5, D, "atom-wise", "gaussian", "hip", sigma=0.7)
    fast = mv.create_voxelizer(0.5, D, "atom-wise", "gaussian", "hip", sigma=0.7, overlap_prepass=True)
    for v in (serial, fast):
        v.debug_option("direct", 0)
    for rep in range(4):
        xyz32 = torch.as_tensor(rng.uniform(-W_ / 2, W_ / 2, (N, 3)) + 3.0, dtype=torch.float32, device="cuda")
        cen32 = torch.full((3,), 3.0, dtype=torch.float32, device="cuda")
        feat64 = torch.as_tensor(rng.random((N, C_)), dtype=torch.float64, device="cuda")  # converted to float32 by the layer
        rad64 = torch.as_tensor(rng.uniform(0.8, 1.9, N), dtype=torch.float64, device="cuda")
        got = fast.forward(xyz32, cen32, feat64, rad64)
        want = serial.forward(xyz32, cen32, feat64, rad64)
        assert torch.equal(got, want), rep
        ty = torch.as_tensor(rng.integers(0, 5, N), dtype=torch.int64, device="cuda")  # int32 copy made by the layer
        assert torch.equal(fast.forward(xyz32, cen32, ty, rad64), serial.forward(xyz32, cen32, ty, rad64)), rep


def test_per_molecule_fast_path_replayed_with_changing_arguments(mv):
    """One voxelizer object driven like the reference harness (test/test_time_numpy.py:11-15) but with everything
    changing between calls: atom counts on both sides of every internal limit (one round of rows, one scan segment,
    the direct / binned switch), fresh tensors (new pointers), a device-resident centre, random transforms, radii_type
    reassigned on the live object (base/voxelizer.py:44-47) and a density switch. Every call equals the oracle."""
    import torch

    from molvoxel_amd.voxelizer.hip.transform import do_transform, draw_forward_transform
    from oracle import c_oracle

    rng = np.random.default_rng(2024)
    D, C_ = 48, 10
    W_ = 0.5 * (D - 1)
    v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.5)
    grid = v.get_empty_grid(C_, batch_size=2)
    sizes = [33, 1, 48, 49, 500, 3295, 4096, 4097, 9000, 64, 2, 8192, 8193, 700]
    step = 0
    for radii_type in ("scalar", "atom-wise", "channel-wise", "scalar"):
        v.radii_type = radii_type
        for density in ("gaussian", "binary"):
            v.density_type = density  # (back to gaussian resets sigma to 0.5: quirk Q12)
            for n in sizes[step % 3::3]:
                step += 1
                xyz = rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)) + 5.0
                center = np.full(3, 5.0) + rng.uniform(-0.3, 0.3, 3)
                feats = rng.random((n, C_)).astype(np.float32)
                radii = {"scalar": 1.0 + 0.1 * (step % 4), "atom-wise": rng.uniform(0.8, 1.8, n).astype(np.float32),
                         "channel-wise": rng.uniform(0.8, 1.8, C_).astype(np.float32)}[radii_type]
                d_xyz, d_cen, d_f = v.asarray(xyz, "coords"), v.asarray(center, "center"), v.asarray(feats, "features")
                d_r = radii if np.isscalar(radii) else v.asarray(radii, "radii")
                tr, rot = (0.5, True) if step % 2 else (0.0, False)
                np.random.seed(step)
                out = v.forward(d_xyz, d_cen, d_f, d_r, tr, rot, out_grid=grid[step % 2])
                np.random.seed(step)
                translation, quaternion = draw_forward_transform(tr, rot)
                moved = do_transform(xyz - center, None, translation, quaternion)
                ref = c_oracle.voxelize(moved, feats, radii, dimension=D, radii_type=radii_type, density=density, sigma=0.5)
                got = out.cpu().numpy()
                if density == "binary":
                    assert np.array_equal(got != 0, ref != 0), (radii_type, density, n)
                    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, float(ref.max())), (radii_type, density, n)
                else:
                    assert_gaussian(got, ref)


def test_batches_cut_for_the_infinity_cache_match_one_launch(mv):
    """Batches whose pre-pass data exceed the Infinity Cache budget run chunk by chunk (pre-pass, voxelize, pre-pass,
    voxelize ...; production budget 288 MB = 256 cfg-2 molecules). With the budget lowered, a ragged batch with a dense
    cluster (slabs beyond line + extension in every chunk), empty molecules and per-molecule transforms must give the same bits as
    the single-launch run and match the oracle."""
    from oracle import c_oracle

    rng = np.random.default_rng(77)
    D = 32
    W_ = 0.5 * (D - 1)
    sizes = [300, 0, 1200, 45, 2200, 0, 700, 64, 1, 900, 1500, 30, 400, 0, 800, 650, 5, 1000]
    coords = [rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)) for n in sizes]
    coords[4] = rng.normal(0.0, 0.5, (sizes[4], 3))
    feats = [rng.random((n, 12)).astype(np.float32) for n in sizes]
    centers = rng.uniform(-1, 1, (len(sizes), 3))
    offsets = np.cumsum([0] + sizes)
    allc = np.concatenate([c + centers[b] for b, c in enumerate(coords)])
    outs = {}
    for budget_kb in (0, 2000, 500, 100):  # 0 = production budget: one launch
        v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.6, output="numpy")
        v.debug_option("direct", 0)
        v.debug_option("mall_budget_kb", budget_kb)
        outs[budget_kb] = v.forward_batch(allc, offsets, centers, np.concatenate(feats), 1.1).copy()
    for k in (2000, 500, 100):
        assert np.array_equal(outs[k], outs[0]), k
    for b in (0, 2, 4, 10, 17):
        assert_gaussian(outs[0][b], c_oracle.voxelize(coords[b], feats[b], 1.1, dimension=D, sigma=0.6))
    assert not outs[0][1].any() and not outs[0][5].any()


def test_non_finite_and_huge_coordinates_never_contribute(mv):
    """NaN / infinite / astronomically large coordinates fail every comparison of the rule in the reference
    (numpy/voxelizer.py:487-492), so such atoms contribute nothing; both routes must agree bit for bit with each other
    and with the grid of the finite atoms alone (the direct kernel's float32 scan must not drop or invent anything)."""
    import torch

    rng = np.random.default_rng(31337)
    D = 32
    W_ = 0.5 * (D - 1)
    n = 600
    xyz = rng.uniform(-W_ / 2, W_ / 2, (n, 3))
    bad = xyz.copy()
    bad[5] = [np.nan, 0.0, 0.0]
    bad[17] = [np.inf, 1.0, -1.0]
    bad[40] = [-np.inf, np.nan, 2.0]
    bad[99] = [1e300, 1e300, 1e300]
    bad[123] = [3e38, -3e38, 0.5]
    bad[200] = [1e20, 0.0, 0.0]
    keep = np.ones(n, bool)
    keep[[5, 17, 40, 99, 123, 200]] = False
    f = rng.random((n, 8)).astype(np.float32)
    for radii_type, radii in (("scalar", 1.2), ("atom-wise", rng.uniform(0.8, 1.6, n).astype(np.float32))):
        v = mv.create_voxelizer(0.5, D, radii_type, "gaussian", "hip", sigma=0.6)
        outs = []
        for route in (0, 1):
            v.debug_option("direct", route)
            r = radii if np.isscalar(radii) else v.asarray(radii, "radii")
            outs.append(v.forward_features(v.asarray(bad, "coords"), None, v.asarray(f, "features"), r).clone())
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
        r_ok = radii if np.isscalar(radii) else v.asarray(radii[keep], "radii")
        clean = v.forward_features(v.asarray(xyz[keep], "coords"), None, v.asarray(f[keep], "features"), r_ok)
        assert torch.equal(outs[0], clean)


@pytest.mark.parametrize("D,C_,shift", [(1, 1, 0), (2, 3, 1), (3, 32, 2), (5, 32, 3), (7, 33, 0), (31, 32, 1), (33, 64, 0),
                                        (49, 32, 0), (50, 32, 2), (63, 40, 3), (64, 32, 1), (65, 32, 0), (66, 8, 2), (71, 16, 1),
                                        (101, 4, 3), (72, 32, 0), (88, 8, 0), (104, 33, 0), (120, 16, 0), (127, 5, 0), (128, 4, 0), (136, 2, 0), (150, 2, 1), (200, 1, 0)])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
def test_run_wise_write_out_of_rows_that_are_not_whole_quads(mv, D, C_, shift, density):
    """Grids with D % 4 != 0, or whose first float is not 16-byte aligned (`shift` floats into an aligned buffer), are
    written run by run (store_runs: aligned 16-byte stores inside each contiguous run, 4-byte stores at its ends; whole-row
    slabs up to D = 128 - 9 ... 16 waves per slab beyond 64 -, one run per row segment beyond; the aligned sizes above 64
    in the list cover the same slab plans with the float4 write-out). A batch of two molecules into a buffer with guard floats on both
    sides: both grids equal the oracle's, the guards stay untouched. 32-channel chunks take voxelize_runs_kernel, the
    remainder chunk and narrower grids the per-lane-range kernels."""
    import torch

    from oracle import c_oracle

    rng = np.random.default_rng(1000 * D + C_)
    W_ = 0.5 * (D - 1)
    n = min(600, 40 + 3 * D * D)
    v = mv.create_voxelizer(0.5, D, "scalar", density, "hip")
    mols = [(rng.uniform(-W_ / 2 - 1, W_ / 2 + 1, (n, 3)), rng.random((n, C_)).astype(np.float32)) for _ in range(2)]
    per = C_ * D**3
    guard = 64
    flat = torch.full((guard + shift + 2 * per + guard,), 7.0, dtype=torch.float32, device=v.device)
    grid = flat[guard + shift:guard + shift + 2 * per].view(2, C_, D, D, D)
    coords = v.asarray(np.concatenate([m[0] for m in mols]), "coords")
    feats = v.asarray(np.concatenate([m[1] for m in mols]), "features")
    got = v.forward_batch(coords, np.array([0, n, 2 * n], dtype=np.int64), None, feats, 1.2, out_grid=grid)
    assert got.data_ptr() == grid.data_ptr()
    out = grid.cpu().numpy()
    for b, (xyz, f) in enumerate(mols):
        ref = c_oracle.voxelize(xyz, f, 1.2, dimension=D, density=density)
        if density == "binary":
            assert_exact(out[b], ref)
        else:
            assert_gaussian(out[b], ref)
    host = flat.cpu().numpy()
    assert (host[:guard + shift] == 7.0).all() and (host[guard + shift + 2 * per:] == 7.0).all()
    # the same molecules one by one (the one-launch route where it applies), into the slices of the same buffer
    flat.fill_(7.0)
    for route in (0, 1):
        v.debug_option("direct", route)
        for b, (xyz, f) in enumerate(mols):
            v.forward(v.asarray(xyz, "coords"), None, v.asarray(f, "features"), 1.2, out_grid=grid[b])
        assert np.array_equal(grid.cpu().numpy(), out)
    host = flat.cpu().numpy()
    assert (host[:guard + shift] == 7.0).all() and (host[guard + shift + 2 * per:] == 7.0).all()


@pytest.mark.parametrize("D", [30, 49, 70])
def test_channel_wise_features_on_a_grid_of_odd_rows(mv, D):
    """Channel-wise radii grouped by radius (the grouped matrix-core launch) on grids written run by run."""
    from oracle import c_oracle

    rng = np.random.default_rng(D)
    W_ = 0.5 * (D - 1)
    n, C_ = 300, 12
    xyz = rng.uniform(-W_ / 2, W_ / 2, (n, 3))
    f = rng.random((n, C_)).astype(np.float32)
    radii = np.repeat(np.float32([0.9, 1.3, 1.1]), 4)
    v = mv.create_voxelizer(0.5, D, "channel-wise", "gaussian", "hip", output="numpy")
    out = v.forward(xyz, None, f, radii)
    assert_gaussian(out, c_oracle.voxelize(xyz, f, radii, dimension=D, radii_type="channel-wise"))
