"""Channels-last (NDHWC) grids on the GPU: `grid_layout="channels_last"` writes the strides of torch.channels_last_3d straight
from the voxelize kernels. The contract is bit identity with the contiguous-layout voxelizer on the same inputs (only addresses
differ), every element written once per call, and - so that the feature is pinned to the reference and not only to its sibling
path - the CPU oracle under tests/tolerance.py."""
import zlib

import numpy as np
import pytest

from tests import goldens
from tests.test_hip_fuzz import _draw
from tests.tolerance import assert_gaussian, assert_north_star

pytestmark = pytest.mark.gpu

CL = "channels_last"


def _pair(res, D, radii_type, density, **kw):
    """(contiguous-layout voxelizer, channels-last voxelizer) with the same settings."""
    import molvoxel_amd as mv

    a = mv.create_voxelizer(res, D, radii_type, density, library="hip", **kw)
    b = mv.create_voxelizer(res, D, radii_type, density, library="hip", grid_layout=CL, **kw)
    assert a.grid_layout == "contiguous" and b.grid_layout == CL
    return a, b


def _molecule(rng, D, res, n, C_):
    W = res * (D - 1)
    xyz = rng.uniform(-W / 2 - 1.0, W / 2 + 1.0, (n, 3))
    feats = rng.random((n, C_)).astype(np.float32)
    feats[rng.random((n, C_)) < 0.2] = 0.0
    types = rng.integers(0, C_, n).astype(np.int16)
    if n:
        types[0] = C_ - 1
    return xyz, feats, types


def _radii(rng, radii_type, n, C_, res):
    s = res / 0.5
    return {"scalar": 1.0 * s, "atom-wise": (rng.uniform(0.7, 1.6, n) * s).astype(np.float32),
            "channel-wise": (rng.uniform(0.7, 1.6, C_) * s).astype(np.float32)}[radii_type]


def _is_cl(g):
    import torch

    return (g if g.dim() == 5 else g.unsqueeze(0)).is_contiguous(memory_format=torch.channels_last_3d)


def _same(g_cl, g):
    import torch

    assert g_cl.shape == g.shape and g_cl.dtype == g.dtype
    assert not torch.isnan(g_cl.float()).any()
    assert torch.equal(g_cl, g)
    assert torch.equal(g_cl.contiguous(), g)


def _single_both(a, b, mode, xyz, chan, radii, center=None, routes=(0, 1), **kw):
    """The same per-molecule call on both voxelizers, on each route; the channels-last grid is pre-filled with NaN."""
    import torch

    outs = []
    for direct in routes:
        a.debug_option("direct", direct)
        b.debug_option("direct", direct)
        to = lambda v, x, what: None if x is None else (x if np.isscalar(x) else v.asarray(x, what))  # noqa: E731
        what = {"features": "features", "types": "types", "single": None}[mode]
        g = a.forward(to(a, xyz, "coords"), to(a, center, "center"), None if chan is None else to(a, chan, what), to(a, radii, "radii"), **kw)
        out = b.get_empty_grid(g.shape[0])
        out.fill_(float("nan"))
        g_cl = b.forward(to(b, xyz, "coords"), to(b, center, "center"), None if chan is None else to(b, chan, what), to(b, radii, "radii"),
                         out_grid=out, **kw)
        assert g_cl is out and g_cl.data_ptr() == out.data_ptr()
        assert _is_cl(g_cl) and tuple(g_cl.shape) == tuple(g.shape)
        _same(g_cl, g)
        outs.append(g_cl)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "the two routes disagree"
    return outs[0]


def _batch_both(a, b, mode, mols, radii_type, C_, rng, res, routes=(0,)):
    import torch

    coords = np.concatenate([m[0] for m in mols])
    offsets = np.cumsum([0] + [m[0].shape[0] for m in mols]).astype(np.int64)
    chan = None if mode == "single" else np.concatenate([m[1] if mode == "features" else m[2] for m in mols])
    radii = _radii(rng, radii_type, coords.shape[0], C_, res)
    B = len(mols)
    for direct in routes:
        res_ = []
        for v in (a, b):
            v.debug_option("direct", direct)
            ch = None if chan is None else v.asarray(chan, mode)
            r = radii if np.isscalar(radii) else v.asarray(radii, "radii")
            out = v.get_empty_grid(C_, batch_size=B)
            out.fill_(float("nan"))
            g = v.forward_batch(v.asarray(coords, "coords"), offsets, None, ch, r, num_channels=C_, out_grid=out)
            assert g is out
            res_.append(g)
        g, g_cl = res_
        assert g_cl.is_contiguous(memory_format=torch.channels_last_3d) or C_ == 1
        assert tuple(g_cl.shape) == (B, C_) + (a.dimension,) * 3
        _same(g_cl, g)
    return g_cl


# ---- layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [None, "bfloat16"])
def test_strides_and_allocation(dtype):
    import torch

    D, C_, B = 16, 8, 3
    a, b = _pair(0.5, D, "scalar", "gaussian", grid_dtype=dtype)
    e = b.get_empty_grid(C_)
    assert tuple(e.shape) == (C_, D, D, D) and e.stride() == (1, D * D * C_, D * C_, C_)
    assert e.unsqueeze(0).is_contiguous(memory_format=torch.channels_last_3d)
    eb = b.get_empty_grid(C_, batch_size=B)
    ref = torch.empty((B, C_, D, D, D), memory_format=torch.channels_last_3d)
    assert tuple(eb.shape) == tuple(ref.shape) and eb.stride() == ref.stride() and eb.dtype == b.grid_dtype
    z = b.get_empty_grid(C_, batch_size=B, init_zero=True)
    assert z.stride() == ref.stride() and not z.any()
    assert not b.get_empty_grid(C_, init_zero=True).any()
    assert a.get_empty_grid(C_, batch_size=B).is_contiguous()
    rng = np.random.default_rng(1)
    xyz, feats, _ = _molecule(rng, D, 0.5, 60, C_)
    g = b.forward_features(b.asarray(xyz, "coords"), None, b.asarray(feats, "features"), 1.0)
    assert tuple(g.shape) == (C_, D, D, D) and g.stride() == (1, D * D * C_, D * C_, C_)
    assert g.unsqueeze(0).is_contiguous(memory_format=torch.channels_last_3d)
    off = np.array([0, 20, 20, 60], np.int64)
    gb = b.forward_batch(b.asarray(xyz, "coords"), off, None, b.asarray(feats, "features"), 1.0)
    assert tuple(gb.shape) == (B, C_, D, D, D) and gb.is_contiguous(memory_format=torch.channels_last_3d)
    # a channels-last out_grid is written in place; any other out_grid takes the copy path and still gets the values
    out = torch.full((B, C_, D, D, D), float("nan"), dtype=b.grid_dtype, device=b.device).contiguous(memory_format=torch.channels_last_3d)
    ptr = out.data_ptr()
    got = b.forward_batch(b.asarray(xyz, "coords"), off, None, b.asarray(feats, "features"), 1.0, out_grid=out)
    assert got is out and out.data_ptr() == ptr and torch.equal(out, gb)
    plain = torch.full((B, C_, D, D, D), float("nan"), dtype=b.grid_dtype, device=b.device)
    got = b.forward_batch(b.asarray(xyz, "coords"), off, None, b.asarray(feats, "features"), 1.0, out_grid=plain)
    assert got is plain and plain.is_contiguous() and torch.equal(plain, gb)
    assert not gb[1].any()  # the empty molecule: zeros, written
    want = a.forward_batch(a.asarray(xyz, "coords"), off, None, a.asarray(feats, "features"), 1.0)
    _same(gb, want)


def test_setter_rejects_precision_64_on_a_live_handle():
    import molvoxel_amd as mv
    from molvoxel_amd.voxelizer.hip import _lib

    v = mv.create_voxelizer(0.5, 16, precision=64)
    assert v._lib.mvx_set_grid_layout(v._handle, _lib.MVX_LAYOUT_NDHWC) == -1
    assert "precision" in v._lib.mvx_last_error().decode()
    assert v._lib.mvx_set_grid_layout(v._handle, 2) == -1
    assert v._lib.mvx_set_grid_layout(v._handle, _lib.MVX_LAYOUT_NCDHW) == 0


# ---- bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [None, "bfloat16"])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("mode, radii_type", [("features", "scalar"), ("features", "atom-wise"), ("features", "channel-wise"),
                                              ("types", "scalar"), ("types", "atom-wise"), ("types", "channel-wise"),
                                              ("single", "scalar"), ("single", "atom-wise")])
def test_modes_densities_and_radii_types(mode, radii_type, density, dtype):
    D, res, n = 32, 0.5, 400
    for C_ in ((1,) if mode == "single" else (8, 5)):
        rng = np.random.default_rng(zlib.crc32(f"{mode} {radii_type} {density} {C_}".encode()))
        a, b = _pair(res, D, radii_type, density, grid_dtype=dtype)
        xyz, feats, types = _molecule(rng, D, res, n, C_)
        chan = {"features": feats, "types": types, "single": None}[mode]
        _single_both(a, b, mode, xyz, chan, _radii(rng, radii_type, n, C_, res), center=rng.uniform(-1, 1, 3))
        mols = [_molecule(rng, D, res, k, C_) for k in (150, 0, 300)]
        _batch_both(a, b, mode, mols, radii_type, C_, rng, res, routes=(0, 1))


@pytest.mark.parametrize("dtype", [None, "bfloat16"])
@pytest.mark.parametrize("C_", [1, 4, 5, 8, 16, 32, 33, 64, 65, 72])
def test_channel_counts(C_, dtype):
    """Single chunks, remainder chunks (33 = 32 + 1, 65 = 64 + 1, 72 = 64 + 8) and several full chunks; B = 3 batches on the
    binned route (and on the one-launch route where it applies), per-molecule calls on both."""
    D, res = 32, 0.5
    rng = np.random.default_rng(100 + C_)
    a, b = _pair(res, D, "scalar", "gaussian", grid_dtype=dtype)
    mols = [_molecule(rng, D, res, k, C_) for k in (500, 0, 200)]
    _batch_both(a, b, "features", mols, "scalar", C_, rng, res, routes=(0, 1))
    xyz, feats, types = _molecule(rng, D, res, 300, C_)
    _single_both(a, b, "features", xyz, feats, 1.0)
    if C_ in (33, 72):  # channel-wise radii: the grouped launch, chunks of 32 with a partial last chunk
        a, b = _pair(res, D, "channel-wise", "gaussian", grid_dtype=dtype)
        _batch_both(a, b, "features", mols, "channel-wise", C_, rng, res, routes=(0,))


@pytest.mark.parametrize("dtype", [None, "bfloat16"])
@pytest.mark.parametrize("D", [16, 48, 49, 63, 64, 72, 96])
def test_dimensions(D, dtype):
    res = 0.5
    rng = np.random.default_rng(200 + D)
    for C_, B in ((32, 2), (4, 3), (5, 2)):
        if D >= 72 and C_ == 32:
            B = 1
        a, b = _pair(res, D, "scalar", "gaussian", grid_dtype=dtype)
        n = int(4000 * ((D - 1) / 63.0) ** 3 / 4)
        mols = [_molecule(rng, D, res, n, C_) for _ in range(B)]
        _batch_both(a, b, "features", mols, "scalar", C_, rng, res, routes=(0, 1))
        _single_both(a, b, "features", mols[0][0], mols[0][1], 1.0)


@pytest.mark.parametrize("dtype", [None, "bfloat16"])
@pytest.mark.parametrize("blockdim", [8, 5, 12])
def test_blockdims(blockdim, dtype):
    D, res = 40, 0.5
    rng = np.random.default_rng(300 + blockdim)
    for C_, radii_type in ((32, "scalar"), (8, "atom-wise"), (33, "scalar"), (40, "channel-wise")):
        a, b = _pair(res, D, radii_type, "gaussian", grid_dtype=dtype, blockdim=blockdim)
        xyz, feats, types = _molecule(rng, D, res, 600, C_)
        _single_both(a, b, "features", xyz, feats, _radii(rng, radii_type, 600, C_, res))
        mols = [_molecule(rng, D, res, k, C_) for k in (400, 30, 0)]
        _batch_both(a, b, "features", mols, radii_type, C_, rng, res, routes=(0, 1))


@pytest.mark.parametrize("seed", range(6))
def test_random_transforms(seed):
    D, res, C_ = 32, 0.5, (32, 8, 5)[seed % 3]
    rng = np.random.default_rng(400 + seed)
    a, b = _pair(res, D, "scalar", "gaussian", grid_dtype="bfloat16" if seed % 2 else None)
    xyz, feats, _ = _molecule(rng, D, res, 500, C_)
    center = rng.uniform(-2, 2, 3)
    for direct in (0, 1):
        a.debug_option("direct", direct)
        b.debug_option("direct", direct)
        np.random.seed(seed)
        g = a.forward_features(a.asarray(xyz + center, "coords"), a.asarray(center, "center"), a.asarray(feats, "features"), 1.0, 0.7, True)
        np.random.seed(seed)
        g_cl = b.forward_features(b.asarray(xyz + center, "coords"), b.asarray(center, "center"), b.asarray(feats, "features"), 1.0, 0.7, True)
        assert _is_cl(g_cl)
        _same(g_cl, g)
    offsets = np.array([0, 200, 500], np.int64)
    for v in (a, b):
        np.random.seed(seed + 50)
        v.debug_option("direct", 0)
        out = v.forward_batch(v.asarray(xyz, "coords"), offsets, None, v.asarray(feats, "features"), 1.0, random_translation=0.5,
                              random_rotation=True)
        if v is a:
            want = out
    _same(out, want)


@pytest.mark.parametrize("dtype", [None, "bfloat16"])
@pytest.mark.parametrize("C_", [8, 32, 33])
def test_out_grid_four_bytes_off_alignment(C_, dtype):
    """An out_grid that is dense in the layout but whose base is 4 bytes off 16-byte alignment: written in place, element-wise."""
    import torch

    D, res, B = 24, 0.5, 2
    rng = np.random.default_rng(500 + C_)
    a, b = _pair(res, D, "scalar", "gaussian", grid_dtype=dtype)
    mols = [_molecule(rng, D, res, 300, C_) for _ in range(B)]
    coords = np.concatenate([m[0] for m in mols])
    feats = np.concatenate([m[1] for m in mols])
    offsets = np.array([0, 300, 600], np.int64)
    n = B * C_ * D ** 3
    shift = 4 // torch.empty(0, dtype=b.grid_dtype).element_size()
    for direct in (0, 1):
        a.debug_option("direct", direct)
        b.debug_option("direct", direct)
        want = a.forward_batch(a.asarray(coords, "coords"), offsets, None, a.asarray(feats, "features"), 1.0)
        buf = torch.full((n + 64,), float("nan"), dtype=b.grid_dtype, device=b.device)
        assert buf.data_ptr() % 16 == 0
        out = buf[shift:shift + n].view(B, D, D, D, C_).permute(0, 4, 1, 2, 3)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous(memory_format=torch.channels_last_3d)
        got = b.forward_batch(b.asarray(coords, "coords"), offsets, None, b.asarray(feats, "features"), 1.0, out_grid=out)
        assert got is out
        _same(out, want)
        assert torch.isnan(buf[:shift].float()).all() and torch.isnan(buf[shift + n:].float()).all()  # nothing outside the grid
        one = buf[shift:shift + n // B].view(D, D, D, C_).permute(3, 0, 1, 2)
        one.fill_(float("nan"))
        got = b.forward_features(b.asarray(mols[0][0], "coords"), None, b.asarray(mols[0][1], "features"), 1.0, out_grid=one)
        assert got is one
        _same(one, want[0])


def test_host_output_through_the_c_abi():
    """MVX_HOST outputs are supported in this layout: the staging buffer is written channels-last and copied as it is."""
    from molvoxel_amd.voxelizer.hip import _lib

    D, res, C_ = 16, 0.5, 8
    rng = np.random.default_rng(7)
    a, b = _pair(res, D, "scalar", "gaussian")
    xyz, feats, _ = _molecule(rng, D, res, 100, C_)
    want = a.forward_features(a.asarray(xyz, "coords"), None, a.asarray(feats, "features"), 1.0).cpu().numpy()
    xyz = np.ascontiguousarray(xyz, np.float64)
    host = np.full((D, D, D, C_), np.nan, np.float32)
    rc = b._lib.mvx_forward_features(b._handle, xyz.ctypes.data, feats.ctypes.data, None, 1.0, _lib.MVX_RADII_SCALAR, xyz.shape[0], C_,
                                     None, host.ctypes.data, _lib.MVX_HOST, _lib.MVX_HOST, 0)
    assert rc == 0, b._lib.mvx_last_error()
    assert np.array_equal(host.transpose(3, 0, 1, 2), want)


@pytest.mark.parametrize("seed", range(50))
def test_fuzz_configurations(seed):
    """50 configurations drawn with the generator of tests/test_hip_fuzz.py: both layouts, both routes, both element types."""
    case = _draw(seed)
    if case["N"] == 0 and case["mode"] == "types":
        case["mode"], case["chan"] = "features", np.zeros((0, case["C"]), np.float32)
    extra = {} if case["blockdim"] is None else {"blockdim": case["blockdim"]}
    a, b = _pair(case["res"], case["D"], case["radii_type"], case["density"], sigma=case["sigma"],
                 grid_dtype="bfloat16" if seed % 2 else None, **extra)
    _single_both(a, b, case["mode"], case["xyz"], case["chan"], case["radii"], center=case["center"])


# ---- oracle -----------------------------------------------------------------------------------------------------------------------
Z_SMALL, IDX_SMALL = goldens.load("small_cases.npz")


def _one_golden_per_mode():
    seen, picked = set(), []
    for c in IDX_SMALL:
        ref = Z_SMALL[f"{c['id']}/out"]
        if c["mode"] not in seen and (c["mode"] == "single" or ref.shape[0] > 1):
            seen.add(c["mode"])
            picked.append(c)
    return picked


@pytest.mark.parametrize("case", _one_golden_per_mode(), ids=lambda c: c["id"])
def test_reference_goldens(case):
    import molvoxel_amd as mv

    coords, chan, radii = goldens.small_case_inputs(Z_SMALL, case)
    ref = Z_SMALL[f"{case['id']}/out"]
    extra = {} if case["blockdim"] is None else {"blockdim": case["blockdim"]}
    v = mv.create_voxelizer(case["resolution"], case["dimension"], case["radii_type"], case["density"], library="hip",
                            sigma=case["sigma"], grid_layout=CL, **extra)
    for direct in (0, 1):
        v.debug_option("direct", direct)
        what = {"features": "features", "types": "types", "single": None}[case["mode"]]
        kw = {}
        if case["mode"] == "types":
            kw["out_grid"] = v.get_empty_grid(ref.shape[0])
        g = v.forward(v.asarray(coords, "coords"), None, None if chan is None else v.asarray(chan, what),
                      radii if np.isscalar(radii) else v.asarray(radii, "radii"), **kw)
        assert _is_cl(g)
        out = g.cpu().numpy()
        if case["density"] == "binary" and case["mode"] != "features":
            assert np.array_equal(out, ref)
        else:
            assert_gaussian(out, ref)


@pytest.mark.parametrize("cfg, batch", [("cfg2", 4), ("cfg3", 4)])
def test_benchmark_shapes_against_the_oracle(cfg, batch):
    import torch

    import molvoxel_amd as mv
    from molvoxel_amd import workloads as W
    from oracle import c_oracle

    wl = getattr(W, cfg)(batch=batch)
    v = mv.create_voxelizer(wl.resolution, wl.dimension, wl.radii_type, wl.density, library="hip", sigma=wl.sigma, grid_layout=CL)
    coords = np.concatenate([wl.coords[i] - wl.centers[i] for i in range(batch)])
    offsets = np.cumsum([0] + [wl.coords[i].shape[0] for i in range(batch)]).astype(np.int64)
    chan = v.asarray(np.concatenate([wl.channels[i] for i in range(batch)]), wl.mode)
    radii = wl.radii[0]
    assert np.isscalar(radii)
    out = v.get_empty_grid(wl.num_channels, batch_size=batch)
    out.fill_(float("nan"))
    v.debug_option("direct", 0)
    got = v.forward_batch(v.asarray(coords, "coords"), offsets, None, chan, radii, num_channels=wl.num_channels, out_grid=out)
    assert got is out and out.is_contiguous(memory_format=torch.channels_last_3d) and not torch.isnan(out).any()
    for i in (0, batch - 1):
        ref = c_oracle.voxelize(wl.coords[i] - wl.centers[i].reshape(1, 3), wl.channels[i], wl.radii[i], resolution=wl.resolution,
                                dimension=wl.dimension, radii_type=wl.radii_type, density=wl.density, sigma=wl.sigma,
                                num_channels=wl.num_channels)
        o = out[i].cpu().numpy()
        if wl.density == "binary" and wl.mode != "features":
            assert np.array_equal(o, ref)
        else:
            assert_north_star(o, ref)


# ---- autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radii_type", ["scalar", "atom-wise", "channel-wise"])
def test_backward_matches_the_contiguous_voxelizer_bit_for_bit(radii_type):
    import torch

    D, res, C_, n, B = 24, 0.5, 8, 300, 2
    rng = np.random.default_rng(900)
    a, b = _pair(res, D, radii_type, "gaussian", differentiable=True, radii_grad=True, sigma_grad=True,
                 sigma=torch.tensor(0.6, dtype=torch.float64))
    xyz, feats, _ = _molecule(rng, D, res, n, C_)
    xyz = xyz * 0.6
    offsets = np.array([0, 120, n], np.int64)
    upstream = torch.as_tensor(rng.standard_normal((B, C_, D, D, D)).astype(np.float32), device=a.device)
    upstream_cl = upstream.contiguous(memory_format=torch.channels_last_3d)
    grads = []
    for v, up in ((a, upstream), (b, upstream_cl), (b, upstream)):
        coords = v.asarray(xyz, "coords").requires_grad_()
        f = v.asarray(feats, "features").requires_grad_()
        cen = torch.zeros((B, 3), dtype=torch.float64, device=v.device, requires_grad=True)
        sig = torch.tensor(0.6, dtype=torch.float64, device=v.device, requires_grad=True)
        v.set_sigma(sig)
        if radii_type == "scalar":
            r = torch.tensor([1.1], dtype=torch.float32, device=v.device, requires_grad=True)
        else:
            r = v.asarray(_radii(np.random.default_rng(5), radii_type, n, C_, res), "radii").requires_grad_()
        g = v.forward_batch(coords, offsets, cen, f, r)
        assert g.requires_grad and (v is a or g.is_contiguous(memory_format=torch.channels_last_3d))
        (g * up).sum().backward()
        grads.append([t.grad.clone() for t in (coords, f, cen, r, sig)] + [g.detach()])
    for other in grads[1:]:
        for name, x, y in zip(("coords", "features", "center", "radii", "sigma", "grid"), grads[0], other):
            assert torch.equal(x, y), name


# ---- resources --------------------------------------------------------------------------------------------------------------------
def _kernel_resources():
    """tools/regs.py's table: the grid type is every kernel's last template argument."""
    import os

    from tools import regs

    if not all(os.path.exists(o) for o in regs.KERNEL_OBJECTS):
        pytest.skip("kernel objects not built")
    return regs.kernel_resources()


def test_channels_last_kernels_keep_their_accumulators_in_registers():
    """The write-out stores from registers - no LDS tile, no barrier - so the kernels need no more than their contiguous-layout
    twins: 64 registers (8 waves per SIMD) everywhere; no scratch at all in the narrow kernels and the narrow chunks of the slab
    kernel; the 32-channel matrix-core kernels keep the few registers their twins spill while the first two rounds of rows
    are staged (tests/test_kernel_resources.py: scratch <= 32, <= 6 registers) and nothing more. No 1024-thread variants exist
    in this layout. The per-molecule kernel: the bounds of voxelize_pair_kernel."""
    res = _kernel_resources()
    for tag in (", Ndhwc<float>>", ", Ndhwc<__bf16>>"):
        ks = {k: v for k, v in res.items() if k.startswith("voxelize_kernel<") and k.endswith(tag)}
        assert len(ks) == 24 and all(", 512, " in k for k in ks), sorted(ks)  # 5 widths x {gaussian, binary} x {plain, lane ranges} + 4 grouped
        for name, r in ks.items():
            assert r["vgpr"] <= 64, (name, r)
        for gauss in ("true", "false"):
            for ct in (1, 4, 8, 16):
                r = res[f"voxelize_kernel<{ct}, {gauss}, false, 512, false{tag}"]
                assert r["scratch"] == 0 and r["vspill"] == 0, (tag, ct, gauss, r)
            r = res[f"voxelize_kernel<32, {gauss}, false, 512, false{tag}"]
            twin = res[f"voxelize_kernel<32, {gauss}, false, 512, false, float>"]
            assert r["scratch"] <= 32 and r["vspill"] <= 6, (tag, gauss, r)
            assert r["vspill"] <= twin["vspill"] + 1, (tag, gauss, r, twin)
    for tag in (", Ndhwc<float>>", ", Ndhwc<__bf16>>"):
        ks = {k: v for k, v in res.items() if k.startswith("voxelize_narrow_kernel<") and k.endswith(tag)}
        assert len(ks) == 8  # 1 channel x {2, 4} sub-tiles, 4 and 8 channels x 2, Gaussian and binary
        for name, r in ks.items():
            assert r["vspill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 64, (name, r)
    for tag in (", Ndhwc<float>>", ", Ndhwc<__bf16>>"):
        ks = {k: v for k, v in res.items() if k.startswith("voxelize_pair_kernel<") and k.endswith(tag)}
        assert len(ks) == 30
        for name, r in ks.items():
            assert r["vgpr"] <= 128, (name, r)
            assert r["scratch"] <= (0 if f", false, false{tag}" in name else 128), (name, r)
