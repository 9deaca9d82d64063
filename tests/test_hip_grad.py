"""Backward pass on the GPU (differentiable=True, mvx_backward_batch): feature and coordinate gradients against the float64
reference (tests/grad_reference.py), finite differences at precision 64, the adjoint identity, transforms and centres,
determinism, batch independence, bfloat16 grids, types / single modes and the unchanged default."""
import numpy as np
import pytest

from tests.grad_reference import close as _close
from tests.grad_reference import ref_grads as _ref_grads

pytestmark = pytest.mark.gpu


def _vox(D, radii_type="scalar", density="gaussian", **kw):
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, D, radii_type, density, library="hip", differentiable=True, **kw)


def _molecule(seed, N, D, C_, spread=0.45):
    rng = np.random.default_rng(seed)
    W = 0.5 * (D - 1)
    xyz = rng.uniform(-W * spread, W * spread, (N, 3))
    xyz[0] = [W / 2 + 0.3, 0.0, 0.0]  # reaches past the box edge (box cull, clipped range)
    feats = rng.standard_normal((N, C_)).astype(np.float32)
    return rng, xyz, feats


def _grads_features(vox, xyz, feats, radii, G, **kw):
    import torch

    c = torch.tensor(xyz, device="cuda", requires_grad=True)
    f = torch.tensor(feats, device="cuda", requires_grad=True)
    r = radii if np.isscalar(radii) else torch.tensor(radii, device="cuda")
    grid = vox.forward_features(c, None, f, r, **kw)
    assert grid.grad_fn is not None
    (grid.double() * torch.as_tensor(G, device="cuda")).sum().backward()
    return grid, c.grad.cpu().numpy(), f.grad.cpu().numpy()


CASES = [
    ("scalar", "gaussian", 24, 8, 6), ("scalar", "binary", 24, 8, 6), ("atom-wise", "gaussian", 17, 5, 6),
    ("atom-wise", "binary", 33, 12, 6), ("channel-wise", "gaussian", 20, 8, 6), ("channel-wise", "binary", 25, 5, 6),
    # more than 32 channels: the box is walked once per chunk of 32, the coordinate partials carry across chunks and the
    # last chunk is partial (B = 1)
    ("scalar", "gaussian", 18, 8, 48), ("channel-wise", "gaussian", 17, 5, 71), ("atom-wise", "gaussian", 16, 8, 64),
]


@pytest.mark.parametrize("radii_type, density, D, blockdim, C_", CASES)
def test_feature_and_coordinate_gradients_match_the_oracle(radii_type, density, D, blockdim, C_):
    N = 24
    rng, xyz, feats = _molecule(1, N, D, C_)
    radii = {"scalar": 1.3, "atom-wise": rng.uniform(0.8, 2.0, N).astype(np.float32),
             "channel-wise": rng.choice([0.9, 1.4, 2.0], C_).astype(np.float32)}[radii_type]
    if radii_type == "channel-wise" and C_ > 32:
        radii[40] = 2.3  # the largest radius (the cull's) only in the second chunk
    G = rng.standard_normal((C_, D, D, D))
    vox = _vox(D, radii_type, density, blockdim=blockdim)
    _, gc, gf = _grads_features(vox, xyz, feats, radii, G.astype(np.float32))
    gw, bw, gp, bp = _ref_grads(xyz, feats, radii, radii_type, G.astype(np.float32).astype(np.float64), D, density, blockdim)
    _close(gf, gw, bw, "dL/dfeatures")
    if density == "binary":
        assert np.array_equal(gc, np.zeros_like(gc))
    else:
        _close(gc, gp, bp, "dL/dcoords")


def test_binary_density_with_unit_upstream_counts_voxels_exactly():
    from oracle import c_oracle

    D, N, C_ = 21, 30, 3
    rng, xyz, feats = _molecule(2, N, D, C_)
    vox = _vox(D, "scalar", "binary", blockdim=5)
    _, gc, gf = _grads_features(vox, xyz, feats, 1.1, np.ones((C_, D, D, D), np.float32))
    counts = [c_oracle.voxelize(xyz[n:n + 1], None, 1.1, dimension=D, blockdim=5, density="binary").sum() for n in range(N)]
    assert np.array_equal(gf, np.repeat(np.array(counts, np.float32)[:, None], C_, 1))
    assert not np.any(gc)


@pytest.mark.parametrize("radii_type, C_", [("scalar", 3), ("channel-wise", 3), ("channel-wise", 40)])
def test_finite_differences_at_precision_64(radii_type, C_):
    """Channel-wise radii at precision 64 take their own per-channel table (grad_chan_kernel<double>)."""
    import torch

    D, N = 20, 6
    rng, xyz, feats = _molecule(3, N, D, C_, spread=0.3)
    feats = feats.astype(np.float64)
    radii = 1.2 if radii_type == "scalar" else torch.as_tensor(rng.choice([0.9, 1.2, 1.6], C_), device="cuda")
    G = torch.as_tensor(rng.standard_normal((C_, D, D, D)), device="cuda")
    vox = _vox(D, radii_type, precision=64)
    c = torch.tensor(xyz, device="cuda", requires_grad=True)
    f = torch.tensor(feats, device="cuda", requires_grad=True)
    grid = vox.forward_features(c, None, f, radii)
    (grid * G).sum().backward()
    an = c.grad.cpu().numpy()
    # feature gradients by the adjoint identity, per channel: <grid_c, G_c> = sum_n F[n,c] dL/dF[n,c]
    lhs = (grid.detach() * G).sum(dim=(1, 2, 3))
    rhs = (f.detach() * f.grad).sum(0)
    assert torch.allclose(lhs, rhs, rtol=1e-12, atol=1e-12 * float((grid.detach().abs() * G.abs()).sum()))
    plain = _vox(D, radii_type, precision=64)
    ones = torch.ones((1, C_), dtype=torch.float64, device="cuda")

    def support(x):  # where atom n alone reaches, channel by channel
        return (plain.forward_features(torch.tensor(x, device="cuda"), None, ones, radii) != 0).cpu()

    h = 1e-6
    checked = 0
    for n in range(N):
        base = support(xyz[n:n + 1])
        for i in range(3):
            out = []
            for sgn in (1, -1):
                x = xyz.copy()
                x[n, i] += sgn * h
                full = plain.forward_features(torch.tensor(x, device="cuda"), None, torch.tensor(feats, device="cuda"), radii)
                out.append((support(x[n:n + 1]), float((full * G).sum())))
            if not (torch.equal(out[0][0], base) and torch.equal(out[1][0], base)):
                continue  # the support moved: the a.e. derivative does not see the jump
            fd = (out[0][1] - out[1][1]) / (2 * h)
            assert abs(fd - an[n, i]) <= 1e-6 * max(abs(an[n, i]), 1.0), (n, i, fd, an[n, i])
            checked += 1
    assert checked >= 12


@pytest.mark.parametrize("precision", [32, 64])
def test_adjoint_identity_for_features(precision):
    import torch

    D, N, C_ = 19, 40, 5
    rng, xyz, feats = _molecule(4, N, D, C_)
    vox = _vox(D, precision=precision)
    tdt = torch.float32 if precision == 32 else torch.float64
    f = torch.tensor(feats, device="cuda", dtype=tdt, requires_grad=True)
    G = torch.as_tensor(rng.standard_normal((C_, D, D, D)), device="cuda", dtype=tdt)
    grid = vox.forward_features(torch.tensor(xyz, device="cuda"), None, f, 1.4)
    (grid * G).sum().backward()
    lhs = float((grid.detach().double() * G.double()).sum())
    rhs = float((f.detach().double() * f.grad.double()).sum())
    tol = 1e-5 if precision == 32 else 1e-12
    assert abs(lhs - rhs) <= tol * float((grid.detach().double().abs() * G.double().abs()).sum()), (lhs, rhs)


def _rotation(q):
    q0, q1, q2, q3 = q
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def test_transforms_and_centres():
    import torch

    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform
    from molvoxel_amd.voxelizer.hip.voxelizer import transform_on_device

    D, N, C_ = 24, 30, 4
    rng, xyz, feats = _molecule(5, N, D, C_, spread=0.25)
    cen = np.array([0.3, -0.2, 0.1])
    G = torch.as_tensor(rng.standard_normal((C_, D, D, D)), device="cuda", dtype=torch.float32)
    vox = _vox(D)
    np.random.seed(11)
    c = torch.tensor(xyz, device="cuda", requires_grad=True)
    ct = torch.tensor(cen, device="cuda", requires_grad=True)
    f = torch.tensor(feats, device="cuda")
    grid = vox.forward_features(c, ct, f, 1.3, random_translation=0.7, random_rotation=True)
    state = np.random.get_state()[1].copy()
    (grid * G).sum().backward()
    # the same call without the option: same grid, same RNG state
    import molvoxel_amd as mv

    plain = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    np.random.seed(11)
    g0 = plain.forward_features(torch.tensor(xyz, device="cuda"), torch.tensor(cen, device="cuda"), f, 1.3,
                                random_translation=0.7, random_rotation=True)
    assert torch.equal(grid.detach(), g0) and np.array_equal(np.random.get_state()[1], state)
    # gradient at the transformed positions (the records' own bits), then M^T
    np.random.seed(11)
    t, q = draw_forward_transform(0.7, True)
    p = transform_on_device(torch.tensor(xyz, device="cuda") - torch.tensor(cen, device="cuda"), None, t, q)
    pp = p.clone().requires_grad_(True)
    g1 = vox.forward_features(pp, None, f, 1.3)
    assert torch.equal(g1.detach(), g0)
    (g1 * G).sum().backward()
    want = pp.grad.cpu().numpy() @ _rotation(np.asarray(q, np.float64))  # M^T g for every row
    got = c.grad.cpu().numpy()
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    assert torch.equal(ct.grad, -c.grad.sum(0))
    # a numpy centre is accepted and gets no gradient
    c2 = torch.tensor(xyz, device="cuda", requires_grad=True)
    vox.forward_features(c2, cen, f, 1.3).sum().backward()
    assert c2.grad is not None


def test_determinism_and_batch_independence():
    import torch

    D, C_ = 22, 32
    sizes = [17, 0, 25, 9]
    rng = np.random.default_rng(6)
    W = 0.5 * (D - 1)
    mols = [rng.uniform(-W * 0.45, W * 0.45, (n, 3)) for n in sizes]
    feats = [rng.standard_normal((n, C_)).astype(np.float32) for n in sizes]
    G = torch.as_tensor(rng.standard_normal((len(sizes), C_, D, D, D)), device="cuda", dtype=torch.float32)
    vox = _vox(D, blockdim=8)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cen = torch.as_tensor(rng.uniform(-0.5, 0.5, (len(sizes), 3)), device="cuda")

    def batched():
        c = torch.tensor(np.concatenate(mols), device="cuda", requires_grad=True)
        f = torch.tensor(np.concatenate(feats), device="cuda", requires_grad=True)
        ce = cen.clone().requires_grad_(True)
        grid = vox.forward_batch(c, offsets, ce, f, 1.2)
        (grid * G).sum().backward()
        return grid.detach(), c.grad, f.grad, ce.grad

    a, b = batched(), batched()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for i, n in enumerate(sizes):
        c = torch.tensor(mols[i], device="cuda", requires_grad=True)
        f = torch.tensor(feats[i], device="cuda", requires_grad=True)
        ce = cen[i].clone().requires_grad_(True)
        grid = vox.forward_features(c, ce, f, 1.2)
        (grid * G[i]).sum().backward()
        if n:  # (the library's outputs bit for bit; the centre's torch reduction to rounding)
            assert torch.equal(c.grad, a[1][offsets[i]:offsets[i + 1]])
            assert torch.equal(f.grad, a[2][offsets[i]:offsets[i + 1]])
            assert torch.allclose(ce.grad, a[3][i], rtol=1e-12, atol=1e-12 * float(c.grad.abs().sum()))
        else:
            assert not torch.any(a[3][i])


def test_bfloat16_upstream_equals_its_float32_widening():
    import torch

    D, N, C_ = 24, 50, 8
    rng, xyz, feats = _molecule(7, N, D, C_)
    G16 = torch.as_tensor(rng.standard_normal((C_, D, D, D)), device="cuda").to(torch.bfloat16)
    out = []
    for gd in ("bfloat16", None):
        vox = _vox(D, grid_dtype=gd)
        c = torch.tensor(xyz, device="cuda", requires_grad=True)
        f = torch.tensor(feats, device="cuda", requires_grad=True)
        grid = vox.forward_features(c, None, f, 1.3)
        grid.backward(G16 if gd else G16.float())
        out.append((c.grad, f.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("mode, radii_type", [("types", "scalar"), ("types", "atom-wise"), ("types", "channel-wise"),
                                              ("single", "scalar"), ("single", "atom-wise")])
def test_types_and_single_modes_give_coordinate_gradients(mode, radii_type):
    import torch

    D, N, C_ = 23, 28, 4
    rng, xyz, _ = _molecule(8, N, D, C_)
    types = rng.integers(0, C_, N)
    if radii_type != "channel-wise":
        types[3] = C_ + 2  # beyond the channels of the call (num_channels): ignored, as the forward does
    nch = C_ if mode == "types" else 1
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(0.8, 2.0, N).astype(np.float32),
             "channel-wise": rng.choice([1.0, 1.6], C_).astype(np.float32)}[radii_type]
    G = rng.standard_normal((nch, D, D, D)).astype(np.float32)
    vox = _vox(D, radii_type, blockdim=8)
    c = torch.tensor(xyz, device="cuda", requires_grad=True)
    r = radii if np.isscalar(radii) else torch.tensor(radii, device="cuda")
    if mode == "types":
        grid = vox.forward_batch(c, np.array([0, N]), None, torch.tensor(types, device="cuda"), r, num_channels=C_)[0]
    else:
        grid = vox.forward_single(c, None, r)
    assert grid.grad_fn is not None and tuple(grid.shape) == (nch, D, D, D)
    (grid * torch.as_tensor(G, device="cuda")).sum().backward()
    rad = np.asarray(radii)[types] if radii_type == "channel-wise" else radii  # (types mode gathers radii[type])
    rt = "scalar" if np.isscalar(rad) else "atom-wise"
    _, _, gp, bp = _ref_grads(xyz, None, rad, rt, G.astype(np.float64), D, "gaussian", 8, wmode=mode, types=types)
    _close(c.grad.cpu().numpy(), gp, bp, "dL/dcoords")


def test_default_paths_are_unchanged():
    import torch

    import molvoxel_amd as mv

    D, N, C_ = 24, 40, 4
    rng, xyz, feats = _molecule(9, N, D, C_)
    plain = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    diff = _vox(D)
    c = torch.tensor(xyz, device="cuda", requires_grad=True)
    f = torch.tensor(feats, device="cuda")
    g_plain = plain.forward_features(c, None, f, 1.3)
    assert g_plain.grad_fn is None
    g_nograd = diff.forward_features(c.detach(), None, f, 1.3)
    assert g_nograd.grad_fn is None and torch.equal(g_nograd, g_plain)
    with torch.no_grad():
        assert diff.forward_features(c, None, f, 1.3).grad_fn is None
    g = diff.forward_features(c, None, f, 1.3)
    assert g.grad_fn is not None and torch.equal(g.detach(), g_plain)
    with pytest.raises(ValueError, match="out_grid"):
        diff.forward_features(c, None, f, 1.3, out_grid=torch.empty_like(g_plain))
    with pytest.raises(NotImplementedError, match="device"):
        diff.forward_features(torch.tensor(xyz, requires_grad=True), None, feats, 1.3)
    rv = _vox(D, "atom-wise")
    with pytest.raises(NotImplementedError, match="radii"):
        rv.forward_features(c, None, f, torch.full((N,), 1.2, device="cuda", requires_grad=True))


def test_headline_shape_spot_check():
    import torch

    D, N, C_, B = 64, 4000, 32, 4
    rng = np.random.default_rng(10)
    W = 0.5 * (D - 1)
    xyz = [rng.uniform(-W / 2, W / 2, (N, 3)) for _ in range(B)]
    feats = [rng.random((N, C_)).astype(np.float32) for _ in range(B)]
    G = torch.as_tensor(rng.standard_normal((B, C_, D, D, D)), device="cuda", dtype=torch.float32)
    vox = _vox(D)
    c = torch.tensor(np.concatenate(xyz), device="cuda", requires_grad=True)
    f = torch.tensor(np.concatenate(feats), device="cuda", requires_grad=True)
    grid = vox.forward_batch(c, np.arange(B + 1) * N, None, f, 1.0)
    (grid * G).sum().backward()
    gc, gf = c.grad.cpu().numpy(), f.grad.cpu().numpy()
    Gn = G.cpu().numpy().astype(np.float64)
    for b in (0, B - 1):
        pick = rng.choice(N, 25, replace=False)
        sub = xyz[b][pick]
        gw, bw, gp, bp = _ref_grads(sub, feats[b][pick], 1.0, "scalar", Gn[b], D, "gaussian", None)
        _close(gf[b * N + pick], gw, bw, "dL/dfeatures")
        _close(gc[b * N + pick], gp, bp, "dL/dcoords")


def test_overlapped_batches_still_synchronise_on_converted_centres(monkeypatch):
    """differentiable=False, overlap_prepass=True: a float32 centre tensor is converted to float64 on the caller's stream,
    and the library's side stream reads the copy by pointer, so the call must make the caller's stream complete first."""
    import torch

    import molvoxel_amd as mv

    D, C_, sizes = 24, 4, [20, 15, 18]
    rng = np.random.default_rng(12)
    coords = torch.as_tensor(rng.uniform(-5, 5, (sum(sizes), 3)), device="cuda")
    feats = torch.as_tensor(rng.random((sum(sizes), C_)).astype(np.float32), device="cuda")
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cen32 = torch.as_tensor(rng.uniform(-0.5, 0.5, (3, 3)).astype(np.float32), device="cuda")
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", overlap_prepass=True)
    ref = vox.forward_batch(coords, offsets, cen32.double(), feats, 1.3).clone()
    torch.cuda.synchronize()
    calls = []
    real = torch.cuda.Stream.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append(1), real(self))[1])
    grid = vox.forward_batch(coords, offsets, cen32, feats, 1.3)
    assert calls, "the converted centre was handed to the side stream without a synchronisation"
    assert torch.equal(grid, ref)


def test_processing_order_does_not_change_the_gradients():
    """The caller's order (default) and the spatial order ("grad_order" 1) run atoms on other waves; the results are the same bits."""
    import torch

    D, C_, sizes = 32, 40, [300, 1, 257, 0, 120]
    rng = np.random.default_rng(13)
    W = 0.5 * (D - 1)
    coords = torch.as_tensor(rng.uniform(-W * 0.5, W * 0.5, (sum(sizes), 3)), device="cuda")
    feats = torch.as_tensor(rng.standard_normal((sum(sizes), C_)).astype(np.float32), device="cuda")
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    G = torch.randn((len(sizes), C_, D, D, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    out = []
    for order in (1, 0):
        vox = _vox(D, blockdim=12)
        vox.debug_option("grad_order", order)
        c, f = coords.clone().requires_grad_(True), feats.clone().requires_grad_(True)
        grid = vox.forward_batch(c, offsets, None, f, 1.5)
        (grid * G).sum().backward()
        out.append((c.grad, f.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("change", ["density", "sigma", "radii_type"])
def test_settings_changed_between_forward_and_backward_raise(change):
    """The backward reads the voxelizer's density, sigma and radii type: a change after the forward call is an error, not
    the gradients of another grid. Settings restored before backward() give the forward's gradients."""
    import torch

    D, N, C_ = 20, 12, 3
    rng, xyz, feats = _molecule(14, N, D, C_)
    G = torch.as_tensor(rng.standard_normal((C_, D, D, D)), device="cuda", dtype=torch.float32)
    radii = torch.tensor(rng.uniform(0.9, 1.5, N).astype(np.float32), device="cuda")
    sigma = 0.7 if change == "sigma" else 0.5

    def forward(vox):
        c = torch.tensor(xyz, device="cuda", requires_grad=True)
        return c, vox.forward_features(c, None, torch.tensor(feats, device="cuda"), radii)

    def mutate(vox):
        if change == "density":
            vox.density_type = "binary"
        elif change == "sigma":
            vox.density_type = "gaussian"  # (the setter falls back to the default sigma, 0.5)
        else:
            vox.radii_type = "scalar"

    vox = _vox(D, "atom-wise", sigma=sigma)
    c, grid = forward(vox)
    mutate(vox)
    with pytest.raises(RuntimeError, match="changed between the forward call and backward"):
        grid.backward(G)
    if change == "sigma":
        return
    c0, g0 = forward(_vox(D, "atom-wise"))
    g0.backward(G)
    vox = _vox(D, "atom-wise")
    c, grid = forward(vox)
    mutate(vox)
    vox.density_type, vox.radii_type = "gaussian", "atom-wise"
    grid.backward(G)
    assert torch.equal(c.grad, c0.grad) and c.grad.any()
