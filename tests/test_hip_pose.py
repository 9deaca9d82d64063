"""Explicit rigid poses on the GPU: forward_posed_batch / forward_posed_views / select_posed_views against the random path
(same bits), the oracles on tests/pose_reference.py's positions, the views machinery, and the pose gradients
(mvx_pose_grad_batch) against the float64 reference, the chain rule on the call's own dL/dcoords, determinism and batch
independence. Shapes: D = 16 and 24 at resolution 0.5, three molecules of {0, 1, 300} or {37, 150, 300} atoms (300 is more than
4 waves x 64: a lane of the reduction sees a second chunk), centres around (30, -20, 12), |q| in {1, 0.8, 1.25}."""
import functools

import numpy as np
import pytest

from tests import grad_reference as gr
from tests import pose_reference as pr
from tests import views_reference as vr
from tests import hip_support as hip
from tests.tolerance import (GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL, P64_TOL, assert_exact, assert_gaussian)

pytestmark = pytest.mark.gpu

CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.8, 1.25])
FULL, SPARSE = (37, 150, 300), (0, 1, 300)


def _vox(D, radii_type="scalar", density="gaussian", **kw):
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, D, radii_type, density, library="hip", **kw)


@functools.lru_cache(maxsize=None)
def _data(seed, sizes, D, C_, mode, radii_type, precision=32):
    """One batch: offsets, centres, coordinates around them, poses, channels and radii (host arrays; never modified)."""
    rng = np.random.default_rng(seed)
    fp = np.float32 if precision == 32 else np.float64
    B, N = len(sizes), int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    W = 0.5 * (D - 1)
    cen = CEN + rng.normal(0.0, 0.4, (B, 3))
    xyz = np.concatenate([cen[b] + rng.uniform(-0.4 * W, 0.4 * W, (n, 3)) for b, n in enumerate(sizes)]).reshape(N, 3)
    q = rng.standard_normal((B, 4))
    q *= (NORMS[:B] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": rng.integers(0, C_, N), "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[radii_type]
    return dict(off=off, cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, B=B, N=N)


def _posed(vox, d, mode, C_, device=True, **over):
    """forward_posed_batch on the batch `d`, inputs as device tensors or as numpy arrays."""
    a = {k: over.get(k, d[k]) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    if device:
        a = {k: (v if not isinstance(v, np.ndarray) else hip.dev(v)) for k, v in a.items()}
    return vox.forward_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"],
                                   num_channels=C_ if mode == "types" else None)


def _oracle(p, d, mode, C_, D, radii_type, density, precision):
    from oracle import c_oracle, numpy_port

    out = np.zeros((d["B"], C_, D, D, D), np.float32 if precision == 32 else np.float64)
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            continue
        ch = None if d["chan"] is None else d["chan"][lo:hi]
        r = d["radii"][lo:hi] if radii_type == "atom-wise" else d["radii"]
        nc = C_ if mode == "types" else None
        if precision == 32:
            out[b] = c_oracle.voxelize(p[lo:hi], ch, r, dimension=D, radii_type=radii_type, density=density, num_channels=nc)
        else:
            out[b] = numpy_port.voxelize(numpy_port.GridSpec(0.5, D), p[lo:hi], ch, r, radii_type=radii_type, density=density,
                                         num_channels=nc, precision=64)
    return out


# ---- 1. same bits as the random path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, C_", [("features", 32), ("types", 5)])
@pytest.mark.parametrize("seed", [3, 17])
def test_drawn_quaternions_give_the_random_paths_bits(mode, C_, seed):
    import torch

    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform

    D = 16
    d = _data(1, FULL, D, C_, mode, "scalar")
    vox = _vox(D)
    np.random.seed(seed)
    quats = np.array([draw_forward_transform(0.0, True)[1] for _ in range(d["B"])])
    xyz, cen, chan = hip.dev(d["xyz"]), hip.dev(d["cen"]), hip.dev(d["chan"])
    nc = C_ if mode == "types" else None
    got = vox.forward_posed_batch(xyz, d["off"], cen, hip.dev(quats), torch.zeros((d["B"], 3), device="cuda"), chan, 1.25, num_channels=nc)
    np.random.seed(seed)
    ref = vox.forward_batch(xyz, d["off"], cen, chan, 1.25, num_channels=nc, random_rotation=True)
    assert float(ref.abs().sum()) > 0 and torch.equal(got, ref)


# ---- 2. general poses against the oracle -----------------------------------------------------------------------------------
ORACLE_CASES = [
    # mode, C, radii type, density, precision, sizes, D, direct (None: the plan's choice), device inputs
    ("features", 4, "scalar", "gaussian", 32, FULL, 16, 1, True),
    ("features", 4, "scalar", "gaussian", 32, FULL, 16, 0, True),
    ("features", 32, "atom-wise", "gaussian", 32, SPARSE, 16, 0, True),
    ("features", 33, "channel-wise", "gaussian", 32, FULL, 16, None, False),
    ("features", 4, "channel-wise", "binary", 32, FULL, 24, None, True),
    ("types", 5, "channel-wise", "gaussian", 32, FULL, 24, 1, False),
    ("types", 5, "atom-wise", "binary", 32, SPARSE, 16, 0, True),
    ("single", 1, "scalar", "gaussian", 32, (300,), 16, None, True),   # B = 1: the record is not passed by value
    ("single", 1, "atom-wise", "binary", 32, (37,), 24, None, False),  # B = 1, host inputs: folded on the host
    ("features", 4, "scalar", "gaussian", 64, FULL, 16, None, True),
    ("types", 5, "atom-wise", "gaussian", 64, (150,), 16, None, True),
    ("single", 1, "scalar", "binary", 64, SPARSE, 24, None, False),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, precision, sizes, D, direct, device", ORACLE_CASES)
def test_posed_grids_match_the_oracle_on_the_reference_positions(mode, C_, radii_type, density, precision, sizes, D, direct, device):
    d = _data(2, sizes, D, C_, mode, radii_type, precision)
    vox = _vox(D, radii_type, density, precision=precision)
    if direct is not None:
        vox.debug_option("direct", direct)
    got = _posed(vox, d, mode, C_, device).cpu().numpy()
    if direct is not None:
        assert vox.last_plan()["route"] == direct  # (MVX_ROUTE_DIRECT = 1, MVX_ROUTE_BINNED = 0)
    p = pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])
    ref = _oracle(p, d, mode, C_, D, radii_type, density, precision)
    assert np.count_nonzero(ref) > 0
    if density == "binary" and mode != "features":
        assert_exact(got, ref)
    else:
        assert_gaussian(got, ref, *(() if precision == 32 else (P64_TOL,)))


def test_poses_without_centres_and_in_other_dtypes():
    """centers=None is c = 0; float32 quaternions and float64 translations are widened / rounded as documented."""
    import torch

    D, C_ = 16, 4
    d = _data(2, FULL, D, C_, "features", "scalar")
    vox = _vox(D)
    q32 = d["q"].astype(np.float32)
    shifted = d["xyz"] - np.repeat(d["cen"], np.diff(d["off"]), axis=0)
    got = vox.forward_posed_batch(hip.dev(shifted), d["off"], None, hip.dev(q32), hip.dev(d["t"]), hip.dev(d["chan"]), 1.25)
    ref = _posed(vox, d, "features", C_, True, xyz=shifted, cen=np.zeros((3, 3)), q=q32.astype(np.float64),
                 t=d["t"].astype(np.float32))
    assert torch.equal(got, ref)
    p = pr.batch_positions(shifted, d["off"], None, q32.astype(np.float64), d["t"])
    assert_gaussian(got.cpu().numpy(), _oracle(p, d, "features", C_, D, "scalar", "gaussian", 32))


@pytest.mark.parametrize("kw", [dict(grid_dtype="bfloat16"), dict(grid_layout="channels_last")], ids=["bfloat16", "channels_last"])
def test_other_grid_types_hold_the_float32_posed_grid(kw):
    import torch

    D, C_ = 16, 32
    d = _data(2, FULL, D, C_, "features", "scalar")
    base = _posed(_vox(D), d, "features", C_)
    got = _posed(_vox(D, **kw), d, "features", C_)
    if "grid_dtype" in kw:
        assert got.dtype == torch.bfloat16 and torch.equal(got, base.to(torch.bfloat16))
    else:
        assert got.is_contiguous(memory_format=torch.channels_last_3d)
        assert torch.equal(got, base.contiguous(memory_format=torch.channels_last_3d))


# ---- 3. views --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud(D, C_, mode, radii_type):
    """One shared cloud wider than the box and three poses whose centres lie inside it."""
    rng = np.random.default_rng(9)
    N, B = 300, 3
    xyz = CEN + rng.uniform(-6.0, 6.0, (N, 3))
    cen = CEN + rng.uniform(-2.0, 2.0, (B, 3))
    q = rng.standard_normal((B, 4))
    q *= (NORMS / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    chan = {"features": rng.standard_normal((N, C_)).astype(np.float32), "types": rng.integers(0, C_, N), "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(np.float32),
             "channel-wise": rng.uniform(1.0, 1.5, C_).astype(np.float32)}[radii_type]
    return dict(xyz=xyz, cen=cen, q=q, t=t, chan=chan, radii=radii, N=N, B=B, off=np.arange(B + 1, dtype=np.int64) * N)


def _repeat(c):
    rep = lambda x: None if x is None else np.concatenate([x] * c["B"])  # noqa: E731
    return rep(c["xyz"]), rep(c["chan"]), (rep(c["radii"]) if isinstance(c["radii"], np.ndarray) and c["radii"].shape[0] == c["N"] else c["radii"])


@pytest.mark.parametrize("mode, C_, radii_type, device", [("features", 32, "scalar", True), ("features", 4, "channel-wise", False),
                                                           ("types", 5, "atom-wise", True), ("single", 1, "scalar", False)])
def test_posed_views_equal_the_posed_batch_on_the_repeated_cloud(mode, C_, radii_type, device):
    import torch

    D = 16
    c = _cloud(D, C_, mode, radii_type)
    vox = _vox(D, radii_type)
    conv = hip.dev if device else (lambda x: x)
    nc = C_ if mode == "types" else None
    got = vox.forward_posed_views(conv(c["xyz"]), conv(c["cen"]), conv(c["q"]), conv(c["t"]), conv(c["chan"]), conv(c["radii"]),
                                  num_channels=nc)
    xyz, chan, radii = _repeat(c)
    ref = vox.forward_posed_batch(conv(xyz), c["off"], conv(c["cen"]), conv(c["q"]), conv(c["t"]), conv(chan), conv(radii),
                                  num_channels=nc)
    assert float(ref.abs().sum()) > 0 and torch.equal(got, ref)


@pytest.mark.parametrize("mode, C_, radii_type, source", [("single", 1, "scalar", "scalar"), ("types", 5, "atom-wise", "atom-wise"),
                                                           ("features", 4, "channel-wise", "channel-features")])
def test_posed_selection_is_the_reference_selection(mode, C_, radii_type, source):
    D = 16
    c = _cloud(D, C_, mode, radii_type)
    vox = _vox(D, radii_type)
    index, offsets = vox.select_posed_views(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["q"]), hip.dev(c["t"]), hip.dev(c["chan"]), hip.dev(c["radii"]))
    p = pr.view_positions(c["xyz"], c["cen"], c["q"], c["t"])
    ref_index, ref_offsets = vr.select_exact(p, 0.5, D, source, c["radii"], types=c["chan"] if mode == "types" else None,
                                             num_channels=C_ if mode == "types" else None)
    assert 0 < ref_offsets[-1] < c["B"] * c["N"]  # the cull keeps some atoms and drops some
    assert vr.selection_mismatch(index.cpu().numpy(), np.asarray(offsets), ref_index, ref_offsets) is None


# ---- 4. gradients ----------------------------------------------------------------------------------------------------------
def _upstream(seed, B, C_, D, precision):
    G = np.random.default_rng(seed).standard_normal((B, C_, D, D, D))
    return G.astype(np.float32).astype(np.float64) if precision == 32 else G


@functools.lru_cache(maxsize=None)
def _reference_grads(seed, sizes, D, C_, mode, radii_type, precision):
    """Per molecule: pose_reference.pose_grads from grad_reference.reference on the posed positions (computed once)."""
    d = _data(seed, sizes, D, C_, mode, radii_type, precision)
    G = _upstream(seed, d["B"], C_, D, precision)
    p = pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])
    out = []
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        r = d["radii"][lo:hi] if radii_type == "atom-wise" else d["radii"]
        o = gr.reference(p[lo:hi], G[b], r, radii_type, w=d["chan"][lo:hi] if mode == "features" else None, mode=mode,
                         types=d["chan"][lo:hi] if mode == "types" else None, precision=precision)
        out.append(pr.pose_grads(d["xyz"][lo:hi], d["cen"][b], d["q"][b], *o["coords"]))
    return out


def _pose_backward(vox, d, mode, C_, G, radii=None, pose_dtype=None):
    """One forward_posed_batch + backward with everything that can require grad doing so; returns the tensors."""
    import torch

    pd = pose_dtype or torch.float64
    xyz = hip.dev(d["xyz"], True)
    cen, q, t = (torch.tensor(d[k], device="cuda", dtype=pd, requires_grad=True) for k in ("cen", "q", "t"))
    chan = hip.dev(d["chan"], mode == "features")
    r = d["radii"] if radii is None else radii
    r = r if not isinstance(r, np.ndarray) else hip.dev(r, vox.radii_grad)
    grid = vox.forward_posed_batch(xyz, d["off"], cen, q, t, chan, r, num_channels=C_ if mode == "types" else None)
    assert grid.grad_fn is not None
    (grid.double() * torch.as_tensor(G, device="cuda")).sum().backward()
    return dict(xyz=xyz, cen=cen, q=q, t=t, chan=chan, radii=r, grid=grid)


def _check_against_reference(out, ref, precision, sizes):
    rel, abs_ = (GRAD_REL, GRAD_ABS) if precision == 32 else (GRAD64_REL, GRAD64_ABS)
    worst = 0.0
    for b, o in enumerate(ref):
        for name, key in (("center", "cen"), ("quaternion", "q"), ("translation", "t")):
            val, bound = o[name]
            got = out[key].grad[b].double().cpu().numpy()
            assert sizes[b] < 37 or np.all(val != 0)  # (the comparison is about something)
            worst = max(worst, gr.close(got, val, bound, f"molecule {b} dL/d{name}", rel, abs_))
    return worst


def _check_chain_rule(out, d):
    """The float64 chain rule on the call's own coords.grad: rtol 1e-12, atol 1e-12 * sum |terms| (the centre check's rule)."""
    gc = out["xyz"].grad.cpu().numpy()
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        o = pr.from_coords_grad(d["xyz"][lo:hi], d["cen"][b], d["q"][b], gc[lo:hi])
        for name, key in (("center", "cen"), ("quaternion", "q"), ("translation", "t")):
            val, scale = o[name]
            got = out[key].grad[b].double().cpu().numpy()
            assert np.all(np.abs(got - val) <= 1e-12 * np.abs(val) + 1e-12 * scale), (b, name, got, val)


GRAD_CASES = [("features", 4, "scalar", 32, FULL, 16), ("types", 5, "atom-wise", 32, SPARSE, 16), ("single", 1, "scalar", 64, FULL, 24),
              ("features", 4, "channel-wise", 64, SPARSE, 16)]


@pytest.mark.parametrize("extras", [False, True], ids=["pose-only", "with-radii-and-sigma"])
@pytest.mark.parametrize("mode, C_, radii_type, precision, sizes, D", GRAD_CASES)
def test_pose_gradients_match_the_reference(mode, C_, radii_type, precision, sizes, D, extras):
    import torch

    d = _data(4, sizes, D, C_, mode, radii_type, precision)
    G = _upstream(4, d["B"], C_, D, precision)
    kw = dict(precision=precision, differentiable=True)
    radii = None
    if extras:
        sigma = torch.tensor(0.5, dtype=torch.float64, requires_grad=True)
        kw.update(radii_grad=True, sigma_grad=True, sigma=sigma)
        if radii_type == "scalar":
            radii = torch.tensor([1.25], dtype=torch.float64, requires_grad=True)
    vox = _vox(D, radii_type, **kw)
    out = _pose_backward(vox, d, mode, C_, G, radii)
    for k in ("cen", "q", "t"):
        assert out[k].grad.shape == out[k].shape and out[k].grad.dtype == out[k].dtype
    worst = _check_against_reference(out, _reference_grads(4, sizes, D, C_, mode, radii_type, precision), precision, sizes)
    print(f"{mode} {radii_type} p{precision}: worst |got - ref| / bar = {worst:.3g}")
    _check_chain_rule(out, d)
    if extras:  # the radius and sigma gradients arrive in the same backward, and the pose rows are the same bits without them
        rg = radii.grad if radii is not None else out["radii"].grad
        assert rg is not None and bool(torch.isfinite(rg).all()) and float(rg.abs().sum()) > 0
        assert sigma.grad is not None and float(sigma.grad.abs()) > 0
        plain = _pose_backward(_vox(D, radii_type, precision=precision, differentiable=True), d, mode, C_, G)
        for k in ("cen", "q", "t", "xyz"):
            assert torch.equal(out[k].grad, plain[k].grad), k


def test_pose_gradients_in_the_callers_dtypes():
    """float32 poses: the block holds their values widened, and the gradients come back as float32 tensors."""
    import torch

    D, C_ = 16, 4
    d = _data(4, FULL, D, C_, "features", "scalar")
    G = _upstream(4, d["B"], C_, D, 32)
    vox = _vox(D, differentiable=True)
    out = _pose_backward(vox, d, "features", C_, G, pose_dtype=torch.float32)
    widened = dict(d, **{k: d[k].astype(np.float32).astype(np.float64) for k in ("cen", "q", "t")})
    ref = _pose_backward(vox, widened, "features", C_, G)
    assert torch.equal(out["grid"], ref["grid"])
    for k in ("cen", "q", "t"):
        assert out[k].grad.dtype == torch.float32 and out[k].grad.shape == out[k].shape
        assert torch.equal(out[k].grad, ref[k].grad.to(torch.float32)) and bool(out[k].grad.any())


def test_binary_density_gives_exact_zeros_for_q_and_t():
    D, C_ = 16, 4
    d = _data(4, FULL, D, C_, "features", "scalar")
    out = _pose_backward(_vox(D, "scalar", "binary", differentiable=True), d, "features", C_, _upstream(4, d["B"], C_, D, 32))
    for k in ("q", "t", "cen", "xyz"):
        assert not bool(out[k].grad.any()), k
    assert bool(out["chan"].grad.any())


def test_the_pose_path_leaves_coordinate_and_feature_gradients_as_they_are():
    """coords.grad and features.grad are, bit for bit, forward_batch's on the pre-posed positions (dL/dp transposed back with
    the conjugate quaternion, in the sandwich product's operation order)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _quaternion

    D, C_ = 16, 4
    d = _data(4, FULL, D, C_, "features", "scalar")
    G = _upstream(4, d["B"], C_, D, 32)
    vox = _vox(D, differentiable=True)
    out = _pose_backward(vox, d, "features", C_, G)
    p = torch.tensor(pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"]), device="cuda", requires_grad=True)
    f = hip.dev(d["chan"], True)
    grid = vox.forward_batch(p, d["off"], None, f, 1.25)
    assert torch.equal(grid, out["grid"])
    (grid.double() * torch.as_tensor(G, device="cuda")).sum().backward()
    assert torch.equal(f.grad, out["chan"].grad)
    gp = p.grad.cpu().numpy()
    back = np.empty_like(gp)
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        q0, q1, q2, q3 = (float(v) for v in d["q"][b])
        back[lo:hi] = _quaternion.rotate(gp[lo:hi], (q0, -q1, -q2, -q3))
    assert np.array_equal(out["xyz"].grad.cpu().numpy(), back)


# ---- 5. determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [FULL, SPARSE])
def test_pose_rows_are_deterministic_and_independent_of_the_batch(sizes):
    import torch

    D, C_ = 16, 4
    d = _data(5, sizes, D, C_, "features", "scalar")
    G = _upstream(5, d["B"], C_, D, 32)
    vox = _vox(D, differentiable=True)
    one = _pose_backward(vox, d, "features", C_, G)
    two = _pose_backward(vox, d, "features", C_, G)
    rows = torch.cat([one[k].grad for k in ("cen", "q", "t")], dim=1)
    assert torch.equal(rows, torch.cat([two[k].grad for k in ("cen", "q", "t")], dim=1))
    assert bool(torch.isfinite(rows).all())
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            assert not bool(rows[b].any())  # a molecule without atoms: exact zeros
            continue
        alone = dict(d, off=np.array([0, hi - lo], np.int64), xyz=d["xyz"][lo:hi], chan=d["chan"][lo:hi], cen=d["cen"][b:b + 1],
                     q=d["q"][b:b + 1], t=d["t"][b:b + 1], B=1)
        solo = _pose_backward(vox, alone, "features", C_, G[b:b + 1])
        assert torch.equal(torch.cat([solo[k].grad for k in ("cen", "q", "t")], dim=1)[0], rows[b]), b
        assert bool(rows[b].any())


# ---- 6. views gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, C_, radii_type", [("features", 4, "scalar"), ("types", 5, "atom-wise")])
def test_posed_views_gradients_match_the_repeated_cloud(mode, C_, radii_type):
    import torch

    D = 16
    c = _cloud(D, C_, mode, radii_type)
    G = torch.as_tensor(_upstream(6, c["B"], C_, D, 32), device="cuda")
    vox = _vox(D, radii_type, differentiable=True)
    nc = C_ if mode == "types" else None

    def leaves():
        return [torch.tensor(c[k], device="cuda", requires_grad=True) for k in ("cen", "q", "t")]

    xyz = hip.dev(c["xyz"], True)
    cen, q, t = leaves()
    grid = vox.forward_posed_views(xyz, cen, q, t, hip.dev(c["chan"]), hip.dev(c["radii"]), num_channels=nc)
    (grid.double() * G).sum().backward()
    rx, rchan, rradii = _repeat(c)
    xyz2 = hip.dev(rx, True)
    cen2, q2, t2 = leaves()
    grid2 = vox.forward_posed_batch(xyz2, c["off"], cen2, q2, t2, hip.dev(rchan), hip.dev(rradii), num_channels=nc)
    assert torch.equal(grid, grid2)
    (grid2.double() * G).sum().backward()
    gc2 = xyz2.grad.cpu().numpy().reshape(c["B"], c["N"], 3)
    for b in range(c["B"]):  # each view's pose: its own gradient, within the summation-order rule
        o = pr.from_coords_grad(c["xyz"], c["cen"][b], c["q"][b], gc2[b])
        for name, got, ref in (("center", cen, cen2), ("quaternion", q, q2), ("translation", t, t2)):
            a, r = got.grad[b].cpu().numpy(), ref.grad[b].cpu().numpy()
            assert np.any(r != 0)
            assert np.all(np.abs(a - r) <= 1e-12 * np.abs(r) + 1e-12 * o[name][1]), (b, name, a, r)
    # the shared cloud: the views' per-atom gradients summed
    total, scale = gc2.sum(0), np.abs(gc2).sum(0)
    assert np.all(np.abs(xyz.grad.cpu().numpy() - total) <= 1e-12 * np.abs(total) + 1e-12 * scale)


# ---- 7. no host visit ------------------------------------------------------------------------------------------------------
def test_device_poses_never_visit_the_host():
    import torch

    D, C_ = 16, 4
    d = _data(7, FULL, D, C_, "features", "scalar")
    G = torch.as_tensor(_upstream(7, d["B"], C_, D, 32), device="cuda", dtype=torch.float32)
    vox = _vox(D, differentiable=True)
    xyz, chan = hip.dev(d["xyz"]), hip.dev(d["chan"])

    def step():
        cen, q, t = (torch.tensor(d[k], device="cuda", requires_grad=True) for k in ("cen", "q", "t"))
        torch.cuda.synchronize()
        return cen, q, t

    def run(cen, q, t):
        grid = vox.forward_posed_batch(xyz, d["off"], cen, q, t, chan, 1.25)
        (grid * G).sum().backward()

    ref = step()
    run(*ref)  # (first call: allocations)
    got = step()
    canary = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            canary.item()  # the mode is implemented: a synchronising read is an error
        run(*got)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(got, ref):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
