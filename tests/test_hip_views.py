"""forward_views / select_views on the GPU: many boxes of one shared point cloud.

The bar is bit equality with forward_batch on the cloud repeated B times (same seed, hence the same transforms): the compact
batch holds, per view, the atoms that pass the box cull in atom order, and a slab's candidate list never contains a culled atom,
so every voxel sums the same terms in the same order. On top of that: parity with the C oracle view by view, the selection on
the cull face and against the grids, determinism, gradients against the repeated cloud, the 10GS pocket, and a call cut into
molecule chunks."""
import os

import numpy as np
import pytest

from tests import hip_support as hip
from tests import views_reference as vr
from tests.tolerance import assert_exact, assert_gaussian
from tests.views_rows import CUBE  # noqa: F401  (clouds are uniform in a cube of this edge, centred at the origin)
from tests.views_rows import centers as _centers
from tests.views_rows import cloud as _cloud

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _vox(D, res, radii_type="scalar", density="gaussian", variant="float32", **kw):
    import molvoxel_amd as mv

    if variant == "bfloat16":
        kw["grid_dtype"] = "bfloat16"
    elif variant == "channels_last":
        kw["grid_layout"] = "channels_last"
    elif variant == "precision64":
        kw["precision"] = 64
    return mv.create_voxelizer(res, D, radii_type, density, "hip", output="torch", **kw)


def _repeat(x, B):
    import torch

    if x is None or np.isscalar(x):
        return x
    return x.repeat((B,) + (1,) * (x.ndim - 1)) if torch.is_tensor(x) else np.tile(x, (B,) + (1,) * (x.ndim - 1))


def _both(vox, xyz, cen, chan, radii, C, xf, atom_radii, seed=7):
    """(forward_views, forward_batch on the repeated cloud) with the same seed."""
    B, N = cen.shape[0], xyz.shape[0]
    kw = dict(random_rotation=True, random_translation=1.0) if xf else {}
    nc = dict(num_channels=C) if (chan is not None and chan.ndim == 1) else {}
    np.random.seed(seed)
    got = vox.forward_views(xyz, cen, chan, radii, **nc, **kw)
    np.random.seed(seed)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    ref = vox.forward_batch(_repeat(xyz, B), offsets, cen, _repeat(chan, B), _repeat(radii, B) if atom_radii else radii, **nc, **kw)
    return got, ref


# ---- 1. bit equality with the repeated cloud --------------------------------------------------------------------------------
# A thinned cross product: every value of every axis appears, and every row runs without a transform and with a seeded random
# rotation + translation. (N, D, res, B, mode, C, radii_type, density, variant, direct)
ROWS = [
    (0, 8, 0.5, 5, "features", 3, "scalar", "gaussian", "float32", None),
    (1, 16, 1.0, 1, "single", 1, "scalar", "binary", "float32", 0),
    (1, 16, 1.0, 1, "single", 1, "atom-wise", "gaussian", "float32", 1),
    (63, 24, 0.5, 67, "types", 5, "channel-wise", "gaussian", "float32", None),
    (64, 8, 1.0, 5, "features", 32, "channel-wise", "gaussian", "float32", None),
    (65, 16, 0.5, 67, "features", 33, "atom-wise", "binary", "bfloat16", None),
    (257, 24, 1.0, 1, "features", 32, "scalar", "gaussian", "channels_last", 0),
    (257, 24, 1.0, 1, "features", 3, "atom-wise", "gaussian", "float32", 1),
    (1025, 16, 1.0, 5, "types", 4, "atom-wise", "binary", "precision64", None),
    (1025, 24, 1.0, 67, "features", 32, "scalar", "gaussian", "float32", None),
    (3000, 24, 1.0, 5, "features", 33, "channel-wise", "gaussian", "channels_last", None),
    (3000, 16, 0.5, 67, "single", 1, "scalar", "gaussian", "bfloat16", None),
    (3000, 8, 1.0, 5, "features", 3, "scalar", "gaussian", "precision64", None),
    (3000, 24, 1.0, 1, "types", 6, "scalar", "binary", "float32", 0),
    (3000, 24, 1.0, 1, "features", 32, "atom-wise", "gaussian", "float32", 1),
]


@pytest.mark.parametrize("xf", [False, True], ids=["plain", "random"])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(x) for x in r))
def test_views_equal_the_repeated_cloud_bit_for_bit(row, xf):
    import torch

    N, D, res, B, mode, C, radii_type, density, variant, direct = row
    vox = _vox(D, res, radii_type, density, variant)
    if direct is not None:
        vox.debug_option("direct", direct)
    xyz, chan, radii = _cloud(N + D + B, N, mode, C, radii_type)
    cen = _centers(N, B, xyz)
    if B == 1 and N:
        cen[0] = xyz[N // 2]
    x = hip.dev(xyz)
    ch = hip.dev(chan, dtype=vox._tfp if mode == "features" else None)
    r = hip.dev(radii)
    got, ref = _both(vox, x, hip.dev(cen), ch, r, C, xf, radii_type == "atom-wise")
    assert got.shape == ref.shape == (B, C, D, D, D) and got.dtype == ref.dtype
    assert torch.equal(got, ref)
    if B >= 2:
        assert not bool(got[0].any())  # the view 1 000 A away
    if N >= 63 and B > 2:
        assert bool(got.any())


def test_all_inclusive_view_far_view_and_host_inputs():
    import torch

    # the whole cloud fits the box of the view centred on it (10 A cube, 23 A box); host (numpy) inputs are uploaded once
    vox = _vox(24, 1.0)
    xyz, feat, _ = _cloud(3, 700, "features", 8, "scalar", edge=10.0)
    cen = np.array([[1000.0, 0, 0], [0, 0, 0], [3.0, -2.0, 1.0], [30.0, 0, 0], [-8.0, 8.0, 8.0]])
    index, offsets = vox.select_views(xyz, cen, radii=1.5)
    counts = np.diff(offsets)
    assert counts[0] == 0 and counts[1] == 700 and offsets[-1] == index.numel()
    assert torch.equal(index[offsets[1]:offsets[2]].cpu(), torch.arange(700))
    got, ref = _both(vox, xyz, cen, feat, 1.5, 8, False, False)
    assert torch.equal(got, ref)
    dev, _ = _both(vox, hip.dev(xyz), hip.dev(cen), hip.dev(feat), 1.5, 8, False, False)
    assert torch.equal(got, dev)
    out = vox.get_empty_grid(8, batch_size=5)
    assert vox.forward_views(xyz, cen, feat, 1.5, out_grid=out) is out and torch.equal(out, ref)


# ---- 2. oracle parity, view by view -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, density", [("features", "gaussian"), ("types", "binary"), ("types", "gaussian")])
def test_views_against_the_c_oracle(mode, density):
    from oracle import c_oracle

    D, res, C = 16, 1.0, 5
    vox = _vox(D, res, "scalar", density)
    xyz, chan, _ = _cloud(11, 1500, mode, C, "scalar")
    cen = _centers(11, 6, xyz)
    nc = dict(num_channels=C) if mode == "types" else {}
    got = vox.forward_views(hip.dev(xyz), hip.dev(cen), hip.dev(chan), 1.5, **nc).cpu().numpy()
    for b in range(cen.shape[0]):
        ref = c_oracle.voxelize(xyz - cen[b], chan, 1.5, resolution=res, dimension=D, density=density, **nc)
        (assert_exact if density == "binary" else assert_gaussian)(got[b], ref)


# ---- 3. the selection is right and really culls -----------------------------------------------------------------------------
@pytest.mark.parametrize("radii_type", ["scalar", "atom-wise"])
def test_selection_on_the_cull_face(radii_type):
    vox = _vox(16, 0.5, radii_type)  # half = 3.75, r = 1.5: the face at 5.25
    for axis in range(3):
        xyz, expect = vr.face_cloud(0.5, 16, 1.5, axis)
        radii = 1.5 if radii_type == "scalar" else np.full(6, 1.5, np.float32)
        index, offsets = vox.select_views(xyz, np.zeros((1, 3)), radii=radii)
        assert np.array_equal(index.cpu().numpy(), np.flatnonzero(expect)) and list(offsets) == [0, 2]


def test_selection_covers_every_contributing_atom_and_culls():
    D, res, B, N, r = 16, 1.0, 9, 3000, 1.5
    vox = _vox(D, res, "scalar", "binary")
    xyz, _, _ = _cloud(5, N, "single", 1, "scalar")
    cen = _centers(5, B, xyz)
    index, offsets = vox.select_views(hip.dev(xyz), hip.dev(cen), radii=r)
    index = index.cpu().numpy()
    assert offsets[0] == 0 and offsets[-1] == index.size and index.dtype == np.int64
    expect = vr.select(xyz, cen, r, res, D)
    bound = vr.count_within(xyz, cen, r, res, D, res)
    for b in range(B):
        mine = index[offsets[b]:offsets[b + 1]]
        assert np.all(np.diff(mine) > 0)
        assert np.array_equal(mine, expect[b])
        assert mine.size <= bound[b] < N / 4
    # every atom with a nonzero voxel in its own grid of the repeated-cloud call is selected: atom n alone, as channel n
    sub = np.arange(0, N, 25)
    types = np.full(N, len(sub), np.int64)
    types[sub] = np.arange(len(sub))
    offs = np.arange(B + 1, dtype=np.int64) * N
    grids = vox.forward_batch(np.tile(xyz, (B, 1)), offs, cen, np.tile(types, B), r, num_channels=len(sub) + 1)
    hit = grids[:, :len(sub)].flatten(2).any(dim=2).cpu().numpy()
    for b in range(B):
        assert set(sub[hit[b]]) <= set(index[offsets[b]:offsets[b + 1]])
    assert hit.any()


def test_rotated_selection_covers_every_contributing_atom():
    """The same under a seeded random rotation and translation per view (the numpy restatement covers identity views only):
    every atom with a nonzero voxel in the repeated-cloud grid of a view is selected for it, in ascending order, and the
    rotated views still cull (a rotation keeps the cloud's density, so the loose identity bound of N / 4 holds for them too)."""
    D, res, B, N, r = 16, 1.0, 9, 3000, 1.5
    vox = _vox(D, res, "scalar", "binary")
    xyz, _, _ = _cloud(6, N, "single", 1, "scalar")
    cen = _centers(6, B, xyz)
    kw = dict(random_rotation=True, random_translation=1.0)
    np.random.seed(3)
    index, offsets = vox.select_views(hip.dev(xyz), hip.dev(cen), radii=r, **kw)
    index = index.cpu().numpy()
    sub = np.arange(0, N, 25)
    types = np.full(N, len(sub), np.int64)
    types[sub] = np.arange(len(sub))
    offs = np.arange(B + 1, dtype=np.int64) * N
    np.random.seed(3)
    grids = vox.forward_batch(np.tile(xyz, (B, 1)), offs, cen, np.tile(types, B), r, num_channels=len(sub) + 1, **kw)
    hit = grids[:, :len(sub)].flatten(2).any(dim=2).cpu().numpy()
    assert offsets[-1] == index.size and hit.any()
    for b in range(B):
        mine = index[offsets[b]:offsets[b + 1]]
        assert np.all(np.diff(mine) > 0) and mine.size < N / 4
        assert set(sub[hit[b]]) <= set(mine)


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    import torch

    vox = _vox(16, 1.0, "atom-wise")
    xyz, feat, radii = _cloud(9, 3000, "features", 32, "atom-wise")
    cen = _centers(9, 67, xyz)
    args = (hip.dev(xyz), hip.dev(cen), hip.dev(feat))
    i0, o0 = vox.select_views(*args, radii=hip.dev(radii))
    g0 = vox.forward_views(*args, hip.dev(radii))
    i1, o1 = vox.select_views(*args, radii=hip.dev(radii))
    g1 = vox.forward_views(*args, hip.dev(radii))
    assert torch.equal(i0, i1) and np.array_equal(o0, o1) and torch.equal(g0, g1) and i0.numel() > 0


# ---- 5. gradients -----------------------------------------------------------------------------------------------------------
def test_gradients_equal_the_repeated_cloud():
    import torch

    D, res, B, N, C = 16, 1.0, 5, 600, 4
    vox = _vox(D, res, "atom-wise", differentiable=True, radii_grad=True)
    xyz, feat, radii = _cloud(13, N, "features", C, "atom-wise", edge=24.0)
    cen = hip.dev(_centers(13, B, xyz))
    x, f, r = hip.dev(xyz), hip.dev(feat), hip.dev(radii)
    index, offsets = vox.select_views(x, cen, f, r)
    w = torch.rand((B, C, D, D, D), device=vox.device, generator=torch.Generator(vox.device).manual_seed(1))

    def leaves(*ts):
        return [t.clone().requires_grad_(True) for t in ts]

    xs, fs, rs = leaves(x[index], f[index], r[index])
    (vox.forward_batch(xs, offsets, cen, fs, rs) * w).sum().backward()
    xr, fr, rr = leaves(x.repeat(B, 1), f.repeat(B, 1), r.repeat(B))
    (vox.forward_batch(xr, np.arange(B + 1, dtype=np.int64) * N, cen, fr, rr) * w).sum().backward()
    rows = torch.cat([index[offsets[b]:offsets[b + 1]] + b * N for b in range(B)])
    keep = torch.zeros(B * N, dtype=torch.bool, device=vox.device)
    keep[rows] = True
    for small, big in ((xs, xr), (fs, fr), (rs, rr)):
        assert torch.equal(small.grad, big.grad[rows])
        assert not bool(big.grad[~keep].any())
    assert bool(xs.grad.any())
    # through forward_views autograd sums the views into the shared tensors
    xv, fv, rv = leaves(x, f, r)
    (vox.forward_views(xv, cen, fv, rv) * w).sum().backward()
    assert xv.grad.shape == x.shape and xv.grad.dtype == x.dtype and fv.grad.shape == f.shape and rv.grad.shape == r.shape
    # (float64 coordinate gradients: the per-view rows are the bits checked above, summed over <= B views in another order -
    # differences of a few ulp of the largest term, which is of order 1 here)
    ref = xr.grad.reshape(B, N, 3).sum(0)
    torch.testing.assert_close(xv.grad, ref, rtol=1e-9, atol=1e-9)


def test_differentiable_views_with_overlap_prepass():
    """overlap_prepass lets the library's side stream read a batched call's inputs without waiting for the caller's stream.
    forward_views' autograd path makes its inputs (the gathered rows) on the caller's stream a moment before the call, so it
    must order them first: grids and gradients equal those of a voxelizer without the option, bit for bit."""
    import torch

    D, res, B, N, C = 16, 1.0, 12, 3000, 8
    xyz, feat, _ = _cloud(21, N, "features", C, "scalar")
    out = []
    for overlap in (False, True):
        vox = _vox(D, res, differentiable=True, overlap_prepass=overlap)
        cen = hip.dev(_centers(21, B, xyz))
        x = hip.dev(xyz).requires_grad_(True)
        f = hip.dev(feat).requires_grad_(True)
        for _ in range(2):  # (the second call runs its pre-pass under the first call's voxelize launches)
            x.grad = f.grad = None
            g = vox.forward_views(x, cen, f, 1.5)
            g.sum().backward()
        out.append((g.detach().clone(), x.grad.clone(), f.grad.clone()))
        torch.cuda.synchronize()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert bool(out[0][0].any()) and bool(out[0][1].any())


# ---- 6. real data: the 10GS pocket ------------------------------------------------------------------------------------------
def test_10gs_pocket_views():
    import torch

    from molvoxel_amd.etc import mol as M
    from oracle import c_oracle

    pocket = M.read_pdb(os.path.join(GOLD, "10gs", "10gs_pocket_nowater.pdb"))
    xyz = pocket.coords
    types = np.asarray(M.AtomTypeGetter(["C", "N", "O", "S"], unknown=True).types_of_keys(pocket.symbols), np.int64)
    N = xyz.shape[0]
    cen = xyz[np.arange(8) * (N // 8)]  # eight views centred on atoms spread over the file
    vox = _vox(24, 1.0)
    got, ref = _both(vox, hip.dev(xyz), hip.dev(cen), hip.dev(types), 1.5, 5, False, False)
    assert torch.equal(got, ref) and bool(got.any())
    assert_gaussian(got[0].cpu().numpy(), c_oracle.voxelize(xyz - cen[0], types, 1.5, resolution=1.0, dimension=24, num_channels=5))


# ---- 7. a call cut into molecule chunks ----------------------------------------------------------------------------------------
def test_chunked_views_call():
    import torch

    vox = _vox(16, 1.0)
    xyz, feat, _ = _cloud(17, 3000, "features", 8, "scalar")
    cen = _centers(17, 67, xyz)
    args = (hip.dev(xyz), hip.dev(cen), hip.dev(feat), 1.5)
    whole = vox.forward_views(*args)
    vox.debug_option("chunks", 2)
    vox.debug_option("mall_budget_kb", 64)
    cut = vox.forward_views(*args)
    assert vox.last_plan()["nchunk"] > 1
    assert torch.equal(cut, whole)
    _, ref = _both(vox, *args[:3], 1.5, 8, False, False)
    assert torch.equal(cut, ref)
