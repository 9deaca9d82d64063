"""Moments of many views of one shared cloud on the GPU (moments_views / moments_posed_views, mvx_moments_views) and their gradients
(mvx_moments_backward_views, moments_grad=True), each view against its own target where the call brings one per view.

Shapes: the cloud of tests/test_hip_score_views.py - 150 atoms in a blob of 20 A around (30, -20, 12), D = 16 at 0.5 A, five views
of which view 1 keeps nothing, atom 0 outside every view - as a features row (C = 5), a types row with channel-wise radii and a
binary single-channel row; a features row of C = 33 at D = 24 (two channel chunks with a remainder: channel offset and view stride
meet); nine views of the base row where a cut into two chunks needs eight; three views of C = 4 at D = 72 (the 1 024-thread
instantiation), forward only.

* Forward, to the bit: moments_batch on coords[index], the gathered channels / radii and select_views' offsets; with and without a
  target; two runs; the caller's selection and the entry's own; bfloat16 and channels-last voxelizers.
* Per-view targets, to the bit: row b of a (B, C, D, D, D) call is row b of the call that shares target[b], uncut, in two chunks and
  with one view per chunk - what a chunk-relative view index would break.
* Exactness: tests/moments_reference.moments_of on forward_views' float32 grids within moments_reference.bound.
* Gradients: rows to the bit against mvx_moments_backward_batch on the compact batch, reduced gradients against views_reduce of the
  rows, cuts of the scratch against the uncut bits, seeded dL/dm against tests/moments_grad_reference.py and autograd on -NCC
  against the grid path of a differentiable voxelizer, both under GRAD_REL * bound + GRAD_ABS of tests/tolerance.py.

Measured (run with -s for the figures): worst |got - exact| / bound of the moments 8.6e-4 (the atom-wise row); worst
|got - ref| / (GRAD_REL * bound + GRAD_ABS) of the rows 0.038 (C = 33); autograd against the grid path 0.0019 for coords, 0.0025
for features, 5.4e-4 and below for centres, quaternions and translations.
"""
import functools

import numpy as np
import pytest

from tests import grad_reference as GR
from tests import moments_grad_reference as MG
from tests import moments_reference as MR
from tests import pose_reference as PR
from tests import views_reference as VW
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID
from tests.tolerance import GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.9, 1.1])
RES = 0.5
SEED = 41  # the rotated leg seeds numpy's global generator

# id: mode, C, radii type, density, D, views
ROWS = {
    "base": ("features", 5, "scalar", "gaussian", 16, 5),
    "atoms": ("features", 5, "atom-wise", "gaussian", 16, 5),
    "chunks": ("features", 33, "scalar", "gaussian", 24, 5),
    "types": ("types", 5, "channel-wise", "gaussian", 16, 5),
    "binary": ("single", 1, "scalar", "binary", 16, 5),
    "nine": ("features", 5, "scalar", "gaussian", 16, 9),
    "big": ("features", 4, "scalar", "gaussian", 72, 3),
}
SMALL = ["base", "atoms", "chunks", "types", "binary"]
DEAD_ATOM = 7  # row "atoms": an atom with radius 0 that view 0 looks straight at


@functools.lru_cache(maxsize=None)
def _data(row_id):
    """One cloud and B poses of it (host arrays; never modified). View 1 looks at empty space; atom 0 lies outside every view."""
    mode, C_, radii_type, density, D, B = ROWS[row_id]
    rng = np.random.default_rng(500 + sorted(ROWS).index(row_id))
    N = 150
    xyz = CEN + rng.uniform(-10.0, 10.0, (N, 3))
    xyz[0] += [100.0, -80.0, 90.0]
    cen = xyz[rng.integers(1, N, B)] + rng.normal(0.0, 0.5, (B, 3))
    cen[1] = CEN + 60.0
    if row_id == "atoms":
        cen[0] = xyz[DEAD_ATOM] + 0.3
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.3, 0.3, (B, 3))
    chan = {"features": rng.standard_normal((N, C_)).astype(np.float32), "types": rng.integers(0, C_, N), "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(np.float32),
             "channel-wise": rng.uniform(1.0, 1.5, C_).astype(np.float32)}[radii_type]
    if row_id == "atoms":
        radii[DEAD_ATOM] = 0.0
    d = dict(xyz=xyz, cen=cen, q=q, t=t, chan=chan, radii=radii, B=B, N=N, mode=mode, C=C_, radii_type=radii_type, density=density,
             D=D, id=row_id)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _target(row_id, per_view):
    """A seeded float32 target of mixed signs, (C, D, D, D) or one per view (B, C, D, D, D) (never modified)."""
    d = _data(row_id)
    shape = ((d["B"],) if per_view else ()) + (d["C"],) + (d["D"],) * 3
    t = np.random.default_rng(900 + sorted(ROWS).index(row_id)).standard_normal(shape).astype(np.float32)
    t.setflags(write=False)
    return t


def _new_vox(row_id, **kw):
    import molvoxel_amd as mv

    d = _data(row_id)
    return mv.create_voxelizer(RES, d["D"], d["radii_type"], d["density"], library="hip", **kw)


@functools.lru_cache(maxsize=None)
def _vox(row_id, **kw):
    return _new_vox(row_id, **kw)


def _take(x, index):
    return x if (x is None or np.isscalar(x)) else x[index]


def _tensors(d, **over):
    return {k: over.get(k, hip.dev(d[k])) for k in ("xyz", "cen", "q", "t", "chan", "radii")}


def _views(vox, d, target=None, transform="posed", **over):
    """moments_posed_views, or moments_views under the random rotations of np.random.seed(transform)."""
    a = _tensors(d, **over)
    if transform == "posed":
        return vox.moments_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], target=target, num_channels=hip.nc(d))
    np.random.seed(transform)
    return vox.moments_views(a["xyz"], a["cen"], a["chan"], a["radii"], target=target, num_channels=hip.nc(d), random_rotation=True)


def _batch(vox, d, index, offsets, target=None, transform="posed", **over):
    """The same records on the gathered rows: moments_posed_batch / moments_batch on coords[index], channels[index] and offsets."""
    a = _tensors(d, **over)
    r = _take(a["radii"], index) if d["radii_type"] == "atom-wise" else a["radii"]
    xyz = over["rows"] if "rows" in over else a["xyz"][index]
    chan = over["chan_rows"] if "chan_rows" in over else _take(a["chan"], index)
    if transform == "posed":
        return vox.moments_posed_batch(xyz, offsets, a["cen"], a["q"], a["t"], chan, r, target=target, num_channels=hip.nc(d))
    np.random.seed(transform)
    return vox.moments_batch(xyz, offsets, a["cen"], chan, r, target=target, num_channels=hip.nc(d), random_rotation=True)


@functools.lru_cache(maxsize=None)
def _selection(row_id, transform="posed"):
    """(index on the device, host offsets) of a row's views, as select_views returns them (never modified)."""
    d = _data(row_id)
    a = _tensors(d)
    vox = _vox(row_id)
    if transform == "posed":
        index, offsets = vox._select_views(a["xyz"], a["cen"], a["chan"], a["radii"], num_channels=hip.nc(d), posed=(a["q"], a["t"]))
    else:
        np.random.seed(transform)
        index, offsets = vox._select_views(a["xyz"], a["cen"], a["chan"], a["radii"], random_rotation=True, num_channels=hip.nc(d))
    offsets.setflags(write=False)
    return index, offsets


def _cull_source(d):
    if d["radii_type"] in ("scalar", "atom-wise"):
        return d["radii_type"]
    return "by-type" if d["mode"] == "types" else "channel-features"


# ---- the C entries through ctypes -----------------------------------------------------------------------------------------------
def _views_spec(vox, d):
    """The call record of a row's posed views as the Python layer builds it for the library."""
    import torch

    a = _tensors(d)
    with torch.no_grad():
        return vox._views_call(a["xyz"], a["cen"], a["chan"], a["radii"], hip.nc(d), posed=(a["q"], a["t"]), device=True)


def _batch_spec(vox, d, index, offsets):
    """... and of the compact batch of a selection."""
    import torch

    a = _tensors(d)
    r = _take(a["radii"], index) if d["radii_type"] == "atom-wise" else a["radii"]
    with torch.no_grad():
        return vox._batch_call(a["xyz"][index], offsets, a["cen"], _take(a["chan"], index), r, hip.nc(d), posed=(a["q"], a["t"]),
                               device=True)


def _stride(d, T):
    return d["C"] * d["D"] ** 3 if (T is not None and T.dim() == 5) else 0


def _abi_forward(vox, d, index, offsets, T, stride=None):
    """mvx_moments_views through ctypes with a selection (or None): (rc, moments full of NaN where nothing was written)."""
    import torch

    call = _views_spec(vox, d)
    out = hip.nan((d["B"], d["C"], 2 if T is None else 3))
    rc = vox._lib.mvx_moments_views(*call.views_args(vox), hip.ptr(index), None if index is None else offsets.ctypes.data, hip.ptr(T),
                                    _stride(d, T) if stride is None else stride, out.data_ptr(), vox._stream())
    torch.cuda.synchronize()
    return rc, out


def _rows_views(vox, d, index, offsets, gm, T, stride=None, check=True):
    """mvx_moments_backward_views through ctypes: (grad_coords_rows, grad_features_rows or None), or the return code."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    call = _views_spec(vox, d)
    total = int(offsets[-1])
    g = torch.tensor(np.ascontiguousarray(gm, np.float64), device="cuda")
    gc, gf = hip.nan((total, 3)), (hip.nan((total, d["C"]), torch.float32) if d["mode"] == "features" else None)
    rc = vox._lib.mvx_moments_backward_views(*call.views_args(vox), index.data_ptr(), offsets.ctypes.data, hip.ptr(T),
                                             _stride(d, T) if stride is None else stride, g.data_ptr(), gc.data_ptr(), hip.ptr(gf),
                                             vox._stream())
    torch.cuda.synchronize()
    if not check:
        return rc
    _lib.check(rc)
    return gc, gf


def _rows_batch(vox, d, index, offsets, gm, T):
    """mvx_moments_backward_batch through ctypes on the compact batch of the selection."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    call = _batch_spec(vox, d, index, offsets)
    total = int(offsets[-1])
    g = torch.tensor(np.ascontiguousarray(gm, np.float64), device="cuda")
    gc, gf = hip.nan((total, 3)), (hip.nan((total, d["C"]), torch.float32) if d["mode"] == "features" else None)
    _lib.check(vox._lib.mvx_moments_backward_batch(*call.batch_args(vox), hip.ptr(T), g.data_ptr(), gc.data_ptr(), hip.ptr(gf), vox._stream()))
    torch.cuda.synchronize()
    return gc, gf


def _same(a, b):
    import torch

    return (a[1] is None) == (b[1] is None) and all(
        x is None or (not torch.isnan(x).any() and torch.equal(x, y)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _dm(row_id, K):
    """Seeded dL/dm of mixed signs, different for every view and channel: (B, C, K) float64 (never modified)."""
    d = _data(row_id)
    g = np.random.default_rng(1300 + sorted(ROWS).index(row_id) + K).standard_normal((d["B"], d["C"], K))
    g.setflags(write=False)
    return g


# ---- 1. forward, to the bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", SMALL + ["big"])
def test_moments_are_the_batch_entrys_bits_on_the_gathered_rows(row_id):
    import torch

    d = _data(row_id)
    B, N, C_ = d["B"], d["N"], d["C"]
    vox = _vox(row_id)
    index, offsets = _selection(row_id)
    counts = np.diff(offsets)
    assert counts[1] == 0 and counts.max() < N and np.count_nonzero(counts) == B - 1 and counts.sum() > 40
    assert 0 not in index.cpu().numpy()  # (atom 0 is outside every view)
    if row_id == "base":
        # the selection is the forward's (no (view, atom) pair near a cull bound, so the restatement decides as the kernel does)
        p = PR.view_positions(d["xyz"], d["cen"], d["q"], d["t"])
        cull = (p, RES, d["D"], _cull_source(d), d["radii"], 32, None, None)
        assert float(VW.margin(*cull).min()) > 1e-9
        assert VW.selection_mismatch(index.cpu().numpy(), offsets, *VW.select_exact(*cull)) is None
    T = hip.dev(_target(row_id, False))
    with_t, plain = _views(vox, d, T), _views(vox, d)
    assert with_t.dtype == torch.float64 and with_t.is_cuda and tuple(with_t.shape) == (B, C_, 3) and tuple(plain.shape) == (B, C_, 2)
    assert not with_t.requires_grad
    assert torch.equal(with_t, _batch(vox, d, index, offsets, T)) and torch.equal(plain, _batch(vox, d, index, offsets))
    assert torch.equal(with_t[..., :2], plain)  # the first two moments do not depend on the target
    assert torch.equal(_views(vox, d, T), with_t) and torch.equal(_views(vox, d), plain)  # two runs
    assert not with_t[1].any() and not torch.signbit(with_t[1]).any()  # a view that keeps no atom: exact zeros
    assert bool((with_t[0, :, 1] > 0).any()) and bool((with_t[B - 1, :, 1] > 0).any())
    # the caller's selection and the entry's own, through the C entry
    for Tk in (T, None):
        rc1, own = _abi_forward(vox, d, None, None, Tk)
        rc2, given = _abi_forward(vox, d, index, offsets, Tk)
        assert rc1 == 0 and rc2 == 0 and torch.equal(own, given) and torch.equal(own, with_t if Tk is not None else plain)


@pytest.mark.parametrize("row_id", ["base", "types", "binary"])
def test_rotated_views_draw_as_the_batch_entry_draws(row_id):
    import torch

    d = _data(row_id)
    vox = _vox(row_id)
    index, offsets = _selection(row_id, SEED)
    T = hip.dev(_target(row_id, False))
    got = _views(vox, d, T, SEED)
    drawn = np.random.rand()
    assert torch.equal(got, _batch(vox, d, index, offsets, T, SEED))
    assert np.random.rand() == drawn  # the same draws were consumed
    assert not torch.equal(got, _views(vox, d, T))  # (the rotations reach the call)


@pytest.mark.parametrize("row_id, kw", [("base", dict(grid_dtype="bfloat16")), ("chunks", dict(grid_layout="channels_last")),
                                        ("types", dict(grid_dtype="bfloat16", grid_layout="channels_last"))])
def test_bfloat16_and_channels_last_voxelizers_give_the_float32_bits(row_id, kw):
    import torch

    d = _data(row_id)
    T = hip.dev(_target(row_id, True))
    other = _vox(row_id, **kw)
    assert torch.equal(_views(other, d, T), _views(_vox(row_id), d, T))
    assert torch.equal(_views(other, d), _views(_vox(row_id), d))
    a = _tensors(d)  # the handle still writes its own grid type afterwards
    grid = other.forward_posed_views(a["xyz"], a["cen"][:1], a["q"][:1], a["t"][:1], a["chan"], a["radii"], num_channels=hip.nc(d))
    assert grid.dtype == (torch.bfloat16 if "grid_dtype" in kw else torch.float32)


def test_views_that_keep_nothing_and_a_cloud_without_atoms():
    import torch

    d = _data("base")
    vox = _new_vox("base", differentiable=True, moments_grad=True)
    T = hip.dev(_target("base", True))
    a = _tensors(d, xyz=hip.dev(d["xyz"], True), chan=hip.dev(d["chan"], True))
    far = hip.dev(d["cen"] + 500.0)
    m = vox.moments_posed_views(a["xyz"], far, a["q"], a["t"], a["chan"], 1.25, target=T)
    assert m.requires_grad and tuple(m.shape) == (5, 5, 3) and not m.any() and not torch.signbit(m).any()
    (m * hip.dev(_dm("base", 3))).sum().backward()
    assert tuple(a["xyz"].grad.shape) == (150, 3) and not a["xyz"].grad.any()
    assert tuple(a["chan"].grad.shape) == (150, 5) and not a["chan"].grad.any()
    plain = _vox("base")
    none = plain.moments_posed_views(hip.dev(d["xyz"])[:0], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"])[:0], 1.25, target=T)
    assert tuple(none.shape) == (5, 5, 3) and not none.any() and not torch.signbit(none).any()
    assert tuple(plain.moments_posed_views(hip.dev(d["xyz"])[:0], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"])[:0], 1.25).shape) == (5, 5, 2)


# ---- 2. one target per view ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shared_rows(row_id):
    """Row b of the call that shares target[b] among all views, for every b: (B, C, 3) (never modified)."""
    import torch

    d = _data(row_id)
    T = hip.dev(_target(row_id, True))
    return torch.stack([_views(_vox(row_id), d, T[b])[b] for b in range(d["B"])])


@pytest.mark.parametrize("row_id", SMALL + ["big"])
def test_a_view_reads_its_own_target(row_id):
    import torch

    d = _data(row_id)
    got = _views(_vox(row_id), d, hip.dev(_target(row_id, True)))
    assert tuple(got.shape) == (d["B"], d["C"], 3)
    assert torch.equal(got, _shared_rows(row_id))
    other = _views(_vox(row_id), d, hip.dev(_target(row_id, True)[0]))  # (the targets differ, and the views see it)
    assert torch.equal(other[..., :2], got[..., :2]) and not torch.equal(other[2:, :, 2], got[2:, :, 2])


@pytest.mark.parametrize("row_id, option, value, nchunk", [
    ("nine", "chunks", 2, 2), ("nine", "mall_budget_kb", 1, 9), ("base", "mall_budget_kb", 1, 5), ("chunks", "mall_budget_kb", 1, 5),
    ("types", "mall_budget_kb", 1, 5), ("binary", "mall_budget_kb", 1, 5)])
def test_a_view_reads_its_own_target_in_every_chunk(row_id, option, value, nchunk):
    """The view of the CALL picks the target, not the view of the launch's chunk: with a chunk-relative index every chunk behind the
    first would read the first chunk's targets."""
    import torch

    d = _data(row_id)
    vox = _new_vox(row_id)  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option(option, value)
    got = _views(vox, d, hip.dev(_target(row_id, True)))
    plan = vox.last_plan()
    assert plan["nchunk"] == nchunk, plan  # the cut really happened
    assert torch.equal(got, _shared_rows(row_id))
    assert torch.equal(_views(vox, d, hip.dev(_target(row_id, False))), _views(_vox(row_id), d, hip.dev(_target(row_id, False))))


def test_the_rules_that_read_the_handle():
    """A stride that is neither 0 nor C * D^3, the configurations the walk does not serve and the target's alignment, for both
    entries, with real handles; and what a good call of the backward entry leaves alone."""
    import molvoxel_amd as mv
    import torch

    d = _data("base")
    vox = _vox("base")
    index, offsets = _selection("base")
    T = hip.dev(_target("base", True))
    for stride in (7, 5 * 16 ** 3 - 4, 33 * 16 ** 3):
        rc, out = _abi_forward(vox, d, None, None, T, stride=stride)
        assert rc == MVX_ERR_INVALID and "target_view_stride" in vox._lib.mvx_last_error().decode() and torch.isnan(out).all()
        rc = _rows_views(vox, d, index, offsets, _dm("base", 3), T, stride=stride, check=False)
        assert rc == MVX_ERR_INVALID and "target_view_stride" in vox._lib.mvx_last_error().decode()
    mk = lambda D, rt="scalar", **kw: mv.create_voxelizer(0.5, D, rt, "gaussian", library="hip", **kw)  # noqa: E731
    for other, rt, radii, target, words in [
        (mk(16, precision=64), 0, None, T, "precision 64"),
        (mk(16, "channel-wise"), 2, torch.ones(5, device="cuda"), T, "channel-wise radii with features"),
        (mk(18), 0, None, T, "no multiple of 4"),
        (mk(24, blockdim=12), 0, None, T, "per-lane ranges"),
        (vox, 0, None, torch.zeros(5 * 16 ** 3 + 1, device="cuda")[1:], "16-byte aligned"),
    ]:
        call = _views_spec(vox, d)
        head = (other._handle,) + call.views_args(vox)[1:4] + (hip.ptr(radii), 1.25, rt) + call.views_args(vox)[7:]
        gm, gc = hip.nan((5, 5, 3)), hip.nan((int(offsets[-1]), 3))
        for rc in (vox._lib.mvx_moments_views(*head, None, None, target.data_ptr(), 0, gm.data_ptr(), None),
                   vox._lib.mvx_moments_backward_views(*head, index.data_ptr(), offsets.ctypes.data, target.data_ptr(), 0, gm.data_ptr(),
                                                       gc.data_ptr(), None, None)):
            msg = vox._lib.mvx_last_error().decode()
            assert rc == MVX_ERR_INVALID and msg.startswith("moments:" if "aligned" not in words else "target") and words in msg, (rc, msg)
    # no views: MVX_OK and nothing written, whatever else is missing
    call = _views_spec(vox, d)
    head = call.views_args(vox)[:9] + (None, 0)
    assert vox._lib.mvx_moments_views(*head, None, None, None, 0, None, None) == 0
    assert vox._lib.mvx_moments_backward_views(*head, index.data_ptr(), None, None, 0, None, hip.nan((1, 3)).data_ptr(), None, None) == 0
    # a good call overwrites every row
    gc, gf = _rows_views(vox, d, index, offsets, _dm("base", 3), T)
    assert not torch.isnan(gc).any() and not torch.isnan(gf).any()


# ---- 3. exactness against the grids of forward_views ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", SMALL + ["big"])
def test_moments_are_those_of_forward_views_grids(row_id):
    import torch

    d = _data(row_id)
    vox = _vox(row_id)
    a = _tensors(d)
    grids = vox.forward_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], num_channels=hip.nc(d))
    assert grids.dtype == torch.float32 and tuple(grids.shape) == (d["B"], d["C"]) + (d["D"],) * 3
    g = grids.cpu().numpy()
    T = _target(row_id, True)
    pairs = [MR.moments_and_bound(g[b], T[b]) for b in range(d["B"])]  # (every view against its own target)
    ref, bnd = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got = _views(vox, d, hip.dev(T)).cpu().numpy()
    err = np.abs(got - ref)
    live = bnd > 0
    assert live.any() and (np.abs(ref[..., 2]) > 0).any()
    print(f"MOMENTS_VIEWS_EXACT {row_id}: worst |got - exact| / bound = {float((err[live] / bnd[live]).max()):.3g}, "
          f"largest moment {float(np.abs(ref).max()):.6g}")
    assert (err <= bnd).all(), float((err - bnd).max())  # (where the bound is 0 - no atom reaches the channel - equality with 0)
    assert not got[1].any()
    if d["density"] == "binary":  # sums of small integers: voxel counts
        assert np.array_equal(got[..., :2], ref[..., :2]) and (got[..., :2] == np.round(got[..., :2])).all()
        assert got[..., 0].max() > 100


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------------
GRAD_ROWS = ["base", "atoms", "chunks", "types", "binary"]


@pytest.mark.parametrize("row_id", GRAD_ROWS)
def test_rows_are_the_batch_entrys_bits_on_the_compact_batch(row_id):
    import torch

    d = _data(row_id)
    vox = _vox(row_id)
    index, offsets = _selection(row_id)
    T = hip.dev(_target(row_id, False))
    for Tk, K in ((T, 3), (None, 2)):
        got = _rows_views(vox, d, index, offsets, _dm(row_id, K), Tk)
        assert _same(got, _rows_batch(vox, d, index, offsets, _dm(row_id, K), Tk)), (row_id, K)
        assert _same(_rows_views(vox, d, index, offsets, _dm(row_id, K), Tk), got)  # two runs
        if d["density"] == "binary":
            assert not got[0].any()  # the a.e. derivative
        else:
            assert bool(got[0].any()) and (got[1] is None or bool(got[1].any()))
    if row_id == "atoms":  # an atom that is selected but dead (radius 0 inside the box of view 0): exact-zero rows
        idx = index.cpu().numpy()
        slot = np.flatnonzero(idx[:offsets[1]] == DEAD_ATOM)
        assert slot.size == 1
        gc, gf = _rows_views(vox, d, index, offsets, _dm(row_id, 3), T)
        assert not gc[slot[0]].any() and not gf[slot[0]].any() and bool(gc[:offsets[1]].any())  # (M^T 0 may be -0: it compares equal)


@functools.lru_cache(maxsize=None)
def _uncut_rows(row_id, with_target):
    d = _data(row_id)
    index, offsets = _selection(row_id)
    return _rows_views(_vox(row_id), d, index, offsets, _dm(row_id, 3 if with_target else 2),
                       hip.dev(_target(row_id, True)) if with_target else None)


@pytest.mark.parametrize("row_id", ["base", "chunks", "types"])
def test_rows_of_a_view_come_from_its_own_target(row_id):
    """Per-view targets against the shared-target call with target[b]: the rows of view b, to the bit."""
    import torch

    d = _data(row_id)
    index, offsets = _selection(row_id)
    gc, gf = _uncut_rows(row_id, True)
    T = _target(row_id, True)
    for b in range(d["B"]):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi == lo:
            continue
        sc, sf = _rows_views(_vox(row_id), d, index, offsets, _dm(row_id, 3), hip.dev(T[b]))
        assert torch.equal(gc[lo:hi], sc[lo:hi]) and (gf is None or torch.equal(gf[lo:hi], sf[lo:hi])), (row_id, b)
        if b >= 2 and d["density"] != "binary":  # (... and not from another view's)
            assert not torch.equal(gc[:lo], sc[:lo])


@pytest.mark.parametrize("row_id, option, value, nchunk", [
    # D = 16, C = 5: 80 KiB of grids per view - three views fit 240 KiB, one fits 1 KiB
    ("base", "mgrad_scratch_kb", 240, 2), ("base", "mgrad_scratch_kb", 1, 5), ("types", "mgrad_scratch_kb", 1, 5),
    # D = 24, C = 33: 1 782 KiB per view
    ("chunks", "mgrad_scratch_kb", 5400, 2), ("chunks", "mgrad_scratch_kb", 1, 5),
    ("nine", "chunks", 2, 2), ("base", "mall_budget_kb", 1, 5)])
def test_cuts_of_the_backward_give_the_uncut_bits_with_a_target_per_view(row_id, option, value, nchunk):
    d = _data(row_id)
    vox = _new_vox(row_id)
    vox.debug_option(option, value)
    index, offsets = _selection(row_id)
    for with_target in (True, False):
        got = _rows_views(vox, d, index, offsets, _dm(row_id, 3 if with_target else 2), hip.dev(_target(row_id, True)) if with_target else None)
        plan = vox.last_plan()
        assert plan["nchunk"] == nchunk, plan  # the cut really happened, and the entry reports it
        assert _same(got, _uncut_rows(row_id, with_target)), (row_id, with_target)


@functools.lru_cache(maxsize=None)
def _grids(row_id):
    d = _data(row_id)
    a = _tensors(d)
    g = _vox(row_id).forward_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], num_channels=hip.nc(d)).cpu().numpy()
    assert g.dtype == np.float32
    g.setflags(write=False)
    return g


def _rows_reference(d, idx, offsets, grids, gm, target, rows=None):
    """The float64 reference of the rows `rows` (default: all) of a selection: dict of (total, ...) arrays, zero where not asked for -
    "p" / "p_bound": dL/dp before the pose's rotation, "coords" / "coords_bound": dL/dcoords = M^T dL/dp, "features" /
    "features_bound". The bounds are the reference with |a0| + |a1| |g| + |a2| |t| for G (tests/moments_grad_reference.py)."""
    total, C_ = int(offsets[-1]), d["C"]
    take = np.arange(total) if rows is None else np.asarray(sorted(rows))
    out = {k: np.zeros((total, 3)) for k in ("p", "p_bound", "coords", "coords_bound")}
    out.update(features=np.zeros((total, C_)), features_bound=np.zeros((total, C_)))
    for b in range(d["B"]):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        mine = take[(take >= lo) & (take < hi)] - lo
        if not mine.size:
            continue
        sel = idx[lo:hi]
        p = PR.positions(d["xyz"][sel], d["cen"][b], d["q"][b], d["t"][b])
        tb = None if target is None else (target[b] if target.ndim == 5 else target)
        G, Gabs = MG.upstream(grids[b], gm[b], tb)
        kw = dict(mode=d["mode"], density=d["density"], atoms=mine.tolist())
        if d["mode"] == "features":
            kw["w"] = d["chan"][sel]
        elif d["mode"] == "types":
            kw["types"] = d["chan"][sel]
        radii = d["radii"][sel] if d["radii_type"] == "atom-wise" else d["radii"]
        val = GR.reference(p, G, radii, d["radii_type"], **kw)
        bnd = GR.reference(p, Gabs, radii, d["radii_type"], **kw)
        M = PR.rotation(d["q"][b])
        at = lo + mine
        out["p"][at], out["p_bound"][at] = val["coords"][0], bnd["coords"][1]
        out["coords"][at], out["coords_bound"][at] = val["coords"][0] @ M, bnd["coords"][1] @ np.abs(M)
        if d["mode"] == "features":
            out["features"][at], out["features_bound"][at] = val["features"][0], bnd["features"][1]
    return out, take


@pytest.mark.parametrize("row_id", ["base", "atoms", "chunks", "types"])
def test_seeded_upstreams_match_the_float64_reference(row_id):
    d = _data(row_id)
    vox = _vox(row_id)
    index, offsets = _selection(row_id)
    idx = index.cpu().numpy()
    total = int(offsets[-1])
    rows = np.random.default_rng(3).choice(total, min(total, 64 if row_id == "chunks" else 96), replace=False)
    if row_id == "atoms":  # (the atom of radius 0 has exact-zero rows, checked elsewhere: the reference would divide by its radius)
        rows = rows[idx[rows] != DEAD_ATOM]
    worst = 0.0
    for per_view, K in ((True, 3), (False, 3), (None, 2)):
        target = None if per_view is None else _target(row_id, per_view)
        gm = _dm(row_id, K)
        gc, gf = _rows_views(vox, d, index, offsets, gm, hip.dev(target))
        ref, take = _rows_reference(d, idx, offsets, _grids(row_id), gm, target, rows)
        worst = max(worst, GR.close(gc.cpu().numpy()[take], ref["coords"][take], ref["coords_bound"][take],
                                    f"{row_id} K={K} per_view={per_view} coords", GRAD_REL, GRAD_ABS))
        assert (ref["coords_bound"][take] > 0).any(axis=1).sum() > 0.3 * len(take)
        if gf is not None:
            worst = max(worst, GR.close(gf.cpu().numpy()[take], ref["features"][take], ref["features_bound"][take],
                                        f"{row_id} K={K} per_view={per_view} features", GRAD_REL, GRAD_ABS))
    print(f"MOMENTS_VIEWS_GRAD_WORST {row_id}: worst |got - ref| / (GRAD_REL * bound + GRAD_ABS) = {worst:.3g}")


def _leaves(d, features):
    import torch

    out = dict(xyz=hip.dev(d["xyz"], True), cen=hip.dev(d["cen"], True), q=hip.dev(d["q"], True), t=hip.dev(d["t"], True))
    if features:
        out["chan"] = hip.dev(d["chan"], True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row_id, per_view", [("base", True), ("atoms", False), ("chunks", True), ("types", True)])
def test_shared_gradients_are_views_reduce_of_the_rows(row_id, per_view):
    """L = (m * W).sum() has dL/dm = W: coords.grad and features.grad are views_reduce of the entry's rows for W, to the bit; pose
    gradients are mvx_pose_grad_batch's on those rows - with a shared target the compact batch's own autograd gradients; two runs
    give the same bits; nothing is recorded without the flag."""
    import torch

    d = _data(row_id)
    N, features = d["N"], d["mode"] == "features"
    vox = _vox(row_id, differentiable=True, moments_grad=True)
    T = hip.dev(_target(row_id, per_view))
    W = hip.dev(_dm(row_id, 3))

    def run():
        a = _leaves(d, features)
        m = _views(vox, d, T, **a)
        assert m.requires_grad and m.dtype == torch.float64
        (m * W).sum().backward()
        return a, m.detach()

    a, m = run()
    again, _ = run()
    for k in a:
        assert a[k].grad is not None and torch.equal(a[k].grad, again[k].grad), k  # deterministic
    assert torch.equal(m, _views(_vox(row_id), d, T))  # the recorded call gives the plain call's bits
    index, offsets = _selection(row_id)
    gc, gf = _rows_views(_vox(row_id), d, index, offsets, _dm(row_id, 3), T)
    assert torch.equal(a["xyz"].grad, vox.views_reduce(gc, index, offsets, N)) and a["xyz"].grad.dtype == torch.float64
    assert bool(a["xyz"].grad.any()) and not a["xyz"].grad[0].any()  # (atom 0 is in no view)
    if features:
        assert torch.equal(a["chan"].grad, vox.views_reduce(gf, index, offsets, N)) and a["chan"].grad.dtype == torch.float32
        assert bool(a["chan"].grad.any())
    # centres and poses per view: the reduction of the rows the entry wrote
    spec = _views_spec(vox, d)
    spec.offsets = np.asarray(offsets)
    gp = vox._pose_backward(spec, hip.dev(d["xyz"])[index], gc)
    assert torch.equal(a["cen"].grad, gp[:, :3]) and torch.equal(a["q"].grad, gp[:, 3:7]) and torch.equal(a["t"].grad, gp[:, 7:])
    assert bool(a["q"].grad.any()) and not a["q"].grad[1].any()
    if not per_view:  # the compact batch with leaves of its own
        b = _leaves(d, features)
        rows = b.pop("xyz").detach()[index].requires_grad_()
        chan_rows = b.pop("chan").detach()[index].requires_grad_() if features else _take(hip.dev(d["chan"]), index)
        (_batch(vox, d, index, offsets, T, rows=rows, chan_rows=chan_rows, **b) * W).sum().backward()
        assert torch.equal(rows.grad, gc) and (not features or torch.equal(chan_rows.grad, gf))
        for k in b:
            assert torch.equal(a[k].grad, b[k].grad), k
    # without the flag, in no_grad mode and without leaves nothing is recorded
    plain = _vox(row_id, differentiable=True)
    assert not _views(plain, d, T, **_leaves(d, features)).requires_grad
    with torch.no_grad():
        assert not _views(vox, d, T, **_leaves(d, features)).requires_grad
    assert not _views(vox, d, T).requires_grad


def _ncc_loss(m, tt):
    """-sum over views and channels of m2 / sqrt(m1 * sum t^2); a channel no atom reaches contributes 0 (the small constant)."""
    import torch

    return -(m[..., 2] / torch.sqrt(m[..., 1] * tt + 1e-6)).sum()


def _moments_of(grids, T):
    import torch

    g = grids.double()
    return torch.stack([g.sum((2, 3, 4)), (g * g).sum((2, 3, 4)), (g * T.double()).sum((2, 3, 4))], dim=-1)


def test_autograd_gives_the_gradients_of_the_ncc_loss_of_the_grid_path():
    """-NCC of every view against its own target, through the moments and through forward_posed_views' grids of a differentiable
    voxelizer: coords, features, centres, quaternions and translations agree within the float64 reference's bounds for the
    upstream this loss has at these moments (per shared atom: the bounds of its rows added over the views)."""
    import torch

    row_id = "base"
    d = _data(row_id)
    B, N = d["B"], d["N"]
    vox = _vox(row_id, differentiable=True, moments_grad=True)
    plain = _vox(row_id, differentiable=True)
    T = hip.dev(_target(row_id, True))
    tt = (T.double() ** 2).sum((2, 3, 4))
    x = _leaves(d, True)
    m = _views(vox, d, T, **x)
    assert m.requires_grad
    _ncc_loss(m, tt).backward()
    y = _leaves(d, True)
    grids = plain.forward_posed_views(y["xyz"], y["cen"], y["q"], y["t"], y["chan"], 1.25)
    assert grids.requires_grad
    _ncc_loss(_moments_of(grids, T), tt).backward()
    md = m.detach().clone().requires_grad_()
    _ncc_loss(md, tt).backward()
    gm = md.grad.cpu().numpy()
    index, offsets = _selection(row_id)
    idx = index.cpu().numpy()
    ref, _ = _rows_reference(d, idx, offsets, grids.detach().cpu().numpy(), gm, _target(row_id, True))
    bc, bf = np.zeros((N, 3)), np.zeros((N, d["C"]))
    np.add.at(bc, idx, ref["coords_bound"])
    np.add.at(bf, idx, ref["features_bound"])
    close = lambda k, bound: GR.close(x[k].grad.cpu().numpy(), y[k].grad.cpu().numpy(), bound, k, GRAD_REL, GRAD_ABS)  # noqa: E731
    assert (bc > 0).any() and bool((x["xyz"].grad != 0).any()) and bool((x["chan"].grad != 0).any())
    worst = {"coords": close("xyz", bc), "features": close("chan", bf)}
    bounds = {"center": [], "quaternion": [], "translation": []}
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        pg = PR.pose_grads(d["xyz"][idx[lo:hi]], d["cen"][b], d["q"][b], ref["p"][lo:hi], ref["p_bound"][lo:hi])
        for k in bounds:
            bounds[k].append(pg[k][1])
    for k, name in (("center", "cen"), ("quaternion", "q"), ("translation", "t")):
        assert bool((x[name].grad != 0).any()) and not x[name].grad[1].any()
        worst[k] = close(name, np.stack(bounds[k]))
    print(f"MOMENTS_VIEWS_AUTOGRAD base: moments path against grid path, worst ratios {worst}")


def test_a_change_of_density_between_forward_and_backward_is_refused():
    d = _data("base")
    vox = _new_vox("base", differentiable=True, moments_grad=True)
    m = _views(vox, d, None, xyz=hip.dev(d["xyz"], True))
    vox.density_type = "binary"
    with pytest.raises(RuntimeError, match="changed between the forward call and backward"):
        m.sum().backward()
