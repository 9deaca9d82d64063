"""select_views / forward_views where the small shapes of test_hip_views.py do not reach: scans of more than one count per
thread, more than 65 535 views in one launch, an index buffer that turns out too small, gather pieces of 4, 8 and 16 bytes from
bases that are not 16-byte aligned, and the selection of every radii source, rotated views included, against the float64
restatement of tests/views_reference.py entry by entry.

Everything here is integer bookkeeping with an exact answer: index and offsets are compared with ==, grids with torch.equal.
tests/test_views_host.py proves on the host that no (view, atom) pair of a seeded row lies within 1e-9 A of a cull bound, so no
atom is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import hip_support as hip
from tests import views_reference as vr
from tests import views_rows as rows
from tests.abi import MVX_ERR_INVALID
from tests.tolerance import assert_exact, assert_gaussian

pytestmark = pytest.mark.gpu

MVX_OK = 0


def _vox(D, res, radii_type="scalar", density="gaussian", precision=32):
    import molvoxel_amd as mv

    return mv.create_voxelizer(res, D, radii_type, density, "hip", output="torch", precision=precision)


def _check(index, offsets, ref_index, ref_offsets):
    msg = vr.selection_mismatch(index.cpu().numpy(), offsets, ref_index, ref_offsets)
    assert msg is None, msg


def _grids(vox, xyz, cen, chan, radii, xf, atom_radii, seed=7, **nc):
    """(forward_views, forward_batch on the cloud repeated B times - fresh, aligned copies) with the same seed."""
    B, N = cen.shape[0], xyz.shape[0]
    kw = rows.TRANSFORM if xf else {}
    np.random.seed(seed)
    got = vox.forward_views(xyz, cen, chan, radii, **nc, **kw)
    np.random.seed(seed)
    rep = lambda x: x.repeat((B,) + (1,) * (x.ndim - 1))  # noqa: E731
    ref = vox.forward_batch(rep(xyz), np.arange(B + 1, dtype=np.int64) * N, cen, None if chan is None else rep(chan),
                            rep(radii) if atom_radii else radii, **nc, **kw)
    return got, ref


# ---- a. the scan past one count per thread, and the launch grid past 65 535 views --------------------------------------------
@pytest.mark.parametrize("case", rows.SCAN_CASES, ids=rows.case_id)
def test_scan_rows_equal_the_reference(case):
    row, rotated = case
    xyz, cen, radii = rows.row_inputs(row)
    ref_index, ref_offsets, _ = rows.row_reference(row, rotated)
    vox = _vox(row.D, row.res, row.radii)
    np.random.seed(rows.row_seed(row))
    index, offsets = vox.select_views(hip.dev(xyz), hip.dev(cen), radii=hip.dev(radii), **(rows.TRANSFORM if rotated else {}))
    _check(index, offsets, ref_index, ref_offsets)


# ---- b. forward_views at scale: the handle-owned index with per = 3, feature rows of 8 bytes ----------------------------------
@pytest.mark.parametrize("xf", [False, True], ids=["identity", "rotated"])
def test_forward_views_at_scale_equals_the_repeated_cloud(xf):
    import torch

    B, N, D, C_ = 1100, 1100, 8, 2
    vox = _vox(D, 1.0)
    xyz, feat, _ = rows.cloud(41, N, "features", C_, "scalar")
    cen = rows.centers(41, B, xyz)
    got, ref = _grids(vox, hip.dev(xyz), hip.dev(cen), hip.dev(feat), 1.5, xf, False)
    assert got.shape == (B, C_, D, D, D) and torch.equal(got, ref)
    assert not bool(got[0].any()) and int(got.flatten(1).any(dim=1).sum()) > B // 2


# ---- c. an index buffer that is too small ------------------------------------------------------------------------------------
def _all_inclusive():
    rng = np.random.default_rng(51)
    xyz = rng.uniform(-3.0, 3.0, (3000, 3))  # D 16, res 1.0, r 1.5: a view keeps |p| < 9, so every view below keeps every atom
    cen = rng.uniform(-1.0, 1.0, (400, 3))
    return xyz, cen


def test_select_views_grows_a_too_small_index_buffer():
    import torch

    xyz, cen = _all_inclusive()
    B, N = cen.shape[0], xyz.shape[0]
    assert B * N > 1 << 20
    vox = _vox(16, 1.0)
    x = hip.dev(xyz)
    expect = torch.arange(N, device=vox.device).repeat(B)
    for call in range(2):  # the first call finds 2^20 entries too few; the second sizes the buffer from the first one's total
        index, offsets = vox.select_views(x, hip.dev(cen), radii=1.5)
        assert np.array_equal(offsets, np.arange(B + 1, dtype=np.int64) * N), call
        assert index.dtype == torch.int64 and torch.equal(index, expect), call
        assert vox._views_total == B * N
    index, offsets = vox.select_views(x, hip.dev(cen + [1000.0, 0.0, 0.0]), radii=1.5)
    assert index.numel() == 0 and not offsets.any() and offsets.shape == (B + 1,)


def test_c_abi_reports_a_too_small_buffer_and_leaves_it_untouched():
    import torch

    xyz, cen = _all_inclusive()
    cen = cen[:7]
    cen[3] = [1000.0, 0.0, 0.0]  # one empty view among them
    B, N = cen.shape[0], xyz.shape[0]
    ref_index, ref_offsets = vr.select_exact(vr.view_positions(xyz, cen), 1.0, 16, "scalar", 1.5)
    total = int(ref_offsets[-1])
    assert total == (B - 1) * N
    vox = _vox(16, 1.0)
    x = hip.dev(xyz)
    keep = []
    xfs, _ = vox._make_xforms(B, cen, _lib.MVX_DEVICE, 0.0, False, keep)
    sentinel = -7
    index = torch.full((total,), sentinel, dtype=torch.int64, device=vox.device)
    offsets = np.full(B + 1, -1, np.int64)

    def call(cap):
        torch.cuda.synchronize()
        return vox._lib.mvx_select_views(vox._handle, x.data_ptr(), None, None, 1.5, _lib.MVX_RADII_SCALAR, _lib.MODES["single"], N, 1,
                                         C.addressof(xfs), B, index.data_ptr(), cap, offsets.ctypes.data, _lib.MVX_DEVICE, vox._stream())

    assert call(total - 1) == MVX_ERR_INVALID
    assert b"index_capacity" in vox._lib.mvx_last_error()
    assert np.array_equal(offsets, ref_offsets)  # filled completely
    torch.cuda.synchronize()
    assert bool((index == sentinel).all())  # nothing written
    offsets[:] = -1
    assert call(total) == MVX_OK
    _check(index, offsets, ref_index, ref_offsets)


# ---- d. gather widths and bases ----------------------------------------------------------------------------------------------
def _gather_width(row_bytes, tensor):
    """gather_width of mvx_capi.hip for a source row; the destination is the handle's own allocation (256-byte aligned)."""
    bits = tensor.data_ptr() | row_bytes
    return 16 if bits % 16 == 0 else (8 if bits % 8 == 0 else 4)


def _offset_view(vox, array, skip):
    """`array` as a contiguous view that starts `skip` elements into a larger device tensor."""
    import torch

    flat = torch.as_tensor(np.ascontiguousarray(array), device=vox.device).reshape(-1)
    big = torch.empty(flat.numel() + skip + 16, dtype=flat.dtype, device=vox.device)
    big[skip:skip + flat.numel()] = flat
    return big[skip:skip + flat.numel()].view(array.shape)


# (id, precision, mode, C, radii_type, types dtype, which array starts off its allocation's base, by how many elements,
#  the width the features / types / radii / coords rows must take)
GATHER_ROWS = [
    ("f32-C1", 32, "features", 1, "scalar", None, None, 0, dict(chan=4)),
    ("f32-C2", 32, "features", 2, "scalar", None, None, 0, dict(chan=8)),
    ("f32-C4", 32, "features", 4, "scalar", None, None, 0, dict(chan=16)),
    ("f32-C6", 32, "features", 6, "scalar", None, None, 0, dict(chan=8)),
    ("f64-C1", 64, "features", 1, "scalar", None, None, 0, dict(chan=8)),
    ("f64-C2", 64, "features", 2, "scalar", None, None, 0, dict(chan=16)),
    ("f64-C3", 64, "features", 3, "scalar", None, None, 0, dict(chan=8)),
    ("f32-atom-radii", 32, "features", 4, "atom-wise", None, None, 0, dict(chan=16, radii=4)),
    ("f64-atom-radii", 64, "features", 2, "atom-wise", None, None, 0, dict(chan=16, radii=8)),
    ("types-int32", 32, "types", 5, "scalar", np.int32, None, 0, dict()),
    ("types-int64", 32, "types", 5, "atom-wise", np.int64, None, 0, dict(radii=4)),
    ("f32-C4-base+4", 32, "features", 4, "scalar", None, "chan", 1, dict(chan=4)),
    ("f32-C4-base+8", 32, "features", 4, "scalar", None, "chan", 2, dict(chan=8)),
    ("coords-base+24", 32, "features", 4, "scalar", None, "coords", 3, dict(chan=16, coords=8)),
    ("f32-radii-base+4", 32, "features", 4, "atom-wise", None, "radii", 1, dict(chan=16, radii=4)),
    ("f64-radii-base+8", 64, "features", 2, "atom-wise", None, "radii", 1, dict(chan=16, radii=8)),
]


@pytest.mark.parametrize("xf", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("row", GATHER_ROWS, ids=lambda r: r[0])
def test_gather_widths_and_bases(row, xf):
    import torch

    _, precision, mode, C_, radii_type, tdtype, off_what, skip, widths = row
    N, B, D = 700, 5, 16
    vox = _vox(D, 1.0, radii_type, precision=precision)
    xyz, chan, radii = rows.cloud(61 + C_, N, mode, C_, radii_type, edge=24.0)
    cen = rows.centers(61, B, xyz)
    esz = precision // 8
    if mode == "features":
        chan = chan.astype(vox.fp)
    else:
        chan = chan.astype(tdtype)
    if radii_type == "atom-wise":
        radii = radii.astype(vox.fp)
    place = lambda name, a: _offset_view(vox, a, skip) if off_what == name else hip.dev(a)  # noqa: E731
    x, ch, r = place("coords", xyz), place("chan", chan), (place("radii", radii) if radii_type == "atom-wise" else radii)
    # what the library is handed: the wrapper passes tensors of the right type through, whatever their base
    c_in, ch_in, r_in, _, _ = vox._views_inputs(x, ch, mode, r, C_)
    assert c_in.data_ptr() == x.data_ptr() and c_in.data_ptr() % 16 == (8 if off_what == "coords" else 0)
    assert _gather_width(24, c_in) == widths.get("coords", 8)
    if mode == "features":
        assert ch_in.data_ptr() == ch.data_ptr() and ch_in.data_ptr() % 16 == (skip * esz if off_what == "chan" else 0)
        assert _gather_width(C_ * esz, ch_in) == widths["chan"]
    else:
        assert ch_in.dtype == torch.int32 and _gather_width(4, ch_in) == 4
    if radii_type == "atom-wise":
        assert r_in.data_ptr() == r.data_ptr() and r_in.data_ptr() % 16 == (skip * esz if off_what == "radii" else 0)
        assert _gather_width(esz, r_in) == widths["radii"]
    nc = dict(num_channels=C_) if mode == "types" else {}
    got, ref = _grids(vox, x, hip.dev(cen), ch, r, xf, radii_type == "atom-wise", **nc)
    assert torch.equal(got, ref) and bool(got[1:].any()) and not bool(got[0].any())


# ---- e. the selection of every radii source against the reference ------------------------------------------------------------
@pytest.mark.parametrize("case", rows.SOURCE_CASES, ids=lambda c: f"{c[0].id}-{'rotated' if c[1] else 'identity'}")
def test_selection_of_every_radii_source_equals_the_reference(case):
    row, rotated = case
    xyz, cen, chan, radii = rows.source_inputs(row)
    ref_index, ref_offsets, _ = rows.source_reference(row, rotated)
    vox = _vox(row.D, row.res, row.radii_type, precision=row.precision)
    if row.mode == "features":
        chan = chan.astype(vox.fp)
    np.random.seed(rows.source_seed(row))
    index, offsets = vox.select_views(hip.dev(xyz), hip.dev(cen), hip.dev(chan), hip.dev(radii),
                                      **(rows.TRANSFORM if rotated else {}))
    _check(index, offsets, ref_index, ref_offsets)


@pytest.mark.parametrize("source, precision", [("channel-features", 32), ("channel-features", 64), ("atom-wise", 32),
                                               ("atom-wise", 64), ("scalar", 32)])
def test_selection_one_ulp_either_side_of_each_bound(source, precision):
    """res 0.3, D 17: half = 2.4 and half + 1.7 are no float32 values, so the float32-evaluated bound of channel-wise features
    at precision 32, the plain float64 one at precision 64 and the rounded sums of the atom-wise form all differ."""
    res, D = 0.3, 17
    fp = np.float32 if precision == 32 else np.float64
    radii_type = {"channel-features": "channel-wise", "atom-wise": "atom-wise", "scalar": "scalar"}[source]
    vox = _vox(D, res, radii_type, precision=precision)
    for axis in range(3):
        if source == "channel-features":
            radius = np.array([1.1, 1.7, 0.9], np.float32).astype(fp)
        else:
            radius = fp(np.float32(1.7)) if source == "atom-wise" else float(np.float32(1.7))
        xyz, keep = vr.edge_cloud(res, D, source, radius, precision, axis, reach=4)
        assert list(keep) == ([True] * 4 + [False] * 4) * 2
        chan = np.zeros((16, 3), fp) if source == "channel-features" else None
        radii = np.full(16, radius, fp) if source == "atom-wise" else radius
        index, offsets = vox.select_views(hip.dev(xyz), hip.dev(np.zeros((1, 3))), hip.dev(chan), hip.dev(radii))
        _check(index, offsets, np.flatnonzero(keep).astype(np.int64), np.array([0, 8], np.int64))


# ---- f. types outside [0, C) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radii_type, density", [("scalar", "gaussian"), ("atom-wise", "gaussian"), ("scalar", "binary")])
def test_types_outside_the_range_never_pass(radii_type, density):
    import torch

    from oracle import c_oracle

    N, B, D, res, C_ = 1500, 6, 16, 1.0, 5
    vox = _vox(D, res, radii_type, density)
    xyz, _, radii = rows.cloud(71, N, "types", C_, radii_type)
    cen = rows.centers(71, B, xyz)
    pool = np.array([-3, -1, 0, 1, 2, 3, 4, 5, 9, 2**31 - 1], np.int64)
    types = pool[np.random.default_rng(72).integers(0, pool.size, N)]
    inside = (types >= 0) & (types < C_)
    assert 0.3 < inside.mean() < 0.7
    x, t, c = hip.dev(xyz), hip.dev(types), hip.dev(cen)
    r = hip.dev(radii)
    got, ref = _grids(vox, x, c, t, r, False, radii_type == "atom-wise", num_channels=C_)
    assert got.shape == (B, C_, D, D, D) and torch.equal(got, ref)
    got_xf, ref_xf = _grids(vox, x, c, t, r, True, radii_type == "atom-wise", num_channels=C_)
    assert torch.equal(got_xf, ref_xf)
    got = got.cpu().numpy()
    for b in range(B):
        oracle = c_oracle.voxelize(xyz[inside] - cen[b], types[inside], radii[inside] if radii_type == "atom-wise" else radii,
                                   resolution=res, dimension=D, density=density, radii_type=radii_type, num_channels=C_)
        (assert_exact if density == "binary" else assert_gaussian)(got[b], oracle)
    assert got[1:].any()
    index, offsets = vox._select_views(x, c, t, r, num_channels=C_)
    seen = index.cpu().numpy()
    assert seen.size > 0 and inside[seen].all()
    ref_index, ref_offsets = vr.select_exact(vr.view_positions(xyz, cen), res, D, radii_type, radii, types=types.astype(np.int16),
                                             num_channels=C_)
    _check(index, offsets, ref_index, ref_offsets)
