"""Scores of many views of one shared cloud without a GPU: the two C ABI entries (mvx_score_views, mvx_views_reduce) and the
checks they make before they touch a device, the errors the Python layer raises before it
needs the library, the numpy restatement of the reduction checked against a dense scatter, and view_reduce_kernel's registers
read from mvx_views_reduce.o. (A stride that is neither 0 nor C * D^3 is judged against the handle's dimension:
tests/test_hip_score_views.py checks it with a real handle.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call, header_text, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)
from tests import views_reduce_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = records([0])


def _score(handle=None, mode=0, coords=P, channels=P, radii=None, radii_type=0, N=3, C_=4, xforms=ONE, B=1, index=None,
           offsets=None, field=P, stride=0, scores=P, atom_scores=None, grad_coords=None, grad_features=None):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_score_views, handle, mode, coords, channels, radii, 1.0, radii_type, N, C_,
                None if xforms is None else C.addressof(xforms), B, index, None if off is None else off.ctypes.data,
                field, stride, scores, atom_scores, grad_coords, grad_features, None)


@pytest.mark.parametrize("kw, words", [
    # what validate_views rejects
    (dict(mode=3), "bad mode"),
    (dict(mode=-1), "bad mode"),
    (dict(radii_type=7), "radii_type"),
    (dict(B=-1), "B and N must be"),
    (dict(N=-1), "B and N must be"),
    (dict(C_=0), "C > 0"),
    (dict(xforms=None), "xforms must not be null"),
    (dict(mode=2, C_=1, radii_type=2, radii=P), "Channel-Wise"),
    (dict(mode=2, C_=3), "single mode has one channel"),
    (dict(coords=None), "coords must not be null"),
    (dict(radii_type=1), "radii array required"),
    (dict(radii_type=2), "radii array required"),
    (dict(mode=1, channels=None), "types must not be null"),
    (dict(N=1 << 31), "too many atoms"),
    (dict(), "null handle"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR | _lib.MVX_XF_ROTATE])), "other flag bit"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR], ptr=None)), "center_ptr"),
    # what mvx_score_batch rejects for field, stride and scores (and its rule for grad_features)
    (dict(scores=None), "scores must not be null"),
    (dict(field=None), "field must not be null"),
    (dict(field=None, index=P, offsets=(0, 2)), "field must not be null"),
    (dict(stride=-1), "field_view_stride"),
    (dict(stride=-4 * 16 ** 3), "field_view_stride"),
    (dict(mode=1, index=P, offsets=(0, 2), grad_features=P), "grad_features"),
    (dict(channels=None), "channels must not be null"),
    # per-row outputs without an index
    (dict(atom_scores=P), "need an index"),
    (dict(grad_coords=P), "need an index"),
    (dict(grad_features=P), "need an index"),
    (dict(offsets=(0, 2), atom_scores=P), "need an index"),
    # an index without offsets, and bad offsets
    (dict(index=P), "offsets_host must not be null"),
    (dict(index=P, offsets=(1, 3)), "offsets[0]"),
    (dict(index=P, B=2, xforms=records([0, 0]), offsets=(0, 3, 2)), "non-decreasing"),
    (dict(index=P, offsets=(0, 1 << 31)), "2^31"),
])
def test_score_views_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _score(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_score_views_gets_as_far_as_the_handle_with_good_arguments():
    for kw in (dict(), dict(index=P, offsets=(0, 2)), dict(index=P, offsets=(0, 2), atom_scores=P, grad_coords=P, grad_features=P),
               dict(index=P, offsets=(0, 0), field=None), dict(B=0, xforms=None, scores=None, field=None),
               dict(N=0, coords=None, channels=None, field=None), dict(stride=4 * 16 ** 3)):
        rc, msg = _score(**kw)
        assert rc == MVX_ERR_INVALID and "null handle" in msg, (kw, rc, msg)


def _reduce(handle=None, index=P, offsets=(0, 2, 3), B=2, N=4, rows=P, width=3, row_type=1, out=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_views_reduce, handle, index, None if off is None else off.ctypes.data, B, N, rows, width, row_type, out, None)


@pytest.mark.parametrize("kw, words", [
    (dict(B=-1), "B and N must be"),
    (dict(N=-1), "B and N must be"),
    (dict(width=0), "width must be > 0"),
    (dict(width=-3), "width must be > 0"),
    (dict(row_type=2), "row_type"),
    (dict(row_type=-1), "row_type"),
    (dict(offsets=None), "offsets_host must not be null"),
    (dict(offsets=(1, 2, 3)), "offsets[0]"),
    (dict(offsets=(0, 3, 2)), "non-decreasing"),
    (dict(offsets=(0, 2, 1 << 31)), "2^31"),
    (dict(index=None), "index / rows"),
    (dict(rows=None), "index / rows"),
    (dict(out=None), "out must not be null"),
    (dict(), "null handle"),
])
def test_views_reduce_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _reduce(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_views_reduce_needs_no_arrays_where_sizes_are_zero():
    for kw in (dict(offsets=(0, 0, 0), index=None, rows=None), dict(B=0, offsets=None, index=None, rows=None),
               dict(N=0, out=None), dict(row_type=0)):
        rc, msg = _reduce(**kw)
        assert rc == MVX_ERR_INVALID and "null handle" in msg, (kw, rc, msg)


def test_the_row_types_are_the_headers():
    assert (_lib.MVX_ROW_FLOAT, _lib.MVX_ROW_DOUBLE) == (0, 1)
    assert re.search(r"enum mvx_row_type \{ MVX_ROW_FLOAT = 0, MVX_ROW_DOUBLE = 1 \}", header_text())


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), centers=np.zeros((B, 3)), channels=rng.standard_normal((N, C_)).astype(np.float32),
                radii=1.0)


POSE = dict(quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)))


def test_voxelizer_has_the_score_views_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    one = inspect.signature(Voxelizer.score_views).parameters
    assert list(one) == ["self", "coords", "centers", "channels", "radii", "field", "num_channels", "random_translation",
                         "random_rotation", "per_atom"]
    pos = inspect.signature(Voxelizer.score_posed_views).parameters
    assert list(pos) == ["self", "coords", "centers", "quaternions", "translations", "channels", "radii", "field", "num_channels",
                         "per_atom"]
    assert one["num_channels"].default is None and one["random_translation"].default == 0.0
    assert one["random_rotation"].default is False and one["per_atom"].default is False
    assert pos["num_channels"].default is None and pos["per_atom"].default is False
    assert list(inspect.signature(Voxelizer.views_reduce).parameters) == ["self", "rows", "index", "offsets", "num_atoms"]


def test_scores_of_views_need_torch_output():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_views(field=F, **_args())
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_posed_views(field=F, **_args(), **POSE)


def test_a_field_that_requires_grad_is_not_supported():
    import torch

    F = torch.zeros((4, 16, 16, 16), requires_grad=True)
    for diff in (False, True):
        with pytest.raises(NotImplementedError, match="dS/dfield is the grid itself"):
            _fake(differentiable=diff).score_views(field=F, **_args())
        with pytest.raises(NotImplementedError, match="dS/dfield is the grid itself"):
            _fake(differentiable=diff).score_posed_views(field=F, **_args(), **POSE)


def test_radii_and_sigma_that_require_grad_are_not_supported():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    a = _args()
    r = torch.ones(6, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to radii"):
        _fake("atom-wise", differentiable=True, radii_grad=True).score_views(field=F, **dict(a, radii=r))
    with pytest.raises(NotImplementedError, match="no gradient with respect to radii"):
        _fake("atom-wise", differentiable=True, radii_grad=True).score_posed_views(field=F, **dict(a, radii=r), **POSE)
    sig = torch.tensor(0.5, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to sigma"):
        _fake(differentiable=True, sigma_grad=True, _sigma_src=(sig, sig._version, 0.5)).score_views(field=F, **a)
    rs = torch.tensor([1.0], requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to a scalar radius"):
        _fake(differentiable=True, radii_grad=True).score_views(field=F, **dict(a, radii=rs))


@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 16, 16, 16), (3, 4, 16, 16, 16), (2, 5, 16, 16, 16), ()])
def test_a_field_of_the_wrong_shape_is_an_assertion_error(shape):
    import torch

    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_views(field=torch.zeros(shape), **_args())
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_posed_views(field=torch.zeros(shape), **_args(), **POSE)
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):
        _fake().score_posed_views(field=torch.zeros((4, 16, 16, 16)), quaternions=np.ones((2, 3)), translations=np.zeros((2, 3)), **_args())


# ---- the numpy restatement of the reduction ----------------------------------------------------------------------------------
def test_the_numpy_reduction_agrees_with_a_dense_scatter():
    assert vr.self_check()


# ---- kernel resources --------------------------------------------------------------------------------------------------------
def test_view_reduce_kernel_keeps_its_partials_in_registers():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_views_reduce.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_views_reduce.o not built")
    assert obj in regs.KERNEL_OBJECTS
    res = {k: v for k, v in regs.kernel_resources(obj).items() if "view_reduce_kernel" in k}
    assert sorted(res) == sorted(f"view_reduce_kernel<{t}, {nc}>" for t in ("float", "double") for nc in (1, 4, 32)), sorted(res)
    for k, r in res.items():
        nc = int(re.search(r", (\d+)>", k).group(1))
        assert r["vspill"] == 0 and r["sspill"] == 0 and r["scratch"] == 0, (k, r)
        assert r["lds"] == 4 * nc * 8, (k, r)  # the four waves' partials, nothing else
        # 32 double partials are 64 registers; with the row in flight the widest variant stays within two waves per SIMD of 256
        assert r["vgpr"] <= (192 if nc == 32 else 32), (k, r)
