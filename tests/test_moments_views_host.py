"""Moments of many views of one shared cloud without a GPU: the two C ABI entries (mvx_moments_views, mvx_moments_backward_views)
and every check they make before they touch a device, in order; the errors the Python layer
raises before it needs the library. The handle is looked at last by the rules that need no device: where a rule sits behind the
handle rule (the records of explicit poses) the handle is P in a call that still fails, so P is never dereferenced. The rules
behind those read the handle (the stride against C * D^3, the configurations named "moments:", the target's alignment):
tests/test_hip_moments_views.py checks them with a real one."""
import inspect

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call, declarations, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)
from tests.test_reject_order_host import _addr, _check, _off  # (the same scaffolding for tables of two mistakes)

BIG = 1 << 31
POSE = _lib.MVX_XF_POSE_PTR
ONE, TWO = records([0]), records([0, 0])
BAD_POSE = records([POSE | _lib.MVX_XF_ROTATE])

M_HANDLE = "null handle"
M_MODE_V = "bad mode"
M_RTYPE = "bad radii_type"
M_BNC = "B and N must be >= 0 and C > 0"
M_XF_V = "xforms must not be null (a view of the whole cloud is a record with flags = 0)"
M_CHANWISE = "Channel-Wise Radii Type is not supported"
M_SINGLE_V = "single mode has one channel"
M_COORDS = "coords must not be null"
M_RADII = "radii array required"
M_TYPES_V = "types must not be null"
M_MANY = "too many atoms"
M_CHANNELS = "channels must not be null"
M_POSE = "a MVX_XF_POSE_PTR record must have every other flag bit clear and a non-null center_ptr"
M_OFFNULL_IDX = "offsets_host must not be null with an index"
M_OFF0 = "offsets[0] must be 0"
M_OFFDEC = "offsets must be non-decreasing"
M_MANY_IDX = "too many atoms: offsets[B] must stay below 2^31"
M_MOMENTS = "moments must not be null"
M_STRIDE = "target_view_stride must be 0 (one shared target) or C * D^3 (one target per view)"
M_GM = "grad_moments must not be null"
M_GF = "grad_features exists in features mode only"
M_BOTH = "grad_coords and grad_features are both null"
# (the text mvx_score_views has for its per-row outputs: tests/test_reject_order_host.py)
M_NEED_INDEX = ("atom_scores, grad_coords and grad_features need an index: their rows are laid out in selection order "
                "(mvx_select_views)")


def _views_chain(own_first_kw):
    """The rules every views entry shares, in order (device arrays only: no memory kind to get wrong). own_first_kw: what breaks
    the entry's first own rule."""
    return [
        (dict(mode=3, rt=7), M_MODE_V),
        (dict(rt=7, B=-1), M_RTYPE),
        (dict(C_=0, xforms=None), M_BNC),
        (dict(N=-1, xforms=None), M_BNC),
        (dict(xforms=None, mode=2, rt=2, radii=P), M_XF_V),
        (dict(mode=2, rt=2, radii=P, C_=3), M_CHANWISE),
        (dict(mode=2, C_=3, coords=None), M_SINGLE_V),
        (dict(coords=None, rt=1), M_COORDS),
        (dict(rt=1, mode=1, channels=None), M_RADII),
        (dict(mode=1, channels=None, N=BIG), M_TYPES_V),
        (dict(N=BIG, **own_first_kw), M_MANY),
    ]


def _mviews(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, N=3, C_=4, xforms=ONE, B=1, index=None, offsets=None, target=P,
            stride=0, moments=P):
    keep, off = _off(offsets)
    return call(_lib.load().mvx_moments_views, h, mode, coords, channels, radii, 1.0, rt, N, C_, _addr(xforms), B, index, off, target,
                stride, moments, None)


def _bviews(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, N=3, C_=4, xforms=ONE, B=1, index=P, offsets=(0, 2), target=P,
            stride=0, gm=P, gc=P, gf=P):
    keep, off = _off(offsets)
    return call(_lib.load().mvx_moments_backward_views, h, mode, coords, channels, radii, 1.0, rt, N, C_, _addr(xforms), B, index, off,
                target, stride, gm, gc, gf, None)


def test_moments_views_reports_the_earlier_of_two_mistakes():
    _check(_mviews, _views_chain(dict(moments=None)) + [
        (dict(moments=None, stride=-1), M_MOMENTS),
        (dict(moments=None, index=P), M_MOMENTS),
        (dict(stride=-1, index=P), M_STRIDE),
        (dict(stride=-4 * 16 ** 3, channels=None), M_STRIDE),
        # (null offsets cannot also hold wrong values: "offsets_host must not be null" is paired with the rules behind the offsets)
        (dict(index=P, channels=None), M_OFFNULL_IDX),
        (dict(index=P, offsets=(1, 0)), M_OFF0),
        (dict(index=P, B=2, xforms=TWO, offsets=(0, 1 << 32, BIG)), M_OFFDEC),
        (dict(index=P, offsets=(0, BIG), channels=None), M_MANY_IDX),
        (dict(channels=None), M_CHANNELS),  # (and a null handle)
        (dict(channels=None, index=P, offsets=(0, 2), xforms=BAD_POSE), M_CHANNELS),
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE), M_POSE),
        (dict(h=P, xforms=BAD_POSE, index=P, offsets=(0, 2), stride=5), M_POSE),  # (the stride is judged behind the records)
    ])


def test_moments_views_gets_as_far_as_the_handle_with_good_arguments():
    for kw in (dict(), dict(target=None), dict(index=P, offsets=(0, 2)), dict(index=P, offsets=(0, 0), target=None),
               dict(B=0, xforms=None, moments=None, target=None), dict(N=0, coords=None, channels=None),
               dict(stride=4 * 16 ** 3), dict(stride=5),  # (neither 0 nor C * D^3: only a handle knows D)
               dict(mode=1), dict(mode=2, C_=1, channels=None)):
        rc, msg = _mviews(**kw)
        assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (kw, rc, msg)


def test_moments_backward_views_reports_the_earlier_of_two_mistakes():
    _check(_bviews, _views_chain(dict(gm=None)) + [
        (dict(gm=None, mode=1), M_GM),
        (dict(gm=None, gc=None, gf=None), M_GM),
        (dict(mode=1, gc=None), M_GF),
        (dict(mode=1, stride=-1), M_GF),
        (dict(gc=None, gf=None, stride=-1), M_BOTH),
        (dict(gc=None, gf=None, index=None), M_BOTH),
        (dict(stride=-1, index=None), M_STRIDE),
        (dict(index=None, channels=None), M_NEED_INDEX),
        (dict(index=None, offsets=None), M_NEED_INDEX),
        (dict(offsets=None, channels=None), M_OFFNULL_IDX),
        (dict(offsets=(1, 0)), M_OFF0),
        (dict(B=2, xforms=TWO, offsets=(0, 1 << 32, BIG)), M_OFFDEC),
        (dict(offsets=(0, BIG), channels=None), M_MANY_IDX),
        (dict(channels=None), M_CHANNELS),  # (and a null handle)
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE), M_POSE),
        (dict(h=P, xforms=BAD_POSE, stride=5), M_POSE),
    ])


def test_moments_backward_views_gets_as_far_as_the_handle_with_good_arguments():
    for kw in (dict(), dict(target=None), dict(gf=None), dict(gc=None), dict(mode=1, gf=None), dict(mode=2, C_=1, channels=None, gf=None),
               dict(offsets=(0, 0)), dict(B=0, xforms=None, gm=None, offsets=None, index=P), dict(N=0, coords=None, channels=None),
               dict(stride=4 * 16 ** 3), dict(stride=5)):
        rc, msg = _bviews(**kw)
        assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (kw, rc, msg)


def test_the_batch_entries_keep_their_prototypes():
    """The stride is an argument of the views entries alone: mvx_moments_batch and mvx_moments_backward_batch are as they were."""
    for name, count in (("mvx_moments_batch", 14), ("mvx_moments_backward_batch", 16)):
        params = declarations()[name][1]
        assert len(params) == count == len(_lib.SIGNATURES[name][1]) and "stride" not in " ".join(t + n for t, n in params), name


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), centers=np.zeros((B, 3)), channels=rng.standard_normal((N, C_)).astype(np.float32),
                radii=1.0)


POSE_KW = dict(quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)))


def _both(vox, **kw):
    """The two public entries with the same arguments."""
    return (lambda: vox.moments_views(**kw)), (lambda: vox.moments_posed_views(**kw, **POSE_KW))


def test_voxelizer_has_the_moments_views_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    one = inspect.signature(Voxelizer.moments_views).parameters
    assert list(one) == ["self", "coords", "centers", "channels", "radii", "target", "num_channels", "random_translation",
                         "random_rotation"]
    pos = inspect.signature(Voxelizer.moments_posed_views).parameters
    assert list(pos) == ["self", "coords", "centers", "quaternions", "translations", "channels", "radii", "target", "num_channels"]
    assert one["target"].default is None and one["num_channels"].default is None
    assert one["random_translation"].default == 0.0 and one["random_rotation"].default is False
    assert pos["target"].default is None and pos["num_channels"].default is None


@pytest.mark.parametrize("attrs, kw, words", [
    (dict(precision=64), {}, "precision 64"),
    (dict(radii_type="channel-wise"), dict(radii=np.ones(4, np.float32)), "channel-wise radii with features"),
    (dict(dimension=18), {}, "no multiple of 4"),
    (dict(dimension=24, blockdim=12), {}, "blockdim=12"),
])
def test_the_unsupported_configurations_name_moments_views_and_the_way_out(attrs, kw, words):
    attrs = dict(attrs)
    vox = _fake(attrs.pop("radii_type", "scalar"), attrs.pop("dimension", 16), **attrs)
    for call in _both(vox, **dict(_args(), **kw)):
        with pytest.raises(NotImplementedError) as e:
            call()
        msg = str(e.value)
        assert msg.startswith("moments_views does not support") and words in msg and "forward_views(...)" in msg, msg


def test_moments_of_views_need_torch_output_and_a_target_of_the_grids_shape():
    import torch

    for call in _both(_fake(output="numpy"), **_args()):
        with pytest.raises(ValueError, match="moments_views / moments_posed_views need output='torch'"):
            call()
    for shape in [(4, 16, 16), (3, 16, 16, 16), (3, 4, 16, 16, 16), (2, 5, 16, 16, 16), (1, 2, 4, 16, 16, 16), ()]:
        for call in _both(_fake(), target=torch.zeros(shape), **_args()):
            with pytest.raises(AssertionError, match="target does not match dimension"):
                call()
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):
        _fake().moments_posed_views(quaternions=np.ones((2, 3)), translations=np.zeros((2, 3)), **_args())
    with pytest.raises(AssertionError, match="centers does not match dimension"):
        _fake().moments_views(**dict(_args(), centers=np.zeros(3)))


def test_a_good_target_of_either_shape_gets_as_far_as_the_library():
    """(C, D, H, W) and (B, C, D, H, W) pass the rules: the fake has no library, and the call fails only there."""
    import torch

    for shape in [(4, 16, 16, 16), (2, 4, 16, 16, 16)]:
        for call in _both(_fake(), target=torch.zeros(shape), **_args()):
            with pytest.raises(Exception) as e:
                call()
            assert not isinstance(e.value, (AssertionError, ValueError, NotImplementedError)), repr(e.value)


def test_a_target_radii_or_sigma_that_requires_grad_is_refused_on_a_moments_grad_voxelizer():
    import torch

    a = _args()
    T = torch.zeros((2, 4, 16, 16, 16), requires_grad=True)
    on = dict(differentiable=True, _mgrad=True)
    for call in _both(_fake(**on), target=T, **a):
        with pytest.raises(ValueError, match="no gradient with respect to the target"):
            call()
    r = torch.ones(6, requires_grad=True)
    for call in _both(_fake("atom-wise", radii_grad=True, **on), **dict(a, radii=r)):
        with pytest.raises(ValueError, match="no gradient with respect to radii"):
            call()
    sig = torch.tensor(0.5, requires_grad=True)
    for call in _both(_fake(sigma_grad=True, _sigma_src=(sig, sig._version, 0.5), **on), **a):
        with pytest.raises(ValueError, match="no gradient with respect to sigma"):
            call()
    # without the flag the tensors are read as values: the call gets past the guards (and fails at the missing library)
    for call in _both(_fake(differentiable=True), target=T, **a):
        with pytest.raises(Exception) as e:
            call()
        assert not isinstance(e.value, (AssertionError, ValueError, NotImplementedError)), repr(e.value)


def test_a_voxelizer_made_with_new_still_has_every_default():
    """tests/fake_voxelizer.py sets none of the attributes the moments entries read beyond the constructor's: the class defaults
    serve (no moments_grad, one sum part, no selection yet)."""
    vox = _fake()
    assert "_mgrad" not in vars(vox) and vox._mgrad is False and vox._views_total == 0
    for name in ("moments_views", "moments_posed_views", "_moments_views", "_moments_backward_views"):
        assert callable(getattr(vox, name))
